"""CPU: the FASTA rules' plain restatement (spec_fasta_files.py) equals the host route `read_fasta_records` on every
case; the host route reads .gz names through gzip; the C ABI and the command line know the device route."""
import gzip
import os
import re

import numpy as np
import pytest

import spec_fasta_files as spec
from fasta_cases import CASES, MISSING, SELECTIONS
from graph_kmer_index_amd import _lib, bgzf
from graph_kmer_index_amd.snp_kmer_finder import read_fasta_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gki_fasta_parse_count", "gki_fasta_parse_names", "gki_fasta_parse_emit")


def write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def assert_host_equals_spec(path, data, names):
    want_names, want, _ = spec.read(data, names, path)
    got_names, got = read_fasta_records(path, names)
    assert list(got_names) == want_names
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == np.uint8 and g.tobytes() == w


@pytest.mark.parametrize("name", list(CASES))
def test_spec_equals_host_route(name, tmp_path):
    path = write(tmp_path / "ref.fa", CASES[name])
    for names in [None] + SELECTIONS.get(name, []):
        assert_host_equals_spec(path, CASES[name], names)


@pytest.mark.parametrize("name", list(MISSING))
def test_missing_name_is_the_same_key_error(name, tmp_path):
    path = write(tmp_path / "ref.fa", CASES[name])
    with pytest.raises(KeyError) as want:
        spec.read(CASES[name], [MISSING[name]], path)
    with pytest.raises(KeyError) as got:
        read_fasta_records(path, [MISSING[name]])
    assert got.value.args == want.value.args and "records: " in got.value.args[0]


def test_every_selection_names_a_case():
    assert set(SELECTIONS) <= set(CASES) and set(MISSING) <= set(CASES)
    found = spec.records(CASES["name_twice"])[0]
    assert found.count("x") == 2 and spec.records(CASES["empty_name_twice"])[0][:2] == ["", ""]
    assert spec.records(CASES["no_name"])[0] == ["", "desc"]           # bytes.split(): the first word behind the '>'


@pytest.mark.parametrize("name", ["many_records", "many_records_crlf_open_end", "name_twice"])
def test_host_route_reads_gzip_and_bgzf(name, tmp_path):
    data = CASES[name]
    plain = write(tmp_path / "ref.fa", data)
    zipped = write(tmp_path / "ref_gzip.fa.gz", gzip.compress(data))
    blocked = str(tmp_path / "ref_bgzf.fa.gz")
    bgzf.write_bgzf(blocked, data, block_size=97)                       # members end mid-line and mid-header
    with open(blocked, "rb") as f:
        assert bgzf.is_bgzf(f.read(64))
    want_names, want = read_fasta_records(plain)
    for path in (zipped, blocked):
        for names in [None] + SELECTIONS.get(name, []):
            assert_host_equals_spec(path, data, names)
        got_names, got = read_fasta_records(path)
        assert got_names == want_names and all(np.array_equal(a, b) for a, b in zip(got, want))


def test_new_symbols_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "gki.h")).read()
    assert "FASTA files" in text
    declared = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, declared), name
        assert name in _lib.SYMBOLS
        assert hasattr(_lib.load(), name)


@pytest.mark.parametrize("command", [["make", "-o", "out", "-R", "ref.fa", "-n", "1"],
                                     ["make_reference_kmer_index", "-o", "out", "-r", "ref.fa", "-n", "1"],
                                     ["make_graph", "-o", "out", "-r", "ref.fa", "-v", "v.vcf"]])
def test_command_line_accepts_fasta_parse(command):
    from graph_kmer_index_amd.command_line_interface import build_parser
    parser = build_parser()
    assert parser.parse_args(command).fasta_parse == "auto"
    for choice in ("auto", "host", "device"):
        assert parser.parse_args(command + ["--fasta-parse", choice]).fasta_parse == choice
    with pytest.raises(SystemExit):
        parser.parse_args(command + ["--fasta-parse", "elsewhere"])


def test_fasta_parse_choice_is_checked():
    from graph_kmer_index_amd.fasta_files import resolve_fasta_parse
    assert resolve_fasta_parse("host") == "host" and resolve_fasta_parse("device") == "device"
    assert resolve_fasta_parse("auto") in ("host", "device")
    with pytest.raises(ValueError):
        resolve_fasta_parse("elsewhere")
