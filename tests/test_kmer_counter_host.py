"""Host side of KmerCounter / KmerFrequencyIndex (no GPU): scalar accessors from host arrays, files, command-line options,
and KmerFrequencyIndex.get against what the reference's get returned on the same arrays."""
import os

import numpy as np
import pytest

import spec_kmer_counter as spec
from graph_kmer_index_amd import KmerCounter, KmerFrequencyIndex
from graph_kmer_index_amd.kmer_counter import SORT_TILE, choose_modulo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_choose_modulo_and_tile_constant():
    assert [choose_modulo(n) for n in (0, 999999, 1000000, 9999999, 10000000)] == \
        [2000003, 2000003, 19999999, 19999999, 200000003]
    src = open(os.path.join(ROOT, "graph_kmer_index_amd", "csrc", "gki_count.hip")).read()
    assert "constexpr int CB = 256;" in src and "constexpr int CI = 16;" in src and SORT_TILE == 256 * 16


def test_scalar_get_frequency_and_files(tmp_path):
    keys = np.array([3, 10, 1 << 40, (1 << 62) - 1], dtype=np.uint64)
    counts = np.array([1, 70000, 1 << 33, 2], dtype=np.int64)
    c = KmerCounter(keys, counts, modulo=2000003)
    table = spec.DictCounter(keys, counts)
    for q in (0, 2, 3, 4, 10, 1 << 40, (1 << 40) + 1, (1 << 62) - 1, 1 << 62, (1 << 64) - 1, np.uint64(10), np.int64(3)):
        assert c.get_frequency(q) == table.get_frequency(q)
        assert isinstance(c.get_frequency(q), int)
    assert KmerCounter(np.zeros(0, np.uint64), np.zeros(0, np.int64)).get_frequency(5) == 0
    c.to_file(str(tmp_path / "counter"))
    back = KmerCounter.from_file(str(tmp_path / "counter.npz"))
    assert np.array_equal(back._kmers, keys) and np.array_equal(back._counts, counts) and back._modulo == 2000003
    with pytest.raises(FileNotFoundError):
        KmerCounter.from_file(str(tmp_path / "none"))
    np.savez(str(tmp_path / "other.npz"), x=np.arange(3))
    with pytest.raises(ValueError, match="npstructures"):
        KmerCounter.from_file(str(tmp_path / "other.npz"))
    with pytest.raises(ValueError):
        KmerCounter(keys, counts[:2])


def test_frequency_index_get_is_the_references(tmp_path):
    rec = spec.golden()["frequency_index"]
    for name in spec.frequency_index_inputs():
        idx = KmerFrequencyIndex(np.array(rec[name]["kmers"], dtype=np.uint64), np.array(rec[name]["frequencies"], dtype=np.int64))
        for q, want in zip(rec[name]["probes"], rec[name]["get"]):
            if want == "IndexError":
                with pytest.raises(IndexError):
                    idx.get(np.uint64(q))
            else:
                assert int(idx.get(np.uint64(q))) == want
        idx.to_file(str(tmp_path / name))
        back = KmerFrequencyIndex.from_file(str(tmp_path / name))
        assert sorted(np.load(tmp_path / (name + ".npz")).files) == ["frequencies", "kmers"]
        assert np.array_equal(back._kmers, idx._kmers) and np.array_equal(back._frequencies, idx._frequencies)


def test_cli_options_and_frequency_source_choice(tmp_path):
    from graph_kmer_index_amd.command_line_interface import build_parser, load_frequency_source
    p = build_parser()
    a = p.parse_args(["count_kmers", "-f", "flat", "-o", "out"])
    assert (a.flat_kmers, a.out_file_name, a.modulo, a.subsample_ratio) == ("flat", "out", 0, 1)
    a = p.parse_args(["count_kmers", "-f", "flat", "-o", "out", "-m", "1000003", "-s", "3"])
    assert (a.modulo, a.subsample_ratio) == (1000003, 3)
    a = p.parse_args(["make_kmer_frequency_index", "-r", "ref", "-o", "out"])
    assert (a.reference_kmers, a.out_file_name) == ("ref", "out")
    KmerCounter(np.array([5], np.uint64), np.array([2], np.int64)).to_file(str(tmp_path / "counter"))
    a = p.parse_args(["sample_kmers_from_structural_variants", "-g", "g", "-V", "v", "-k", "31", "-o", "o", "-I",
                      str(tmp_path / "counter")])
    source = load_frequency_source(a, "sample_kmers_from_structural_variants")
    assert isinstance(source, KmerCounter) and source.get_frequency(5) == 2
    a.kmer_counter = None
    with pytest.raises(ValueError, match="-i"):
        load_frequency_source(a, "sample_kmers_from_structural_variants")
