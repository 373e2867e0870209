"""-m gpu: VCF text parsed on the device (csrc/gki_vcf_parse.hip, graph_kmer_index_amd/vcf_files.py) against the rules of
tests/spec_vcf_parse.py and against VariantArrays.from_vcf, the host route that stays the oracle: the C ABI array for array,
the bad lines, the capacities, the three encodings of a file at several piece sizes, what stays allocated, and the
--vcf-parse flag of make_unique_variant_kmers.  Every comparison is exact."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import spec_vcf_parse as spec
import uvk_simple_cases as uvk
import vcf_cases as cases
from graph_kmer_index_amd import _lib, bgzf, read_files, vcf_files
from graph_kmer_index_amd.unique_variant_kmers import VariantArrays, VariantToNodesArrays
from test_vcf_parse_spec import assert_same_variants, host_arrays

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = 2          # GKI_ERR_BAD_ARG
GUARD = 0x5A


def device_count(d, n):
    out = vcf_files.vcf_count(d, n)
    return dict(zip(("n_lines", "n_variants", "n_runs", "n_name_bytes", "first_bad_variant", "first_bad_kind"), out))


def emit_with_guards(d, n, n_variants, n_runs, n_name_bytes, guard=3):
    """(status, positions, is_snp, chrom_run, run_name_start, run_names, guards untouched) of one emit call into buffers
    with `guard` entries behind each capacity, filled with GUARD bytes beforehand."""
    shapes = ((n_variants, np.int64), (n_variants, np.int8), (n_variants, np.int32), (n_runs + 1, np.int64),
              (n_name_bytes, np.uint8))
    bufs = [_lib.DeviceArray(max(m, 0) + guard, dt) for m, dt in shapes]
    for b in bufs:
        _lib.check(_lib.load().gki_memset(b.ptr, GUARD, b.nbytes))
    rc = _lib.load().gki_vcf_parse_emit(d.ptr, n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n_variants, bufs[3].ptr, n_runs,
                                        bufs[4].ptr, n_name_bytes)
    host = [b.to_host() for b in bufs]
    for b in bufs:
        b.free()
    filler = [np.frombuffer(bytes([GUARD]) * np.dtype(dt).itemsize, dtype=dt)[0] for _, dt in shapes]
    kept = all((h[max(m, 0):] == f).all() for h, (m, _), f in zip(host, shapes, filler))
    untouched = all((h == f).all() for h, f in zip(host, filler))
    return rc, [h[:max(m, 0)] for h, (m, _) in zip(host, shapes)], kept, untouched


def assert_abi_equals_spec(data, d, n):
    want = spec.parse(data)
    got = device_count(d, n)
    assert got == {"n_lines": want["n_lines"], "n_variants": len(want["positions"]), "n_runs": len(want["run_name_start"]) - 1,
                   "n_name_bytes": len(want["run_names"]), "first_bad_variant": -1, "first_bad_kind": 0}
    rc, arrays, kept, _ = emit_with_guards(d, n, got["n_variants"], got["n_runs"], got["n_name_bytes"])
    assert rc == 0 and kept
    for a, key in zip(arrays, ("positions", "is_snp", "chrom_run", "run_name_start", "run_names")):
        assert a.dtype == want[key].dtype and np.array_equal(a, want[key]), key


# ------------------------------------------------------------------ the C ABI and parse_vcf_on_device
@pytest.mark.parametrize("name", sorted(cases.GOOD))
def test_good_case_equals_spec_and_host(name, tmp_path):
    data = cases.GOOD[name]
    d = _lib.DeviceArray.from_host(np.frombuffer(data, dtype=np.uint8))
    assert_abi_equals_spec(data, d, len(data))
    d.free()
    positions, is_snp, chrom_run, run_names, n_lines = vcf_files.parse_vcf_on_device(data)
    want = spec.parse(data)
    assert n_lines == want["n_lines"] and run_names == spec.run_name_list(want)
    assert (positions.dtype, is_snp.dtype, chrom_run.dtype) == (np.int64, np.int8, np.int32)
    pieces = vcf_files.VariantPieces()
    pieces.add(positions, is_snp, chrom_run, run_names, n_lines)
    assert_same_variants(pieces.variant_arrays(), host_arrays(tmp_path, data))


@pytest.mark.parametrize("name", cases.UNALIGNED)
def test_unaligned_device_address(name):
    """A view one byte into a DeviceArray: the line-end pass takes its byte loads; the answer is the same."""
    data = cases.GOOD[name]
    whole = _lib.DeviceArray.from_host(np.frombuffer(b"\n" + data + b"9\t9\t.\tA\tC\n", dtype=np.uint8))
    view = whole.view(1, len(data))
    assert view.ptr.value % 16 == 1
    assert_abi_equals_spec(data, view, len(data))
    got = vcf_files.parse_vcf_on_device(view)
    assert np.array_equal(got[0], spec.parse(data)["positions"])
    whole.free()


def test_names_are_decoded_as_utf8():
    data = "chré\t5\t.\tA\tC\nchré\t6\t.\tA\tC\né\t7\n".encode("utf-8")
    positions, is_snp, chrom_run, run_names, n_lines = vcf_files.parse_vcf_on_device(np.frombuffer(data, dtype=np.uint8))
    assert run_names == ["chré", "é"] and chrom_run.tolist() == [0, 0, 1] and is_snp.tolist() == [1, 1, -1]


# ------------------------------------------------------------------ bad lines
@pytest.mark.parametrize("name", sorted(cases.BAD))
def test_bad_case(name, tmp_path):
    data, line, kind = cases.BAD[name]
    d = _lib.DeviceArray.from_host(np.frombuffer(data, dtype=np.uint8))
    got = device_count(d, len(data))                    # reported, and the call returned 0
    want = spec.parse(data)
    assert (got["first_bad_variant"], got["first_bad_kind"]) == (line, kind)
    assert (got["n_lines"], got["n_variants"]) == (want["n_lines"], len(want["positions"]))
    rc, _, _, untouched = emit_with_guards(d, len(data), got["n_variants"], got["n_runs"], got["n_name_bytes"])
    assert rc == BAD_ARG and untouched
    d.free()
    path = str(tmp_path / "bad.vcf")
    with open(path, "wb") as fh:
        fh.write(data)
    for chunk_bytes in (8 if len(data) < 200 else 4096, None):      # the number is the file's, whatever piece shows it
        with pytest.raises(ValueError) as e:
            vcf_files.variant_arrays_from_file(path, chunk_bytes=chunk_bytes)
        assert str(e.value) == str(vcf_files.bad_line_error(line, kind))
        if kind == 1:
            assert str(e.value) == spec.KIND1_TEXT % line
    with pytest.raises(ValueError):
        vcf_files.parse_vcf_on_device(data)


# ------------------------------------------------------------------ capacities
def test_capacity_one_too_small_writes_nothing():
    data = cases.GOOD["prefix_names"]
    d = _lib.DeviceArray.from_host(np.frombuffer(data, dtype=np.uint8))
    c = device_count(d, len(data))
    full = (c["n_variants"], c["n_runs"], c["n_name_bytes"])
    assert min(full) > 0
    for short in range(3):
        caps = [x - (1 if i == short else 0) for i, x in enumerate(full)]
        rc, _, _, untouched = emit_with_guards(d, len(data), *caps)
        assert rc == BAD_ARG and untouched, short
    rc, _, kept, _ = emit_with_guards(d, len(data), *full)
    assert rc == 0 and kept
    d.free()
    with pytest.raises(_lib.GkiError):
        _lib.check(_lib.load().gki_vcf_parse_count(None, -1, None, None, None, None, None, None))


# ------------------------------------------------------------------ files
def _file_lines():
    """200 data lines on three chromosomes behind a header, an indel every seventh line and a few genotype columns."""
    out = [cases.HEADER[:-1] + b"\tFORMAT\tS1\tS2\tS3\n"]
    for i in range(200):
        chrom = (b"chr1", b"chr10", b"chrX")[0 if i < 90 else 1 if i < 150 else 2]
        ref, alt = (b"AC", b"A") if i % 7 == 3 else (b"A", b"G")
        out.append(b"%s\t%d\trs%d\t%s\t%s\t50\tPASS\tDP=%d\tGT\t0|1\t1|1\t0|0\n" % (chrom, 1000 + 13 * i, i, ref, alt, i))
    return b"".join(out)


@pytest.fixture(scope="module")
def three_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("vcf_files")
    data = _file_lines()
    paths = {"plain": str(d / "v.vcf"), "gzip": str(d / "v_gzip.vcf.gz"), "bgzf": str(d / "v_bgzf.vcf.gz")}
    with open(paths["plain"], "wb") as fh:
        fh.write(data)
    with open(paths["gzip"], "wb") as fh:
        fh.write(gzip.compress(data))
    bgzf.write_bgzf(paths["bgzf"], data, block_size=777)             # lines span members
    return paths, VariantArrays.from_vcf(paths["plain"])


@pytest.mark.parametrize("encoding", ["plain", "gzip", "bgzf"])
def test_file_routes_equal_host(three_files, encoding):
    paths, want = three_files
    assert len(want) == 200 and len(set(want.chromosomes.tolist())) == 3 and set(want.is_snp.tolist()) == {0, 1}
    assert_same_variants(VariantArrays.from_vcf(paths[encoding]), want)
    for chunk_bytes in (64, 1000, vcf_files.DEFAULT_CHUNK_BYTES):
        assert_same_variants(vcf_files.variant_arrays_from_file(paths[encoding], chunk_bytes=chunk_bytes), want)
    assert_same_variants(vcf_files.variant_arrays_from_file(paths[encoding], chunk_bytes=1000, inflate="host"), want)
    assert_same_variants(VariantArrays.from_vcf_on_device(paths[encoding]), want)


def test_routes_and_inflate_choice(three_files):
    paths, want = three_files
    assert read_files.reads_file_route(paths["bgzf"]) == "bgzf-device"
    assert read_files.reads_file_route(paths["gzip"]) == "gzip-host" and read_files.reads_file_route(paths["plain"]) == "raw"
    assert_same_variants(vcf_files.variant_arrays_from_file(paths["bgzf"], chunk_bytes=1000, inflate="device"), want)
    with pytest.raises(ValueError) as e:
        vcf_files.variant_arrays_from_file(paths["gzip"], inflate="device")
    assert "is not a BGZF file" in str(e.value)
    with pytest.raises(ValueError):
        vcf_files.variant_arrays_from_file(paths["plain"], inflate="gpu")


def test_empty_file_gives_the_hosts_empty_arrays(tmp_path):
    for name, data in (("empty.vcf", b""), ("headers.vcf", cases.HEADER)):
        want = host_arrays(tmp_path, data, name)
        got = vcf_files.variant_arrays_from_file(str(tmp_path / name))
        assert len(got) == 0
        assert_same_variants(got, want)


def _balance(run):
    """device mallocs minus device frees over `run`, the pool emptied before and after."""
    lib = _lib.load()
    _lib.check(lib.gki_trim())
    before = _lib.pool_stats()
    run()
    _lib.check(lib.gki_trim())
    after = _lib.pool_stats()
    return (after[0] - before[0]) - (after[1] - before[1])


def test_nothing_stays_allocated(three_files, tmp_path):
    paths, _ = three_files
    for encoding in ("plain", "bgzf"):
        assert _balance(lambda: vcf_files.variant_arrays_from_file(paths[encoding], chunk_bytes=1000)) == 0, encoding
    bad = str(tmp_path / "bad.vcf.gz")
    bgzf.write_bgzf(bad, _file_lines() + b"chrX\t12x\t.\tA\tC\n" + _file_lines(), block_size=777)

    def run_bad():
        with pytest.raises(ValueError) as e:
            vcf_files.variant_arrays_from_file(bad, chunk_bytes=1000)
        assert str(e.value) == str(vcf_files.bad_line_error(200, 2))
    assert _balance(run_bad) == 0


# ------------------------------------------------------------------ command line
def _run_cli(args, tmp_path):
    subprocess.run([sys.executable, "-m", "graph_kmer_index_amd.command_line_interface"] + args, check=True,
                   env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp_path))


def test_cli_device_and_host_parse_write_the_same_columns(tmp_path):
    case = min(uvk.load_cases(), key=lambda c: len(c["variants"]["positions"]))
    pos, chrom, lines, is_snp, ref, var = uvk.case_variants(case)
    uvk.case_graph(case).to_file(str(tmp_path / "graph.npz"))
    VariantToNodesArrays(ref, var).to_file(str(tmp_path / "v2n.npz"))
    uvk.write_vcf(tmp_path / "v.vcf", pos, chrom, is_snp)
    with open(tmp_path / "v.vcf", "rb") as fh:
        bgzf.write_bgzf(str(tmp_path / "v.vcf.gz"), fh.read(), block_size=100)
    assert read_files.reads_file_route(str(tmp_path / "v.vcf.gz")) == "bgzf-device"
    base = ["make_unique_variant_kmers", "-g", "graph.npz", "-V", "v2n.npz", "-k", str(case["k"]), "-m",
            str(case["max_variant_nodes"]), "-v", "v.vcf.gz", "-S", "True"]
    _run_cli(base + ["--vcf-parse", "device", "-o", "device"], tmp_path)
    _run_cli(base + ["--vcf-parse", "host", "-o", "host"], tmp_path)
    device, host = np.load(tmp_path / "device.npz"), np.load(tmp_path / "host.npz")
    assert sorted(device.files) == sorted(host.files) and len(device["hashes"]) > 0
    for key in host.files:
        assert device[key].dtype == host[key].dtype and np.array_equal(device[key], host[key]), key
    for key, b in zip(("hashes", "nodes", "ref_offsets", "allele_frequencies"), uvk.expected(case)):
        assert np.array_equal(device[key], b)
