"""-m gpu: text deflated into BGZF members on the device (csrc/gki_bgzf_deflate.hip, graph_kmer_index_amd/bgzf.py;
DESIGN.md 4.22).  Every vector of tests/deflate_cases.py is checked by zlib and gzip on the host and is byte-equal to
what the host program built from the same core writes (tests/deflate_core_main.cpp); then the writer, the genotyped VCF
and the two commands.  Every comparison is exact."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import deflate_cases as cases
import read_file_cases as text_cases
import spec_genotype as spec
from graph_kmer_index_amd import _lib, bgzf
from graph_kmer_index_amd.command_line_interface import main
from graph_kmer_index_amd.genotyper import write_genotyped_vcf
from graph_kmer_index_amd.unique_variant_kmers import VariantToNodesArrays
from graph_kmer_index_amd.vcf_files import variant_arrays_from_file
from test_deflate_core_cpu import build_program, run_program
from test_gpu_genotype import calls_for, case, model_of, vcf_text
from test_gpu_read_files import small_index, write

pytestmark = pytest.mark.gpu


def deflate(text, block_size):
    out, n = bgzf.deflate_on_device(text, block_size)
    got = out.to_host(n).tobytes()
    out.free()
    return got


@pytest.fixture(scope="module")
def on_device():
    """Every vector through gki_bgzf_deflate, once; read only."""
    return {name: deflate(*cases.vectors()[name]) for name in cases.NAMES}


@pytest.fixture(scope="module")
def on_host(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("deflate_host"))
    program = build_program(tmp)
    return None if program is None else run_program(program, tmp, cases.NAMES)


@pytest.mark.parametrize("name", cases.NAMES)
def test_members_are_bgzf_that_zlib_and_gzip_read_back(on_device, name):
    cases.check_members(name, on_device[name])


def test_every_vector_is_byte_equal_to_the_host_programs(on_device, on_host):
    if on_host is None:
        pytest.skip("no C++ compiler here built the host program")
    assert [name for name in cases.NAMES if on_device[name] != on_host[name]] == []


def test_the_same_input_gives_the_same_bytes_again(on_device):
    for name in ("vcf_3_members", "many_1025+1", "fastq"):
        assert deflate(*cases.vectors()[name]) == on_device[name]


def test_round_trip_through_the_inflate_kernel(on_device):
    for name in ("vcf_3_members", "many_65+1", "random", "zeros", "dna"):
        data = on_device[name]
        members, left = bgzf.scan_all(data)
        assert left == 0
        out = bgzf.inflate_on_device(data, members)
        assert out.to_host().tobytes() == cases.vectors()[name][0], name
        out.free()


def test_device_input_member_ends_and_kernel_time():
    text, block_size = cases.vectors()["many_65+1"]
    lib = _lib.load()
    with _lib.DeviceScope() as s:
        d_in = s.on_device(np.frombuffer(text, dtype=np.uint8), np.uint8)
        out, n = bgzf.deflate_on_device(d_in, block_size, n=len(text) - 150)
        s.keep(out)
        ms = C.c_float(-1)
        assert lib.gki_bgzf_deflate_kernel_ms(C.byref(ms)) == 0 and 0 < ms.value < 1000
        got = out.to_host(n).tobytes()
        assert got == deflate(text[:-150], block_size)
        bound, n_out, n_members = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        assert lib.gki_bgzf_deflate_bound(len(text), block_size, C.byref(bound)) == 0
        assert bound.value == len(text) + 31 * 66
        ends = s.array(66, np.int64)
        packed = s.array(bound.value, np.uint8)
        assert lib.gki_bgzf_deflate(d_in.ptr, len(text), block_size, packed.ptr, bound.value, C.byref(n_out), C.byref(n_members),
                                    ends.ptr) == 0
        assert n_members.value == 66
        scanned, left = bgzf.scan_all(packed.to_host(n_out.value).tobytes())
        assert left == 0 and [m[4] for m in scanned] == ends.to_host().tolist() and ends.to_host()[-1] == n_out.value
        # no bytes: no member, nothing launched
        assert lib.gki_bgzf_deflate(None, 0, block_size, None, 0, C.byref(n_out), C.byref(n_members), None) == 0
        assert (n_out.value, n_members.value) == (0, 0)
        assert lib.gki_bgzf_deflate_kernel_ms(C.byref(ms)) == 0 and ms.value == 0


def test_bad_arguments_are_refused_and_nothing_is_written():
    lib = _lib.load()
    text = cases.vectors()["many_63+0"][0]
    with _lib.DeviceScope() as s:
        d_in = s.on_device(np.frombuffer(text, dtype=np.uint8), np.uint8)
        bound = len(text) + 31 * 63
        out = s.on_device(np.full(bound + 64, 0xAA, dtype=np.uint8), np.uint8)
        n_out, n_members, b = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
        for args in ((d_in.ptr, len(text), 0, out.ptr, out.n), (d_in.ptr, len(text), 0xff01, out.ptr, out.n),
                     (d_in.ptr, -1, 100, out.ptr, out.n), (d_in.ptr, len(text), 100, out.ptr, -1),
                     (None, len(text), 100, out.ptr, out.n), (d_in.ptr, len(text), 100, None, out.n),
                     (d_in.ptr, len(text), 100, out.ptr, bound - 1)):
            assert lib.gki_bgzf_deflate(*args, C.byref(n_out), C.byref(n_members), None) == 2, args[1:3]
            assert (n_out.value, n_members.value) == (0, 0)
        assert b"below the bound" in lib.gki_last_error()
        assert not (out.to_host() != 0xAA).any()             # nothing was written by any of them
        for n, block_size in ((-1, 100), (5, 0), (5, 0xff01)):
            assert lib.gki_bgzf_deflate_bound(n, block_size, C.byref(b)) == 2 and b.value == 0
        assert lib.gki_bgzf_deflate(d_in.ptr, len(text), 100, out.ptr, bound, C.byref(n_out), C.byref(n_members), None) == 0
        got = out.to_host()
        assert n_members.value == 63 and not (got[n_out.value:] != 0xAA).any()
        assert gzip.decompress(got[:n_out.value].tobytes() + bgzf.EOF_MEMBER) == text


# ------------------------------------------------------------------ the writer
def test_the_file_does_not_depend_on_how_the_text_was_cut_into_writes(tmp_path):
    text = cases.vectors()["vcf"][0][:20000]
    files = {}
    for cut in (1, 99, 100, 101, 6000, len(text)):
        path = str(tmp_path / ("cut%d.gz" % cut))
        with bgzf.BgzfWriter(path, 100) as w:
            if cut == 1:                                     # byte by byte for the first 450 bytes, then the rest
                for a in range(450):
                    w.write(text[a:a + 1])
                w.write(text[450:])
            else:
                for a in range(0, len(text), cut):
                    w.write(text[a:a + cut])
        assert (w.bytes_in, w.bytes_out) == (len(text), os.path.getsize(path))
        files[cut] = open(path, "rb").read()
    assert len(set(files.values())) == 1
    assert files[1] == deflate(text, 100) + bgzf.EOF_MEMBER and gzip.decompress(files[1]) == text
    assert bgzf.is_bgzf(files[1][:18])


def test_device_writes_a_whole_buffer_a_streamed_file_and_an_empty_one(tmp_path):
    text = cases.vectors()["vcf_3_members"][0]
    whole, streamed, from_device, empty = (str(tmp_path / n) for n in ("whole.gz", "streamed.gz", "device.gz", "empty.gz"))
    plain = write(tmp_path, "plain.txt", text)
    assert bgzf.write_bgzf_on_device(whole, text) == os.path.getsize(whole)
    bgzf.write_bgzf_on_device(streamed, plain, chunk_bytes=7001)
    d = _lib.DeviceArray.from_host(np.frombuffer(text, dtype=np.uint8))
    with bgzf.BgzfWriter(from_device) as w:
        w.write_device(d, 70000)
        w.write_device(d.view(70000, d.n - 70000))
    d.free()
    want = open(whole, "rb").read()
    assert want == deflate(text, 0xff00) + bgzf.EOF_MEMBER
    assert open(streamed, "rb").read() == want and open(from_device, "rb").read() == want
    bgzf.write_bgzf_on_device(empty, b"")
    assert open(empty, "rb").read() == bgzf.EOF_MEMBER
    with pytest.raises(ValueError, match="closed"):
        w.write(b"more")


def test_failure_paths_remove_the_output_file(tmp_path):
    path = str(tmp_path / "out.gz")
    with pytest.raises(RuntimeError, match="stop"):
        with bgzf.BgzfWriter(path, 100) as w:
            w.write(b"x" * 1000)
            assert os.path.exists(path)
            raise RuntimeError("stop")
    assert not os.path.exists(path)
    with pytest.raises(ValueError):
        with bgzf.BgzfWriter(path) as w:
            w.write_device(np.zeros(4, np.uint8))            # not a DeviceArray
    assert not os.path.exists(path)


# ------------------------------------------------------------------ the genotyped VCF
def test_write_genotyped_vcf_as_bgzf(tmp_path):
    n = 333
    text = vcf_text(n)
    call, gq = calls_for(n, 2, 5)
    plain_in, none_out = write(tmp_path, "in.vcf", text), str(tmp_path / "none.vcf")
    assert write_genotyped_vcf(plain_in, none_out, call, gq, 2, "NA12") == n
    want = open(none_out, "rb").read()
    assert want == spec.genotyped_vcf(text, call, gq, 2, "NA12")             # "none" is what it was
    assert write_genotyped_vcf(plain_in, none_out, call, gq, 2, "NA12", compress="none") == n
    assert open(none_out, "rb").read() == want
    outs = {}
    for chunk_bytes in (1000, None):
        out = str(tmp_path / ("out%s.vcf.gz" % chunk_bytes))
        kw = {} if chunk_bytes is None else {"chunk_bytes": chunk_bytes}
        timings = {}
        assert write_genotyped_vcf(plain_in, out, call, gq, 2, "NA12", compress="bgzf", timings=timings, **kw) == n
        outs[chunk_bytes] = open(out, "rb").read()
        assert bgzf.is_bgzf(outs[chunk_bytes][:18]) and timings["deflate_ms"] > 0
        assert gzip.decompress(outs[chunk_bytes]) == want
        got = variant_arrays_from_file(out, inflate="device")
        ref = variant_arrays_from_file(none_out)
        assert len(got.positions) == n
        for k in ("positions", "chromosomes", "line_numbers", "is_snp"):
            assert np.array_equal(getattr(got, k), getattr(ref, k)), k
    assert outs[1000] == outs[None]                          # the pieces do not show in the file
    out = str(tmp_path / "bad.vcf.gz")
    with pytest.raises(ValueError, match="data lines"):
        write_genotyped_vcf(plain_in, out, call[:-1], gq[:-1], 2, chunk_bytes=1000, compress="bgzf")
    assert not os.path.exists(out)


def test_the_genotype_command_writes_bgzf_for_a_gz_name(tmp_path):
    c = case("v257_p2_b5")
    text = vcf_text(c.n_lines)
    files = {n: str(tmp_path / n) for n in ("v2n", "model", "counts.npy", "in.vcf", "out.vcf", "out.vcf.gz", "plain.gz")}
    VariantToNodesArrays(c.ref_nodes, c.var_nodes).to_file(files["v2n"])
    model_of(c).to_file(files["model"])
    np.save(files["counts.npy"], c.sample_rows[0])
    open(files["in.vcf"], "wb").write(text)
    common = ["genotype", "-V", files["v2n"] + ".npz", "-M", files["model"], "-c", files["counts.npy"], "-v", files["in.vcf"]]
    assert main(common + ["-o", files["out.vcf"], "--compress", "auto"]) == 0
    assert main(common + ["-o", files["out.vcf.gz"], "--compress", "auto", "--chunk-bytes", "700"]) == 0
    assert main(common + ["-o", files["plain.gz"]]) == 0     # the default stays plain text whatever the name
    want = open(files["out.vcf"], "rb").read()
    assert want.startswith(b"##") and open(files["plain.gz"], "rb").read() == want
    packed = open(files["out.vcf.gz"], "rb").read()
    assert bgzf.is_bgzf(packed[:18]) and gzip.decompress(packed) == want


def test_the_bgzf_command_and_map_on_its_result(tmp_path):
    k = 31
    index, _ = small_index(k, 0)
    index.to_file(str(tmp_path / "index"))
    plain = write(tmp_path, "reads.fa", text_cases.GOLDEN_CASES["stream"])
    packed = str(tmp_path / "reads.fa.gz")
    assert main(["bgzf", "-i", plain, "-o", packed, "--block-size", "700", "--chunk-bytes", "1999"]) == 0
    data = open(packed, "rb").read()
    assert bgzf.is_bgzf(data[:18]) and gzip.decompress(data) == text_cases.GOLDEN_CASES["stream"]
    assert data == deflate(text_cases.GOLDEN_CASES["stream"], 700) + bgzf.EOF_MEMBER
    base = ["map", "-i", str(tmp_path / "index"), "-k", str(k)]
    assert main(base + ["-f", plain, "-o", str(tmp_path / "a.npy")]) == 0
    assert main(base + ["-f", packed, "-o", str(tmp_path / "b.npy"), "--inflate", "device"]) == 0
    a, b = np.load(str(tmp_path / "a.npy")), np.load(str(tmp_path / "b.npy"))
    assert a.sum() > 0 and np.array_equal(a, b)
    missing = str(tmp_path / "no.gz")
    with pytest.raises(FileNotFoundError):
        main(["bgzf", "-i", str(tmp_path / "missing.fa"), "-o", missing])
    assert not os.path.exists(missing)
