"""The haplotype matrix on the device (vcf_files.py, csrc/gki_vcf_gt.hip) against the plain-Python rules of
tests/spec_haplotype_matrix.py: codes, phased and names of every named case, byte for byte, in memory, from a device
buffer and from plain, BGZF and gzip files cut into pieces; the refused inputs with their line and kind on the same
routes; the C ABI's output buffers between guard bytes; the allele-frequency kernel of the same walk as a cross-check; the
bit planes at every tile edge and past 2^31 bytes; and the command line."""
import ctypes as C
import gzip

import numpy as np
import pytest

import spec_haplotype_matrix as spec
from haplotype_matrix_cases import ERROR_CASES, GOOD_CASES, GUARD_TEXT, header_of
from vcf_af_cases import gt_line, text_of

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xAA
_SPEC = {}


def spec_of(name):
    if name not in _SPEC:
        _SPEC[name] = spec.haplotype_matrix(**GOOD_CASES[name])
    return _SPEC[name]


def assert_equals_spec(got, want):
    codes, phased, n_samples, names = want
    assert got.codes.dtype == np.uint8 and got.codes.shape == codes.shape and np.array_equal(got.codes, codes)
    assert got.phased.dtype == np.uint8 and np.array_equal(got.phased, phased)
    assert got.n_samples == n_samples and got.sample_names == names


def write_encodings(tmp_path, text):
    from graph_kmer_index_amd import bgzf
    paths = {"plain": str(tmp_path / "v.vcf"), "bgzf": str(tmp_path / "v_bgzf.vcf.gz"), "gzip": str(tmp_path / "v_gzip.vcf.gz")}
    with open(paths["plain"], "wb") as f:
        f.write(text)
    bgzf.write_bgzf(paths["bgzf"], text, block_size=777)                # lines span members
    with open(paths["gzip"], "wb") as f:
        f.write(gzip.compress(text))
    return paths


def routes(case, paths):
    """Every way the text reaches the kernel, as calls: in memory, whole files, and pieces of 64 bytes and of one line."""
    from graph_kmer_index_amd.vcf_files import haplotype_matrix_from_file, haplotype_matrix_on_device
    kw = {"ploidy": case["ploidy"], "n_samples": case["n_samples"]}
    calls = [lambda: haplotype_matrix_on_device(case["text"], **kw), lambda: haplotype_matrix_from_file(paths["plain"], **kw)]
    for encoding in ("plain", "bgzf", "gzip"):
        for chunk_bytes in (64, 1):
            calls.append(lambda e=encoding, c=chunk_bytes: haplotype_matrix_from_file(paths[e], chunk_bytes=c, **kw))
    return calls


@pytest.mark.parametrize("name", sorted(GOOD_CASES))
def test_case_equals_spec_on_every_route(name, tmp_path):
    from graph_kmer_index_amd import _lib
    from graph_kmer_index_amd.vcf_files import haplotype_matrix_on_device
    case = GOOD_CASES[name]
    for call in routes(case, write_encodings(tmp_path, case["text"])):
        assert_equals_spec(call(), spec_of(name))
    with _lib.DeviceScope() as s:
        d = s.on_device(np.frombuffer(case["text"], dtype=np.uint8), np.uint8)
        assert_equals_spec(haplotype_matrix_on_device(d, case["ploidy"], case["n_samples"]), spec_of(name))


@pytest.mark.parametrize("name", sorted(ERROR_CASES))
def test_error_case_names_the_lowest_line_on_every_route(name, tmp_path):
    from graph_kmer_index_amd.vcf_files import HaplotypeMatrixError
    case, at, kind = ERROR_CASES[name]
    for call in routes(case, write_encodings(tmp_path, case["text"])):
        with pytest.raises(ValueError) as e:
            call()
        assert isinstance(e.value, HaplotypeMatrixError) and (e.value.line, e.value.kind) == (at, kind)
        assert "data line %d:" % at in str(e.value)


def test_error_line_numbers_carry_across_pieces(tmp_path):
    from graph_kmer_index_amd import bgzf
    from graph_kmer_index_amd.vcf_files import HaplotypeMatrixError, haplotype_matrix_from_file
    good = [gt_line([b"0|1", b"1|1"], pos=i + 1) for i in range(100)]
    for bad, kind in ((gt_line([b"0|1", b"0|"]), 3), (gt_line([b"0|1"]), 4), (gt_line([b"0|1", b"0/1/1"]), 5)):
        text = text_of(good + [bad, good[0], bad], header=header_of(2))
        bgzf.write_bgzf(str(tmp_path / "v.vcf.gz"), text, block_size=500)
        with open(str(tmp_path / "v.vcf"), "wb") as f:
            f.write(text)
        for path in ("v.vcf", "v.vcf.gz"):
            with pytest.raises(HaplotypeMatrixError) as e:
                haplotype_matrix_from_file(str(tmp_path / path), chunk_bytes=64)
            assert (e.value.line, e.value.kind) == (100, kind)


def test_bad_arguments():
    from graph_kmer_index_amd import _lib
    from graph_kmer_index_amd.vcf_files import haplotype_matrix_on_device
    for ploidy in (0, 9):
        with pytest.raises(ValueError):
            haplotype_matrix_on_device(GOOD_CASES["s_from_the_header"]["text"], ploidy=ploidy)
    with pytest.raises(ValueError):
        haplotype_matrix_on_device(b"", n_samples=-1)
    lib = _lib.load()
    with _lib.DeviceScope() as s:
        d = s.array(64, np.uint8)
        none = C.c_void_p(None)
        for args in ((d.ptr, 8, 0, 1, 0, d.ptr, d.ptr), (d.ptr, 8, 0, 1, 9, d.ptr, d.ptr), (d.ptr, -1, 0, 1, 2, d.ptr, d.ptr),
                     (d.ptr, 8, 0, -1, 2, d.ptr, d.ptr), (none, 8, 0, 1, 2, d.ptr, d.ptr), (d.ptr, 8, 1, 1, 2, none, d.ptr),
                     (d.ptr, 8, 1, 1, 2, d.ptr, none)):
            assert lib.gki_vcf_haplotype_matrix(*args, None, None, None, None) == 2
        assert lib.gki_vcf_haplotype_matrix(none, 0, 0, 5, 2, none, none, None, None, None, None) == 0
        for args in ((d.ptr, -1, 1, d.ptr, d.ptr), (d.ptr, 1, -1, d.ptr, d.ptr), (none, 1, 1, d.ptr, d.ptr),
                     (d.ptr, 1, 1, none, d.ptr), (d.ptr, 1, 1, d.ptr, none)):
            assert lib.gki_haplotype_planes(*args, None) == 2
        assert lib.gki_haplotype_planes(none, 0, 7, none, none, None) == 0
        assert lib.gki_haplotype_planes(none, 7, 0, none, none, None) == 0


def guarded(scope, n):
    """n bytes on the device behind and in front of GUARD bytes, all FILL: (the whole buffer, a pointer to the n bytes)"""
    from graph_kmer_index_amd import _lib
    whole = scope.array(n + 2 * GUARD, np.uint8)
    _lib.check(_lib.load().gki_memset(whole.ptr, FILL, whole.n))
    return whole, C.c_void_p(whole.ptr.value + GUARD)


def inside(whole, n):
    """The n bytes between the guards, after checking that the guards still hold FILL."""
    h = whole.to_host()
    assert np.all(h[:GUARD] == FILL) and np.all(h[GUARD + n:] == FILL)
    return h[GUARD:GUARD + n]


@pytest.mark.parametrize("text,ploidy", [(GUARD_TEXT, 2), (GUARD_TEXT, 1), (GOOD_CASES["samples_300"]["text"], 2),
                                         (GOOD_CASES["gts_longer_than_a_window"]["text"], 3),
                                         (GOOD_CASES["mixed_file"]["text"], 2)])
def test_c_abi_writes_all_of_its_output_and_nothing_else(text, ploidy):
    from graph_kmer_index_amd import _lib
    codes, phased, n_samples, _, faults = spec.matrix_with_faults(text, ploidy)
    n_variants = len(phased)
    with _lib.DeviceScope() as s:
        d_text = s.on_device(np.frombuffer(text, dtype=np.uint8), np.uint8)
        d_codes, p_codes = guarded(s, codes.size)
        d_phased, p_phased = guarded(s, n_variants)
        found, bad, kind, ms = C.c_int64(0), C.c_int64(-1), C.c_int(0), C.c_float(0)
        _lib.check(_lib.load().gki_vcf_haplotype_matrix(d_text.ptr, d_text.n, n_variants, n_samples, ploidy, p_codes, p_phased,
                                                        C.byref(found), C.byref(bad), C.byref(kind), C.byref(ms)))
        assert found.value == n_variants and (bad.value, kind.value) == (faults[0] if faults else (-1, 0))
        assert np.array_equal(inside(d_codes, codes.size).reshape(codes.shape), codes)
        assert np.array_equal(inside(d_phased, n_variants), phased)
        assert _lib.load().gki_vcf_haplotype_matrix(d_text.ptr, d_text.n, n_variants + 1, n_samples, ploidy, p_codes, p_phased,
                                                    C.byref(found), None, None, None) == 2 and found.value == n_variants


@pytest.mark.parametrize("name", sorted(GOOD_CASES))
def test_allele_frequency_kernel_agrees_with_the_codes(name):
    from graph_kmer_index_amd.vcf_files import allele_frequencies_on_device, haplotype_matrix_on_device
    case = GOOD_CASES[name]
    matrix = haplotype_matrix_on_device(**{"buf" if k == "text" else k: v for k, v in case.items()})
    ref_af, alt_af, _ = allele_frequencies_on_device(case["text"], "genotypes")
    want = spec.frequencies_of(matrix.codes, spec.data_lines(case["text"]))
    assert np.array_equal(ref_af.view(np.uint64), want[0].view(np.uint64))
    assert np.array_equal(alt_af.view(np.uint64), want[1].view(np.uint64))


# ---------------------------------------------------------------------------------------------------- the bit planes

def T():
    from graph_kmer_index_amd.vcf_files import PLANES_TILE_SLOTS
    return PLANES_TILE_SLOTS


SLOTS = {"0": lambda t: 0, "1": lambda t: 1, "2": lambda t: 2, "T-1": lambda t: t - 1, "T": lambda t: t,
         "T+1": lambda t: t + 1, "2T+3": lambda t: 2 * t + 3}
_CODES = {}


def random_codes(n_variants, n_slots):
    """Bytes 0..3 and, one in sixteen, a byte outside them, which sets neither bit."""
    if (n_variants, n_slots) not in _CODES:
        rng = np.random.default_rng([n_variants, n_slots, 7])
        codes = rng.integers(0, 4, size=(n_variants, n_slots)).astype(np.uint8)
        other = rng.integers(4, 256, size=codes.shape).astype(np.uint8)
        _CODES[n_variants, n_slots] = np.where(rng.random(codes.shape) < 1 / 16, other, codes)
    return _CODES[n_variants, n_slots]


@pytest.mark.parametrize("n_variants", [0, 1, 63, 64, 65, 127, 128, 129])
@pytest.mark.parametrize("slots", sorted(SLOTS))
def test_planes_at_every_tile_edge(n_variants, slots):
    from graph_kmer_index_amd import _lib
    n_slots = SLOTS[slots](T())
    codes = random_codes(n_variants, n_slots)
    n_words = (n_variants + 63) // 64
    want = spec.planes_by_packbits(codes)
    with _lib.DeviceScope() as s:
        d_codes, p_codes = guarded(s, codes.size)
        if codes.size:
            _lib.check(_lib.load().gki_memcpy_h2d(p_codes, _lib.hptr(np.ascontiguousarray(codes)), codes.size))
        outs = [guarded(s, n_slots * n_words * 8) for _ in range(2)]
        _lib.check(_lib.load().gki_haplotype_planes(p_codes, n_variants, n_slots, outs[0][1], outs[1][1], None))
        for (whole, _), w in zip(outs, want):
            got = inside(whole, n_slots * n_words * 8).view(np.uint64).reshape(n_slots, n_words)
            assert np.array_equal(got, w)
            if n_variants % 64 and n_slots:                # the bits at and beyond V
                assert not np.any(got[:, -1] >> np.uint64(n_variants % 64))


def test_planes_method_equals_the_spec():
    from graph_kmer_index_amd.vcf_files import HaplotypeMatrix
    codes = random_codes(129, T() + 1) & 3
    m = HaplotypeMatrix(codes[:, :T()], np.ones(129, np.uint8), T() // 2, 2)
    for got, want in zip(m.planes(), spec.planes_by_packbits(m.codes)):
        assert got.dtype == np.uint64 and np.array_equal(got, want)
    small = HaplotypeMatrix(codes[:5, :6], np.ones(5, np.uint8), 3, 2)
    for got, want in zip(small.planes(), spec.planes(small.codes)):
        assert np.array_equal(got, want)


def test_planes_past_two_gib_of_codes():
    """H = 8, V = 2^28 + 65: row v lies at byte 8 v, so rows 2^28 - 1 and 2^28 lie either side of byte 2^31 -- an offset
    formed in 32 bits would wrap there.  The codes are filled on the device (a constant 1, then a few rows from the host):
    filling 2 GiB on the host and uploading them takes longer than the rest of the suite's plane tests together."""
    from graph_kmer_index_amd import _lib
    lib = _lib.load()
    n_slots, n_variants = 8, 2 ** 28 + 65
    n_words = (n_variants + 63) // 64
    changed = {0: [0, 3, 0, 0, 2, 0, 0, 0], 2 ** 28 - 1: [0, 0, 0, 0, 0, 0, 3, 0], 2 ** 28: [2, 0, 0, 3, 0, 0, 0, 0],
               2 ** 28 + 1: [0] * 8, n_variants - 1: [3, 0, 0, 0, 0, 0, 0, 200]}
    with _lib.DeviceScope() as s:
        d_codes = s.array(n_variants * n_slots, np.uint8)
        _lib.check(lib.gki_memset(d_codes.ptr, 1, d_codes.n))
        for v, row in changed.items():
            _lib.check(lib.gki_memcpy_h2d(C.c_void_p(d_codes.ptr.value + v * n_slots), _lib.hptr(np.array(row, np.uint8)), n_slots))
        planes = [s.array(n_slots * n_words, np.uint64) for _ in range(2)]
        for p in planes:
            _lib.check(lib.gki_memset(p.ptr, FILL, p.nbytes))
        _lib.check(lib.gki_haplotype_planes(d_codes.ptr, n_variants, n_slots, planes[0].ptr, planes[1].ptr, None))
        ref_bits, alt_bits = (p.to_host().reshape(n_slots, n_words) for p in planes)
    want_ref = np.zeros((n_slots, n_words), dtype=np.uint64)
    want_alt = np.full((n_slots, n_words), ~np.uint64(0), dtype=np.uint64)
    want_alt[:, -1] = np.uint64((1 << (n_variants % 64)) - 1)
    for v, row in changed.items():
        for h, code in enumerate(row):
            want_alt[h, v // 64] &= ~np.uint64(1 << (v % 64))
            if code == 0:
                want_ref[h, v // 64] |= np.uint64(1 << (v % 64))
    assert np.array_equal(ref_bits, want_ref) and np.array_equal(alt_bits, want_alt)


# ---------------------------------------------------------------------------------------------------- the command line

@pytest.mark.parametrize("encoding", ["plain", "bgzf"])
def test_command_line_writes_what_the_api_returns(tmp_path, encoding):
    from graph_kmer_index_amd.command_line_interface import build_parser
    from graph_kmer_index_amd.vcf_files import HaplotypeMatrix, haplotype_matrix_from_file
    text = GOOD_CASES["mixed_file"]["text"]
    path, out = write_encodings(tmp_path, text)[encoding], str(tmp_path / "haplotypes")
    args = build_parser().parse_args(["make_haplotype_matrix", "-v", path, "-o", out, "--planes", "True", "--chunk-bytes", "4096"])
    args.func(args)
    back, api = HaplotypeMatrix.from_file(out), haplotype_matrix_from_file(path)
    assert_equals_spec(back, spec_of("mixed_file"))
    assert_equals_spec(api, spec_of("mixed_file"))
    assert (back.ploidy, api.ploidy) == (2, 2)
    saved = np.load(out + ".npz")
    for key, plane in zip(("ref_bits", "alt_bits"), spec.planes_by_packbits(api.codes)):
        assert np.array_equal(saved[key], plane)
    out3 = str(tmp_path / "triploid")
    args = build_parser().parse_args(["make_haplotype_matrix", "-v", path, "-o", out3, "-p", "3", "-s", "37"])
    args.func(args)
    triploid = HaplotypeMatrix.from_file(out3)
    assert triploid.codes.shape == (api.n_variants, 111) and "ref_bits" not in np.load(out3 + ".npz").files
    assert np.array_equal(triploid.codes.reshape(-1, 37, 3)[:, :, :2].reshape(api.n_variants, -1), api.codes)
    assert np.all(triploid.codes.reshape(-1, 37, 3)[:, :, 2] == 3)
