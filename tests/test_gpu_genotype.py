"""GPU tests of the genotyper and of the genotyped VCF's text against the plain-Python spec
(tests/spec_genotype.py) on the cases of tests/genotype_cases.py.

The fitted means, n_alt, the sums S and T and the estimated coverage are compared exactly, doubles bit by bit.  A log
likelihood may differ from the spec's by 2^-46 (abs_terms(v, g) + abs_terms(v, best)): a dozen correctly rounded operations
and a log within 1 ulp, against the magnitude of the terms, with about a factor of 8 to spare.  A call is compared wherever
the spec's best and second best differ by more than their two tolerances, a quality unless the spec's q lies within 4.343
tolerances of an integer, where one off is accepted.  tests/test_genotype_spec.py shows on the CPU (float64 against
np.longdouble) that no kept line of any case falls under either exception; here no case may leave more than 1 % of its kept
lines to them."""
import ctypes as C
import functools

import numpy as np
import pytest

import bgzf_cases
import spec_genotype as spec
from genotype_cases import CASE_NAMES, COVERAGES, case
from graph_kmer_index_amd import _lib
from graph_kmer_index_amd.genotyper import Genotyper, Genotypes, genotyped_lines_on_device, write_genotyped_vcf
from graph_kmer_index_amd.haplotype_paths import NodeCountModel
from graph_kmer_index_amd.unique_variant_kmers import VariantToNodesArrays

pytestmark = pytest.mark.gpu
TILE = 4096


def model_of(c, histogram=None, count_sum=None, samples=None):
    return NodeCountModel(c.histogram if histogram is None else histogram, c.count_sum if count_sum is None else count_sum,
                          31, c.ploidy, c.n_bins, c.samples if samples is None else samples)


def genotyper_of(c, **kw):
    return Genotyper(model_of(c), VariantToNodesArrays(c.ref_nodes, c.var_nodes), **kw)


@functools.lru_cache(maxsize=None)
def spec_fit(name):
    c = case(name)
    return spec.fit(c.histogram, c.count_sum, c.var_nodes, len(c.samples))


@functools.lru_cache(maxsize=None)
def spec_calls(name, row, estimated):
    """The spec's calls of one sample row, computed once and shared; read only."""
    c, f = case(name), spec_fit(name)
    x = c.sample_rows[row]
    lam = spec.coverage(spec.scale(x, c.ref_nodes, c.var_nodes), f.n_individuals, f.total) if estimated else COVERAGES[row]
    return lam, spec.call(f, c.ref_nodes, c.var_nodes, x, lam)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_calls(c, got_call, got_gq, got_loglik, want, what):
    """One row against the spec by the module docstring's rules; returns the largest |error| / tolerance of a log likelihood."""
    kept = np.flatnonzero(c.var_nodes != 0)
    assert np.array_equal(got_call[c.var_nodes == 0], want.call[c.var_nodes == 0])          # -1
    assert not got_gq[c.var_nodes == 0].any()
    excluded, worst = 0, 0.0
    for v in kept:
        best = int(want.call[v])
        tol = [2.0 ** -46 * (spec.abs_terms(want, v, g) + spec.abs_terms(want, v, best)) for g in range(c.ploidy + 1)]
        if got_loglik is not None:
            for g in range(c.ploidy + 1):
                err = abs(float(got_loglik[v][g]) - float(want.loglik[v][g]))
                worst = max(worst, err / tol[g])
                assert err <= tol[g], (what, v, g, got_loglik[v][g], want.loglik[v][g], tol[g])
        second = max((g for g in range(c.ploidy + 1) if g != best), key=lambda g: want.L[v][g])
        gap_tol = tol[second] + tol[best]
        q = float(want.q[v])
        if want.L[v][best] - want.L[v][second] <= gap_tol:
            excluded += 1
            assert got_call[v] in (best, second), (what, v)
        elif q < 99 + 4.343 * gap_tol and abs(q - round(q)) <= 4.343 * gap_tol:
            excluded += 1
            assert got_call[v] == best and abs(int(got_gq[v]) - int(want.gq[v])) <= 1, (what, v)
        else:
            assert got_call[v] == best and got_gq[v] == want.gq[v], (what, v, got_call[v], got_gq[v], best, want.gq[v], q)
    assert excluded * 100 <= len(kept), (what, excluded, len(kept))
    return worst


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fit_scale_and_call_equal_the_spec(name):
    c = case(name)
    if c.n_lines == 0:
        with pytest.raises(ValueError, match="total is 0"):
            genotyper_of(c)
        return
    f = spec_fit(name)
    worst = 0.0
    with genotyper_of(c) as g:
        assert g.mean.shape == (c.n_lines, 2, c.ploidy + 1) and g.n_alt.shape == (c.n_lines, c.ploidy + 1)
        assert np.array_equal(bits(g.mean), bits(f.mean)) and np.array_equal(g.n_alt, f.n_alt) and g.n_alt.dtype == np.uint32
        assert g.total == f.total
        with _lib.DeviceScope() as s:
            sums = g.scale(s.on_device(c.sample_rows.reshape(-1), np.uint32), 3, c.n_nodes)
        assert sums.tolist() == [spec.scale(x, c.ref_nodes, c.var_nodes) for x in c.sample_rows]
        # a batch of three rows at given coverages, with the log likelihoods
        batch = g.genotype(c.sample_rows, COVERAGES, loglik=True)
        assert batch.call.shape == batch.gq.shape == (3, c.n_lines) and batch.loglik.shape == (3, c.n_lines, c.ploidy + 1)
        assert (batch.call.dtype, batch.gq.dtype, batch.loglik.dtype) == (np.int8, np.uint8, np.float64)
        assert batch.coverage.tolist() == list(COVERAGES)
        assert not batch.loglik[:, c.var_nodes == 0].any()
        for r in range(3):
            worst = max(worst, assert_calls(c, batch.call[r], batch.gq[r], batch.loglik[r], spec_calls(name, r, False)[1], (name, r)))
        # the same batch at estimated coverages, without them
        estimated = g.genotype(c.sample_rows)
        assert estimated.loglik is None
        for r in range(3):
            lam, want = spec_calls(name, r, True)
            assert bits(estimated.coverage[r]) == bits(lam)
            assert_calls(c, estimated.call[r], estimated.gq[r], None, want, (name, r, "estimated"))
        # one row alone: no leading axis, equal to its row of the batch
        one = g.genotype(c.sample_rows[0], loglik=True)
        assert one.call.shape == (c.n_lines,) and one.loglik.shape == (c.n_lines, c.ploidy + 1) and one.coverage.shape == (1,)
        assert np.array_equal(one.call, estimated.call[0]) and np.array_equal(one.gq, estimated.gq[0])
        assert_calls(c, one.call, one.gq, one.loglik, spec_calls(name, 0, True)[1], (name, 0, "alone"))
        assert one.loglik.max(axis=1).tolist() == [0.0] * c.n_lines       # the best genotype's is exactly 0
    print("%s: largest |error| / tolerance of a log likelihood %.3f" % (name, worst))


def test_genotypes_files(tmp_path):
    c = case("v65_p2_b5")
    with genotyper_of(c) as g:
        for loglik in (True, False):
            got = g.genotype(c.sample_rows[:2], 1.5, loglik=loglik)
            got.to_file(str(tmp_path / "calls"))
            back = Genotypes.from_file(str(tmp_path / "calls"))
            assert np.array_equal(back.call, got.call) and np.array_equal(back.gq, got.gq)
            assert back.coverage.tolist() == [1.5, 1.5] and (back.loglik is None) == (not loglik)
            if loglik:
                assert np.array_equal(back.loglik, got.loglik)
    with pytest.raises(ValueError, match="closed"):
        g.genotype(c.sample_rows[0])


def test_every_value_error():
    c = case("v65_p2_b5")
    v2n = VariantToNodesArrays(c.ref_nodes, c.var_nodes)
    kept = np.flatnonzero(c.var_nodes != 0)
    # fit, kind 1: a kept line without any populated entry of an allele; the lowest line is named
    histogram = c.histogram.copy()
    histogram[kept[9], 1] = 0
    histogram[kept[20]] = 0
    with pytest.raises(ValueError, match="data line %d: an allele has no populated" % kept[9]):
        Genotyper(model_of(c, histogram), v2n)
    # fit, kind 2: an allele's entries do not hold N individuals
    histogram = c.histogram.copy()
    histogram[kept[30], 0, 0, 0] += 1
    with pytest.raises(ValueError, match="data line %d: .*do not hold" % kept[30]):
        Genotyper(model_of(c, histogram), v2n)
    with pytest.raises(ValueError, match="do not hold"):
        Genotyper(model_of(c, samples=c.samples + [6]), v2n)
    # another V
    with pytest.raises(ValueError, match="data lines"):
        Genotyper(model_of(c), VariantToNodesArrays(c.ref_nodes[:-1], c.var_nodes[:-1]))
    # T == 0
    with pytest.raises(ValueError, match="total is 0"):
        Genotyper(model_of(c, count_sum=np.zeros_like(c.count_sum)), v2n)
    for kw in ({"error": 0.0}, {"error": float("inf")}, {"pseudo_count": 0.0}, {"pseudo_count": float("nan")}):
        with pytest.raises(ValueError, match="positive and finite"):
            Genotyper(model_of(c), v2n, **kw)
    with Genotyper(model_of(c), v2n) as g:
        for coverage in (0.0, -1.0, float("inf"), float("nan"), [1.0, 0.0]):
            with pytest.raises(ValueError, match="positive and finite"):
                g.genotype(c.sample_rows[:2], coverage)
        rows = c.sample_rows[:2].copy()
        rows[1] = 0
        rows[1][0] = 5                                     # node 0 is no line's
        with pytest.raises(ValueError, match="row 1 has no count"):
            g.genotype(rows)
        assert g.genotype(rows, 1.0).call.shape == (2, c.n_lines)         # S is not needed when the coverage is given
    lib = _lib.load()
    assert lib.gki_genotype_call(None, None, None, None, 4, 9, 3, None, 1, 8, None, 0.01, 1.0, None, None, None, None) == 2
    assert lib.gki_genotype_fit(None, None, None, 4, 2, 1, 3, None, None, None, None, None, None) == 2


def test_recovery_of_the_model_individuals_own_genotypes():
    """On haplotype_count_model_cases.model_case(): every diploid individual's own summed row, genotyped at coverage 1.
    The device's calls are the spec's, and the spec's calls agree with the individual's true alt copy number at least as
    often as "always the line's most frequent genotype" does (computed here on the CPU from the spec's output)."""
    from haplotype_count_model_cases import model_case
    from graph_kmer_index_amd import CollisionFreeKmerIndex, DenseKmerFinder
    from graph_kmer_index_amd.haplotype_paths import HaplotypePaths
    from graph_kmer_index_amd.vcf_files import HaplotypeMatrix
    c, k, ploidy = model_case(), 31, 2
    finder = DenseKmerFinder(c.graph, k, max_variant_nodes=4)
    finder.find()
    index = CollisionFreeKmerIndex.from_flat_kmers(finder.get_flat_kmers(v="1"), modulo=2_000_003)
    v2n = VariantToNodesArrays(c.ref_nodes, c.var_nodes)
    n_individuals = c.n_slots // ploidy
    with HaplotypePaths(c.graph, v2n, HaplotypeMatrix(c.codes, np.ones(len(c.codes), np.uint8), n_individuals, ploidy)) as paths:
        model = paths.node_count_model(index, k, None, 5, c.graph.n_nodes)
        slots = paths.node_counts_by_difference(list(range(c.n_slots)), index, k, c.graph.n_nodes)
    rows = np.stack([slots[i * ploidy:(i + 1) * ploidy].sum(axis=0, dtype=np.uint32) for i in range(n_individuals)])
    f = spec.fit(model.histogram, model.count_sum, c.var_nodes, n_individuals)
    with Genotyper(model, v2n) as g:
        got = g.genotype(rows, 1.0)
    truth = (c.codes == 1).reshape(len(c.codes), n_individuals, ploidy).sum(axis=2)          # [V][individual]
    kept = np.flatnonzero(np.asarray(c.var_nodes) != 0)
    most_frequent = np.array([np.bincount(truth[v], minlength=ploidy + 1).argmax() for v in range(len(truth))])
    right = baseline = 0
    for i in range(n_individuals):
        want = spec.call(f, c.ref_nodes, c.var_nodes, rows[i], 1.0)
        assert np.array_equal(got.call[i], want.call), i
        right += int(np.count_nonzero(want.call[kept] == truth[kept, i]))
        baseline += int(np.count_nonzero(most_frequent[kept] == truth[kept, i]))
    assert right >= baseline, (right, baseline)


# ------------------------------------------------------------------------------------------------ the text

def lines_on_device(text, call, gq, ploidy):
    """The genotyped data lines of `text` as one piece, as bytes."""
    call, gq = np.asarray(call, dtype=np.int8), np.asarray(gq, dtype=np.uint8)
    with _lib.DeviceScope() as s:
        d_text = s.on_device(np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, np.uint8), np.uint8)
        d_call = s.on_device(call if len(call) else np.zeros(1, np.int8), np.int8)
        d_gq = s.on_device(gq if len(gq) else np.zeros(1, np.uint8), np.uint8)
        out, n_out, n_data = genotyped_lines_on_device(s, d_text, len(text), d_call, d_gq, 0, len(call), ploidy)
        return (out.to_host(n_out).tobytes() if n_out else b""), n_data


def site(i, info=b".", more=b""):
    return b"1\t%d\trs%d\tA\tC\t.\tPASS\t%s%s" % (100 + i, i, info, more)


def calls_for(n, ploidy, seed):
    rng = np.random.default_rng([n, ploidy, seed])
    call = rng.integers(-1, ploidy + 1, size=n).astype(np.int8)
    gq = rng.choice(np.array([0, 5, 9, 10, 42, 98, 99], dtype=np.uint8), size=n)
    return call, gq


@pytest.mark.parametrize("ploidy", [1, 2, 3])
def test_the_lines_equal_the_spec(ploidy):
    header = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\n"
    many = [site(i) if i % 3 else site(i, b"AF=0.25", b"\tGT\t0|1") for i in range(700)]    # more than a tile of output
    texts = {
        "eight fields, a line end at the file's end": header + b"\n".join(many[:5]) + b"\n",
        "eight fields, none at the file's end": header + b"\n".join(many[:5]),
        "nine and more fields": b"\n".join(site(i, b"X", b"\tGT:DP\t0/1:3\t1/1:4") for i in range(70)) + b"\n",
        "CRLF": header.replace(b"\n", b"\r\n") + b"\r\n".join(many[:40]) + b"\r\n",
        "blank and comment lines between": b"\n \t\n" + many[0] + b"\n\n#x\n" + many[1] + b"\n   \n",
        "more than a tile": b"\n".join(many) + b"\n",
        "a line longer than a tile": many[0] + b"\n" + site(1, b"L=" + b"ACGT" * 2500) + b"\n" + many[2] + b"\n",
        "a long line whose ninth field is long too": site(1, b"L=" + b"AC" * 3000, b"\t" + b"x" * 9000) + b"\n" + many[2] + b"\n",
        "an empty eighth field": b"1\t2\t3\t4\t5\t6\t7\t\n" + b"1\t2\t3\t4\t5\t6\t7\t\tGT\n",
    }
    for what, text in texts.items():
        n = sum(1 for _, is_data in spec.lines_of(text) if is_data)
        call, gq = calls_for(n, ploidy, len(text))
        got, n_data = lines_on_device(text, call, gq, ploidy)
        assert n_data == n and got == spec.data_lines_text(text, call, gq, ploidy), what
    # one- and two-digit qualities, 99, a no-call and every call, by hand
    text = b"\n".join(site(i) for i in range(ploidy + 4)) + b"\n"
    call, gq = [-1] + list(range(ploidy + 1)) + [0, 0], [50] + [7] * (ploidy + 1) + [10, 99]
    got, _ = lines_on_device(text, call, gq, ploidy)
    assert got == spec.data_lines_text(text, call, gq, ploidy)
    assert got.split(b"\n")[0].endswith(b"GT:GQ\t" + b"/".join([b"."] * ploidy) + b":.") and got.endswith(b":99\n")


def test_line_ends_at_every_offset_across_a_tile_boundary():
    """The second line's output ends 8 bytes in front of the first tile's end, ..., 8 bytes behind it: its last lane's 16
    bytes begin at every offset of the line's suffix and of the next line's fields."""
    first, third = site(0), site(2)
    call, gq = [1, 2, 0], [8, 31, 99]
    suffix = len(b"\tGT:GQ\t0/1:8\n")                      # of the first line; the second's is one longer
    for shift in range(-8, 9):
        fill = TILE + shift - (len(first) + suffix) - (len(site(1, b"")) + suffix + 1)
        text = b"\n".join([first, site(1, b"N" * fill), third]) + b"\n"
        want = spec.data_lines_text(text, call, gq, 2)
        assert want.index(b"\n", len(first) + suffix) + 1 == TILE + shift
        assert lines_on_device(text, call, gq, 2)[0] == want, shift


def test_header_only_and_empty_inputs_and_files(tmp_path):
    assert lines_on_device(b"", [], [], 2) == (b"", 0)
    assert lines_on_device(b"##a=b\n#CHROM\tPOS\n\n", [], [], 2) == (b"", 0)
    for i, text in enumerate([b"", b"##a=b\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\ts\n"]):
        name, out = str(tmp_path / ("in%d.vcf" % i)), str(tmp_path / ("out%d.vcf" % i))
        open(name, "wb").write(text)
        assert write_genotyped_vcf(name, out, [], [], 2, "who") == 0
        assert open(out, "rb").read() == spec.genotyped_vcf(text, [], [], 2, "who")


def vcf_text(n):
    head = (b"##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"x\">\n##contig=<ID=1>\n"
            b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\n")
    return head + b"".join(site(i, b"AF=0.5" if i % 4 else b".", b"\tGT\t0|1\t1|1") + b"\n" for i in range(n))


def test_files_in_small_pieces_and_bgzf(tmp_path):
    n = 333
    text = vcf_text(n)
    call, gq = calls_for(n, 2, 5)
    want = spec.genotyped_vcf(text, call, gq, 2, "NA12")
    plain, gz, out = str(tmp_path / "in.vcf"), str(tmp_path / "in.vcf.gz"), str(tmp_path / "out.vcf")
    open(plain, "wb").write(text)
    cuts = list(range(0, len(text), 5000)) + [len(text)]
    open(gz, "wb").write(bgzf_cases.file_bytes([bgzf_cases.member(text[a:b]) for a, b in zip(cuts[:-1], cuts[1:])] +
                                               [bgzf_cases.member(b"")]))
    # pieces of about 1000 bytes begin at data lines that are no multiples of 64
    firsts = []
    timings = {}
    assert write_genotyped_vcf(plain, out, call, gq, 2, "NA12", chunk_bytes=1000, timings=timings) == n
    assert open(out, "rb").read() == want and timings["lengths_ms"] > 0
    from graph_kmer_index_amd.text_files import iter_line_chunks
    with open(plain, "rb") as f:
        at = 0
        for piece in iter_line_chunks(f, 1000):
            firsts.append(at)
            at += sum(1 for _, is_data in spec.lines_of(piece) if is_data)
    assert len(firsts) > 10 and any(x % 64 for x in firsts)
    assert write_genotyped_vcf(gz, out, call, gq, 2, "NA12", chunk_bytes=6000, inflate="device") == n
    assert open(out, "rb").read() == want
    assert write_genotyped_vcf(gz, out, call, gq, 2, "NA12", inflate="host") == n
    assert open(out, "rb").read() == want
    # the file's data lines are not V: one call too few, one too many; the output is removed
    import os
    for calls in (call[:-1], np.append(call, 0)):
        with pytest.raises(ValueError, match="data lines"):
            write_genotyped_vcf(plain, out, calls, np.zeros(len(calls), np.uint8), 2, chunk_bytes=1000)
        assert not os.path.exists(out)


def test_both_fault_kinds_are_named_by_line(tmp_path):
    lines = [site(i) for i in range(200)]
    lines[150] = b"1\t250\t.\tA\tC\t.\tPASS"               # seven fields
    lines[70] = b"1\t170"
    text = b"\n".join(lines) + b"\n"
    call, gq = np.zeros(200, np.int8), np.zeros(200, np.uint8)
    with pytest.raises(ValueError, match="data line 70: fewer than eight fields"):
        lines_on_device(text, call, gq, 2)
    call[60], call[90] = 3, -2
    with pytest.raises(ValueError, match="data line 60: a call outside"):
        lines_on_device(text, call, gq, 2)
    call[60] = 2
    with pytest.raises(ValueError, match="data line 70: fewer than eight fields"):
        lines_on_device(text, call, gq, 2)
    name, out = str(tmp_path / "in.vcf"), str(tmp_path / "out.vcf")
    open(name, "wb").write(text)
    with pytest.raises(ValueError, match="data line 70: fewer than eight fields"):      # numbered in the file, not the piece
        write_genotyped_vcf(name, out, call, gq, 2, chunk_bytes=500)


def test_the_emit_call_refuses_a_fault_and_a_small_capacity_and_writes_nothing():
    lib = _lib.load()
    text = b"\n".join(site(i) for i in range(100)) + b"\n"
    call, gq = calls_for(100, 2, 1)
    want = spec.data_lines_text(text, call, gq, 2)
    with _lib.DeviceScope() as s:
        d_text = s.on_device(np.frombuffer(text, dtype=np.uint8), np.uint8)
        d_call, d_gq = s.on_device(call, np.int8), s.on_device(gq, np.uint8)
        d_bad = s.on_device(np.where(np.arange(100) == 40, 5, call), np.int8)
        out = s.on_device(np.full(len(want) + 64, 0xAA, dtype=np.uint8), np.uint8)
        n_out = C.c_int64(-1)
        args = (d_text.ptr, len(text), d_call.ptr, d_gq.ptr, 100, 2, out.ptr)
        assert lib.gki_vcf_genotypes_emit(*args, len(want) - 1, C.byref(n_out), None) == 2
        assert b"needs %d bytes" % len(want) in lib.gki_last_error() and n_out.value == 0
        assert lib.gki_vcf_genotypes_emit(d_text.ptr, len(text), d_bad.ptr, d_gq.ptr, 100, 2, out.ptr, out.n, C.byref(n_out), None) == 2
        assert b"data line 40" in lib.gki_last_error() and n_out.value == 0
        assert lib.gki_vcf_genotypes_emit(d_text.ptr, len(text), d_call.ptr, d_gq.ptr, 99, 2, out.ptr, out.n, C.byref(n_out), None) == 2
        assert lib.gki_vcf_genotypes_emit(d_text.ptr, len(text), d_call.ptr, d_gq.ptr, 100, 0, out.ptr, out.n, C.byref(n_out), None) == 2
        assert lib.gki_vcf_genotypes_emit(d_text.ptr, len(text), d_call.ptr, d_gq.ptr, 100, 2, C.c_void_p(out.ptr.value + 4), out.n - 4, C.byref(n_out), None) == 2
        assert not (out.to_host() != 0xAA).any()           # nothing was written by any of them
        assert lib.gki_vcf_genotypes_emit(*args, len(want), C.byref(n_out), None) == 0
        got = out.to_host()
        assert n_out.value == len(want) and got[:len(want)].tobytes() == want and not (got[len(want):] != 0xAA).any()


def test_the_genotype_command_from_files_to_a_vcf(tmp_path):
    from graph_kmer_index_amd.command_line_interface import main
    c = case("v257_p2_b5")
    text = vcf_text(c.n_lines)
    files = {n: str(tmp_path / n) for n in ("v2n", "model", "counts.npy", "in.vcf", "out.vcf", "ll")}
    VariantToNodesArrays(c.ref_nodes, c.var_nodes).to_file(files["v2n"])
    model_of(c).to_file(files["model"])
    np.save(files["counts.npy"], c.sample_rows[0])
    open(files["in.vcf"], "wb").write(text)
    common = ["genotype", "-V", files["v2n"] + ".npz", "-M", files["model"], "-c", files["counts.npy"], "-v", files["in.vcf"],
              "-o", files["out.vcf"]]
    assert main(common + ["-s", "NA7", "-L", files["ll"]]) == 0
    lam, want = spec_calls("v257_p2_b5", 0, True)
    assert open(files["out.vcf"], "rb").read() == spec.genotyped_vcf(text, want.call, want.gq, 2, "NA7")
    assert np.load(files["ll"] + ".npy").shape == (c.n_lines, 3)
    assert main(common + ["--coverage", str(COVERAGES[0]), "--chunk-bytes", "700"]) == 0
    want = spec_calls("v257_p2_b5", 0, False)[1]
    assert open(files["out.vcf"], "rb").read() == spec.genotyped_vcf(text, want.call, want.gq, 2, "sample")
