"""The genotyper's spec (tests/spec_genotype.py) checked on the CPU: against a brute-force Poisson, the
fallback rule and the text writer on hand-written inputs, how stable the cases' calls are, and that the header, the binding
and the parser know the new names.  No device."""
import math
import os
import re

import numpy as np
import pytest

import spec_genotype as spec
from conftest import ROOT
from genotype_cases import CASE_NAMES, COVERAGES, case
from graph_kmer_index_amd import _lib
from graph_kmer_index_amd.command_line_interface import build_parser

NEW_SYMBOLS = ["gki_genotype_fit", "gki_genotype_scale", "gki_genotype_call", "gki_vcf_genotypes_count", "gki_vcf_genotypes_emit"]


def fitted(name):
    c = case(name)
    return c, spec.fit(c.histogram, c.count_sum, c.var_nodes, len(c.samples))


@pytest.mark.parametrize("name", ["v65_p2_b5", "v65_p3_b5", "v64_p8_b2"])
def test_the_calls_are_those_of_a_brute_force_poisson(name):
    """L leaves out -lgamma(x + 1), the same for every g: the argmax and the normalised values are those of the full
    Poisson log probabilities, summed with math.lgamma."""
    c, f = fitted(name)
    e, alpha, lam, P = 0.01, 1.0, 0.8, c.ploidy
    for row in c.sample_rows[[0, 2]]:
        o = spec.call(f, c.ref_nodes, c.var_nodes, row, lam, e, alpha)
        for v in np.flatnonzero(c.var_nodes != 0):
            x = [int(row[c.ref_nodes[v]]), int(row[c.var_nodes[v]])]
            full = []
            for g in range(P + 1):
                m = [lam * (f.mean[v][0][P - g] + e), lam * (f.mean[v][1][g] + e)]
                log_p = sum(x[a] * math.log(m[a]) - m[a] - math.lgamma(x[a] + 1) for a in range(2))
                full.append(log_p + math.log((int(f.n_alt[v][g]) + alpha) / (len(c.samples) + (P + 1) * alpha)))
            scale = max(spec.abs_terms(o, v, g) for g in range(P + 1)) + math.lgamma(max(x) + 1)
            assert np.allclose(np.array(full) - max(full), o.loglik[v], rtol=0, atol=1e-12 * scale)
            if sorted(full)[-1] - sorted(full)[-2] > 1e-9 * scale:
                assert int(np.argmax(full)) == o.call[v]


def test_the_fallback_rule_on_a_hand_written_table():
    # one kept line, ploidy 4, two bins; allele 0 populated at c = 1 and 3 (a tie at c = 2, gaps on either side), allele 1
    # populated at c = 4 only: the means fall by 1 a copy and are clamped at 0
    histogram = np.zeros((2, 2, 5, 2), dtype=np.uint32)
    count_sum = np.zeros((2, 2, 5), dtype=np.uint64)
    histogram[0, 0, 1], count_sum[0, 0, 1] = [1, 2], 30    # mean 10
    histogram[0, 0, 3], count_sum[0, 0, 3] = [0, 4], 7     # mean 1.75
    histogram[0, 1, 4], count_sum[0, 1, 4] = [3, 4], 17    # mean 17 / 7
    f = spec.fit(histogram, count_sum, [5, 0], 7)
    assert f.mean[0][0].tolist() == [9.0, 10.0, 11.0, 1.75, 2.75]
    assert f.mean[0][1].tolist() == [0.0, 0.0, 17 / 7 - 2, 17 / 7 - 1, 17 / 7]
    assert f.n_alt[0].tolist() == [0, 0, 0, 0, 7] and f.total == 54
    assert not f.mean[1].any() and not f.n_alt[1].any()    # the line that is not kept
    with pytest.raises(ValueError, match="data line 0.*hold 8"):
        spec.fit(histogram, count_sum, [5, 0], 8)
    with pytest.raises(ValueError, match="data line 1.*no populated"):
        spec.fit(histogram, count_sum, [5, 6], 7)
    with pytest.raises(ValueError, match="model has 2"):
        spec.fit(histogram, count_sum, [5], 7)
    count_sum[:] = 0
    with pytest.raises(ValueError, match="total is 0"):
        spec.fit(histogram, count_sum, [5, 0], 7)


def test_scale_and_coverage():
    x = np.array([9, 1, 2, 3, 4], dtype=np.uint32)
    assert spec.scale(x, [1, 3, 3], [2, 0, 7]) == 1 + 2 + 3           # line 1 is not kept, node 7 lies beyond the row
    assert spec.coverage(6, 4, 48) == 0.5
    with pytest.raises(ValueError):
        spec.coverage(0, 4, 48)


def test_call_and_quality_on_a_hand_worked_line():
    f = spec.Fit()
    f.mean = np.array([[[0.0, 5.0, 10.0], [0.0, 5.0, 10.0]]])
    f.n_alt = np.array([[1, 1, 1]], dtype=np.uint32)
    f.n_individuals = 3
    o = spec.call(f, [1], [2], np.array([0, 5, 5], dtype=np.uint32), 1.0)
    assert o.call.tolist() == [1] and o.loglik[0][1] == 0.0 and o.loglik[0][0] < 0
    assert abs(o.loglik[0][0] - o.loglik[0][2]) < 1e-13    # the same terms in another order
    # the priors are equal; g = 1: both nodes at mean 5, g = 0 and 2: one node at mean 10, the other at 0
    het, hom = 2 * (5 * math.log(5.01) - 5.01), 5 * math.log(10.01) - 10.01 + 5 * math.log(0.01) - 0.01
    want_q = spec.PHRED * (het - hom)
    assert abs(float(o.q[0]) - want_q) < 1e-9 and o.gq.tolist() == [99]
    o = spec.call(f, [1], [0], np.array([0, 5, 5], dtype=np.uint32), 1.0)
    assert o.call.tolist() == [-1] and o.gq.tolist() == [0] and not o.loglik.any()
    for bad in ({"lam": 0.0}, {"lam": math.inf}, {"error": 0.0}, {"pseudo_count": -1.0}, {"lam": math.nan}):
        with pytest.raises(ValueError):
            spec.call(f, [1], [2], np.zeros(3, np.uint32), **{"lam": 1.0, **bad})


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_cases_calls_do_not_hang_on_rounding(name):
    """The GPU test accepts either call where the spec's best and second best lie within their tolerances, and a quality
    one off where q lies that close to an integer.  Evaluated here in float64 and in np.longdouble over every case, row and
    coverage (given and estimated): no call differs between the two and no kept line falls under either exception, so the
    GPU test compares every line exactly."""
    c = case(name)
    if c.n_lines == 0:
        return
    f = spec.fit(c.histogram, c.count_sum, c.var_nodes, len(c.samples))
    for r, row in enumerate(c.sample_rows):
        estimated = spec.coverage(spec.scale(row, c.ref_nodes, c.var_nodes), f.n_individuals, f.total)
        for lam in (COVERAGES[r], estimated):
            o = spec.call(f, c.ref_nodes, c.var_nodes, row, lam)
            wide = spec.call(f, c.ref_nodes, c.var_nodes, row, lam, dtype=np.longdouble)
            assert np.array_equal(o.call, wide.call) and np.array_equal(o.gq, wide.gq)
            assert excluded_lines(c, o) == ([], [])


def tolerance(o, v, g):
    return 2.0 ** -46 * (spec.abs_terms(o, v, g) + spec.abs_terms(o, v, int(o.call[v])))


def excluded_lines(c, o):
    """(lines whose call may go either way, lines whose quality may be one off) by the GPU test's two exceptions."""
    calls, qualities = [], []
    for v in np.flatnonzero(c.var_nodes != 0):
        best = int(o.call[v])
        second = max((g for g in range(c.ploidy + 1) if g != best), key=lambda g: o.L[v][g])
        tol = tolerance(o, v, second) + tolerance(o, v, best)
        if o.L[v][best] - o.L[v][second] <= tol:
            calls.append(int(v))
        q = float(o.q[v])
        if q < 99 + 4.343 * tol and abs(q - round(q)) <= 4.343 * tol:
            qualities.append(int(v))
    return calls, qualities


TEXT = (b"##fileformat=VCFv4.2\r\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"old\">\n##contig=<ID=1>\n"
        b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\ts2\n"
        b"1\t5\t.\tA\tC\t.\tPASS\tAF=0.5\tGT\t0|1\t1|1\n"
        b"\n \t \n"
        b"1\t9\trs1\tG\tGT\t30\t.\t.\r\n"
        b"#a comment between data lines\n"
        b"1\t12\t.\tT\tA\t.\t.\tX\t")


def test_the_writer_on_hand_written_lines():
    want = (b"##fileformat=VCFv4.2\n##contig=<ID=1>\n" + b"\n".join(spec.FORMAT_LINES) + b"\n"
            b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tNA1\n"
            b"1\t5\t.\tA\tC\t.\tPASS\tAF=0.5\tGT:GQ\t0/1:7\n"
            b"1\t9\trs1\tG\tGT\t30\t.\t.\tGT:GQ\t./.:.\n"
            b"1\t12\t.\tT\tA\t.\t.\tX\tGT:GQ\t1/1:99\n")
    assert spec.genotyped_vcf(TEXT, [1, -1, 2], [7, 55, 99], 2, "NA1") == want
    assert spec.data_lines_text(b"1\t2\t3\t4\t5\t6\t7\t8", [0], [10], 1) == b"1\t2\t3\t4\t5\t6\t7\t8\tGT:GQ\t0:10\n"
    assert spec.data_lines_text(b"1\t2\t3\t4\t5\t6\t7\t\n", [3], [0], 3) == b"1\t2\t3\t4\t5\t6\t7\t\tGT:GQ\t1/1/1:0\n"
    assert spec.header_text(b"", "s") == b"\n".join(spec.FORMAT_LINES) + b"\n" + spec.COLUMNS + b"\tFORMAT\ts\n"
    assert spec.data_lines_text(b"", [], [], 2) == b""
    with pytest.raises(ValueError, match="data line 1: fewer than eight"):
        spec.data_lines_text(b"1\t2\t3\t4\t5\t6\t7\t8\n1\t2\t3\t4\t5\t6\t7\n1\t2\n", [0, 0, 0], [0, 0, 0], 2)
    with pytest.raises(ValueError, match="data line 0: a call outside"):
        spec.data_lines_text(b"1\t2\t3\t4\t5\t6\t7\t8\n1\t2\n", [3, 0], [0, 0], 2)
    with pytest.raises(ValueError, match="data line 0: a call outside"):
        spec.data_lines_text(b"1\t2\t3\t4\t5\t6\t7\t8\n", [-2], [0], 2)
    with pytest.raises(ValueError, match="1 data lines"):
        spec.data_lines_text(b"1\t2\t3\t4\t5\t6\t7\t8\n", [0, 0], [0, 0], 2)
    with pytest.raises(ValueError, match="more than 1"):
        spec.data_lines_text(b"1\t2\t3\t4\t5\t6\t7\t8\n" * 2, [0], [0], 2)


def test_the_products_header_is_the_specs(tmp_path):
    from graph_kmer_index_amd.genotyper import header_text
    for i, text in enumerate([TEXT, b"", b"##a=b\n", b"1\t2\t3\t4\t5\t6\t7\t8\n##late=1\n", b"#CHROM\tPOS\tID\n1\t2\n"]):
        name = str(tmp_path / ("in%d.vcf" % i))
        open(name, "wb").write(text)
        assert header_text(name, "who") == spec.header_text(text, "who"), i


def test_the_five_symbols_are_declared_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gki.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert _lib.SYMBOLS[name][1][-1] == _lib.C.POINTER(_lib.C.c_float), name      # the trailing kernel_ms


def test_the_parser_accepts_genotype():
    args = build_parser().parse_args(["genotype", "-V", "v2n", "-M", "model", "-c", "counts.npy", "-v", "in.vcf.gz", "-o",
                                      "out.vcf", "-s", "NA1", "--coverage", "0.7", "--error", "0.02", "--pseudo-count", "2",
                                      "-L", "ll"])
    assert (args.variant_to_nodes, args.model, args.counts, args.vcf, args.out_file_name) == ("v2n", "model", "counts.npy", "in.vcf.gz", "out.vcf")
    assert (args.sample_name, args.coverage, args.error, args.pseudo_count, args.loglik) == ("NA1", 0.7, 0.02, 2.0, "ll")
    args = build_parser().parse_args(["genotype", "-V", "a", "-M", "b", "-c", "c", "-v", "d", "-o", "e"])
    assert (args.sample_name, args.coverage, args.error, args.pseudo_count, args.loglik) == ("sample", None, 0.01, 1.0, None)
    assert args.func.__name__ == "genotype"
