"""The rules of DESIGN.md 4.21 (include/gki.h, "genotyping" and "genotyped VCF text") as plain Python / NumPy: the fit of
the count model, a sample's coverage, the calls, and the text of the genotyped VCF with its header.  No device and nothing
of graph_kmer_index_amd: this is the oracle of tests/test_gpu_genotype.py, itself checked in tests/test_genotype_spec.py."""
import math

import numpy as np

PHRED = 4.342944819032518                                  # 10 / ln 10
STRIP = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"                 # what str.strip() removes from ASCII text
FORMAT_LINES = [b'##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
                b'##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality, phred-scaled, at most 99">']
COLUMNS = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"


class Fit:
    """mean float64[V][2][P + 1], n_alt uint32[V][P + 1], total int, n_individuals int"""


def fit(histogram, count_sum, var_nodes, n_individuals):
    """The fit of a model (histogram uint32[V][2][P + 1][n_bins], count_sum uint64[V][2][P + 1]).  ValueError naming the
    lowest line at fault, and for a model total of 0."""
    histogram, count_sum = np.asarray(histogram), np.asarray(count_sum)
    v_lines, _, entries, _ = histogram.shape
    if len(var_nodes) != v_lines:
        raise ValueError("the model has %d data lines, variant-to-nodes has %d" % (v_lines, len(var_nodes)))
    n = histogram.sum(axis=3, dtype=np.int64)
    f = Fit()
    f.mean = np.zeros((v_lines, 2, entries), dtype=np.float64)
    f.n_alt = np.zeros((v_lines, entries), dtype=np.uint32)
    f.total, f.n_individuals = 0, int(n_individuals)
    for v in range(v_lines):
        if int(var_nodes[v]) == 0:
            continue
        populated = [[c for c in range(entries) if n[v][a][c] > 0] for a in range(2)]
        if not populated[0] or not populated[1]:
            raise ValueError("data line %d: an allele has no populated entry" % v)
        if int(n[v][0].sum()) != f.n_individuals or int(n[v][1].sum()) != f.n_individuals:
            raise ValueError("data line %d: an allele's entries do not hold %d individuals" % (v, f.n_individuals))
        for a in range(2):
            for c in range(entries):
                near = min(populated[a], key=lambda p: (abs(p - c), p))      # nearest, the lower at a tie
                mu = np.float64(count_sum[v][a][near]) / np.float64(n[v][a][near])
                if near != c:
                    mu = np.maximum(np.float64(0.0), mu + np.float64(c - near))
                f.mean[v][a][c] = mu
                f.total += int(count_sum[v][a][c])
        f.n_alt[v] = n[v][1]
    if f.total == 0:
        raise ValueError("the model total is 0")
    return f


def node_count(x, node):
    return int(x[node]) if node < len(x) else 0


def scale(x, ref_nodes, var_nodes):
    """S of one row: the counts of the kept lines' two nodes, summed."""
    return sum(node_count(x, int(r)) + node_count(x, int(a)) for r, a in zip(ref_nodes, var_nodes) if int(a) != 0)


def coverage(s, n_individuals, total):
    if s == 0:
        raise ValueError("the sample has no count on a kept line's node")
    return (float(s) * float(n_individuals)) / float(total)


class Calls:
    """call int8[V], gq uint8[V], loglik[V][P + 1]; and for the tests raw L[V][P + 1], q[V], log_m[V][2][P + 1] (by g),
    m[V][2][P + 1], log_prior[V][P + 1], x[V][2], all in the dtype asked for"""


def call(f, ref_nodes, var_nodes, x, lam, error=0.01, pseudo_count=1.0, dtype=np.float64):
    """The calls of one row x at coverage lam.  `dtype` np.longdouble evaluates the same statements more precisely."""
    t = dtype
    v_lines, entries = f.n_alt.shape
    ploidy = entries - 1
    if not (lam > 0 and math.isfinite(lam)):
        raise ValueError("the coverage must be positive and finite")
    if not (error > 0 and math.isfinite(error)) or not (pseudo_count > 0 and math.isfinite(pseudo_count)):
        raise ValueError("error and pseudo_count must be positive and finite")
    o = Calls()
    o.call = np.full(v_lines, -1, dtype=np.int8)
    o.gq = np.zeros(v_lines, dtype=np.uint8)
    o.loglik = np.zeros((v_lines, entries), dtype=t)
    o.L = np.zeros((v_lines, entries), dtype=t)
    o.q = np.zeros(v_lines, dtype=t)
    o.m = np.zeros((v_lines, 2, entries), dtype=t)
    o.log_m = np.zeros((v_lines, 2, entries), dtype=t)
    o.log_prior = np.zeros((v_lines, entries), dtype=t)
    o.x = np.zeros((v_lines, 2), dtype=t)
    prior_total = t(f.n_individuals) + t(ploidy + 1) * t(pseudo_count)
    for v in range(v_lines):
        if int(var_nodes[v]) == 0:
            continue
        x0, x1 = t(node_count(x, int(ref_nodes[v]))), t(node_count(x, int(var_nodes[v])))
        o.x[v] = x0, x1
        for g in range(entries):
            m0 = t(lam) * (t(f.mean[v][0][ploidy - g]) + t(error))
            m1 = t(lam) * (t(f.mean[v][1][g]) + t(error))
            prior = (t(f.n_alt[v][g]) + t(pseudo_count)) / prior_total
            o.m[v][0][g], o.m[v][1][g] = m0, m1
            o.log_m[v][0][g], o.log_m[v][1][g], o.log_prior[v][g] = np.log(m0), np.log(m1), np.log(prior)
            o.L[v][g] = x0 * np.log(m0) - m0 + x1 * np.log(m1) - m1 + np.log(prior)
        best = int(np.argmax(o.L[v]))                      # the lowest g at the maximum
        others = [o.L[v][g] for g in range(entries) if g != best]
        o.call[v] = best
        o.loglik[v] = o.L[v] - o.L[v][best]
        o.q[v] = t(PHRED) * (o.L[v][best] - max(others))
        o.gq[v] = 99 if o.q[v] >= 99 else int(np.floor(o.q[v]))
    return o


def abs_terms(o, v, g):
    """The magnitude the rounding errors of L[v][g] scale with: sum over a of x_a (|log m_a| + 1) + m_a, and |log pi| + 1."""
    return float(sum(o.x[v][a] * (abs(o.log_m[v][a][g]) + 1) + o.m[v][a][g] for a in range(2)) + abs(o.log_prior[v][g]) + 1)


# ------------------------------------------------------------------------------------------------ the text

def lines_of(text):
    """The lines of VCF text with every '\\r' at a line's end dropped, and whether each is a data line."""
    lines = bytes(text).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    out = []
    for line in lines:
        line = line.rstrip(b"\r")
        out.append((line, len(line) > 0 and not line.startswith(b"#") and len(line.strip(STRIP)) > 0))
    return out


def sample_column(c, quality, ploidy):
    if c < 0:
        return b"/".join([b"."] * ploidy) + b":."
    return b"/".join([b"0"] * (ploidy - c) + [b"1"] * c) + b":" + str(int(quality)).encode()


def data_lines_text(text, calls, gq, ploidy):
    """The genotyped data lines of `text` (one piece or the whole file).  ValueError naming the lowest data line at fault
    and its kind, and when the text's data lines are not len(calls)."""
    out, v = [], 0
    fault = None
    for line, is_data in lines_of(text):
        if not is_data:
            continue
        if v >= len(calls):
            raise ValueError("the text has more than %d data lines" % len(calls))
        fields = line.split(b"\t")
        c = int(calls[v])
        kind = 1 if len(fields) < 8 else 2 if not -1 <= c <= ploidy else 0
        if kind and fault is None:
            fault = (v, kind)
        if not kind:
            out.append(b"\t".join(fields[:8]) + b"\tGT:GQ\t" + sample_column(c, gq[v], ploidy) + b"\n")
        v += 1
    if fault is not None:
        raise ValueError("data line %d: %s" % (fault[0], "fewer than eight fields" if fault[1] == 1 else "a call outside -1 .. ploidy"))
    if v != len(calls):
        raise ValueError("the text has %d data lines, there are %d calls" % (v, len(calls)))
    return b"".join(out)


def header_text(text, sample_name="sample"):
    """The header: the lines in front of the first data line that begin with ##, but for FORMAT lines of GT and GQ; this
    package's two FORMAT lines; the #CHROM line cut to eight columns, the standard one when there is none, with the FORMAT
    and the sample's column."""
    kept, columns = [], None
    for line, is_data in lines_of(text):
        if is_data:
            break
        if line.startswith(b"##"):
            if not line.startswith((b"##FORMAT=<ID=GT,", b"##FORMAT=<ID=GQ,")):
                kept.append(line)
        elif line.startswith(b"#CHROM") and columns is None:
            columns = b"\t".join(line.split(b"\t")[:8])
    columns = (COLUMNS if columns is None else columns) + b"\tFORMAT\t" + sample_name.encode()
    return b"".join(l + b"\n" for l in kept + FORMAT_LINES + [columns])


def genotyped_vcf(text, calls, gq, ploidy, sample_name="sample"):
    return header_text(text, sample_name) + data_lines_text(text, calls, gq, ploidy)
