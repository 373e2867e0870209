"""Named inputs of the genotyper: count models made on the CPU by spec_haplotype_count_model.model from
seeded random rows and codes, with sample rows to genotype.  No graph: line v's nodes are ref 2 v + 1 and var 2 v + 2 among
2 V + 1 nodes, so the last line's var node is the last node; node 0 belongs to no line.  Every seventh line is not kept
(var node 0), every fifth has an empty ref node whose count is 0 in every row (an insertion's).  With six individuals the
higher ploidies leave most copy numbers unpopulated, with gaps on either side of a populated one.  The sample rows: row 0
is drawn like an individual, row 1 holds counts of 0 and of 10^6 (never the same count on both nodes of a line), row 2 is drawn at another depth.  A case is built once
per process and is read only."""
import functools

import numpy as np

import spec_haplotype_count_model

N_INDIVIDUALS = 6
DEPTH = 9.0
# name -> (V, ploidy, n_bins)
CASES = {"v%d_p%d_b%d" % c: c for c in
         [(v, 2, 5) for v in (0, 1, 63, 64, 65, 257)] + [(v, p, 5) for v in (65, 257) for p in (1, 3, 8)] +
         [(65, 2, 2), (64, 8, 2)]}
CASE_NAMES = sorted(CASES)
COVERAGES = (1.0, 0.5, 2.5)                                # of the three sample rows, when given


class Case:
    pass


def rows_for(rng, codes_alt, ploidy, ref_nodes, var_nodes, n_nodes, empty_ref, depth):
    """uint32[individuals][n_nodes]: an allele node's count is Poisson(depth x copies + a little noise)."""
    n = codes_alt.shape[1] // ploidy
    rows = np.zeros((n, n_nodes), dtype=np.uint32)
    for i in range(n):
        c_alt = codes_alt[:, i * ploidy:(i + 1) * ploidy].sum(axis=1)
        rows[i][ref_nodes] = rng.poisson(depth * (ploidy - c_alt) + 0.2)
        rows[i][var_nodes] = rng.poisson(depth * c_alt + 0.2)
        rows[i][ref_nodes[empty_ref]] = 0
    rows[:, 0] = 7                                         # node 0 is no line's: never read
    return rows


@functools.lru_cache(maxsize=None)
def case(name):
    v_lines, ploidy, n_bins = CASES[name]
    rng = np.random.default_rng([v_lines, ploidy, n_bins, 2021])
    c = Case()
    c.name, c.ploidy, c.n_bins, c.n_lines = name, ploidy, n_bins, v_lines
    lines = np.arange(v_lines)
    c.ref_nodes = (2 * lines + 1).astype(np.uint32)
    c.var_nodes = (2 * lines + 2).astype(np.uint32)
    if v_lines > 3:
        c.var_nodes[lines % 7 == 3] = 0
    c.n_nodes = 2 * v_lines + 1
    empty_ref = lines % 5 == 1
    c.codes = rng.integers(0, 2, size=(v_lines, N_INDIVIDUALS * ploidy)).astype(np.uint8)
    c.codes[rng.random(c.codes.shape) < 0.05] = 3          # missing calls follow the ref
    c.samples = list(range(N_INDIVIDUALS))
    alt = (c.codes == 1).astype(np.int64)
    c.rows = rows_for(rng, alt, ploidy, c.ref_nodes, np.where(c.var_nodes == 0, 0, c.var_nodes), c.n_nodes, empty_ref, DEPTH)
    c.histogram, c.count_sum = spec_haplotype_count_model.model(c.rows, c.codes, c.ref_nodes, c.var_nodes, c.samples, ploidy,
                                                                n_bins)
    truth = rng.integers(0, 2, size=(v_lines, 2 * ploidy)).astype(np.int64)
    own = rows_for(rng, truth, ploidy, c.ref_nodes, np.where(c.var_nodes == 0, 0, c.var_nodes), c.n_nodes, empty_ref, DEPTH)
    c.sample_rows = np.zeros((3, c.n_nodes), dtype=np.uint32)
    c.sample_rows[0] = own[0]
    # a line's two nodes at (0, 10^6), (10^6, 0) or (10^6, 400000 + v): with equal counts on both, means that mirror one
    # another (as the fallback's steps of one copy make them) tie exactly
    pattern = rng.integers(0, 3, size=v_lines)
    c.sample_rows[1][2 * lines + 1] = np.where(empty_ref | (pattern == 0), 0, 1000000)
    c.sample_rows[1][2 * lines + 2] = np.where(empty_ref | (pattern == 0), 1000000, np.where(pattern == 1, 0, 400000 + lines))
    c.sample_rows[2] = rows_for(rng, truth, ploidy, c.ref_nodes, np.where(c.var_nodes == 0, 0, c.var_nodes), c.n_nodes,
                                empty_ref, 2.5 * DEPTH)[1]
    c.sample_rows[:, c.ref_nodes[empty_ref]] = 0
    for a in (c.ref_nodes, c.var_nodes, c.codes, c.rows, c.histogram, c.count_sum, c.sample_rows):
        a.setflags(write=False)
    return c
