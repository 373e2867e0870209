"""Named inputs of the node counts by difference and of the count model: small graphs with their
variant-to-nodes tables, built by the graph-build spec from (reference, VCF text) pairs made with the helpers of
tests/graph_build_cases.py, and a code matrix per case.  Slot 0 takes no line, slot 1 every line, slot 2 a random half,
slot 3 holds codes 2 and 3 beside 0 and 1; a case of at most eight lines adds one slot per line, taken alone, and some add
slots of their own behind those.  Everything is generated here, seeded; a case is built once per process."""
import functools
import zlib

import numpy as np

import spec_graph_build
from graph_build_cases import deletion, every_third_snp, insertion, random_reference, snp, vcf
from haplotype_path_cases import graph_of

KS = (5, 31)
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def letters_of(n, seed):
    return BASES[np.random.default_rng([seed, 3]).integers(0, 4, size=n)].tobytes()


def _inputs():
    """name -> (reference, text, extra slots), an extra slot a function of the number of data lines"""
    c = {}
    big = random_reference(3 * 130 + 40, 51)
    for n in (63, 64, 65, 129):                            # the plane's word edges
        c["lines_%d" % n] = ({"1": big}, vcf(every_third_snp("1", big, n)), ())
    # more than 256 taken lines: more than one block of the segment kernels; every other line too, 6 apart
    r940 = random_reference(3 * 300 + 40, 52)
    c["taken_300"] = ({"1": r940}, vcf(every_third_snp("1", r940, 300)), (lambda v: np.arange(v) % 2,))
    # SNPs k - 2, k - 1, k and k + 1 apart for k = 5, then for k = 31
    r400 = random_reference(400, 53)
    at = [40, 43, 47, 52, 58, 100, 129, 159, 190, 222]
    assert np.diff(at[:5]).tolist() == [3, 4, 5, 6] and np.diff(at[5:]).tolist() == [29, 30, 31, 32]
    c["merge_edges"] = ({"1": r400}, vcf([snp("1", r400, p) for p in at]), (lambda v: np.arange(v) % 2, lambda v: (np.arange(v) + 1) % 2))
    # a site fewer than k letters from the chromosome's start, another that close to its end, for both k
    r120 = random_reference(120, 54)
    c["near_both_ends"] = ({"1": r120}, vcf([snp("1", r120, 3), snp("1", r120, 118)]), ())
    c["first_and_last_base"] = ({"1": r120}, vcf([snp("1", r120, 1), snp("1", r120, 120)]), ())
    # an insertion (empty ref allele) and a deletion (empty alt allele), alone and touching a neighbouring SNP
    r300 = random_reference(300, 55)
    c["indels"] = ({"1": r300}, vcf([insertion("1", r300, 40, b"ACGTT"), deletion("1", r300, 90, 4),
                                    insertion("1", r300, 139, b"GG"), snp("1", r300, 140),
                                    deletion("1", r300, 199, 3), snp("1", r300, 203)]),
                   (lambda v: np.array([0, 0, 1, 1, 0, 0]), lambda v: np.array([0, 0, 0, 0, 1, 1])))
    # segments of 64 and 65 windows (insertions of 60 and 61 letters at k = 5, of 34 and 35 at k = 31) and the lengths
    # 63, 64 and 200: the wave takes 64 windows a step
    lengths = (34, 35, 60, 61, 63, 64, 200)
    r600 = random_reference(600, 56)
    c["long_insertions"] = ({"1": r600}, vcf([insertion("1", r600, 50 + 70 * i, letters_of(n, 60 + i))
                                             for i, n in enumerate(lengths)]), ())
    # adjacent SNPs: the second and third own one window each when all are taken
    c["adjacent_snps"] = ({"1": r120}, vcf([snp("1", r120, 50), snp("1", r120, 51), snp("1", r120, 52)]), ())
    a, b20, b4, d = random_reference(80, 57), random_reference(20, 58), random_reference(4, 59), random_reference(75, 60)
    c["short_chromosome_20"] = ({"a": a, "b": b20, "c": d}, vcf([snp("a", a, 9), insertion("a", a, 50, b"TT"), snp("b", b20, 10),
                                                                deletion("c", d, 20, 4), snp("c", d, 72)]), ())
    c["short_chromosome_4"] = ({"a": a, "b": b4, "c": d}, vcf([snp("a", a, 78), snp("b", b4, 2), snp("c", d, 2),
                                                              deletion("c", d, 40, 2)]), ())
    return c


INPUTS = _inputs()
CASE_NAMES = sorted(INPUTS)


class Case:
    pass


def codes_for(name, var_nodes, extra=()):
    """uint8[V][H], seeded by the case's name."""
    v = len(var_nodes)
    rng = np.random.default_rng([zlib.crc32(name.encode()), 11])
    columns = [np.zeros(v, np.uint8), np.ones(v, np.uint8), rng.integers(0, 2, size=v), rng.integers(0, 4, size=v)]
    kept = np.flatnonzero(np.asarray(var_nodes) != 0)
    columns[3][kept[0::3]] = 2                             # codes 2 and 3 stand on kept lines, beside 0 and 1
    columns[3][kept[1::3]] = 3
    if len(kept) > 2:
        columns[3][kept[2::3]] = 1
    if v <= 8:
        columns += [np.arange(v) == i for i in range(v)]
    columns += [f(v) for f in extra]
    return np.stack(columns, axis=1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(name):
    reference, text, extra = INPUTS[name]
    c = Case()
    c.name, c.reference, c.text = name, reference, text
    c.build = spec_graph_build.build(reference, text)
    c.graph = graph_of(c.build)
    c.ref_nodes, c.var_nodes = c.build.ref_nodes, c.build.var_nodes
    c.codes = codes_for(name, c.var_nodes, extra)
    c.n_slots = c.codes.shape[1]
    c.starts = [c.graph.chromosome_start_nodes[x] for x in sorted(c.graph.chromosome_start_nodes)]
    return c


@functools.lru_cache(maxsize=None)
def model_case():
    """Four diploid individuals over seven lines; at line 0 they are hom-ref, het, hom-alt and het the other way round.
    The same matrix is eight haploid individuals."""
    r = random_reference(20000, 61)                        # long enough for counts in the hundreds at k = 5
    c = Case()
    c.name, c.reference = "model", {"1": r}
    c.text = vcf([snp("1", r, 30), snp("1", r, 80), insertion("1", r, 120, b"ACGTACGTAC"), deletion("1", r, 170, 5),
                  snp("1", r, 230), snp("1", r, 233), snp("1", r, 15000)])
    c.build = spec_graph_build.build(c.reference, c.text)
    c.graph = graph_of(c.build)
    c.ref_nodes, c.var_nodes = c.build.ref_nodes, c.build.var_nodes
    rng = np.random.default_rng(62)
    c.codes = rng.integers(0, 2, size=(len(c.var_nodes), 8)).astype(np.uint8)
    c.codes[0] = [0, 0, 0, 1, 1, 1, 1, 0]
    c.codes[4] = [2, 1, 3, 0, 1, 2, 1, 3]                  # other alleles and missing calls follow the ref
    c.n_slots = 8
    c.starts = [c.graph.chromosome_start_nodes[x] for x in sorted(c.graph.chromosome_start_nodes)]
    return c
