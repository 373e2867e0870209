"""Named inputs of the haplotype paths: a graph with its variant-to-nodes table, built by the graph-build
spec from the (reference, VCF text) pairs of tests/graph_build_cases.py and from a few more made here, and a seeded code
matrix with H >= 5 slots: 0 all-ref, 1 all-alt, 2 and 3 random, 4 holding codes 2 and 3 on kept lines; some cases add
slots of their own behind those.  Everything is generated here, seeded; a case is built once per process."""
import functools
import zlib

import numpy as np

import spec_graph_build
from graph_build_cases import (GOOD_CASES, RANDOM_CASES, deletion, every_third_snp, insertion, random_reference, snp,
                               vcf)
from graph_kmer_index_amd.graph import GraphArrays

TILE = 4096                                                # output letters per workgroup of the spelling kernel


def _extra_inputs():
    """name -> (reference, text, extra slots), an extra slot a function of the number of data lines"""
    c = {}
    big = random_reference(3 * 130 + 10, 21)
    for n in (63, 64, 65, 129):                            # the plane's word edges
        c["lines_%d" % n] = ({"1": big}, vcf(every_third_snp("1", big, n)), ())
    # a cut at each of the 16 offsets of a 16-byte block: SNPs 17 apart; alt taken everywhere and at every other line
    r400 = random_reference(400, 22)
    c["snps_17_apart"] = ({"1": r400}, vcf([snp("1", r400, 2 + 17 * i) for i in range(23)]),
                          (lambda v: np.arange(v) % 2, lambda v: (np.arange(v) + 1) % 2))
    r10, r16, r17 = random_reference(10, 23), random_reference(16, 24), random_reference(17, 25)
    c["output_of_10"] = ({"1": r10}, vcf([snp("1", r10, 5)]), ())
    c["output_of_16"] = ({"1": r16}, vcf([snp("1", r16, 8), snp("1", r16, 16)]), ())
    c["output_of_16_or_17"] = ({"1": r17}, vcf([deletion("1", r17, 8, 1)]), ())
    c["output_of_16_or_19"] = ({"1": r16}, vcf([insertion("1", r16, 15, b"ACG")]), ())
    # more than two tiles; alt taken puts a cut on the last byte of tile 0 and 1 and on the first of tile 1 and 2, ref
    # taken one byte further on
    tiles = random_reference(3 * TILE + 100, 26)
    c["cuts_on_tile_edges"] = ({"1": tiles}, vcf([snp("1", tiles, p) for p in (TILE, TILE + 1, 2 * TILE, 2 * TILE + 1)]), ())
    a, b, d = random_reference(50, 27), random_reference(20, 28), random_reference(45, 29)
    c["short_chromosome"] = ({"a": a, "b": b, "c": d}, vcf([snp("a", a, 9), insertion("a", a, 30, b"TT"), snp("b", b, 10),
                                                            deletion("c", d, 20, 4), snp("c", d, 40)]), ())
    return c


EXTRA_INPUTS = _extra_inputs()
CASE_NAMES = sorted(GOOD_CASES) + sorted(EXTRA_INPUTS)
COUNT_CASES = tuple(RANDOM_CASES) + ("two_chromosomes", "short_chromosome")      # node counts are compared on these


class Case:
    pass


def graph_of(b):
    """A spec build's arrays as GraphArrays."""
    return GraphArrays(b.node_size, b.seq, b.edge_start, b.edges, b.is_ref, b.allele_freq, b.exists, b.first_node,
                       b.chromosome_start_nodes, b.node_to_ref_offset, b.rev_start, b.rev_edges)


def codes_for(name, var_nodes, extra=()):
    """uint8[V][5 + len(extra)], seeded by the case's name."""
    v = len(var_nodes)
    rng = np.random.default_rng([zlib.crc32(name.encode()), 7])
    codes = np.zeros((v, 5 + len(extra)), dtype=np.uint8)
    codes[:, 1] = 1
    codes[:, 2] = rng.integers(0, 2, size=v)
    codes[:, 3] = rng.random(v) < 0.8
    codes[:, 4] = rng.integers(0, 4, size=v)
    kept = np.flatnonzero(np.asarray(var_nodes) != 0)
    codes[kept[0::3], 4] = 2                               # codes 2 and 3 stand on kept lines, beside 0 and 1
    codes[kept[1::3], 4] = 3
    for i, f in enumerate(extra):
        codes[:, 5 + i] = f(v)
    return codes


@functools.lru_cache(maxsize=None)
def case(name):
    reference, text, extra = EXTRA_INPUTS[name] if name in EXTRA_INPUTS else GOOD_CASES[name] + ((),)
    c = Case()
    c.name, c.reference, c.text = name, reference, text
    c.build = spec_graph_build.build(reference, text)
    c.graph = graph_of(c.build)
    c.ref_nodes, c.var_nodes = c.build.ref_nodes, c.build.var_nodes
    c.codes = codes_for(name, c.var_nodes, extra)
    c.n_slots = c.codes.shape[1]
    return c
