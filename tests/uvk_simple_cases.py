"""Graphs and variants for simple selection (find_kmers_over_variants): SNPs, deletions of several bases and insertions,
with the VCF anchor convention for indels, and the stored cases of tests/golden/uvk_simple_reference.json.gz
(tests/golden/make_golden_uvk_simple.py: the reference's own output with use_simple=True)."""
import gzip
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "uvk_simple_reference.json.gz")


def random_sites(rng, length, n_sites, gap_lo, gap_hi, first=45, kinds=("snp", "del", "ins"), max_del=12, max_ins=40):
    """(sequence, sites) of one chromosome: sites = [(offset p, kind, alt sequence, ref length)] in ascending order, the next
    site gap_lo .. gap_hi - 1 bases after the end of the last one's ref allele."""
    seq = "".join(rng.choice(list("acgt"), length))
    sites, p = [], first
    while p < length - 60 and len(sites) < n_sites:
        kind = str(rng.choice(list(kinds)))
        if kind == "snp":
            sites.append((p, kind, "acgt"[("acgt".index(seq[p]) + 1 + int(rng.integers(0, 3))) % 4], 1))
        elif kind == "del":
            sites.append((p, kind, "", int(rng.integers(1, max_del + 1))))
        else:
            sites.append((p, kind, "".join(rng.choice(list("acgt"), int(rng.integers(1, max_ins + 1)))), 0))
        p += sites[-1][3] + int(rng.integers(gap_lo, gap_hi))
    return seq, sites


def sites_graph(chromosomes):
    """obgraph-style dicts of chromosomes [(sequence, sites)]: node sequences, edges, linear-ref nodes, chromosome start
    nodes, and one row (POS, chromosome, ref node, alt node, is_snp) per site.  A site is a linear node up to it, its ref
    allele (linear; empty for an insertion) and its alt allele (empty for a deletion), both leading to the next linear node.
    POS is 1-based: a SNP's own base, an indel's anchor -- the base before the site."""
    ns, ed, lin, starts, rows = {}, {}, [], [], []
    nid = 0
    for c, (seq, sites) in enumerate(chromosomes):
        prev = 0
        starts.append(nid)
        for p, kind, alt, ref_len in sites:
            ns[nid] = seq[prev:p]
            ns[nid + 1], ns[nid + 2] = seq[p:p + ref_len], alt
            ed[nid], ed[nid + 1], ed[nid + 2] = [nid + 1, nid + 2], [nid + 3], [nid + 3]
            lin += [nid, nid + 1]
            rows.append((p + 1 if kind == "snp" else p, c + 1, nid + 1, nid + 2, int(kind == "snp")))
            nid += 3
            prev = p + ref_len
        ns[nid] = seq[prev:]
        lin.append(nid)
        nid += 1
    return ns, ed, lin, starts, rows


def graph_arrays(ns, ed, lin, starts):
    from graph_kmer_index_amd.graph import GraphArrays
    return GraphArrays.from_dicts(ns, ed, lin, chromosome_start_nodes=starts)


# ------------------------------------------------------------------ stored cases
def load_cases():
    with gzip.open(GOLDEN, "rt") as fh:
        return json.load(fh)["cases"]


def case_graph(case):
    gr = case["graph"]
    return graph_arrays({int(n): s for n, s in gr["node_sequences"].items()}, {int(n): e for n, e in gr["edges"].items()},
                        gr["linear_ref_nodes"], gr["chromosome_start_nodes"])


def case_variants(case):
    """(positions, chromosomes, line numbers, is_snp, ref nodes by line, alt nodes by line)."""
    v = case["variants"]
    return (np.array(v["positions"], np.int64), np.array(v["chromosomes"], np.int64), np.array(v["lines"], np.int64),
            np.array(v["is_snp"], np.int8), np.array(case["ref_nodes"], np.int64), np.array(case["var_nodes"], np.int64))


def expected(case):
    e = case["expected"]
    return (np.array(e["hashes"], dtype=np.uint64), np.array(e["nodes"], dtype=np.uint32),
            np.array(e["ref_offsets"], dtype=np.uint64), np.array(e["allele_frequencies"], dtype=np.float32))


def write_vcf(path, positions, chromosomes, is_snp):
    """A VCF whose REF / ALT lengths type the variants: one base each for a SNP, an anchor plus bases for an indel."""
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n")
        for p, c, s in zip(positions, chromosomes, is_snp):
            f.write("%s\t%d\t.\t%s\t%s\n" % (c, p, "A" if s else "AC", "C" if s else "A"))
