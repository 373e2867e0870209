"""Variants of synthetic graphs for the UniqueVariantKmersFinder tests: one per (linear node with two or more
successors, non-linear successor), POS = ref offset of the linear successor + 1, ref node = the linear successor."""
import numpy as np


def bubble_variants(g, k, extra_alts=True):
    ntro = np.asarray(g.node_to_ref_offset, dtype=np.int64)
    lin_end = int(g.node_size[(g.is_ref != 0)].sum())
    refs, alts, pos = [], [], []
    for u in np.nonzero((np.diff(g.edge_start) >= 2) & (g.is_ref != 0))[0].tolist():
        succ = g.edges[g.edge_start[u]:g.edge_start[u + 1]].tolist()
        lin = [s for s in succ if g.is_ref[s]]
        others = [s for s in succ if not g.is_ref[s]]
        if not lin or not others:
            continue
        p = int(ntro[lin[0]]) + 1
        if p - 2 - 4 * (len(range(2, k - 2)[::4]) - 1) < 0 or p - 2 >= lin_end:
            continue
        for a in (others if extra_alts else others[:1]):
            refs.append(lin[0]); alts.append(a); pos.append(p)
    return np.array(refs, np.int64), np.array(alts, np.int64), np.array(pos, np.int64)


# ------------------------------------------------------------------ planted graphs (tests/golden/make_golden_uvk.py)
def _other(b, r):
    return "acgt"[("acgt".index(b) + 1 + r) % 4]


def planted_chromosome(rng, length, n_snps, n_dels=0, n_repeats=0, cluster=0):
    """(sequence, sites): a random chromosome with
      * n_repeats copies of the 40 bases around an SNP site (30 before it, its ref base, 9 after) planted elsewhere, so
        that the two earliest starts of that variant see k-mers of frequency 2 and the later ones do not;
      * n_dels one-base deletions inside 80-base runs of 'a' (the ref window and the alt window share a hash);
      * a cluster of `cluster` SNPs three bases apart (more than 500 windows from one start with max_variant_nodes 6);
    sites = sorted [(offset, kind, alt)], kind 'snp' or 'del'."""
    seq = list("".join(rng.choice(list("acgt"), length)))
    taken = np.zeros(length, bool)
    sites = []

    def free(a, b):
        return a >= 0 and b <= length and not taken[a:b].any()

    for _ in range(n_dels):
        for _try in range(200):
            a = int(rng.integers(40, length - 120))
            if free(a - 4, a + 84):
                seq[a:a + 80] = "a" * 80
                taken[a - 4:a + 84] = True
                sites.append((a + 40, "del", ""))
                break
    if cluster:
        for _try in range(200):
            a = int(rng.integers(40, length - 80))
            if free(a - 4, a + 3 * cluster + 4):
                taken[a - 4:a + 3 * cluster + 4] = True
                for i in range(cluster):
                    p = a + 3 * i
                    sites.append((p, "snp", _other(seq[p], int(rng.integers(0, 3)))))
                break
    snps = 0
    for _try in range(50 * n_snps):
        if snps == n_snps:
            break
        p = int(rng.integers(40, length - 40))
        if free(p - 8, p + 8):
            taken[p - 8:p + 8] = True
            sites.append((p, "snp", _other(seq[p], int(rng.integers(0, 3)))))
            snps += 1
    snp_sites = [s for s in sites if s[1] == "snp"]
    for i in range(min(n_repeats, len(snp_sites))):
        p = snp_sites[i][0]
        for _try in range(500):
            b = int(rng.integers(0, length - 45))
            if free(b, b + 45) and not (b + 45 > p - 45 and b < p + 45):
                seq[b:b + 40] = seq[p - 30:p + 10]
                taken[b:b + 45] = True
                break
    return "".join(seq), sorted(sites)


def planted_graph(chromosomes):
    """obgraph-style dicts of one or more chromosomes [(sequence, sites)]: node_sequences, edges, linear nodes,
    chromosome start nodes, and the variants [(POS, chromosome, ref node, alt node)]."""
    ns, ed, lin, starts, variants = {}, {}, [], [], []
    nid = 0
    for c, (seq, sites) in enumerate(chromosomes):
        prev = 0
        starts.append(nid)
        for p, kind, alt in sites:
            ns[nid] = seq[prev:p]
            lin.append(nid)
            ns[nid + 1], ns[nid + 2] = seq[p], alt
            ed[nid] = [nid + 1, nid + 2]
            ed[nid + 1] = [nid + 3]
            ed[nid + 2] = [nid + 3]
            lin.append(nid + 1)
            variants.append((p + 1, c + 1, nid + 1, nid + 2))
            nid += 3
            prev = p + 1
        ns[nid] = seq[prev:]
        lin.append(nid)
        nid += 1
    return ns, ed, lin, starts, variants
