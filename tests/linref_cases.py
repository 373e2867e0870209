"""The small cases of tests/golden/linear_reference.npz, shared by its generator (tests/golden/
make_golden_linear_reference.py, which runs the reference on them) and by the tests that read it."""
import os
import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_reference.npz")

_ALPHABET = np.frombuffer(b"ACGT", dtype=np.uint8)
_ODD = np.frombuffer(b"NnRYKMSWBDHVacgtacgt", dtype=np.uint8)       # N runs, IUPAC codes, lower case


def random_sequence(rng, n):
    """ACGT with a few runs of N, lower-case stretches and scattered IUPAC letters."""
    seq = _ALPHABET[rng.integers(0, 4, n)].copy()
    for _ in range(max(1, n // 400)):
        a = int(rng.integers(0, n))
        seq[a:a + int(rng.integers(1, 40))] = ord("N")
    for _ in range(max(1, n // 300)):
        a = int(rng.integers(0, n))
        b = a + int(rng.integers(1, 60))
        seq[a:b] |= 0x20
    odd = rng.integers(0, n, max(1, n // 50))
    seq[odd] = _ODD[rng.integers(0, len(_ODD), len(odd))]
    return seq


def make_cases():
    """(name, sequence uint8, k, spacing, t, G, reverse complement) -- a few dozen, every parameter of the issue's grid
    drawn at least once: k in {1, 4, 16, 17, 31}, spacing in {1, 2, 3, 31, 50}, t in {2, 3}, G equal to, below and slightly
    above a multiple of 10 * t * spacing (never so far above the sequence that an interval holds no whole k-mer)."""
    rng = np.random.default_rng(20240607)
    cases = []
    grid = [(k, s) for k in (1, 4, 16, 17, 31) for s in (1, 2, 3, 31, 50)]
    for i, (k, s) in enumerate(grid):
        t = (2, 3)[i % 2]
        unit = 10 * t * s
        m = int(rng.integers(1, max(2, 2900 // unit + 1)))
        kind = i % 3
        if kind == 0:
            g = m * unit                                 # equal to a multiple
        elif kind == 1:
            g = m * unit + unit - int(rng.integers(1, unit))         # below one
        else:
            g = m * unit + int(rng.integers(1, unit))    # slightly above one (the surplus positions are never emitted)
        per = (g // s) // (10 * t)
        # every interval holds a whole k-mer; the last one is clipped by the end of the sequence in some cases
        n = per * (10 * t - 1) * s + k + int(rng.integers(0, per * s + 8))
        seq = random_sequence(rng, n)
        cases.append(("k%d_s%d_t%d_G%d_n%d" % (k, s, t, g, n), seq, k, s, t, g, bool(i % 2 == 0) or k == 31))
    # the last interval clipped by the end of the sequence (its end position lies past the last whole k-mer)
    seq = random_sequence(rng, 1017)
    cases.append(("clipped_k31_s1_t2", seq, 31, 1, 2, 1017, True))
    cases.append(("clipped_k16_s3_t3", seq, 16, 3, 3, 1017, False))
    return cases


def load_golden():
    d = np.load(GOLDEN)
    names = [str(x) for x in d["names"]]
    out = []
    for i, name in enumerate(names):
        p = d["params_%d" % i]
        out.append(dict(name=name, seq=d["seq_%d" % i], k=int(p[0]), spacing=int(p[1]), t=int(p[2]), G=int(p[3]), rc=bool(p[4]),
                        hashes=d["hashes_%d" % i], nodes=d["nodes_%d" % i], allele_frequencies=d["af_%d" % i],
                        n_ref_offsets=int(p[5])))
    index = {k: dict(seq=d["rki_seq"], kmers=d["rki_kmers_%d" % k], ref_position_to_index=d["rki_r2i_%d" % k]) for k in (16, 17)}
    return out, index
