"""The NumPy reference of the read side (tests/read_side_ref.py) against the oracle, on the CPU: per-read hashing on
both strands, the probe against a loop of oracle.index_get, and hashing + probing + counting against oracle.map_reads.
tests/test_gpu_read_side_edges.py rests on this reference at sizes the oracle's loops are too slow for."""
import numpy as np
import pytest

from oracle import oracle
from read_side_ref import build_index_ref, contains_ref, count_nodes_ref, hash_reads_ref, probe_ref

COMPLEMENT = str.maketrans("ACGTacgt", "TGCAtgca")       # Seq.reverse_complement on these alphabets: N, R, - stay
KS = (1, 2, 16, 31)
MAX_HITS = (1, 3, 2 ** 62)
N_NODES = 700
INDEX_KEYS = ("_hashes_to_index", "_n_kmers", "_kmers", "_nodes", "_ref_offsets", "_frequencies", "_allele_frequencies")


def mixed_reads(k, seed):
    """A few hundred reads from ACGTacgt with some other letters, lengths around k and around the 64-letter steps."""
    rng = np.random.default_rng(seed)
    lengths = [0, 1, k - 1, k, k + 1, 63, 64, 65, 63 + k, 64 + k, 127 + k, 128 + k, 200] * 20
    lengths += rng.integers(0, 300, size=60).tolist() + [1000]
    alphabet = np.frombuffer(b"ACGTacgt" * 6 + b"Nn-*RY", dtype=np.uint8)
    reads = [alphabet[rng.integers(0, len(alphabet), size=int(n))].tobytes().decode() for n in lengths]
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def packed(reads):
    letters = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
    read_start = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    return letters, read_start


def oracle_strand(reads, k, strand):
    return [oracle.read_kmers(r.translate(COMPLEMENT)[::-1] if strand else r, k) for r in reads]


@pytest.mark.parametrize("k", KS)
def test_hash_reads_ref_equals_oracle_read_kmers_per_read(k):
    reads = mixed_reads(k, 100 + k)
    letters, read_start = packed(reads)
    for strand in (0, 1):
        want = oracle_strand(reads, k, strand)
        got, out_start = hash_reads_ref(letters, read_start, k, strand)
        assert got.dtype == np.uint64 and out_start.dtype == np.int64
        assert np.array_equal(np.diff(out_start), [len(w) for w in want])
        assert np.array_equal(got, np.concatenate(want))
    # a slice of a longer letter array: read_start need not begin at 0 nor end at the last letter
    got, out_start = hash_reads_ref(letters, read_start[5:40], k, 1)
    assert np.array_equal(got, np.concatenate(oracle_strand(reads[5:39], k, 1)))
    assert out_start[0] == 0 and out_start[-1] == len(got)


def test_hash_reads_ref_no_reads_and_no_windows():
    for letters, read_start in ((np.zeros(0, np.uint8), [0]), (np.frombuffer(b"ACG", np.uint8), [0, 0, 3, 3])):
        got, out_start = hash_reads_ref(letters, np.array(read_start, np.int64), 4, 0)
        assert len(got) == 0 and np.array_equal(out_start, np.zeros(len(read_start), np.int64))


def small_index(seed, modulo, skip_frequencies=False, n=4000, pool_size=900):
    """A few thousand records; with modulo < pool_size a bucket holds several k-mers, their records interleaved."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 4 ** 31, size=pool_size, dtype=np.uint64)
    kmers = pool[rng.integers(0, pool_size, size=n)]
    kmers[:40] = pool[0]                                   # one k-mer of 40 or more records
    nodes = rng.integers(0, N_NODES + 50, size=n).astype(np.uint32)
    refs = rng.integers(0, 4, size=n).astype(np.uint64)    # few distinct offsets: frequencies 1..4, below the record count
    af = np.arange(n, dtype=np.float32)                    # names the input record, hence the payload position
    orc = oracle.index_build(kmers, nodes, refs, af, modulo=modulo, skip_frequencies=skip_frequencies)
    return pool, (kmers, nodes, refs, af), orc


@pytest.mark.parametrize("modulo,skip_frequencies", [(257, False), (1, False), (100003, False), (61, True)])
def test_build_index_ref_equals_oracle_index_build(modulo, skip_frequencies):
    _, cols, orc = small_index(modulo, modulo, skip_frequencies)
    got = build_index_ref(*cols, modulo=modulo, skip_frequencies=skip_frequencies)
    for name in INDEX_KEYS:
        assert got[name].dtype == orc[name].dtype, name
        assert np.array_equal(got[name], orc[name]), name
    assert skip_frequencies or orc["_frequencies"].max() == 4


@pytest.mark.parametrize("modulo,skip_frequencies", [(257, False), (1, False), (100003, False), (61, True)])
def test_probe_ref_equals_a_loop_of_oracle_index_get(modulo, skip_frequencies):
    pool, _, orc = small_index(modulo, modulo, skip_frequencies)
    rng = np.random.default_rng(modulo + 1)
    absent = rng.integers(0, 4 ** 31, size=150, dtype=np.uint64)
    queries = np.concatenate([pool[:250], absent, pool[:20], pool[:3] + np.uint64(modulo)])
    for max_hits in MAX_HITS:
        hit_start, positions, query_index = probe_ref(orc, queries, max_hits)
        assert hit_start[0] == 0 and hit_start[-1] == len(positions) == len(query_index)
        assert np.array_equal(query_index, np.repeat(np.arange(len(queries)), np.diff(hit_start)))
        dropped = 0
        for i, q in enumerate(queries):
            got = positions[hit_start[i]:hit_start[i + 1]]
            want = oracle.index_get(orc, int(q), max_hits)
            if want[0] is None:
                assert len(got) == 0
                dropped += bool((orc["_kmers"] == q).any())
                continue
            assert len(got) and (np.diff(got) > 0).all()
            for name, column in zip(("_nodes", "_ref_offsets", "_frequencies", "_allele_frequencies"), want):
                assert np.array_equal(orc[name][got], column), name
        assert (dropped > 0) == (max_hits < 4 and not skip_frequencies)       # the frequency rule was exercised
        counts, hits = count_nodes_ref(orc, queries, max_hits, N_NODES)
        nodes = orc["_nodes"][positions].astype(np.int64)
        assert hits == len(positions) and hits > counts.sum() > 0             # some nodes lie beyond n_counts
        assert np.array_equal(counts, np.bincount(nodes[nodes < N_NODES], minlength=N_NODES))
    assert np.array_equal(contains_ref(orc, queries), np.isin(queries, orc["_kmers"]))


@pytest.mark.parametrize("k", KS)
def test_count_nodes_of_hashed_reads_equals_oracle_map_reads(k):
    reads = mixed_reads(k, 200 + k)
    letters, read_start = packed(reads)
    rng = np.random.default_rng(300 + k)
    fwd, _ = hash_reads_ref(letters, read_start, k, 0)
    rev, _ = hash_reads_ref(letters, read_start, k, 1)
    # a third of the forward k-mers and a different sixth of the reverse-strand ones, some of them several times
    distinct_f, distinct_r = np.unique(fwd), np.unique(rev)
    chosen = np.concatenate([rng.permutation(distinct_f)[:-(-len(distinct_f) // 3)],
                             rng.permutation(distinct_r)[:-(-len(distinct_r) // 6)]])
    kmers = np.concatenate([chosen, chosen[::3], chosen[::3], chosen[::6], chosen[::6]])
    n = len(kmers)
    nodes = rng.integers(0, N_NODES + 50, size=n).astype(np.uint32)
    refs = rng.integers(0, 1000, size=n).astype(np.uint64)
    orc = oracle.index_build(kmers, nodes, refs, np.ones(n, np.float32), modulo=1009)
    assert orc["_frequencies"].max() > 3
    hashes = {1: fwd, 2: rev, 3: np.concatenate([fwd, rev])}
    for strands in (1, 2, 3):
        for max_hits in MAX_HITS:
            want, want_kmers, want_hits = oracle.map_reads(orc, letters, read_start, k, N_NODES, strands, max_hits)
            counts, hits = count_nodes_ref(orc, hashes[strands], max_hits, N_NODES)
            assert want_kmers == len(hashes[strands]) and hits == want_hits and hits > 0
            assert np.array_equal(counts, want)
    # max_hits matters: the k-mers of more than three distinct offsets go at 3
    assert count_nodes_ref(orc, fwd, 3, N_NODES)[1] < count_nodes_ref(orc, fwd, 2 ** 62, N_NODES)[1]
