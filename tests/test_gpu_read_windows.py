"""-m gpu: the one walk under the read side (csrc/gki_read_windows.h walk_span_windows) through its three users --
k_hash_reads (csrc/gki_hash.hip HashSink), k_probe_reads and k_probe_segments (csrc/gki_probe.hip ProbeSink) -- at the
edges of a 64-letter step, and the tagged form of the shared candidate queue (CandQueue<true>, k_probe_contains) at the
edges of a 64-candidate group.  The references are tests/read_side_ref.py and NumPy; every comparison is exact."""
import numpy as np
import pytest

from graph_kmer_index_amd import CollisionFreeKmerIndex, FlatKmers, _lib
from graph_kmer_index_amd.read_kmers import hash_reads
from read_side_ref import build_index_ref, contains_ref, count_nodes_ref, hash_reads_ref

pytestmark = pytest.mark.gpu

MAX = 2 ** 62
WAVE = 64                    # csrc/gki_common.h GKI_WAVE: the letters of a step, the candidates of a drained group
GRID_ITEMS = 2048 * 256      # csrc/gki_common.h stream_grid: at most 256 * 8 blocks of 256 threads
N_NODES = 500


def device_index(kmers, nodes, modulo):
    """(DeviceIndex, the same index from a stable NumPy argsort)."""
    refs, af = np.arange(len(kmers), dtype=np.uint64), np.ones(len(kmers), np.float32)
    idx = CollisionFreeKmerIndex.from_flat_kmers(FlatKmers(kmers, nodes, refs, af), modulo=modulo)
    ref = build_index_ref(kmers, nodes, refs, af, modulo)
    assert np.array_equal(idx._kmers, ref["_kmers"]) and np.array_equal(idx._nodes, ref["_nodes"])
    return idx._device_index(), ref


# ------------------------------------------------------------------ the walk at the step boundaries
def step_boundary_reads(k, rng):
    """Reads whose window counts are 0, 1, 2, 63, 64, 65, 128 and 129 -- the last step of the walk puts out 63, 64 (a
    full step, then none), 1 and 64 windows -- and an empty read in the middle; letters from ACGTNacgtn, an N at the
    first letter of one read and at the last letter of another."""
    lengths = np.array([k - 1, k, k + 1, k + 62, 0, k + 63, k + 64, k + 127, k + 128], dtype=np.int64)
    read_start = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=read_start[1:])
    letters = np.frombuffer(b"ACGTNacgtn", np.uint8)[rng.integers(0, 10, size=int(read_start[-1]))]
    letters[read_start[5]] = ord("N")                   # the first letter of the read of k + 63
    letters[read_start[7] - 1] = ord("N")               # the last letter of the read of k + 64
    return letters, read_start


@pytest.mark.parametrize("k", [1, 2, 16, 31])
def test_both_strands_at_the_step_boundaries(k):
    """HashSink<1> stores the walk's reverse-complement word of window j at n_out - 1 - j, where the kernel before it
    walked the read backwards: the order must hold where n_out is not a multiple of 64, where the last step is full, and
    where a letter outside ACGT is the first or the last of the read.  The same reads then go through k_probe_reads
    for every strand mask, and the same letters through k_probe_segments as overlapping segments, added and taken away."""
    rng = np.random.default_rng(4100 + k)
    letters, read_start = step_boundary_reads(k, rng)
    want = {strand: hash_reads_ref(letters, read_start, k, strand) for strand in (0, 1)}
    for strand in (0, 1):
        hashes, out_start = hash_reads((letters, read_start), k, strand)
        assert np.array_equal(out_start, want[strand][1]), strand
        assert np.array_equal(hashes, want[strand][0]), strand
    fwd, rev = want[0][0], want[1][0]
    assert len(fwd) == len(rev) == 0 + 1 + 2 + 63 + 64 + 65 + 128 + 129
    # the index: a third of the distinct forward k-mers and a sixth of the reverse-strand ones that are not among them
    distinct_f = np.unique(fwd)
    chosen_f = rng.permutation(distinct_f)[:-(-len(distinct_f) // 3)]
    others_r = np.setdiff1d(np.unique(rev), chosen_f)
    chosen_r = rng.permutation(others_r)[:-(-len(others_r) // 6)]
    assert len(chosen_f) and len(chosen_r) and not np.isin(chosen_r, chosen_f).any()
    kmers = np.concatenate([chosen_f, chosen_r, chosen_f[::2]])
    dev, ref = device_index(kmers, rng.integers(0, N_NODES, size=len(kmers)).astype(np.uint32), 10007)
    c_f, h_f = count_nodes_ref(ref, fwd, MAX, N_NODES)
    c_r, h_r = count_nodes_ref(ref, rev, MAX, N_NODES)
    assert h_f > 0 and h_r > 0
    for strands, counts, n_kmers, n_hits in ((1, c_f, len(fwd), h_f), (2, c_r, len(rev), h_r),
                                             (3, c_f + c_r, len(fwd) + len(rev), h_f + h_r)):
        got, got_kmers, got_hits = dev.count_nodes_from_reads(letters, read_start, k, N_NODES, strands, MAX)
        assert (got_kmers, got_hits) == (n_kmers, n_hits), strands
        assert np.array_equal(got.to_host(N_NODES), counts), strands
        got.free()
    # segments that overlap one another: every 40 letters one of up to 129 windows, and one of every boundary count
    n = len(letters)
    seg_start = np.concatenate([np.arange(0, n - k + 1, 40), [0, 1, 2, 3, 5, 7, 11]]).astype(np.int64)
    seg_windows = np.concatenate([np.full(len(seg_start) - 7, 129), [0, 1, 63, 64, 65, 128, 129]]).astype(np.int64)
    seg_windows = np.minimum(seg_windows, n - (k - 1) - seg_start)
    assert (seg_windows >= 0).all() and (seg_start[1:-7] < seg_start[:-8] + seg_windows[:-8]).all()
    seg_len = np.where(seg_windows > 0, seg_windows + k - 1, 0)
    cut_start = np.zeros(len(seg_start) + 1, dtype=np.int64)
    np.cumsum(seg_len, out=cut_start[1:])
    cut = np.concatenate([letters[a:a + m] for a, m in zip(seg_start, seg_len)])
    seg_f, seg_r = (hash_reads_ref(cut, cut_start, k, strand)[0] for strand in (0, 1))
    assert len(seg_f) == seg_windows.sum()
    (c_f, h_f), (c_r, h_r) = (count_nodes_ref(ref, x, MAX, N_NODES) for x in (seg_f, seg_r))
    d_letters = _lib.DeviceArray.from_host(letters)
    d_counts = _lib.DeviceArray.from_host(np.zeros(N_NODES, np.uint32))
    for sign, counts in ((1, c_f + c_r), (-1, np.zeros(N_NODES, np.int64))):
        got = dev.count_nodes_from_segments(d_letters, seg_start, seg_windows, k, d_counts, N_NODES, strands=3, sign=sign)
        assert got == (len(seg_f) + len(seg_r), h_f + h_r), sign
        assert np.array_equal(d_counts.to_host(N_NODES), counts), sign
    d_letters.free(); d_counts.free()


# ------------------------------------------------------------------ the tagged queue at the edges of a group
def fp_bit(kmers):
    """csrc/gki_probe.hip fp_bit: which of the 16 fingerprint bits of its bucket's directory word a k-mer tests."""
    x = ((kmers >> np.uint64(32)) * np.uint64(0x9E3779B1) ^ (kmers & np.uint64(0xFFFFFFFF)) * np.uint64(0x85EBCA77))
    return np.uint32(1) << ((x & np.uint64(0xFFFFFFFF)) >> np.uint64(28)).astype(np.uint32)


@pytest.fixture(scope="module")
def contains_case():
    """An index of 3 000 k-mers at modulo 10 007 (buckets of a few k-mers: every fingerprint set is scanned, none is all
    ones), and what the queries are made of: present k-mers; absent k-mers with the bucket and the fingerprint bit of a
    present one, which survive the directory word and die in the row scan; k-mers of empty buckets, which do not survive."""
    modulo = 10007
    rng = np.random.default_rng(65)
    kmers = np.unique(rng.integers(0, 4 ** 31 // 2, size=3000, dtype=np.uint64))
    dev, ref = device_index(kmers, rng.integers(0, N_NODES, size=len(kmers)).astype(np.uint32), modulo)
    assert ref["_n_kmers"].max() <= WAVE
    fp_set = np.zeros(modulo, dtype=np.uint32)
    np.bitwise_or.at(fp_set, (kmers % np.uint64(modulo)).astype(np.int64), fp_bit(kmers))
    # present p -> the first p + modulo * t (t = 1, 2, ..) that is absent and tests the bit p set
    decoys = []
    for p in kmers[:200]:
        tries = p + np.uint64(modulo) * np.arange(1, 400, dtype=np.uint64)
        ok = (fp_bit(tries) == fp_bit(np.array([p]))[0]) & ~np.isin(tries, kmers)
        decoys.append(tries[np.flatnonzero(ok)[0]])
    decoys = np.array(decoys, dtype=np.uint64)
    empty = np.flatnonzero(ref["_n_kmers"] == 0).astype(np.uint64)
    dead = empty[rng.integers(0, len(empty), size=200)] + np.uint64(modulo) * rng.integers(1, 10 ** 9, size=200).astype(np.uint64)

    def survives(q):
        return (fp_set[(q % np.uint64(modulo)).astype(np.int64)] & fp_bit(q)) != 0
    assert survives(kmers).all() and survives(decoys).all() and not survives(dead).any()
    return dev, ref, kmers, decoys, dead, survives


@pytest.mark.parametrize("n_candidates", [WAVE - 1, WAVE, WAVE + 1])
def test_contains_with_a_group_of_the_queue_just_not_full_and_just_over(n_candidates, contains_case):
    """k_probe_contains parks the survivors of the directory word with their query index beside them and scans them once
    64 are there.  The first wave takes the queries lane, GRID_ITEMS + lane and 2 * GRID_ITEMS + lane: its first 64
    queries hold min(n_candidates, 64) survivors -- present k-mers and decoys in turn -- and the 65th is its first query of
    the second trip, so that the wave ends with 63 parked and never a full group, with exactly one full group, and with a
    full group and one left over; every other query of that wave dies at the directory word.  2 * GRID_ITEMS + 3 queries
    make every wave take the second trip and the first wave a third."""
    dev, ref, kmers, decoys, dead, survives = contains_case
    rng = np.random.default_rng(n_candidates)
    q = 2 * GRID_ITEMS + 3
    absent = rng.integers(0, 2 ** 62, size=q, dtype=np.uint64)
    queries = np.where(rng.random(q) < 0.5, kmers[rng.integers(0, len(kmers), size=q)], absent)
    first_wave = np.concatenate([np.arange(WAVE), GRID_ITEMS + np.arange(WAVE), 2 * GRID_ITEMS + np.arange(3)])
    queries[first_wave] = dead[:len(first_wave)]
    candidates = np.empty(n_candidates, dtype=np.uint64)
    candidates[0::2] = kmers[:len(candidates[0::2])]
    candidates[1::2] = decoys[:len(candidates[1::2])]
    queries[first_wave[:WAVE][:n_candidates]] = candidates[:WAVE]
    if n_candidates > WAVE:
        queries[GRID_ITEMS] = candidates[WAVE]
    assert survives(queries[first_wave]).sum() == n_candidates
    assert survives(queries[:WAVE]).sum() == min(n_candidates, WAVE)
    want = np.isin(queries, ref["_kmers"])
    assert want[first_wave].sum() == -(-n_candidates // 2) and 0.4 * q < want.sum() < 0.6 * q
    assert np.array_equal(want, contains_ref(ref, queries))
    flags = dev.contains(queries)
    got = flags.to_host(q)
    flags.free()
    assert np.array_equal(got, want.astype(np.uint8))
