"""A plain NumPy restatement of the read side -- hash reads, probe a CollisionFreeKmerIndex, count nodes -- that shares no
code with the oracle's C (oracle/gki_oracle.c) nor with the kernels.  64-bit integers throughout, no Python loop over
reads, queries or records.  tests/test_read_side_ref.py checks it against the oracle on the CPU; the -m gpu tests of
tests/test_gpu_read_side_edges.py then use it at sizes where a loop of oracle calls would take minutes.

An index is a dict of the seven attribute arrays keyed like `CollisionFreeKmerIndex.properties` (what
`oracle.index_build` returns): _hashes_to_index, _n_kmers, _kmers, _nodes, _ref_offsets, _frequencies,
_allele_frequencies, plus _modulo."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

# letter -> 2-bit code: A/a 0, C/c 1, G/g 2, T/t 3, everything else 0 (read_kmers.py:67-70 via letter_sequence_to_numeric)
FORWARD_CODE = np.zeros(256, dtype=np.uint8)
# the same letter on the reverse strand: 3 - code for ACGT, 0 for every other letter (Seq(read).reverse_complement()
# keeps N, and N hashes as 0)
REVERSE_CODE = np.zeros(256, dtype=np.uint8)
for _letters, _code in (("Aa", 0), ("Cc", 1), ("Gg", 2), ("Tt", 3)):
    for _ch in _letters:
        FORWARD_CODE[ord(_ch)] = _code
        REVERSE_CODE[ord(_ch)] = 3 - _code

_CHUNK = 1 << 17          # windows hashed per matrix product: 2^17 x 31 uint64 = 32 MB


def _repeat_per_item(values, counts):
    return np.repeat(np.asarray(values, dtype=np.int64), counts)


def hash_reads_ref(letters, read_start, k, strand):
    """(hashes uint64[], out_start int64[n_reads + 1]): the k-mer hashes of every read, first base least significant,
    read after read; strand 1 hashes every read reversed and complemented.  The reads are hashed where they lie in
    `letters`: the windows that start inside a read and end inside it are taken from a sliding_window_view of the
    whole (per read reversed, for strand 1) code array and multiplied with 4**arange(k)."""
    letters = np.asarray(letters, dtype=np.uint8)
    read_start = np.asarray(read_start, dtype=np.int64)
    k = int(k)
    first, lens = read_start[:-1], np.diff(read_start)
    n_out = np.maximum(lens - k + 1, 0)
    out_start = np.zeros(len(read_start), dtype=np.int64)
    np.cumsum(n_out, out=out_start[1:])
    total = int(out_start[-1])
    hashes = np.zeros(total, dtype=np.uint64)
    if total == 0:
        return hashes, out_start
    begin, end = int(read_start[0]), int(read_start[-1])
    if strand:
        # letter p of read r comes from first_r + last_r - p: the read walked backwards, in place
        source = _repeat_per_item(first + read_start[1:] - 1, lens) - np.arange(begin, end, dtype=np.int64)
        codes = REVERSE_CODE[letters[source]]
    else:
        codes = FORWARD_CODE[letters[begin:end]]
    # window j of read r starts at letter first_r + j (relative to `begin`)
    window_start = np.arange(total, dtype=np.int64) - _repeat_per_item(out_start[:-1] - (first - begin), n_out)
    windows = sliding_window_view(codes, k)
    powers = np.uint64(4) ** np.arange(k, dtype=np.uint64)
    for a in range(0, total, _CHUNK):
        hashes[a:a + _CHUNK] = windows[window_start[a:a + _CHUNK]].astype(np.uint64) @ powers
    return hashes, out_start


def build_index_ref(kmers, nodes, ref_offsets, allele_frequencies, modulo, skip_frequencies=False, directory=True):
    """CollisionFreeKmerIndex.from_flat_kmers (collision_free_kmer_index.py:423-467) with a STABLE argsort of
    kmers % modulo, so that the records of a bucket keep their input order.  The frequency of a record is the number
    of distinct ref offsets among the records of its k-mer (:267-293), narrowed to uint16.  directory=False leaves the
    two modulo-sized arrays out (None): the probe reference does not read them."""
    kmers = np.asarray(kmers).astype(np.uint64)
    ref_offsets = np.asarray(ref_offsets)
    modulo = int(modulo)
    bucket = (kmers % np.uint64(modulo)).astype(np.int64)
    order = np.argsort(bucket, kind="stable")
    n_kmers = hashes_to_index = None
    if directory:
        n_kmers = np.bincount(bucket, minlength=modulo).astype(np.uint32)
        hashes_to_index = np.zeros(modulo, dtype=np.int32)
        begin = np.cumsum(n_kmers.astype(np.int64)) - n_kmers
        hashes_to_index[n_kmers > 0] = begin[n_kmers > 0]
    frequencies = np.zeros(len(kmers), dtype=np.uint16)
    if not skip_frequencies and len(kmers):
        _, kmer_id = np.unique(kmers, return_inverse=True)
        kmer_id = kmer_id.reshape(-1)
        _, ref_id = np.unique(ref_offsets, return_inverse=True)
        ref_id = ref_id.reshape(-1)
        pair = np.unique(kmer_id.astype(np.int64) * (int(ref_id.max()) + 1) + ref_id)
        distinct = np.bincount(pair // (int(ref_id.max()) + 1), minlength=int(kmer_id.max()) + 1)
        frequencies = distinct[kmer_id][order].astype(np.uint16)
    return dict(_hashes_to_index=hashes_to_index, _n_kmers=n_kmers, _nodes=np.asarray(nodes)[order],
                _ref_offsets=ref_offsets[order], _kmers=kmers[order], _modulo=modulo, _frequencies=frequencies,
                _allele_frequencies=np.asarray(allele_frequencies)[order])


class _Sorted:
    """The index's k-mers, distinct and ascending, with the payload positions of each one in ascending order."""

    def __init__(self, index):
        kmers = np.asarray(index["_kmers"]).astype(np.uint64)
        # Equal k-mers share a bucket, and a stable sort by k-mer keeps their positions ascending: positions[start[i] :
        # start[i] + count[i]] is k-mer i's hits in bucket order, contiguous in the bucket or not.
        self.positions = np.argsort(kmers, kind="stable").astype(np.int64)
        self.distinct, self.start, self.count = np.unique(kmers[self.positions], return_index=True, return_counts=True)
        freq = index.get("_frequencies")
        self.frequencies = freq if isinstance(freq, np.ndarray) and len(freq) == len(kmers) else None


def _sorted_of(index):
    if "_read_side_ref_sorted" not in index:
        index["_read_side_ref_sorted"] = _Sorted(index)
    return index["_read_side_ref_sorted"]


def probe_ref(index, queries, max_hits):
    """CollisionFreeKmerIndex.get (collision_free_kmer_index.py:303-315) for every query: (hit_start int64[q + 1],
    positions int64[hits] into the payload arrays, query index int64[hits]); the hits of a query are the positions j
    with _kmers[j] == query, ascending (bucket order), all of them dropped when the index has frequencies and
    _frequencies[first hit] > max_hits (:312)."""
    s = _sorted_of(index)
    queries = np.asarray(queries).astype(np.uint64)
    hit_start = np.zeros(len(queries) + 1, dtype=np.int64)
    if len(queries) == 0 or len(s.distinct) == 0:
        return hit_start, np.zeros(0, np.int64), np.zeros(0, np.int64)
    at = np.minimum(np.searchsorted(s.distinct, queries), len(s.distinct) - 1)
    found = s.distinct[at] == queries
    first = s.start[at]
    if s.frequencies is not None:
        found &= s.frequencies[s.positions[first]].astype(np.int64) <= min(int(max_hits), 2 ** 62)
    count = np.where(found, s.count[at], 0).astype(np.int64)
    np.cumsum(count, out=hit_start[1:])
    query_index = np.repeat(np.arange(len(queries), dtype=np.int64), count)
    within = np.arange(int(hit_start[-1]), dtype=np.int64) - np.repeat(hit_start[:-1], count)
    return hit_start, s.positions[np.repeat(first, count) + within], query_index


def count_nodes_ref(index, queries, max_hits, n_counts):
    """map_kmers (collision_free_kmer_index.py:210-212): (counts int64[n_counts], hits).  A hit on a node >= n_counts
    is not counted in `counts` but is in `hits`, as the kernels count them."""
    _, positions, _ = probe_ref(index, queries, max_hits)
    nodes = np.asarray(index["_nodes"])[positions].astype(np.int64)
    return np.bincount(nodes[nodes < n_counts], minlength=n_counts)[:n_counts], len(positions)


def contains_ref(index, queries):
    """`kmer in index` (collision_free_kmer_index.py:295-296) for every query: bool[q]."""
    hit_start, _, _ = probe_ref(index, queries, 2 ** 62)
    return np.diff(hit_start) > 0
