// CollisionFreeKmerIndex on MI355X: bucket = kmer % modulo, records stably sorted by bucket,
// bucket directory (first position + length), per-kmer frequencies, batched probe.
//
// This file holds
//   the entry points      gki_index_build*, gki_partition_*by_bucket_range*, gki_reverse_index_build, gki_flag_repeated_kmers:
//                         argument checks, then the row-carrying form or the bucket-range partition (gki_index_rows.hip)
//   the pair-sorting form what the row-carrying form hands back (a group of buckets too large to stream with one workgroup,
//                         2^31 records and more in the reverse index) and what its parity tests compare it with:
//                         k_sort_keys (key of every record + the identity permutation), a stable LSD radix sort of the
//                         (key, index) pairs, 8 bits per pass, only the bits the largest key occupies (per pass: tile
//                         histograms -> scan -> ranked scatter with an in-LDS reorder so every digit's run leaves the CU as one
//                         contiguous store: the pass of gki_radix_tile.h over PairItems), k_pack_rows / k_gather_rows (the
//                         payload packed into 16- or 32-byte rows, permuted once by the sorted index), k_directory /
//                         k_node_directory
//   frequencies           k_frequencies_small for the pair-sorting form; k_frequencies_ranges + k_frequencies_large for the
//                         buckets of more than SMALL_BUCKET records that either form leaves open
//   the lookups           k_lookup, k_count_nodes, k_get_small
// Inside a bucket records keep their input order (stable sort), which is also what the oracle's
// stable restatement produces, so the build is comparable element by element.
#include "gki_index_internal.h"
#include "gki_radix_tile.h"
#include <cstring>
#include <cstdlib>
#include <mutex>

namespace {

constexpr int RB = 256;             // threads per block in the radix kernels
constexpr int RI = 16;              // items per thread
constexpr int RTILE = RB * RI;      // 4096 items per tile
constexpr int RBINS = RADIX_BINS;

// The sort key of every record and the identity permutation: the bucket relative to the slice (collision_free_kmer_index.py:433)
// or, BY_NODE, the node id with sl.n_buckets = the number of nodes.  A key outside the slice is flagged and replaced by one
// inside it (the directory is never indexed out of range).
template <bool BY_NODE>
__global__ __launch_bounds__(256) void k_sort_keys(const void *__restrict__ src, int64_t n, Slice sl, uint32_t *__restrict__ keys,
                                                   uint32_t *__restrict__ idx, int *__restrict__ bad) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint64_t b = BY_NODE ? (uint64_t)((const uint32_t *)src)[i] : ((const uint64_t *)src)[i] % sl.modulo - sl.bucket_begin;
        if (b >= sl.n_buckets) { *bad = 1; b = BY_NODE ? sl.n_buckets - 1 : 0; }
        keys[i] = (uint32_t)b;
        idx[i] = (uint32_t)i;
    }
}

// The (key, index) pairs as the items of gki_radix_tile.h's pass: two u32 arrays in memory, one 8-byte item (the key in its
// low half) in registers and LDS; tile offsets are 32 bits wide (fewer than 2^32 records)
struct PairItems {
    using Offset = uint32_t;
    const uint32_t *__restrict__ keys_in, *__restrict__ vals_in;
    uint32_t *__restrict__ keys_out, *__restrict__ vals_out;
    __device__ __forceinline__ uint64_t load_key(int64_t i) const { return keys_in[i]; }
    __device__ __forceinline__ uint64_t load(int64_t i) const { return (uint64_t)keys_in[i] | ((uint64_t)vals_in[i] << 32); }
    __device__ __forceinline__ void store(int64_t i, uint64_t item) const { keys_out[i] = (uint32_t)item; vals_out[i] = (uint32_t)(item >> 32); }
    static __device__ __forceinline__ uint32_t digit(uint64_t item, int shift) { return ((uint32_t)item >> shift) & 0xFF; }
};

// histogram of one 8-bit digit per tile, stored bin-major: hist[bin * n_tiles + tile]
__global__ __launch_bounds__(RB) void k_radix_hist(const uint32_t *__restrict__ keys, int64_t n, int shift,
                                                   uint32_t *__restrict__ hist, int64_t n_tiles) {
    radix_tile_hist<RB, RI>(PairItems{keys, nullptr, nullptr, nullptr}, n, shift, hist, n_tiles);
}

// stable scatter of one tile
__global__ __launch_bounds__(RB) void k_radix_scatter(const uint32_t *__restrict__ keys_in,
                                                      const uint32_t *__restrict__ vals_in, int64_t n, int shift,
                                                      const uint32_t *__restrict__ offs /* scanned hist */,
                                                      int64_t n_tiles, uint32_t *__restrict__ keys_out,
                                                      uint32_t *__restrict__ vals_out) {
    radix_tile_scatter<RB, RI>(PairItems{keys_in, vals_in, keys_out, vals_out}, n, shift, offs, n_tiles);
}

// Payload permutation.  Gathering four columns by a random index costs four random 64-byte sectors per record
// (measured: 30 ms of a 50 ms build at 3.2e8 records).  The columns are first packed into 32-byte rows (one
// streaming pass), so the random access is one sector per record; the permuted rows are unpacked into the output
// columns with coalesced stores.
// Q 16-byte words per row: (k-mer, ref offset) and, Q = 2, (node, allele frequency, -, -); the reverse index has the first only.
template <int Q>
__global__ __launch_bounds__(256) void k_pack_rows(RecordCols c, int64_t n, uint4 *__restrict__ rows) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t k = c.kmers[i], r = c.refs[i];
        rows[Q * i] = make_uint4((uint32_t)k, (uint32_t)(k >> 32), (uint32_t)r, (uint32_t)(r >> 32));
        if (Q == 2) rows[Q * i + 1] = make_uint4(c.nodes[i], c.af[i], 0u, 0u);
    }
}

template <int Q>
__global__ __launch_bounds__(256) void k_gather_rows(const uint32_t *__restrict__ idx, int64_t n, const uint4 *__restrict__ rows, RecordColsOut o) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t j = idx[i];
        const uint4 a = rows[Q * j], b = Q == 2 ? rows[Q * j + 1] : a;
        o.kmers[i] = ((uint64_t)a.y << 32) | a.x;
        o.refs[i] = ((uint64_t)a.w << 32) | a.z;
        if (Q == 2) { o.nodes[i] = b.x; o.af[i] = b.y; }
    }
}

// end of the run of equal keys starting at i (keys sorted): a short walk, then a binary search -- a k-mer repeated
// millions of times must not cost one lane millions of dependent loads
__device__ __forceinline__ int64_t run_end(const uint32_t *__restrict__ keys, int64_t n, int64_t i, uint32_t b) {
    int64_t e = i + 1;
    const int64_t walk_to = i + 16 < n ? i + 16 : n;
    while (e < walk_to && keys[e] == b) e++;
    if (e < walk_to || e == n) return e;
    int64_t lo = e, hi = n;                       // keys[lo-1] == b; first position with a larger key
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (keys[mid] == b) lo = mid + 1; else hi = mid; }
    return lo;
}

// bucket heads -> directory (collision_free_kmer_index.py:444-457).  A head lane finds the end of its run.
__global__ __launch_bounds__(256) void k_directory(const uint32_t *__restrict__ keys, int64_t n,
                                                   int32_t *__restrict__ hashes_to_index, uint32_t *__restrict__ n_kmers) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t b = keys[i];
        if (i > 0 && keys[i - 1] == b) continue;
        const int64_t e = run_end(keys, n, i, b);
        hashes_to_index[b] = (int32_t)i;
        n_kmers[b] = (uint32_t)(e - i);
    }
}

// set_frequencies (collision_free_kmer_index.py:267-293): for every record, the number of distinct
// ref_offsets among the records of its bucket that carry the same k-mer.  Buckets of up to
// SMALL_BUCKET records: one lane per record.  Larger buckets are queued for k_frequencies_large.
__global__ __launch_bounds__(256) void k_frequencies_small(const uint32_t *__restrict__ keys, int64_t n,
                                                           const int32_t *__restrict__ hashes_to_index,
                                                           const uint32_t *__restrict__ n_kmers,
                                                           const uint64_t *__restrict__ kmers, const uint64_t *__restrict__ refs,
                                                           uint16_t *__restrict__ freq, uint32_t *__restrict__ large_list,
                                                           unsigned int *__restrict__ n_large) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t b = keys[i];
        const int64_t s = hashes_to_index[b];
        const int64_t m = n_kmers[b];
        if (m > SMALL_BUCKET) {
            if (i == s) large_list[atomicAdd(n_large, 1u)] = b;
            continue;
        }
        const uint64_t km = kmers[i];
        int count = 0;
        for (int64_t j = s; j < s + m; j++) {
            if (kmers[j] != km) continue;
            const uint64_t r = refs[j];
            bool dup = false;
            for (int64_t c = s; c < j; c++) dup |= (kmers[c] == km && refs[c] == r);
            count += dup ? 0 : 1;
        }
        freq[i] = (uint16_t)count;            // uint16 as in :270
    }
}

struct Pair { uint64_t kmer, ref; };
__device__ __forceinline__ bool pair_less(const Pair &a, const Pair &b) {
    return a.kmer < b.kmer || (a.kmer == b.kmer && a.ref < b.ref);
}

// One block per large bucket: bitonic sort of its (kmer, ref_offset) pairs in a global scratch
// slice (padded to a power of two with max sentinels), then distinct counting per k-mer.
__global__ __launch_bounds__(256) void k_frequencies_large(const uint32_t *__restrict__ large_list, unsigned int n_large,
                                                           const int32_t *__restrict__ hashes_to_index,
                                                           const uint32_t *__restrict__ n_kmers,
                                                           const uint64_t *__restrict__ kmers, const uint64_t *__restrict__ refs,
                                                           const int64_t *__restrict__ scratch_start, Pair *__restrict__ scratch,
                                                           uint16_t *__restrict__ freq) {
    for (unsigned int li = blockIdx.x; li < n_large; li += gridDim.x) {
        const uint32_t b = large_list[li];
        const int64_t s = hashes_to_index[b];
        const int64_t m = n_kmers[b];
        Pair *p = scratch + scratch_start[li];
        int64_t cap = 1;
        while (cap < m) cap <<= 1;
        for (int64_t i = threadIdx.x; i < cap; i += blockDim.x) {
            Pair v;
            if (i < m) { v.kmer = kmers[s + i]; v.ref = refs[s + i]; } else { v.kmer = ~0ull; v.ref = ~0ull; }
            p[i] = v;
        }
        __syncthreads();
        for (int64_t size = 2; size <= cap; size <<= 1) {
            for (int64_t str = size >> 1; str > 0; str >>= 1) {
                for (int64_t t = threadIdx.x; t < (cap >> 1); t += blockDim.x) {
                    const int64_t lo = ((t / str) * (str << 1)) + (t % str);
                    const int64_t hi = lo + str;
                    const bool up = ((lo & size) == 0);
                    Pair a = p[lo], c = p[hi];
                    if (pair_less(c, a) == up) { p[lo] = c; p[hi] = a; }
                }
                __threadfence_block();
                __syncthreads();
            }
        }
        // every record: distinct refs among pairs with its kmer = (first position of kmer .. last), counting ref changes
        for (int64_t i = threadIdx.x; i < m; i += blockDim.x) {
            const uint64_t km = kmers[s + i];
            int64_t lo = 0, hi = m;                       // first pair with kmer >= km
            while (lo < hi) { int64_t mid = (lo + hi) >> 1; if (p[mid].kmer < km) lo = mid + 1; else hi = mid; }
            int64_t count = 0;
            uint64_t prev = 0;
            for (int64_t j = lo; j < m && p[j].kmer == km; j++) {
                if (j == lo || p[j].ref != prev) count++;
                prev = p[j].ref;
            }
            freq[s + i] = (uint16_t)count;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_large_sizes(const uint32_t *__restrict__ large_list, unsigned int n_large,
                                                     const uint32_t *__restrict__ n_kmers, uint32_t *__restrict__ sizes) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_large; i += gridDim.x * blockDim.x) {
        uint32_t m = n_kmers[large_list[i]], cap = 1;
        while (cap < m) cap <<= 1;
        sizes[i] = cap;
    }
}

// ------------------------------------------------------------------------------------ probe
struct IndexDev {
    const int32_t *h2i; const uint32_t *nk; const uint64_t *kmers; const uint32_t *nodes; const uint64_t *refs;
    const uint16_t *freq; const float *af; uint64_t modulo, bucket_begin, n_buckets;
};

// CollisionFreeKmerIndex.get (collision_free_kmer_index.py:303-315) for one query per lane.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_lookup(IndexDev ix, const uint64_t *__restrict__ queries, int64_t q, int64_t max_hits,
                                                uint32_t *__restrict__ cnt, const int64_t *__restrict__ hit_start,
                                                uint32_t *__restrict__ o_nodes, uint64_t *__restrict__ o_refs,
                                                int64_t *__restrict__ o_query, uint16_t *__restrict__ o_freq,
                                                float *__restrict__ o_af, int64_t *__restrict__ o_pos) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < q; i += stride) {
        const uint64_t km = queries[i];
        const uint64_t b = km % ix.modulo - ix.bucket_begin;          // :304 (slice-relative)
        const bool mine = b < ix.n_buckets;
        const int64_t s = mine ? ix.h2i[b] : 0;                       // :305
        const int64_t m = mine ? ix.nk[b] : 0;                        // :306
        if (!EMIT) {
            uint32_t c = 0;
            bool first = true, too_frequent = false;
            for (int64_t j = s; j < s + m; j++) {
                if (ix.kmers[j] != km) continue;                      // :309
                if (first) { too_frequent = ix.freq && (int64_t)ix.freq[j] > max_hits; first = false; }   // :312
                c++;
            }
            cnt[i] = too_frequent ? 0u : c;
        } else {
            int64_t o = hit_start[i];
            if (hit_start[i + 1] == o) continue;
            for (int64_t j = s; j < s + m; j++) {
                if (ix.kmers[j] != km) continue;
                if (o_nodes) o_nodes[o] = ix.nodes[j];                // :315
                if (o_refs) o_refs[o] = ix.refs[j];
                if (o_query) o_query[o] = i;                          // read_offsets = query index (:365)
                if (o_freq) o_freq[o] = ix.freq ? ix.freq[j] : (uint16_t)0;
                if (o_af) o_af[o] = ix.af[j];
                if (o_pos) o_pos[o] = j;
                o++;
            }
        }
    }
}

// kmer_mapper-style node counting fused with the probe (collision_free_kmer_index.py:210-212 map_kmers,
// CounterKmerIndex.get_node_counts :39-40): counts[node] += 1 for every hit of every query.
__global__ __launch_bounds__(256) void k_count_nodes(IndexDev ix, const uint64_t *__restrict__ queries, int64_t q, int64_t max_hits,
                                                     unsigned int *__restrict__ counts, int64_t n_counts) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < q; i += stride) {
        const uint64_t km = queries[i];
        const uint64_t b = km % ix.modulo - ix.bucket_begin;
        if (b >= ix.n_buckets) continue;
        const int64_t s = ix.h2i[b];
        const int64_t m = ix.nk[b];
        bool first = true;
        for (int64_t j = s; j < s + m; j++) {
            if (ix.kmers[j] != km) continue;
            if (first) { if (ix.freq && (int64_t)ix.freq[j] > max_hits) break; first = false; }
            const uint32_t node = ix.nodes[j];
            if ((int64_t)node < n_counts) atomicAdd(&counts[node], 1u);
        }
    }
}


// Stable LSD sort of (key, value) pairs on the low `bits` bits of the key; ping-pongs between the two
// buffers of each pair, *cur_out = index of the buffers holding the result.
static int radix_sort_pairs(uint32_t *keys[2], uint32_t *vals[2], int64_t n, int bits, uint32_t *hist, uint32_t *offs,
                            void *tmp, int64_t tmp_bytes, hipStream_t s, int *cur_out) {
    const int64_t n_tiles = ceil_div(n, RTILE);
    const int64_t hist_n = (int64_t)RBINS * n_tiles;
    int cur = 0;
    for (int shift = 0; shift < bits; shift += 8) {
        hipLaunchKernelGGL(k_radix_hist, dim3((unsigned)n_tiles), dim3(RB), 0, s, keys[cur], n, shift, hist, n_tiles);
        HIP_TRY(hipGetLastError());
        GKI_TRY(gki_scan_u32_to_u32(hist, hist_n, offs, tmp, tmp_bytes, s));
        hipLaunchKernelGGL(k_radix_scatter, dim3((unsigned)n_tiles), dim3(RB), 0, s, keys[cur], vals[cur], n, shift, offs,
                           n_tiles, keys[1 - cur], vals[1 - cur]);
        HIP_TRY(hipGetLastError());
        cur = 1 - cur;
    }
    *cur_out = cur;
    return GKI_OK;
}

// The scratch of radix_sort_pairs over n pairs, allocated in this order: keys[0], vals[0], keys[1], vals[1], the tiles'
// histograms, their offsets, the scan's temporary.
struct SortScratch {
    DevBuf kv[4], hist_b, offs_b, tmp_b;
    uint32_t *keys[2] = {nullptr, nullptr}, *vals[2] = {nullptr, nullptr}, *hist = nullptr, *offs = nullptr;
    int64_t tmp_bytes = 0;
    int alloc(int64_t n) {
        for (DevBuf &b : kv) HIP_TRY(b.alloc((size_t)n * 4));
        const int64_t hist_n = (int64_t)RBINS * ceil_div(n, RTILE);
        tmp_bytes = gki_scan_tmp_bytes(hist_n);
        HIP_TRY(hist_b.alloc((size_t)hist_n * 4));
        HIP_TRY(offs_b.alloc((size_t)(hist_n + 1) * 4));
        HIP_TRY(tmp_b.alloc((size_t)tmp_bytes));
        keys[0] = kv[0].get<uint32_t>(); vals[0] = kv[1].get<uint32_t>(); keys[1] = kv[2].get<uint32_t>(); vals[1] = kv[3].get<uint32_t>();
        hist = hist_b.get<uint32_t>(); offs = offs_b.get<uint32_t>();
        return GKI_OK;
    }
    int sort(int64_t n, int bits, hipStream_t s, int *cur) { return radix_sort_pairs(keys, vals, n, bits, hist, offs, tmp_b.get(), tmp_bytes, s, cur); }
};

// FlatKmers.get_new_without_singletons (flat_kmers.py:98-125): a record is kept iff an EARLIER record carries the same
// hash.  After the stable sort by bucket the records of a bucket are in input order, so "earlier" = an earlier position
// of the bucket's run; the flag goes back to the record's original position.
__global__ __launch_bounds__(256) void k_flag_repeats(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ perm,
                                                      const uint64_t *__restrict__ kmers, int64_t n,
                                                      const int32_t *__restrict__ first_of_bucket, uint8_t *__restrict__ flags) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const uint32_t me = perm[p];
        const uint64_t km = kmers[me];
        bool seen = false;
        for (int64_t j = first_of_bucket[keys[p]]; j < p && !seen; j++) seen = kmers[perm[j]] == km;
        flags[me] = seen ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------ reverse index
// ReverseKmerIndex.from_flat_kmers (reverse_kmer_index.py:47-60): records stably sorted by node,
// nodes_to_index_positions[node] = first record (uint32), nodes_to_n_hashes[node] = run length (uint16, wraps
// like the NumPy assignment at :56).
// n_hashes of the reverse index is uint16 (the NumPy assignment at reverse_kmer_index.py:56 stores the count modulo 2^16)
__global__ __launch_bounds__(256) void k_narrow_counts(const uint32_t *__restrict__ in, int64_t n, uint16_t *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (uint16_t)in[i];
}

// Node directory of the reverse index, two streaming passes and no search: PASS 0 -- the head of a run records where the
// node's records start; PASS 1 (launched after it) -- the tail of a run records how many there are.  A node has tens of
// records, so "the head lane finds the end of its run" (run_end: 16 steps, then a binary search over the rest of the
// array, ~28 dependent loads across 1.2 GB) took 12.5 ms of the 27 ms build on 3.1e8 records.
template <int PASS>
__global__ __launch_bounds__(256) void k_node_directory(const uint32_t *__restrict__ keys, int64_t n,
                                                        uint32_t *__restrict__ first, uint16_t *__restrict__ count) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t b = keys[i];
        if (PASS == 0) {
            if (i == 0 || keys[i - 1] != b) first[b] = (uint32_t)i;
        } else {
            if (i == n - 1 || keys[i + 1] != b) count[b] = (uint16_t)(i + 1 - (int64_t)first[b]);   // mod 2^16, reverse_kmer_index.py:56
        }
    }
}

}  // namespace

// Frequencies of the buckets in large_list (more than SMALL_BUCKET records each): sizes -> scratch offsets -> one block
// per bucket.  `sizes` is scratch for n_large uint32.
static int frequencies_large_pass(const uint32_t *large_list, unsigned int n_large, uint32_t *sizes, const IndexOut &out, hipStream_t s) {
    hipLaunchKernelGGL(k_large_sizes, dim3(stream_grid(n_large, 256)), dim3(256), 0, s, large_list, n_large, out.n_kmers, sizes);
    HIP_TRY(hipGetLastError());
    const int64_t tmp2_bytes = gki_scan_tmp_bytes(n_large);
    DevBuf starts, tmp2, scratch;
    HIP_TRY(starts.alloc(((size_t)n_large + 1) * 8));
    HIP_TRY(tmp2.alloc((size_t)tmp2_bytes));
    GKI_TRY(gki_scan_u32_to_i64(sizes, n_large, starts.get<int64_t>(), tmp2.get(), tmp2_bytes, s));
    int64_t total = 0;
    HIP_TRY(hipMemcpy(&total, starts.get<int64_t>() + n_large, 8, hipMemcpyDeviceToHost));
    HIP_TRY(scratch.alloc((size_t)total * sizeof(Pair)));
    const unsigned grid = n_large < 2048 ? n_large : 2048;
    hipLaunchKernelGGL(k_frequencies_large, dim3(grid), dim3(256), 0, s, large_list, n_large, out.h2i, out.n_kmers, out.cols.kmers,
                       out.cols.refs, starts.get<const int64_t>(), scratch.get<Pair>(), out.freq);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return GKI_OK;
}

// The frequency pass of the row-carrying form (gki_index_rows.hip) for the rows it left open: ranges [begin, end) of the
// finished columns, each a whole number of buckets.  Same rule as k_frequencies_small, the bucket recomputed from the
// k-mer.
__global__ __launch_bounds__(256) void k_frequencies_ranges(const int64_t *__restrict__ rb, const int64_t *__restrict__ re, int n_ranges,
                                                            uint64_t modulo, uint64_t bucket_begin,
                                                            const int32_t *__restrict__ hashes_to_index, const uint32_t *__restrict__ n_kmers,
                                                            const uint64_t *__restrict__ kmers, const uint64_t *__restrict__ refs,
                                                            uint16_t *__restrict__ freq, uint32_t *__restrict__ large_list,
                                                            unsigned int *__restrict__ n_large) {
    for (int q = blockIdx.x; q < n_ranges; q += gridDim.x) {
        for (int64_t i = rb[q] + threadIdx.x; i < re[q]; i += blockDim.x) {
            const uint64_t km = kmers[i];
            const uint64_t b = km % modulo - bucket_begin;
            const int64_t s = hashes_to_index[b];
            const int64_t m = n_kmers[b];
            if (m > SMALL_BUCKET) {
                if (i == s) large_list[atomicAdd(n_large, 1u)] = (uint32_t)b;
                continue;
            }
            int count = 0;
            for (int64_t j = s; j < s + m; j++) {
                if (kmers[j] != km) continue;
                const uint64_t r = refs[j];
                bool dup = false;
                for (int64_t c = s; c < j; c++) dup |= (kmers[c] == km && refs[c] == r);
                count += dup ? 0 : 1;
            }
            freq[i] = (uint16_t)count;
        }
    }
}

int gki_frequencies_for_rows(const int64_t *d_row_begin, const int64_t *d_row_end, int n_ranges, const Slice &slice,
                             const IndexOut &out, int64_t n, hipStream_t s) {
    if (n_ranges <= 0) return GKI_OK;
    const size_t cap = (size_t)(n / SMALL_BUCKET + 1);
    DevBuf large_list, sizes, n_large_d;
    HIP_TRY(large_list.alloc(cap * 4));
    HIP_TRY(sizes.alloc(cap * 4));
    HIP_TRY(n_large_d.alloc(16));
    HIP_TRY(hipMemsetAsync(n_large_d.get(), 0, 4, s));
    hipLaunchKernelGGL(k_frequencies_ranges, dim3(n_ranges < 4096 ? n_ranges : 4096), dim3(256), 0, s, d_row_begin, d_row_end,
                       n_ranges, slice.modulo, slice.bucket_begin, out.h2i, out.n_kmers, out.cols.kmers, out.cols.refs, out.freq,
                       large_list.get<uint32_t>(), n_large_d.get<unsigned int>());
    HIP_TRY(hipGetLastError());
    unsigned int n_large = 0;
    HIP_TRY(hipMemcpyAsync(&n_large, n_large_d.get(), 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (n_large > 0) GKI_TRY(frequencies_large_pass(large_list.get<uint32_t>(), n_large, sizes.get<uint32_t>(), out, s));
    return GKI_OK;
}

// ------------------------------------------------------------------------------------ host layer of the entry points
static IndexOut index_out(void *h2i, void *n_kmers, void *kmers, void *nodes, void *refs, void *af, void *freq, void *perm) {
    return {(int32_t *)h2i, (uint32_t *)n_kmers, record_cols_out(kmers, nodes, refs, af), (uint16_t *)freq, (uint32_t *)perm};
}

// a build's slice of the buckets, its grouping (where the entry point takes one) and the int32 directory's limit
static int check_slice_args(const Slice &sl, int64_t n, const Grouping *gr = nullptr) {
    if (sl.modulo == 0 || sl.modulo > 0xFFFFFFFFull) return gki_set_error(GKI_ERR_BAD_ARG, "modulo must be in 1..2^32-1");
    if (sl.n_buckets == 0 || sl.bucket_begin + sl.n_buckets > sl.modulo)
        return gki_set_error(GKI_ERR_BAD_ARG, "bucket range [%llu, +%llu) outside [0, modulo)", (unsigned long long)sl.bucket_begin,
                             (unsigned long long)sl.n_buckets);
    if (gr && (gr->group_bits < 0 || gr->group_bits > 10 || (gr->group_bits > 0 && !gr->h_group_start)))
        return gki_set_error(GKI_ERR_BAD_ARG, "group_bits must be in 0..10, with the group bounds when > 0");
    if (n >= (1ll << 31))
        return gki_set_error(GKI_ERR_OVERFLOW, "%lld records: the reference's directory is int32 "
                             "(collision_free_kmer_index.py:453); shard the build", (long long)n);
    return GKI_OK;
}

static int check_part_args(const PartSpec &sp) {
    if (sp.modulo == 0 || sp.modulo > 0xFFFFFFFFull) return gki_set_error(GKI_ERR_BAD_ARG, "modulo must be in 1..2^32-1");
    if (sp.n_parts < 1 || sp.n_parts > 256) return gki_set_error(GKI_ERR_BAD_ARG, "n_parts must be in 1..256");
    if (sp.sub_bits < 0 || (sp.n_parts << sp.sub_bits) > 1024) return gki_set_error(GKI_ERR_BAD_ARG, "n_parts << group_bits must not exceed 1024");
    return GKI_OK;
}

// The front of the pair-sorting form: the key of every record (BY_NODE: its node id, else its bucket in `sl`) with the
// identity permutation, stably sorted by key: sorted keys in ss.keys[*cur], sorted permutation in ss.vals[*cur].
// h_bad (may be NULL: no key can lie outside): read back before the sort, set = a key outside the slice; nothing is
// sorted then and the caller words the refusal.
template <bool BY_NODE>
static int sort_by_key(SortScratch &ss, const void *d_src, int64_t n, const Slice &sl, hipStream_t s, int *cur, int *h_bad) {
    GKI_TRY(ss.alloc(n));
    int *bad = (int *)ss.hist;                    // hist is not in use yet
    HIP_TRY(hipMemsetAsync(bad, 0, 4, s));
    hipLaunchKernelGGL(k_sort_keys<BY_NODE>, dim3(stream_grid(n, 256)), dim3(256), 0, s, d_src, n, sl, ss.keys[0], ss.vals[0], bad);
    HIP_TRY(hipGetLastError());
    if (h_bad) {
        HIP_TRY(hipMemcpyAsync(h_bad, bad, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (*h_bad) return GKI_OK;
    }
    return ss.sort(n, key_bits(sl.n_buckets - 1), s, cur);
}

// The payload permuted by the sorted index through rows of Q 16-byte words (k_pack_rows).  rows_b is the caller's: its free
// waits for the device and belongs at the caller's end.
template <int Q>
static int permute_payload(DevBuf &rows_b, const RecordCols &c, const uint32_t *perm, int64_t n, const RecordColsOut &o, hipStream_t s) {
    HIP_TRY(rows_b.alloc((size_t)n * 16 * Q));
    hipLaunchKernelGGL(k_pack_rows<Q>, dim3(stream_grid(n, 256)), dim3(256), 0, s, c, n, rows_b.get<uint4>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_gather_rows<Q>, dim3(stream_grid(n, 256)), dim3(256), 0, s, perm, n, rows_b.get<const uint4>(), o);
    HIP_TRY(hipGetLastError());
    return GKI_OK;
}

// the pair-sorting form of the build (arguments checked by the caller)
static int build_pairs(const RecordCols &cols, int64_t n, const Slice &sl, int skip_frequencies, const IndexOut &out) {
    hipStream_t s = 0;
    HIP_TRY(hipMemsetAsync(out.h2i, 0, (size_t)sl.n_buckets * 4, s));              // :453
    HIP_TRY(hipMemsetAsync(out.n_kmers, 0, (size_t)sl.n_buckets * 4, s));          // :456
    if (n <= 0) { HIP_TRY(hipStreamSynchronize(s)); return GKI_OK; }
    HIP_TRY(hipMemsetAsync(out.freq, 0, (size_t)n * 2, s));                        // :270
    SortScratch ss;
    DevBuf rows_b;
    int cur = 0, h_bad = 0;
    GKI_TRY(sort_by_key<false>(ss, cols.kmers, n, sl, s, &cur, sl.n_buckets != sl.modulo ? &h_bad : nullptr));
    if (h_bad) return gki_set_error(GKI_ERR_BAD_ARG, "a record's bucket lies outside [%llu, +%llu)",
                                    (unsigned long long)sl.bucket_begin, (unsigned long long)sl.n_buckets);
    uint32_t **keys = ss.keys, **vals = ss.vals;
    GKI_TRY(permute_payload<2>(rows_b, cols, vals[cur], n, out.cols, s));
    if (out.perm) HIP_TRY(hipMemcpyAsync(out.perm, vals[cur], (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_directory, dim3(stream_grid(n, 256)), dim3(256), 0, s, keys[cur], n, out.h2i, out.n_kmers);
    HIP_TRY(hipGetLastError());
    if (!skip_frequencies) {
        // large-bucket work list: at most n / SMALL_BUCKET entries; reuse the spare key/val buffers
        uint32_t *large_list = keys[1 - cur];
        unsigned int *n_large_d = (unsigned int *)ss.hist;
        HIP_TRY(hipMemsetAsync(n_large_d, 0, 4, s));
        hipLaunchKernelGGL(k_frequencies_small, dim3(stream_grid(n, 256)), dim3(256), 0, s, keys[cur], n, out.h2i, out.n_kmers,
                           out.cols.kmers, out.cols.refs, out.freq, large_list, n_large_d);
        HIP_TRY(hipGetLastError());
        unsigned int n_large = 0;
        HIP_TRY(hipMemcpyAsync(&n_large, n_large_d, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (n_large > 0) GKI_TRY(frequencies_large_pass(large_list, n_large, vals[1 - cur], out, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return GKI_OK;
}

// The row-carrying form (gki_index_rows.hip); the pair-sorting form takes over for inputs outside its domain (it sorts on
// the whole key: a grouping of the input is of no use to it and does no harm)
static int build_range(const RecordCols &cols, int64_t n, const Slice &sl, const Grouping &gr, int skip_frequencies, const IndexOut &out) {
    GKI_TRY(check_slice_args(sl, n, &gr));
    if (n > 0) {
        const int r = gki_index_build_rows(cols, RowsIn{}, n, sl, gr, skip_frequencies, 0, out);
        if (r != GKI_NOT_BUILT) return r;
    }
    return build_pairs(cols, n, sl, skip_frequencies, out);
}

// (arguments checked by the caller)
static int partition(const RecordCols &cols, int64_t n, const PartSpec &sp, const RecordColsOut &out_cols, const RowsOut &out_rows,
                     int64_t *h_start) {
    for (int p = 0; p <= (sp.n_parts << sp.sub_bits); p++) h_start[p] = 0;
    if (n <= 0) return GKI_OK;
    // stable passes of the row-carrying build's partition kernel (gki_index_rows.hip)
    return gki_partition_columns_by_part(cols, n, sp, out_cols, out_rows, h_start);
}

extern "C" {

int gki_index_build_pairs(const void *d_kmers, const void *d_nodes, const void *d_ref_offsets, const void *d_af32, int64_t n,
                          uint64_t modulo, uint64_t bucket_begin, uint64_t n_buckets, int skip_frequencies,
                          void *d_hashes_to_index, void *d_n_kmers, void *d_out_kmers, void *d_out_nodes,
                          void *d_out_ref_offsets, void *d_out_af32, void *d_out_frequencies, void *d_out_permutation) {
    const Slice sl = {modulo, bucket_begin, n_buckets};
    GKI_TRY(check_slice_args(sl, n));
    return build_pairs(record_cols(d_kmers, d_nodes, d_ref_offsets, d_af32), n, sl, skip_frequencies,
                       index_out(d_hashes_to_index, d_n_kmers, d_out_kmers, d_out_nodes, d_out_ref_offsets, d_out_af32, d_out_frequencies,
                                 d_out_permutation));
}

int gki_index_build_range_grouped(const void *d_kmers, const void *d_nodes, const void *d_ref_offsets, const void *d_af32, int64_t n,
                                  uint64_t modulo, uint64_t bucket_begin, uint64_t n_buckets, int skip_frequencies,
                                  int group_bits, const int64_t *h_group_start,
                                  void *d_hashes_to_index, void *d_n_kmers, void *d_out_kmers, void *d_out_nodes,
                                  void *d_out_ref_offsets, void *d_out_af32, void *d_out_frequencies, void *d_out_permutation) {
    return build_range(record_cols(d_kmers, d_nodes, d_ref_offsets, d_af32), n, {modulo, bucket_begin, n_buckets}, {group_bits, h_group_start},
                       skip_frequencies,
                       index_out(d_hashes_to_index, d_n_kmers, d_out_kmers, d_out_nodes, d_out_ref_offsets, d_out_af32, d_out_frequencies,
                                 d_out_permutation));
}

int gki_index_build_range(const void *d_kmers, const void *d_nodes, const void *d_ref_offsets, const void *d_af32, int64_t n,
                          uint64_t modulo, uint64_t bucket_begin, uint64_t n_buckets, int skip_frequencies,
                          void *d_hashes_to_index, void *d_n_kmers, void *d_out_kmers, void *d_out_nodes,
                          void *d_out_ref_offsets, void *d_out_af32, void *d_out_frequencies, void *d_out_permutation) {
    return build_range(record_cols(d_kmers, d_nodes, d_ref_offsets, d_af32), n, {modulo, bucket_begin, n_buckets}, {0, nullptr}, skip_frequencies,
                       index_out(d_hashes_to_index, d_n_kmers, d_out_kmers, d_out_nodes, d_out_ref_offsets, d_out_af32, d_out_frequencies,
                                 d_out_permutation));
}

int gki_index_build(const void *d_kmers, const void *d_nodes, const void *d_ref_offsets, const void *d_af32, int64_t n,
                    uint64_t modulo, int skip_frequencies, void *d_hashes_to_index, void *d_n_kmers, void *d_out_kmers,
                    void *d_out_nodes, void *d_out_ref_offsets, void *d_out_af32, void *d_out_frequencies,
                    void *d_out_permutation) {
    return build_range(record_cols(d_kmers, d_nodes, d_ref_offsets, d_af32), n, {modulo, 0, modulo}, {0, nullptr}, skip_frequencies,
                       index_out(d_hashes_to_index, d_n_kmers, d_out_kmers, d_out_nodes, d_out_ref_offsets, d_out_af32, d_out_frequencies,
                                 d_out_permutation));
}

int gki_partition_by_bucket_range_grouped(const void *d_kmers, const void *d_nodes, const void *d_ref_offsets, const void *d_af32,
                                          int64_t n, uint64_t modulo, int n_parts, int group_bits, int64_t max_rows_per_pass,
                                          void *d_out_kmers, void *d_out_nodes, void *d_out_ref_offsets, void *d_out_af32,
                                          int64_t *h_start) {
    const PartSpec sp = {modulo, n_parts, group_bits, max_rows_per_pass};
    GKI_TRY(check_part_args(sp));
    return partition(record_cols(d_kmers, d_nodes, d_ref_offsets, d_af32), n, sp,
                     record_cols_out(d_out_kmers, d_out_nodes, d_out_ref_offsets, d_out_af32), RowsOut{}, h_start);
}

int gki_partition_rows_by_bucket_range(const void *d_kmers, const void *d_nodes, const void *d_ref_offsets, const void *d_af32,
                                       int64_t n, uint64_t modulo, int n_parts, int group_bits, int64_t max_rows_per_pass,
                                       void *d_rows, void *d_keys, int64_t *h_start) {
    const PartSpec sp = {modulo, n_parts, group_bits, max_rows_per_pass};
    GKI_TRY(check_part_args(sp));
    if (!d_rows || !d_keys) return gki_set_error(GKI_ERR_BAD_ARG, "rows and keys buffers are needed");
    return partition(record_cols(d_kmers, d_nodes, d_ref_offsets, d_af32), n, sp, RecordColsOut{}, {(uint64_t *)d_rows, (uint32_t *)d_keys}, h_start);
}

int gki_index_build_range_from_rows(const void *d_rows, const void *d_keys, int64_t n, uint64_t modulo, uint64_t bucket_begin,
                                    uint64_t n_buckets, int skip_frequencies, int group_bits, const int64_t *h_group_start,
                                    void *d_hashes_to_index, void *d_n_kmers, void *d_out_kmers, void *d_out_nodes,
                                    void *d_out_ref_offsets, void *d_out_af32, void *d_out_frequencies) {
    const Slice sl = {modulo, bucket_begin, n_buckets};
    const Grouping gr = {group_bits, h_group_start};
    GKI_TRY(check_slice_args(sl, n, &gr));
    hipStream_t s = 0;
    if (n <= 0) {
        HIP_TRY(hipMemsetAsync(d_hashes_to_index, 0, (size_t)n_buckets * 4, s));       // :453
        HIP_TRY(hipMemsetAsync(d_n_kmers, 0, (size_t)n_buckets * 4, s));               // :456
        HIP_TRY(hipStreamSynchronize(s));
        return GKI_OK;
    }
    if (!d_rows || !d_keys) return gki_set_error(GKI_ERR_BAD_ARG, "rows and keys are needed");
    const int r = gki_index_build_rows(RecordCols{}, {(const uint64_t *)d_rows, (const uint32_t *)d_keys}, n, sl, gr, skip_frequencies, 0,
                                       index_out(d_hashes_to_index, d_n_kmers, d_out_kmers, d_out_nodes, d_out_ref_offsets, d_out_af32,
                                                 d_out_frequencies, nullptr));
    if (r == GKI_NOT_BUILT)
        return gki_set_error(GKI_ERR_OUT_OF_DOMAIN, "the records are outside the row-carrying build's domain (a group of neighbouring buckets with "
                             "more than 2^22 records): build this slice from its columns (gki_index_build_range)");
    return r;
}

int gki_partition_by_bucket_range_chunked(const void *d_kmers, const void *d_nodes, const void *d_ref_offsets, const void *d_af32,
                                          int64_t n, uint64_t modulo, int n_parts, int64_t max_rows_per_pass, void *d_out_kmers,
                                          void *d_out_nodes, void *d_out_ref_offsets, void *d_out_af32, int64_t *h_part_start) {
    return gki_partition_by_bucket_range_grouped(d_kmers, d_nodes, d_ref_offsets, d_af32, n, modulo, n_parts, 0, max_rows_per_pass,
                                                 d_out_kmers, d_out_nodes, d_out_ref_offsets, d_out_af32, h_part_start);
}

int gki_partition_by_bucket_range(const void *d_kmers, const void *d_nodes, const void *d_ref_offsets, const void *d_af32,
                                  int64_t n, uint64_t modulo, int n_parts, void *d_out_kmers, void *d_out_nodes,
                                  void *d_out_ref_offsets, void *d_out_af32, int64_t *h_part_start) {
    return gki_partition_by_bucket_range_grouped(d_kmers, d_nodes, d_ref_offsets, d_af32, n, modulo, n_parts, 0, 0, d_out_kmers,
                                                 d_out_nodes, d_out_ref_offsets, d_out_af32, h_part_start);
}

int gki_flag_repeated_kmers(const void *d_kmers, int64_t n, void *d_flags) {
    if (n <= 0) return GKI_OK;
    if (n >= (1ll << 31)) return gki_set_error(GKI_ERR_OVERFLOW, "%lld records: at most 2^31-1 at a time", (long long)n);
    // a bucket table about twice as large as the input keeps the runs short; its size only has to be odd-ish
    uint64_t modulo = (uint64_t)n * 2 + 1;
    if (modulo > 0xFFFFFFFBull) modulo = 0xFFFFFFFBull;
    hipStream_t s = 0;
    SortScratch ss;
    DevBuf first, cnt;
    int cur = 0;
    GKI_TRY(sort_by_key<false>(ss, d_kmers, n, {modulo, 0, modulo}, s, &cur, nullptr));
    HIP_TRY(first.alloc((size_t)modulo * 4));
    HIP_TRY(cnt.alloc((size_t)modulo * 4));
    hipLaunchKernelGGL(k_directory, dim3(stream_grid(n, 256)), dim3(256), 0, s, ss.keys[cur], n, first.get<int32_t>(), cnt.get<uint32_t>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_flag_repeats, dim3(stream_grid(n, 256)), dim3(256), 0, s, ss.keys[cur], ss.vals[cur],
                       (const uint64_t *)d_kmers, n, first.get<const int32_t>(), (uint8_t *)d_flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return GKI_OK;
}

int gki_reverse_index_build(const void *d_nodes, const void *d_kmers, const void *d_ref_offsets, int64_t n, int64_t n_nodes,
                            void *d_index_positions, void *d_n_hashes, void *d_out_kmers, void *d_out_ref_offsets) {
    if (n_nodes <= 0 || n_nodes > (1ll << 32)) return gki_set_error(GKI_ERR_BAD_ARG, "n_nodes must be in 1..2^32");
    if (n >= (1ll << 32)) return gki_set_error(GKI_ERR_OVERFLOW, "%lld records do not fit the uint32 directory", (long long)n);
    hipStream_t s = 0;
    const RecordCols cols = record_cols(d_kmers, d_nodes, d_ref_offsets, nullptr);
    const RecordColsOut out_cols = record_cols_out(d_out_kmers, nullptr, d_out_ref_offsets, nullptr);
    const Slice nodes = {1, 0, (uint64_t)n_nodes};            // the "buckets" are the nodes
    // GKI_REVERSE_FORM=pairs (read per call): the pair-sorting form, for the parity tests of the path behind the row form
    const char *form = getenv("GKI_REVERSE_FORM");
    const bool pairs_only = form && strcmp(form, "pairs") == 0;
    if (!pairs_only && n > 0 && n < (1ll << 31) && n_nodes < (1ll << 32)) {
        // the row-carrying form (gki_index_rows.hip) with the node id as the key: the payload travels with its key through the
        // staged partition passes and the in-LDS finish leaves the node directory as it goes -- no gather, no separate
        // directory passes (round 4; the pair-sorting form below stays for what lies outside its domain)
        DevBuf nk32;
        HIP_TRY(nk32.alloc((size_t)n_nodes * 4));
        const int r = gki_index_build_rows(cols, RowsIn{}, n, nodes, Grouping{}, 1, 1,
                                           {(int32_t *)d_index_positions, nk32.get<uint32_t>(), out_cols, nullptr, nullptr});
        if (r == GKI_OK) {
            hipLaunchKernelGGL(k_narrow_counts, dim3(stream_grid(n_nodes, 256)), dim3(256), 0, s, nk32.get<const uint32_t>(), n_nodes,
                               (uint16_t *)d_n_hashes);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(s));
        }
        if (r != GKI_NOT_BUILT) return r;
    }                                                 // (nk32 is freed before the pair-sorting form allocates)
    HIP_TRY(hipMemsetAsync(d_index_positions, 0, (size_t)n_nodes * 4, s));      // reverse_kmer_index.py:53
    HIP_TRY(hipMemsetAsync(d_n_hashes, 0, (size_t)n_nodes * 2, s));             // :54
    if (n <= 0) { HIP_TRY(hipStreamSynchronize(s)); return GKI_OK; }
    SortScratch ss;
    DevBuf rows;
    int cur = 0, h_bad = 0;
    GKI_TRY(sort_by_key<true>(ss, d_nodes, n, nodes, s, &cur, &h_bad));
    if (h_bad) return gki_set_error(GKI_ERR_BAD_ARG, "a record's node id is not below n_nodes = %lld", (long long)n_nodes);
    GKI_TRY(permute_payload<1>(rows, cols, ss.vals[cur], n, out_cols, s));
    hipLaunchKernelGGL(k_node_directory<0>, dim3(stream_grid(n, 256)), dim3(256), 0, s, ss.keys[cur], n,
                       (uint32_t *)d_index_positions, (uint16_t *)d_n_hashes);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_node_directory<1>, dim3(stream_grid(n, 256)), dim3(256), 0, s, ss.keys[cur], n,
                       (uint32_t *)d_index_positions, (uint16_t *)d_n_hashes);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return GKI_OK;
}

static IndexDev view_of(const gki_index_view *ix) {
    IndexDev d;
    d.h2i = (const int32_t *)ix->d_hashes_to_index; d.nk = (const uint32_t *)ix->d_n_kmers;
    d.kmers = (const uint64_t *)ix->d_kmers; d.nodes = (const uint32_t *)ix->d_nodes;
    d.refs = (const uint64_t *)ix->d_ref_offsets; d.freq = (const uint16_t *)ix->d_frequencies;
    d.af = (const float *)ix->d_af32; d.modulo = ix->modulo;
    d.bucket_begin = ix->n_buckets ? ix->bucket_begin : 0; d.n_buckets = ix->n_buckets ? ix->n_buckets : ix->modulo;
    return d;
}

int gki_index_count_nodes(const gki_index_view *ix, const void *d_queries, int64_t q, int64_t max_hits, void *d_counts,
                          int64_t n_counts) {
    if (ix->modulo == 0) return gki_set_error(GKI_ERR_BAD_ARG, "modulo is 0");
    if (q <= 0) return GKI_OK;
    hipLaunchKernelGGL(k_count_nodes, dim3(stream_grid(q, 256)), dim3(256), 0, 0, view_of(ix), (const uint64_t *)d_queries, q,
                       max_hits, (unsigned int *)d_counts, n_counts);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

int gki_index_lookup_count(const gki_index_view *ix, const void *d_queries, int64_t q, int64_t max_hits, void *d_hit_start,
                           int64_t *n_hits) {
    *n_hits = 0;
    if (ix->modulo == 0) return gki_set_error(GKI_ERR_BAD_ARG, "modulo is 0");
    if (q <= 0) { HIP_TRY(hipMemset(d_hit_start, 0, 8)); return GKI_OK; }
    int64_t tmp_bytes = gki_scan_tmp_bytes(q);
    DevBuf cnt, tmp;
    HIP_TRY(cnt.alloc((size_t)q * 4));
    HIP_TRY(tmp.alloc((size_t)tmp_bytes));
    hipLaunchKernelGGL(k_lookup<false>, dim3(stream_grid(q, 256)), dim3(256), 0, 0, view_of(ix), (const uint64_t *)d_queries, q,
                       max_hits, cnt.get<uint32_t>(), (const int64_t *)nullptr, (uint32_t *)nullptr, (uint64_t *)nullptr, (int64_t *)nullptr,
                       (uint16_t *)nullptr, (float *)nullptr, (int64_t *)nullptr);
    if (hipGetLastError() != hipSuccess) return gki_set_error(GKI_ERR_HIP, "k_lookup launch failed");
    GKI_TRY(gki_scan_u32_to_i64(cnt.get<const uint32_t>(), q, (int64_t *)d_hit_start, tmp.get(), tmp_bytes, 0));
    int64_t total = 0;
    HIP_TRY(hipMemcpy(&total, (const int64_t *)d_hit_start + q, 8, hipMemcpyDeviceToHost));
    *n_hits = total;
    return GKI_OK;
}

int gki_index_lookup_emit(const gki_index_view *ix, const void *d_queries, int64_t q, int64_t max_hits, const void *d_hit_start,
                          void *d_hit_nodes, void *d_hit_ref_offsets, void *d_hit_query, void *d_hit_frequencies,
                          void *d_hit_af32, void *d_hit_position) {
    if (q <= 0) return GKI_OK;
    hipLaunchKernelGGL(k_lookup<true>, dim3(stream_grid(q, 256)), dim3(256), 0, 0, view_of(ix), (const uint64_t *)d_queries, q,
                       max_hits, (uint32_t *)nullptr, (const int64_t *)d_hit_start, (uint32_t *)d_hit_nodes,
                       (uint64_t *)d_hit_ref_offsets, (int64_t *)d_hit_query, (uint16_t *)d_hit_frequencies, (float *)d_hit_af32,
                       (int64_t *)d_hit_position);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------ scalar get
// CollisionFreeKmerIndex.get (collision_free_kmer_index.py:303-315) for a handful of k-mers: one launch, one wave per
// query, queries and results in pinned host memory the kernel reads and writes directly -- no staging copies, no
// second pass.  A query's hits (positions in the payload arrays, bucket order) land in its own `cap`-sized segment.
namespace {
constexpr int SMALL_Q = 64;                 // queries per call
constexpr int SMALL_CAP = 1024;             // hits kept per query (more: the count says so and the caller goes batched)
struct SmallStage {                         // pinned, device-mapped
    uint64_t query[SMALL_Q];
    int64_t n_hits[SMALL_Q];
    int64_t pos[SMALL_Q * SMALL_CAP];
};
__global__ __launch_bounds__(64) void k_get_small(IndexDev ix, SmallStage *st, int64_t max_hits) {
    const int qi = blockIdx.x, lane = threadIdx.x;
    const uint64_t km = st->query[qi];
    const uint64_t b = km % ix.modulo - ix.bucket_begin;                  // :304
    int64_t total = 0;
    if (b < ix.n_buckets) {
        const int64_t s = ix.h2i[b], m = ix.nk[b];                        // :305-306
        bool first = true;
        for (int64_t j0 = 0; j0 < m; j0 += 64) {
            const int64_t j = s + j0 + lane;
            const bool hit = j0 + lane < m && ix.kmers[j] == km;          // :309
            const uint64_t mask = __ballot(hit);
            if (mask == 0) continue;
            if (first) {                                                  // :312 frequency of the FIRST hit
                const int64_t jf = s + j0 + (__ffsll((unsigned long long)mask) - 1);
                if (ix.freq && (int64_t)ix.freq[jf] > max_hits) { total = 0; break; }
                first = false;
            }
            if (hit) {
                const int64_t o = total + __popcll(mask & ((1ull << lane) - 1ull));
                if (o < SMALL_CAP) st->pos[(int64_t)qi * SMALL_CAP + o] = j;
            }
            total += __popcll(mask);
        }
    }
    if (lane == 0) st->n_hits[qi] = total;
}
std::mutex g_small_mu;
SmallStage *g_small_host = nullptr;         // pinned + portable: every device maps it; its device address is asked for per call.
                                            // 0.5 MB for the life of the process: freeing it from a static destructor would call
                                            // into a HIP runtime that may already be gone
}  // namespace

extern "C" int gki_index_get_small(const gki_index_view *ix, const uint64_t *h_queries, int q, int64_t max_hits,
                                   int64_t *h_n_hits, int64_t *h_positions, int64_t capacity_per_query) {
    if (q < 0 || q > SMALL_Q) return gki_set_error(GKI_ERR_BAD_ARG, "get_small: 0..%d queries per call", SMALL_Q);
    if (capacity_per_query < 0) return gki_set_error(GKI_ERR_BAD_ARG, "get_small: negative capacity");
    if (q == 0) return GKI_OK;
    std::lock_guard<std::mutex> lock(g_small_mu);
    if (!g_small_host) HIP_TRY(hipHostMalloc((void **)&g_small_host, sizeof(SmallStage), hipHostMallocMapped | hipHostMallocPortable));
    SmallStage *g_small_dev = nullptr;              // the mapping of the device that is current NOW (a process may switch devices)
    HIP_TRY(hipHostGetDevicePointer((void **)&g_small_dev, g_small_host, 0));
    for (int i = 0; i < q; i++) g_small_host->query[i] = h_queries[i];
    hipLaunchKernelGGL(k_get_small, dim3((unsigned)q), dim3(64), 0, 0, view_of(ix), g_small_dev, max_hits);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    for (int i = 0; i < q; i++) {
        const int64_t n = g_small_host->n_hits[i];
        h_n_hits[i] = n;                              // may exceed what was kept: min(n, SMALL_CAP, capacity) positions are valid
        int64_t keep = n < SMALL_CAP ? n : SMALL_CAP;
        if (keep > capacity_per_query) keep = capacity_per_query;
        for (int64_t j = 0; j < keep; j++) h_positions[(int64_t)i * capacity_per_query + j] = g_small_host->pos[(int64_t)i * SMALL_CAP + j];
    }
    return GKI_OK;
}
