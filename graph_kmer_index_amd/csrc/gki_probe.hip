// Probe table: a device-only re-layout of a CollisionFreeKmerIndex for the read-side hot loop
// (hash read k-mers -> CollisionFreeKmerIndex.get -> node counts; collision_free_kmer_index.py:210-212, 303-315).
//
// A probe is bound by the number of random 64-byte sectors it touches, not by bytes.  The reference layout costs a
// hit five of them (hashes_to_index, n_kmers, kmers, nodes, frequencies).  The probe table costs
//   * one sector per query:  dir[bucket] = {first record, record count (16 bit, saturating), 16-bit fingerprint set
//     of the bucket's k-mers} -- an empty bucket or a fingerprint miss ends the query here;
//   * one more per candidate bucket: rows[j] = {kmer, node, frequency} in 16 bytes, consecutive inside the bucket.
// Node counts are accumulated with atomics on a uint32[n_nodes] histogram (60 MB at 1.5e7 nodes: cache resident).
//
// Launches: k_probe_rows, k_probe_dir (build the table); k_probe_kmers, k_probe_lookup<EMIT>, k_probe_contains (k-mers
// given); k_probe_reads, k_probe_segments (letters given).  The last two fuse read hashing into the probe: they are the
// walk of gki_read_windows.h -- the one k_hash_reads stores from -- with ProbeSink as its sink, so the letters are loaded
// once for both strands and no k-mer array is ever materialised.  Every kernel that parks the survivors of the directory
// word does so in one CandQueue.
#include "gki_read_windows.h"

struct gki_probe {
    uint2 *dir = nullptr;            // [modulo]
    uint4 *rows = nullptr;           // [n]
    const uint32_t *n_kmers = nullptr;   // the index's own array (borrowed): exact length of saturated buckets
    unsigned long long *counters = nullptr;   // [3] device: hits, k-mers probed, fault word of a segment pass
    uint64_t modulo = 0, bucket_begin = 0, n_buckets = 0;
    int64_t n = 0;
};

namespace {

constexpr uint32_t CNT_SAT = 0xFFFFu;
constexpr int FP_SCAN_MAX = 64;      // buckets longer than this get an all-ones fingerprint set

__device__ __forceinline__ uint32_t fp_bit(uint64_t kmer) {
    const uint32_t x = (uint32_t)(kmer >> 32) * 0x9E3779B1u ^ (uint32_t)kmer * 0x85EBCA77u;
    return 1u << (x >> 28);
}

__global__ __launch_bounds__(256) void k_probe_dir(const int32_t *__restrict__ h2i, const uint32_t *__restrict__ nk,
                                                   const uint64_t *__restrict__ kmers, uint64_t n_buckets,
                                                   uint2 *__restrict__ dir) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < (int64_t)n_buckets; b += stride) {
        const uint32_t m = nk[b];
        const uint32_t s = (uint32_t)h2i[b];
        uint32_t fp = 0;
        if (m > FP_SCAN_MAX) fp = 0xFFFFu;
        else for (uint32_t j = 0; j < m; j++) fp |= fp_bit(kmers[(int64_t)s + j]);
        dir[b] = make_uint2(s, (m < CNT_SAT ? m : CNT_SAT) | (fp << 16));
    }
}

__global__ __launch_bounds__(256) void k_probe_rows(const uint64_t *__restrict__ kmers, const uint32_t *__restrict__ nodes,
                                                    const uint16_t *__restrict__ freq, int64_t n, uint4 *__restrict__ rows) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t k = kmers[i];
        rows[i] = make_uint4((uint32_t)k, (uint32_t)(k >> 32), nodes[i], freq ? (uint32_t)freq[i] : 0u);
    }
}

struct ProbeDev {
    const uint2 *dir; const uint4 *rows; const uint32_t *nk; GkiMod mod;
    uint64_t bucket_begin, n_buckets;      // the directory holds this slice of the buckets only
};

// The bucket relative to the slice; >= n_buckets means the k-mer belongs to another slice (a miss here).
__device__ __forceinline__ uint64_t bucket_of(const ProbeDev &t, uint64_t km) {
    return gki_mod(t.mod, km) - t.bucket_begin;                         // collision_free_kmer_index.py:304
}

// CollisionFreeKmerIndex.get for one k-mer, counting instead of returning (:303-315 + map_kmers :210-212), in two steps.
// Step 1 (every k-mer): the directory word.  ~95 % of the k-mers of a read end there (empty bucket, fingerprint miss).
// Step 2 (the rest): scan the bucket's rows, count the hits.  Done in place, step 2 runs with a few lanes of the wave
// while the others idle behind its dependent loads; instead the survivors are parked in a per-wave LDS queue (ballot +
// prefix sum) and the queue is worked off 64 at a time, one candidate per lane.
constexpr int CQ = 64 + 4 * 64;      // a round adds at most 4 candidates per lane to a residue of < 64

// The queue of one wave: `e` is its CQ entries {k-mer lo, hi, first row, row count} in LDS, declared by the kernel.
// TAGGED keeps an int64 (the query's index) beside every entry, in CQ more LDS words at `tag`; without it `tag` is unused.
// push and drain are wave-uniform calls.
template <bool TAGGED = false>
struct CandQueue {
    uint4 *e;
    int64_t *tag;
    int n = 0;
    __device__ __forceinline__ void push(bool cand, uint64_t km, uint32_t start, uint32_t count, int64_t t = 0) {
        const uint64_t m = __ballot(cand);
        if (cand) {
            const int slot = n + __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
            e[slot] = make_uint4((uint32_t)km, (uint32_t)(km >> 32), start, count);
            if (TAGGED) tag[slot] = t;
        }
        n += __popcll(m);
    }
    // works off the queue in groups of 64 (all of it when `all`): fn(entry[, &tag]), one candidate per lane
    template <class Fn>
    __device__ __forceinline__ void drain(bool all, Fn fn) {
        __builtin_amdgcn_wave_barrier();
        while (n >= 64 || (all && n > 0)) {
            const int first = n >= 64 ? n - 64 : 0;
            const int mine = first + (threadIdx.x & 63);
            if (mine < n) {
                if constexpr (TAGGED) fn(e[mine], &tag[mine]);
                else fn(e[mine]);
            }
            n = first;
        }
        __builtin_amdgcn_wave_barrier();
    }
};

// is (km, relative bucket b, directory word d) a candidate, and how many rows does its bucket hold
__device__ __forceinline__ bool cand_of(const ProbeDev &t, uint64_t km, uint64_t b, uint2 d, uint32_t &count) {
    const uint32_t c16 = d.y & 0xFFFFu;
    if (c16 == 0u || ((d.y >> 16) & fp_bit(km)) == 0u) return false;
    count = c16 == CNT_SAT ? t.nk[b] : c16;
    return true;
}

// the queue's action in the counting kernels: the rows of one candidate, returns its hits.  `add` is what a hit adds to
// its node's count: 1, or 2^32 - 1 where a signed pass takes hits away (uint32 wraps)
__device__ __forceinline__ uint32_t cand_scan(const ProbeDev &t, uint4 e, int64_t max_hits, unsigned int *__restrict__ counts,
                                              int64_t n_counts, uint32_t add) {
    const uint64_t km = ((uint64_t)e.y << 32) | e.x;
    uint32_t hits = 0;
    for (int64_t j = e.z; j < (int64_t)e.z + (int64_t)e.w; j++) {
        const uint4 r = t.rows[j];
        if ((((uint64_t)r.y << 32) | r.x) != km) continue;              // :309
        if (hits == 0u && (int64_t)r.w > max_hits) break;               // :312 (frequency of the first match)
        if ((int64_t)r.z < n_counts) atomicAdd(&counts[r.z], add);
        hits++;
    }
    return hits;
}

constexpr int PROBE_UNROLL = 4;

__global__ __launch_bounds__(256) void k_probe_kmers(ProbeDev t, const uint64_t *__restrict__ queries, int64_t q,
                                                     int64_t max_hits, unsigned int *__restrict__ counts, int64_t n_counts,
                                                     unsigned long long *__restrict__ counters) {
    __shared__ uint4 s_cand[4][CQ];
    const int lane = threadIdx.x & 63;
    CandQueue<> cq{s_cand[threadIdx.x >> 6], nullptr};
    uint64_t hits = 0;
    auto scan = [&](uint4 e) { hits += cand_scan(t, e, max_hits, counts, n_counts, 1u); };
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // wave-uniform trip count (the queue bookkeeping uses ballots): the wave's first lane decides
    for (int64_t w0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); w0 < q; w0 += stride * PROBE_UNROLL) {
        const int64_t i0 = w0 + lane;
        uint64_t km[PROBE_UNROLL], b[PROBE_UNROLL];
        uint2 d[PROBE_UNROLL];
#pragma unroll
        for (int u = 0; u < PROBE_UNROLL; u++) {
            const int64_t i = i0 + u * stride;
            km[u] = i < q ? queries[i] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < PROBE_UNROLL; u++) {
            b[u] = bucket_of(t, km[u]);
            d[u] = ((i0 + u * stride) < q && b[u] < t.n_buckets) ? t.dir[b[u]] : make_uint2(0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < PROBE_UNROLL; u++) {
            uint32_t cnt = 0;
            const bool cand = cand_of(t, km[u], b[u], d[u], cnt);
            cq.push(cand, km[u], d[u].x, cnt);
        }
        cq.drain(false, scan);
    }
    cq.drain(true, scan);
    wave_add64(&counters[0], hits);
}

// Batched CollisionFreeKmerIndex.get on the table (collision_free_kmer_index.py:303-315, 354-391): count pass, then
// (after a scan of the counts) an emit pass writing, per hit, the query index and the hit's position in the payload
// arrays -- rows[j] is record j, so a caller gathers nodes / ref_offsets / frequencies / allele frequencies from its own
// columns.  One or two sectors per query instead of the four to five of the reference layout.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_probe_lookup(ProbeDev t, const uint64_t *__restrict__ queries, int64_t q, int64_t max_hits,
                                                      uint32_t *__restrict__ cnt, const int64_t *__restrict__ hit_start,
                                                      int64_t *__restrict__ o_query, int64_t *__restrict__ o_pos) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < q; i += stride) {
        int64_t o = 0;
        if (EMIT) { o = hit_start[i]; if (hit_start[i + 1] == o) continue; }
        const uint64_t km = queries[i];
        const uint64_t b = bucket_of(t, km);
        uint32_t c = 0;
        if (b < t.n_buckets) {
            const uint2 d = t.dir[b];
            uint32_t m = 0;
            if (cand_of(t, km, b, d, m)) {
                for (int64_t j = d.x; j < (int64_t)d.x + (int64_t)m; j++) {
                    const uint4 r = t.rows[j];
                    if ((((uint64_t)r.y << 32) | r.x) != km) continue;              // :309
                    if (!EMIT && c == 0u && (int64_t)r.w > max_hits) break;         // :312 (frequency of the first match)
                    if (EMIT) { o_query[o] = i; o_pos[o] = j; o++; }
                    c++;
                }
            }
        }
        if (!EMIT) cnt[i] = c;
    }
}

// `kmer in index` (collision_free_kmer_index.py:295-296: get(kmer, max_hits = 10^11) is not None), one flag per query:
// the whitelist test of DenseKmerFinder._add_kmer / _process_whole_node (kmer_finder.py:130-132, 362-365).
__global__ __launch_bounds__(256) void k_probe_contains(ProbeDev t, const uint64_t *__restrict__ queries, int64_t q,
                                                        uint8_t *__restrict__ flags) {
    __shared__ uint4 s_cand[4][CQ];
    __shared__ int64_t s_tag[4][CQ];
    const int lane = threadIdx.x & 63;
    CandQueue<true> cq{s_cand[threadIdx.x >> 6], s_tag[threadIdx.x >> 6]};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // survivors of the directory word (~5 %) are parked and scanned 64 at a time, as in k_probe_kmers
    auto flag_if_present = [&](uint4 e, const int64_t *i) {      // *i is read only once a row matches
        const uint64_t km = ((uint64_t)e.y << 32) | e.x;
        bool found = false;
        for (int64_t j = e.z; j < (int64_t)e.z + (int64_t)e.w && !found; j++) {
            const uint4 r = t.rows[j];
            found = (((uint64_t)r.y << 32) | r.x) == km;
        }
        if (found) flags[*i] = 1;
    };
    for (int64_t w0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); w0 < q; w0 += stride) {
        const int64_t i = w0 + lane;
        bool cand = false;
        uint64_t km = 0;
        uint32_t start = 0, cnt = 0;
        if (i < q) {
            km = queries[i];
            flags[i] = 0;
            const uint64_t b = bucket_of(t, km);
            if (b < t.n_buckets) {
                const uint2 d = t.dir[b];
                cand = cand_of(t, km, b, d, cnt);
                start = d.x;
            }
        }
        cq.push(cand, km, start, cnt, i);
        cq.drain(false, flag_if_present);
    }
    cq.drain(true, flag_if_present);
}

// The walk's sink that probes (gki_read_windows.h): both directory words of a window in flight, the survivors parked,
// the queue drained once per step.  `strands` masks the forward (1) and the reverse-complement (2) k-mer; the read is
// loaded once for both and no k-mer array is ever materialised.  counters[0] += hits, counters[1] += k-mers probed.
struct ProbeSink {
    static constexpr bool NEEDS_FW = true, NEEDS_RC = true;
    const ProbeDev &t;
    CandQueue<> cq;
    int strands;
    int64_t max_hits;
    uint32_t add;
    unsigned int *__restrict__ counts;
    int64_t n_counts;
    unsigned long long *__restrict__ counters;
    uint64_t hits = 0, probed = 0;
    __device__ __forceinline__ void begin(int64_t) {}
    __device__ __forceinline__ void drain(bool all) {
        cq.drain(all, [&](uint4 e) { hits += cand_scan(t, e, max_hits, counts, n_counts, add); });
    }
    __device__ __forceinline__ void window(bool active, int64_t, int64_t, uint64_t fw, uint64_t rc) {
        bool cand_f = false, cand_r = false;
        uint32_t sf = 0, sr = 0, cf = 0, cr = 0;
        if (active) {
            const uint64_t bf = bucket_of(t, fw), br = bucket_of(t, rc);
            const uint2 df = ((strands & 1) && bf < t.n_buckets) ? t.dir[bf] : make_uint2(0u, 0u);      // both directory
            const uint2 dr = ((strands & 2) && br < t.n_buckets) ? t.dir[br] : make_uint2(0u, 0u);      // words in flight
            cand_f = cand_of(t, fw, bf, df, cf); sf = df.x;
            cand_r = cand_of(t, rc, br, dr, cr); sr = dr.x;
            probed += (strands & 1) + ((strands >> 1) & 1);
        }
        cq.push(cand_f, fw, sf, cf);
        cq.push(cand_r, rc, sr, cr);
        drain(false);
    }
    __device__ __forceinline__ void finish() {
        drain(true);
        wave_add64(&counters[0], hits);
        wave_add64(&counters[1], probed);
    }
};

__global__ __launch_bounds__(256) void k_probe_reads(ProbeDev t, const uint8_t *__restrict__ reads,
                                                     const int64_t *__restrict__ read_start, int64_t n_reads, int k,
                                                     int strands, int64_t max_hits, unsigned int *__restrict__ counts,
                                                     int64_t n_counts, unsigned long long *__restrict__ counters) {
    __shared__ uint4 s_cand[4][CQ];
    ProbeSink sink{t, {s_cand[threadIdx.x >> 6], nullptr}, strands, max_hits, 1u, counts, n_counts, counters};
    walk_span_windows(reads, ReadSpans{read_start}, n_reads, k, sink);
}

// One wave per segment of a sequence that stays where it is: the windows' letters are read in place, no
// hash is stored, and every hit adds `add` to its node.  counters[2] is the fault word of SegmentSpans.
__global__ __launch_bounds__(256) void k_probe_segments(ProbeDev t, const uint8_t *__restrict__ letters, int64_t n_letters,
                                                        const int64_t *__restrict__ seg_start,
                                                        const int64_t *__restrict__ seg_windows, int64_t n_segs, int k,
                                                        int strands, int64_t max_hits, uint32_t add,
                                                        unsigned int *__restrict__ counts, int64_t n_counts,
                                                        unsigned long long *__restrict__ counters) {
    __shared__ uint4 s_cand[4][CQ];
    ProbeSink sink{t, {s_cand[threadIdx.x >> 6], nullptr}, strands, max_hits, add, counts, n_counts, counters};
    walk_span_windows(letters, SegmentSpans{seg_start, seg_windows, n_letters, k, &counters[2]}, n_segs, k, sink);
}

ProbeDev dev_of(const gki_probe *p) {
    ProbeDev d; d.dir = p->dir; d.rows = p->rows; d.nk = p->n_kmers; d.mod = gki_mod_of(p->modulo);
    d.bucket_begin = p->bucket_begin; d.n_buckets = p->n_buckets;
    return d;
}

int read_counters(gki_probe *p, int64_t *n_hits, int64_t *n_kmers) {
    unsigned long long h[2] = {0, 0};
    HIP_TRY(hipMemcpy(h, p->counters, sizeof(h), hipMemcpyDeviceToHost));     // synchronises with stream 0
    if (n_hits) *n_hits = (int64_t)h[0];
    if (n_kmers) *n_kmers = (int64_t)h[1];
    return GKI_OK;
}

// every entry that uses a probe table refuses a NULL one
int probe_given(const gki_probe *p, const char *who) {
    return p ? GKI_OK : gki_set_error(GKI_ERR_BAD_ARG, "%s: the probe table is NULL", who);
}

int probe_init(gki_probe *p, const gki_index_view *ix) {
    p->modulo = ix->modulo; p->n = ix->n; p->n_kmers = (const uint32_t *)ix->d_n_kmers;
    p->bucket_begin = ix->n_buckets ? ix->bucket_begin : 0; p->n_buckets = ix->n_buckets ? ix->n_buckets : ix->modulo;
    HIP_TRY(gki_dev_malloc(&p->dir, (size_t)p->n_buckets * sizeof(uint2)));
    HIP_TRY(gki_dev_malloc(&p->rows, (size_t)(ix->n > 0 ? ix->n : 1) * sizeof(uint4)));
    HIP_TRY(gki_dev_malloc(&p->counters, 3 * sizeof(unsigned long long)));
    if (ix->n > 0)
        hipLaunchKernelGGL(k_probe_rows, dim3(stream_grid(ix->n, 256)), dim3(256), 0, 0, (const uint64_t *)ix->d_kmers,
                           (const uint32_t *)ix->d_nodes, (const uint16_t *)ix->d_frequencies, ix->n, p->rows);
    hipLaunchKernelGGL(k_probe_dir, dim3(stream_grid((int64_t)p->n_buckets, 256)), dim3(256), 0, 0,
                       (const int32_t *)ix->d_hashes_to_index, (const uint32_t *)ix->d_n_kmers,
                       (const uint64_t *)ix->d_kmers, p->n_buckets, p->dir);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

}  // namespace

extern "C" {

int gki_probe_create(const gki_index_view *ix, gki_probe **out) {
    *out = nullptr;
    if (ix->modulo == 0 || ix->modulo > 0xFFFFFFFFull) return gki_set_error(GKI_ERR_BAD_ARG, "modulo must be in 1..2^32-1");
    if (ix->n < 0 || ix->n >= (1ll << 32)) return gki_set_error(GKI_ERR_BAD_ARG, "record count must be below 2^32");
    gki_probe *p = new gki_probe();
    const int rc = probe_init(p, ix);
    if (rc != GKI_OK) { (void)gki_probe_destroy(p); return rc; }      // nothing of a half-built probe table stays behind
    *out = p;
    return GKI_OK;
}

int gki_probe_destroy(gki_probe *p) {
    if (!p) return GKI_OK;
    (void)gki_dev_free(p->dir); (void)gki_dev_free(p->rows); (void)gki_dev_free(p->counters);
    delete p;
    return GKI_OK;
}

int gki_probe_count_nodes(gki_probe *p, const void *d_queries, int64_t q, int64_t max_hits, void *d_counts, int64_t n_counts,
                          int64_t *n_hits) {
    if (n_hits) *n_hits = 0;
    GKI_TRY(probe_given(p, "probe_count_nodes"));
    if (q <= 0) return GKI_OK;
    HIP_TRY(hipMemsetAsync(p->counters, 0, 2 * sizeof(unsigned long long), 0));
    hipLaunchKernelGGL(k_probe_kmers, dim3(stream_grid(q, 256)), dim3(256), 0, 0, dev_of(p), (const uint64_t *)d_queries, q,
                       max_hits, (unsigned int *)d_counts, n_counts, p->counters);
    HIP_TRY(hipGetLastError());
    return read_counters(p, n_hits, nullptr);
}

int gki_probe_reads_count_nodes(gki_probe *p, const void *d_reads, const void *d_read_start, int64_t n_reads, int k,
                                int strands, int64_t max_hits, void *d_counts, int64_t n_counts, int64_t *n_kmers,
                                int64_t *n_hits) {
    if (n_hits) *n_hits = 0;
    if (n_kmers) *n_kmers = 0;
    GKI_TRY(probe_given(p, "probe_reads_count_nodes"));
    GKI_TRY(gki_check_k_strands(k, strands));
    if (n_reads <= 0) return GKI_OK;
    HIP_TRY(hipMemsetAsync(p->counters, 0, 2 * sizeof(unsigned long long), 0));
    hipLaunchKernelGGL(k_probe_reads, dim3(span_grid(n_reads)), dim3(256), 0, 0, dev_of(p), (const uint8_t *)d_reads,
                       (const int64_t *)d_read_start, n_reads, k, strands, max_hits, (unsigned int *)d_counts, n_counts,
                       p->counters);
    HIP_TRY(hipGetLastError());
    return read_counters(p, n_hits, n_kmers);
}

int gki_probe_segments_count_nodes(gki_probe *p, const void *d_letters, int64_t n_letters, const void *d_seg_start,
                                   const void *d_seg_windows, int64_t n_segs, int k, int strands, int64_t max_hits, int sign,
                                   void *d_counts, int64_t n_counts, int64_t *n_kmers, int64_t *n_hits) {
    if (n_hits) *n_hits = 0;
    if (n_kmers) *n_kmers = 0;
    GKI_TRY(probe_given(p, "probe_segments_count_nodes"));
    GKI_TRY(gki_check_k_strands(k, strands));
    if (sign != 1 && sign != -1) return gki_set_error(GKI_ERR_BAD_ARG, "probe_segments_count_nodes: sign must be +1 or -1");
    if (n_letters < 0 || n_segs < 0 || n_counts < 0 || (n_letters > 0 && d_letters == nullptr) || (n_counts > 0 && d_counts == nullptr) ||
        (n_segs > 0 && (d_seg_start == nullptr || d_seg_windows == nullptr)))
        return gki_set_error(GKI_ERR_BAD_ARG, "probe_segments_count_nodes: a size is negative or an array is NULL");
    if (n_segs == 0) return GKI_OK;
    HIP_TRY(hipMemsetAsync(p->counters, 0, 3 * sizeof(unsigned long long), 0));
    hipLaunchKernelGGL(k_probe_segments, dim3(span_grid(n_segs)), dim3(256), 0, 0, dev_of(p), (const uint8_t *)d_letters, n_letters,
                       (const int64_t *)d_seg_start, (const int64_t *)d_seg_windows, n_segs, k, strands, max_hits,
                       sign > 0 ? 1u : 0xFFFFFFFFu, (unsigned int *)d_counts, n_counts, p->counters);
    HIP_TRY(hipGetLastError());
    GKI_TRY(read_counters(p, n_hits, n_kmers));
    unsigned long long fault = 0;
    HIP_TRY(hipMemcpy(&fault, p->counters + 2, sizeof(fault), hipMemcpyDeviceToHost));
    if (fault) return gki_set_error(GKI_ERR_BAD_ARG, "probe_segments_count_nodes: a segment reaches outside the %lld letters; it was cut", (long long)n_letters);
    return GKI_OK;
}

int gki_probe_contains(gki_probe *p, const void *d_queries, int64_t q, void *d_flags) {
    GKI_TRY(probe_given(p, "probe_contains"));
    if (q <= 0) return GKI_OK;
    hipLaunchKernelGGL(k_probe_contains, dim3(stream_grid(q, 256)), dim3(256), 0, 0, dev_of(p), (const uint64_t *)d_queries, q,
                       (uint8_t *)d_flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

int gki_probe_lookup_count(gki_probe *p, const void *d_queries, int64_t q, int64_t max_hits, void *d_hit_start, int64_t *n_hits) {
    *n_hits = 0;
    GKI_TRY(probe_given(p, "probe_lookup_count"));
    if (q <= 0) { HIP_TRY(hipMemset(d_hit_start, 0, 8)); return GKI_OK; }
    const int64_t tmp_bytes = gki_scan_tmp_bytes(q);
    DevBuf cnt, tmp;
    HIP_TRY(cnt.alloc((size_t)q * 4));
    HIP_TRY(tmp.alloc((size_t)tmp_bytes));
    hipLaunchKernelGGL(k_probe_lookup<false>, dim3(stream_grid(q, 256)), dim3(256), 0, 0, dev_of(p), (const uint64_t *)d_queries, q,
                       max_hits, cnt.get<uint32_t>(), (const int64_t *)nullptr, (int64_t *)nullptr, (int64_t *)nullptr);
    if (hipGetLastError() != hipSuccess) return gki_set_error(GKI_ERR_HIP, "k_probe_lookup launch failed");
    GKI_TRY(gki_scan_u32_to_i64(cnt.get<const uint32_t>(), q, (int64_t *)d_hit_start, tmp.get(), tmp_bytes, 0));
    int64_t total = 0;
    HIP_TRY(hipMemcpy(&total, (const int64_t *)d_hit_start + q, 8, hipMemcpyDeviceToHost));
    *n_hits = total;
    return GKI_OK;
}

int gki_probe_lookup_emit(gki_probe *p, const void *d_queries, int64_t q, int64_t max_hits, const void *d_hit_start,
                          void *d_hit_query, void *d_hit_position) {
    GKI_TRY(probe_given(p, "probe_lookup_emit"));
    if (q <= 0) return GKI_OK;
    hipLaunchKernelGGL(k_probe_lookup<true>, dim3(stream_grid(q, 256)), dim3(256), 0, 0, dev_of(p), (const uint64_t *)d_queries, q,
                       max_hits, (uint32_t *)nullptr, (const int64_t *)d_hit_start, (int64_t *)d_hit_query, (int64_t *)d_hit_position);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

}  // extern "C"
