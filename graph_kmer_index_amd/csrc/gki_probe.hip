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
// k_probe_reads fuses read hashing into the probe: one wave per read, 64 letters per step turned into bit planes
// with __ballot as in k_hash_reads; the reverse-complement k-mer of every window comes from the same planes, so the
// read is loaded once for both strands and no k-mer array is ever materialised.
#include "gki_common.h"

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
    const uint2 *dir; const uint4 *rows; const uint32_t *nk; uint64_t modulo, inv;   // inv = floor((2^64 - 1) / modulo)
    uint64_t bucket_begin, n_buckets;      // the directory holds this slice of the buckets only
};

// kmer % modulo without the 64-bit division routine: q = mulhi(kmer, inv) is the quotient or one or two short.
// Returns the bucket relative to the slice; >= n_buckets means the k-mer belongs to another slice (a miss here).
__device__ __forceinline__ uint64_t bucket_of(const ProbeDev &t, uint64_t km) {
    uint64_t r = km - __umul64hi(km, t.inv) * t.modulo;
    while (r >= t.modulo) r -= t.modulo;
    return r - t.bucket_begin;                                          // collision_free_kmer_index.py:304
}

// CollisionFreeKmerIndex.get for one k-mer, counting instead of returning (:303-315 + map_kmers :210-212), in two steps.
// Step 1 (every k-mer): the directory word.  ~95 % of the k-mers of a read end there (empty bucket, fingerprint miss).
// Step 2 (the rest): scan the bucket's rows, count the hits.  Done in place, step 2 runs with a few lanes of the wave
// while the others idle behind its dependent loads; instead the survivors are parked in a per-wave LDS queue (ballot +
// prefix sum) and the queue is worked off 64 at a time, one candidate per lane.
constexpr int CQ = 64 + 4 * 64;      // a round adds at most 4 candidates per lane to a residue of < 64

__device__ __forceinline__ void cand_push(uint4 *__restrict__ qe, int &n, bool cand, uint64_t km, uint32_t start, uint32_t count,
                                          int lane) {
    const uint64_t m = __ballot(cand);
    if (cand) qe[n + __popcll(m & ((1ull << lane) - 1ull))] = make_uint4((uint32_t)km, (uint32_t)(km >> 32), start, count);
    n += __popcll(m);
}

// is (km, relative bucket b, directory word d) a candidate, and how many rows does its bucket hold
__device__ __forceinline__ bool cand_of(const ProbeDev &t, uint64_t km, uint64_t b, uint2 d, uint32_t &count) {
    const uint32_t c16 = d.y & 0xFFFFu;
    if (c16 == 0u || ((d.y >> 16) & fp_bit(km)) == 0u) return false;
    count = c16 == CNT_SAT ? t.nk[b] : c16;
    return true;
}

// `add` is what a hit adds to its node's count: 1, or 2^32 - 1 where a signed pass takes hits away (uint32 wraps)
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

// works off the queue in groups of 64 (all of it when `all`); returns this lane's hits
__device__ __forceinline__ uint32_t cand_drain(const ProbeDev &t, const uint4 *__restrict__ qe, int &n, bool all, int64_t max_hits,
                                               unsigned int *__restrict__ counts, int64_t n_counts, int lane,
                                               uint32_t add = 1u) {
    uint32_t hits = 0;
    __builtin_amdgcn_wave_barrier();
    while (n >= 64 || (all && n > 0)) {
        const int first = n >= 64 ? n - 64 : 0;
        const int mine = first + lane;
        if (mine < n) hits += cand_scan(t, qe[mine], max_hits, counts, n_counts, add);
        n = first;
    }
    __builtin_amdgcn_wave_barrier();
    return hits;
}

__device__ __forceinline__ void wave_add(unsigned long long *dst, uint64_t v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, (unsigned long long)v);
}

constexpr int PROBE_UNROLL = 4;

__global__ __launch_bounds__(256) void k_probe_kmers(ProbeDev t, const uint64_t *__restrict__ queries, int64_t q,
                                                     int64_t max_hits, unsigned int *__restrict__ counts, int64_t n_counts,
                                                     unsigned long long *__restrict__ counters) {
    __shared__ uint4 s_cand[4][CQ];
    const int lane = threadIdx.x & 63;
    uint4 *qe = s_cand[threadIdx.x >> 6];
    int n_c = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint64_t hits = 0;
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
            cand_push(qe, n_c, cand, km[u], d[u].x, cnt, lane);
        }
        hits += cand_drain(t, qe, n_c, false, max_hits, counts, n_counts, lane);
    }
    hits += cand_drain(t, qe, n_c, true, max_hits, counts, n_counts, lane);
    wave_add(&counters[0], hits);
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
    __shared__ int64_t s_qi[4][CQ];
    const int lane = threadIdx.x & 63;
    uint4 *qe = s_cand[threadIdx.x >> 6];
    int64_t *qi = s_qi[threadIdx.x >> 6];
    int n_c = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // survivors of the directory word (~5 %) are parked and scanned 64 at a time, as in k_probe_kmers
    auto drain = [&](bool all) {
        __builtin_amdgcn_wave_barrier();
        while (n_c >= 64 || (all && n_c > 0)) {
            const int first = n_c >= 64 ? n_c - 64 : 0;
            const int mine = first + lane;
            if (mine < n_c) {
                const uint4 e = qe[mine];
                const uint64_t km = ((uint64_t)e.y << 32) | e.x;
                bool found = false;
                for (int64_t j = e.z; j < (int64_t)e.z + (int64_t)e.w && !found; j++) {
                    const uint4 r = t.rows[j];
                    found = (((uint64_t)r.y << 32) | r.x) == km;
                }
                if (found) flags[qi[mine]] = 1;
            }
            n_c = first;
        }
        __builtin_amdgcn_wave_barrier();
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
        const uint64_t m = __ballot(cand);
        if (cand) {
            const int slot = n_c + __popcll(m & ((1ull << lane) - 1ull));
            qe[slot] = make_uint4((uint32_t)km, (uint32_t)(km >> 32), start, cnt);
            qi[slot] = i;
        }
        n_c += __popcll(m);
        drain(false);
    }
    drain(true);
}

// 32 low bits -> even bit positions
__device__ __forceinline__ uint64_t spread32(uint64_t x) {
    x &= 0xFFFFFFFFull;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}


// One wave per read.  Forward k-mer of window j: bases j..j+k-1, first base least significant (read_kmers.py:70).
// Reverse strand (read_kmers.py:23-26): the k-mers of str(Seq(read).reverse_complement()) are, window by window,
// the reverse complements of the forward windows, with non-ACGT letters hashing as 0 on both strands
// (Bio.Seq maps N to N): code' = acgt ? 3 - code : 0, window reversed.
//
// The walk is shared by k_probe_reads and k_probe_segments: `spans` says where span r lies in `reads`, spans.at(r, &s, &len).
// A read is [read_start[r], read_start[r + 1]); a segment is seg_windows[r] windows from seg_start[r] on, and segments may
// overlap one another in the letters.
struct ReadSpans {
    const int64_t *__restrict__ read_start;
    __device__ __forceinline__ void at(int64_t r, int64_t *s, int64_t *len) const {
        *s = read_start[r];
        *len = read_start[r + 1] - *s;
    }
};

// Whatever the arrays hold, [s, s + len) lies inside [0, n_letters): a segment that does not is cut to what does, and
// *fault is raised for the entry to report.
struct SegmentSpans {
    const int64_t *__restrict__ seg_start, *__restrict__ seg_windows;
    int64_t n_letters;
    int k;
    unsigned long long *__restrict__ fault;
    __device__ __forceinline__ void at(int64_t r, int64_t *s, int64_t *len) const {
        const int64_t a = seg_start[r], w = seg_windows[r];
        const int64_t a_in = a < 0 ? 0 : a > n_letters ? n_letters : a;
        const int64_t w_in = w < 0 ? 0 : w > n_letters ? n_letters : w;      // w_in + k - 1 cannot overflow
        const int64_t want = w_in > 0 ? w_in + (k - 1) : 0, room = n_letters - a_in;
        if (a != a_in || w != w_in || want > room) atomicOr(fault, 1ull);
        *s = a_in;
        *len = want < room ? want : room;
    }
};

template <class Spans>
__device__ __forceinline__ void probe_spans(const ProbeDev &t, const uint8_t *__restrict__ reads, const Spans &spans,
                                            int64_t n_reads, int k, int strands, int64_t max_hits, uint32_t add,
                                            unsigned int *__restrict__ counts, int64_t n_counts,
                                            unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    __shared__ uint4 s_cand[4][CQ];
    uint4 *qe = s_cand[threadIdx.x >> 6];
    int n_c = 0;
    const uint64_t kmask2 = (1ull << (2 * k)) - 1ull;
    uint64_t hits = 0, probed = 0;
    // Letters are fetched one step ahead (the next 64 letters of this read, or the first 64 of the wave's next read)
    // so that their latency hides behind the directory loads of the current step.
    int64_t r = wave, s = 0, len = 0;
    if (r < n_reads) spans.at(r, &s, &len);
    unsigned ch_next = lane < len ? reads[s + lane] : 0u;
    while (r < n_reads) {
        const int64_t rn = r + n_waves;
        int64_t sn = 0, lenn = 0;
        if (rn < n_reads) spans.at(rn, &sn, &lenn);
        if (len < k) {
            ch_next = lane < lenn ? reads[sn + lane] : 0u;
        } else {
            const int64_t n_out = len - k + 1;
            // The 64 letters of a step become wave-uniform bit planes (__ballot) and are interleaved ONCE per step into
            // the 2-bit stream (scalar work): C0,C1 = this step's 64 bases, N0,N1 = the next step's.  A lane's window is
            // then one funnel shift of that stream, and its reverse complement a complement + bit reversal of the same
            // word (first version: two Morton spreads per window and strand on the vector units).
            uint64_t C0 = 0, C1 = 0, Cm0 = 0, Cm1 = 0;
            for (int64_t c = 0; c == 0 || (c - 1) * 64 < n_out; c++) {
                const unsigned ch = ch_next | 0x20u;                     // 0 (past the end) -> ' ': code 0, not ACGT
                const bool last = c * 64 >= n_out;                       // no further step for this read
                const int64_t i_next = (c + 1) * 64 + lane;
                if (last) ch_next = lane < lenn ? reads[sn + lane] : 0u;
                else ch_next = i_next < len ? reads[s + i_next] : 0u;
                const unsigned code = ch == 'c' ? 1u : ch == 'g' ? 2u : ch == 't' ? 3u : 0u;
                const bool acgt = ch == 'a' || code != 0u;
                const uint64_t lo = __ballot(code & 1u), hi = __ballot(code & 2u), ok = __ballot(acgt);
                const uint64_t N0 = spread32(lo) | (spread32(hi) << 1), N1 = spread32(lo >> 32) | (spread32(hi >> 32) << 1);
                const uint64_t Nm0 = spread32(ok) * 3ull, Nm1 = spread32(ok >> 32) * 3ull;
                const int64_t j = (c - 1) * 64 + lane;
                bool cand_f = false, cand_r = false;
                uint64_t fw = 0, rc = 0;
                uint32_t sf = 0, sr = 0, cf = 0, cr = 0;
                if (c > 0 && j < n_out) {
                    const int sh = (lane & 31) * 2;
                    const bool up = lane >= 32;
                    const uint64_t a = up ? C1 : C0, b = up ? N0 : C1, am = up ? Cm1 : Cm0, bm = up ? Nm0 : Cm1;
                    fw = ((a >> sh) | ((b << 1) << (63 - sh))) & kmask2;
                    const uint64_t m = ((am >> sh) | ((bm << 1) << (63 - sh))) & kmask2;
                    rc = __brevll(~fw & m) >> (64 - 2 * k);              // bases reversed, the two bits of a base swapped
                    rc = ((rc & 0x5555555555555555ull) << 1) | ((rc >> 1) & 0x5555555555555555ull);
                    const uint64_t bf = bucket_of(t, fw), br = bucket_of(t, rc);
                    const uint2 none = make_uint2(0u, 0u);
                    const uint2 df = ((strands & 1) && bf < t.n_buckets) ? t.dir[bf] : none;    // both directory words in flight
                    const uint2 dr = ((strands & 2) && br < t.n_buckets) ? t.dir[br] : none;
                    cand_f = cand_of(t, fw, bf, df, cf); sf = df.x;
                    cand_r = cand_of(t, rc, br, dr, cr); sr = dr.x;
                    probed += (strands & 1) + ((strands >> 1) & 1);
                }
                if (c > 0) {                                             // wave-uniform: the queue uses ballots
                    cand_push(qe, n_c, cand_f, fw, sf, cf, lane);
                    cand_push(qe, n_c, cand_r, rc, sr, cr, lane);
                    hits += cand_drain(t, qe, n_c, false, max_hits, counts, n_counts, lane, add);
                }
                C0 = N0; C1 = N1; Cm0 = Nm0; Cm1 = Nm1;
            }
        }
        r = rn; s = sn; len = lenn;
    }
    hits += cand_drain(t, qe, n_c, true, max_hits, counts, n_counts, lane, add);
    wave_add(&counters[0], hits);
    wave_add(&counters[1], probed);
}

__global__ __launch_bounds__(256) void k_probe_reads(ProbeDev t, const uint8_t *__restrict__ reads,
                                                     const int64_t *__restrict__ read_start, int64_t n_reads, int k,
                                                     int strands, int64_t max_hits, unsigned int *__restrict__ counts,
                                                     int64_t n_counts, unsigned long long *__restrict__ counters) {
    probe_spans(t, reads, ReadSpans{read_start}, n_reads, k, strands, max_hits, 1u, counts, n_counts, counters);
}

// One wave per segment of a sequence that stays where it is: the windows' letters are read in place, no
// hash is stored, and every hit adds `add` to its node.  counters[2] is the fault word of SegmentSpans.
__global__ __launch_bounds__(256) void k_probe_segments(ProbeDev t, const uint8_t *__restrict__ letters, int64_t n_letters,
                                                        const int64_t *__restrict__ seg_start,
                                                        const int64_t *__restrict__ seg_windows, int64_t n_segs, int k,
                                                        int strands, int64_t max_hits, uint32_t add,
                                                        unsigned int *__restrict__ counts, int64_t n_counts,
                                                        unsigned long long *__restrict__ counters) {
    probe_spans(t, letters, SegmentSpans{seg_start, seg_windows, n_letters, k, &counters[2]}, n_segs, k, strands, max_hits,
                add, counts, n_counts, counters);
}

static ProbeDev dev_of(const gki_probe *p) {
    ProbeDev d; d.dir = p->dir; d.rows = p->rows; d.nk = p->n_kmers; d.modulo = p->modulo;
    d.inv = ~0ull / p->modulo; d.bucket_begin = p->bucket_begin; d.n_buckets = p->n_buckets;
    return d;
}

static int read_counters(gki_probe *p, int64_t *n_hits, int64_t *n_kmers) {
    unsigned long long h[2] = {0, 0};
    HIP_TRY(hipMemcpy(h, p->counters, sizeof(h), hipMemcpyDeviceToHost));     // synchronises with stream 0
    if (n_hits) *n_hits = (int64_t)h[0];
    if (n_kmers) *n_kmers = (int64_t)h[1];
    return GKI_OK;
}

}  // namespace

extern "C" {

static int probe_init(gki_probe *p, const gki_index_view *ix) {
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
    if (k < 1 || k > GKI_MAX_K) return gki_set_error(GKI_ERR_BAD_ARG, "k must be in 1..31");
    if (strands < 1 || strands > 3) return gki_set_error(GKI_ERR_BAD_ARG, "strands must be 1 (forward), 2 (reverse) or 3 (both)");
    if (n_reads <= 0) return GKI_OK;
    HIP_TRY(hipMemsetAsync(p->counters, 0, 2 * sizeof(unsigned long long), 0));
    int64_t blocks = ceil_div(n_reads, 4);
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(k_probe_reads, dim3((unsigned)blocks), dim3(256), 0, 0, dev_of(p), (const uint8_t *)d_reads,
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
    if (p == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "probe_segments_count_nodes: the probe table is NULL");
    if (k < 1 || k > GKI_MAX_K) return gki_set_error(GKI_ERR_BAD_ARG, "k must be in 1..31");
    if (strands < 1 || strands > 3) return gki_set_error(GKI_ERR_BAD_ARG, "strands must be 1 (forward), 2 (reverse) or 3 (both)");
    if (sign != 1 && sign != -1) return gki_set_error(GKI_ERR_BAD_ARG, "probe_segments_count_nodes: sign must be +1 or -1");
    if (n_letters < 0 || n_segs < 0 || n_counts < 0 || (n_letters > 0 && d_letters == nullptr) || (n_counts > 0 && d_counts == nullptr) ||
        (n_segs > 0 && (d_seg_start == nullptr || d_seg_windows == nullptr)))
        return gki_set_error(GKI_ERR_BAD_ARG, "probe_segments_count_nodes: a size is negative or an array is NULL");
    if (n_segs == 0) return GKI_OK;
    HIP_TRY(hipMemsetAsync(p->counters, 0, 3 * sizeof(unsigned long long), 0));
    int64_t blocks = ceil_div(n_segs, 4);
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(k_probe_segments, dim3((unsigned)blocks), dim3(256), 0, 0, dev_of(p), (const uint8_t *)d_letters, n_letters,
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
    if (q <= 0) return GKI_OK;
    hipLaunchKernelGGL(k_probe_contains, dim3(stream_grid(q, 256)), dim3(256), 0, 0, dev_of(p), (const uint64_t *)d_queries, q,
                       (uint8_t *)d_flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

int gki_probe_lookup_count(gki_probe *p, const void *d_queries, int64_t q, int64_t max_hits, void *d_hit_start, int64_t *n_hits) {
    *n_hits = 0;
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
    if (q <= 0) return GKI_OK;
    hipLaunchKernelGGL(k_probe_lookup<true>, dim3(stream_grid(q, 256)), dim3(256), 0, 0, dev_of(p), (const uint64_t *)d_queries, q,
                       max_hits, (uint32_t *)nullptr, (const int64_t *)d_hit_start, (int64_t *)d_hit_query, (int64_t *)d_hit_position);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------ random-request rate
// What bounds a probe is not bytes but 64-byte requests that miss L2.  This measures the rate the
// device sustains right now: independent random 8-byte loads from a table of `table_bytes`, 4 in flight per lane.
namespace {
__device__ __forceinline__ uint64_t rr_mix(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}
__global__ __launch_bounds__(256) void k_random_loads(const uint64_t *__restrict__ table, uint64_t n_entries, int64_t n_loads,
                                                      uint64_t *__restrict__ sink) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint64_t acc = 0;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n_loads; i0 += stride * 4) {
        uint64_t v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = table[__umul64hi(rr_mix((uint64_t)(i0 + u * stride)), n_entries)];
#pragma unroll
        for (int u = 0; u < 4; u++) acc ^= v[u];
    }
    if (acc == 0x1234567ull) sink[0] = acc;
}
}  // namespace

extern "C" int gki_measure_random_loads(int64_t table_bytes, int64_t n_loads, double *loads_per_s) {
    *loads_per_s = 0.0;
    if (table_bytes < 4096 || n_loads < 1) return gki_set_error(GKI_ERR_BAD_ARG, "measure_random_loads: bad sizes");
    float ms = 0.f;
    // the 2 GB table is freed on every early exit too (bench.py measures with the whole 3 Gbp output resident)
    DevBuf table, sink;
    HIP_TRY(table.alloc((size_t)table_bytes));
    HIP_TRY(sink.alloc(8));
    HIP_TRY(hipMemset(table.get(), 1, (size_t)table_bytes));
    TimerEvents ev;
    HIP_TRY(hipEventCreate(&ev.e0));
    HIP_TRY(hipEventCreate(&ev.e1));
    for (int rep = 0; rep < 2; rep++) {              // the second launch is the measurement
        HIP_TRY(hipEventRecord(ev.e0, 0));
        hipLaunchKernelGGL(k_random_loads, dim3(2048), dim3(256), 0, 0, table.get<const uint64_t>(), (uint64_t)(table_bytes / 8), n_loads,
                           sink.get<uint64_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev.e1, 0));
        HIP_TRY(hipEventSynchronize(ev.e1));
        HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    }
    if (ms > 0.f) *loads_per_s = (double)n_loads / ((double)ms * 1e-3);
    return GKI_OK;
}
