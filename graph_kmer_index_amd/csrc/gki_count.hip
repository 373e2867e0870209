// KmerCounter / KmerFrequencyIndex on the device (kmer_counter.py:33-43, kmer_frequency_index.py:18-25 of the reference:
// np.unique(kmers, return_counts=True)): the sorted distinct keys of an array of 64-bit k-mer hashes with their counts,
// and a counter over them that answers batched frequency lookups.
//
//   k_count_hist      per tile of CT keys: the histogram of one 8-bit digit, bin-major (hist[bin * n_tiles + tile])
//   (gki_scan_u32_to_i64 over the histograms: the first output position of every (digit, tile), 64 bits wide)
//   k_count_scatter   stable scatter of one tile: ballot ranking per wave, the tile sorted by digit in LDS, then runs of
//                     equal digits stored to consecutive positions.  Key only; least significant digit first; the first
//                     pass reads the caller's array at the caller's stride, so the input is read in place and never written
//                     (both kernels are the pass of gki_radix_tile.h over KeyItems)
//   k_run_count       per tile of the sorted keys: the number of run heads (key != predecessor); their scan gives n_unique
//   k_run_emit        per tile: every head's rank from ballots and the tile's scanned start -> its key and its position
//   k_run_lengths     count of run r = position of head r + 1 (or the number of keys) - position of head r: a run may span
//                     any number of tiles, nothing is narrower than 64 bits
//   k_counter_directory, k_counter_lookup   the prefix directory of GkiCounterView (gki_common.h) and the batched probe
//   k_sv_probe_counter, k_uvk_summarize_counter   the variant-signature passes of gki_frequency.h with the counter as
//                     frequency source
//
// Launches per pass are histogram -> scan -> scatter: no workgroup ever waits for another one.
#include "gki_frequency.h"
#include "gki_radix_tile.h"
#include <memory>

// What the count call leaves for the emit call: the sorted keys and the scanned heads per tile.
struct gki_unique_plan {
    int64_t m = 0, n_unique = 0, n_tiles = 0;
    DevBuf sorted;           // uint64[m]
    DevBuf tile_start;       // int64[n_tiles + 1]: rank of the first head of every tile
};

namespace {

constexpr int CB = 256;              // threads per block
constexpr int CI = 16;               // keys per thread
constexpr int CT = CB * CI;          // 4096 keys per tile (graph_kmer_index_amd/kmer_counter.py SORT_TILE)
constexpr int CBINS = RADIX_BINS;
static_assert(CI * (CB / 64) == 64, "k_run_emit scans its (round, wave) partial counts with one wave");

// The keys as the items of gki_radix_tile.h's pass: read at a stride (the caller's, in the first pass), written densely;
// tile offsets are 64 bits wide (up to 2^33 keys)
struct KeyItems {
    using Offset = int64_t;
    const uint64_t *__restrict__ in; int64_t stride; uint64_t *__restrict__ out;
    __device__ __forceinline__ uint64_t load_key(int64_t i) const { return in[i * stride]; }
    __device__ __forceinline__ uint64_t load(int64_t i) const { return in[i * stride]; }
    __device__ __forceinline__ void store(int64_t i, uint64_t key) const { out[i] = key; }
    static __device__ __forceinline__ uint32_t digit(uint64_t key, int shift) { return (uint32_t)(key >> shift) & 0xFF; }
};

// `bad` is set when a key has a bit at or above key_bits (checked in the first pass only: key_bits == 0 skips it)
__global__ __launch_bounds__(CB) void k_count_hist(const uint64_t *__restrict__ keys, int64_t m, int64_t stride, int shift,
                                                   int key_bits, uint32_t *__restrict__ hist, int64_t n_tiles,
                                                   int *__restrict__ bad) {
    const uint64_t acc = radix_tile_hist<CB, CI>(KeyItems{keys, stride, nullptr}, m, shift, hist, n_tiles);
    if (key_bits > 0 && key_bits < 64 && (acc >> key_bits) != 0ull) atomicOr(bad, 1);
}

__global__ __launch_bounds__(CB) void k_count_scatter(const uint64_t *__restrict__ keys_in, int64_t m, int64_t stride,
                                                      int shift, const int64_t *__restrict__ offs /* scanned hist */,
                                                      int64_t n_tiles, uint64_t *__restrict__ keys_out) {
    radix_tile_scatter<CB, CI>(KeyItems{keys_in, stride, keys_out}, m, shift, offs, n_tiles);
}

// heads of a tile of the sorted keys: element order (round, thread), i.e. the keys' own order
__global__ __launch_bounds__(CB) void k_run_count(const uint64_t *__restrict__ keys, int64_t m,
                                                  uint32_t *__restrict__ tile_heads) {
    __shared__ uint32_t wsum[CB / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * CT;
    uint32_t cnt = 0;
#pragma unroll
    for (int r = 0; r < CI; r++) {
        const int64_t i = base + r * CB + threadIdx.x;
        if (i < m && (i == 0 || keys[i] != keys[i - 1])) ++cnt;
    }
    const uint32_t inc = gki_wave_incl_sum(cnt);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) tile_heads[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(CB) void k_run_emit(const uint64_t *__restrict__ keys, int64_t m,
                                                 const int64_t *__restrict__ tile_start, int64_t n_unique,
                                                 uint64_t *__restrict__ unique, int64_t *__restrict__ head_pos) {
    __shared__ uint32_t part[CI * (CB / 64)];       // heads of (round r, wave w) at r * 4 + w, then their exclusive scan
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * CT;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    uint64_t key[CI];
    uint32_t before[CI];
    uint32_t heads = 0;
#pragma unroll
    for (int r = 0; r < CI; r++) {
        const int64_t i = base + r * CB + threadIdx.x;
        bool head = false;
        key[r] = 0;
        if (i < m) {
            key[r] = keys[i];
            head = i == 0 || key[r] != keys[i - 1];
        }
        const uint64_t b = __ballot(head);
        before[r] = (uint32_t)__popcll(b & lt_mask);
        if (head) heads |= 1u << r;
        if (lane == 0) part[r * (CB / 64) + wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    if (wave == 0) {
        const uint32_t x = part[lane];
        part[lane] = gki_wave_incl_sum(x) - x;
    }
    __syncthreads();
    const int64_t first = tile_start[blockIdx.x];
#pragma unroll
    for (int r = 0; r < CI; r++) {
        if (heads & (1u << r)) {
            const int64_t rank = first + part[r * (CB / 64) + wave] + before[r];
            if (rank < n_unique) {
                unique[rank] = key[r];
                head_pos[rank] = base + r * CB + threadIdx.x;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_run_lengths(const int64_t *__restrict__ head_pos, int64_t n_unique, int64_t m,
                                                     int64_t *__restrict__ counts) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_unique; r += stride)
        counts[r] = (r + 1 < n_unique ? head_pos[r + 1] : m) - head_pos[r];
}

// dir[p] = the first position whose top dir_bits bits are >= p, p = 0 .. 2^dir_bits (the last entry is n)
__global__ __launch_bounds__(256) void k_counter_directory(const uint64_t *__restrict__ keys, int64_t n, int shift,
                                                           int64_t n_dir, int64_t *__restrict__ dir) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p <= n_dir; p += stride) {
        int64_t lo = 0, hi = n;
        if (p == n_dir) lo = n;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if ((int64_t)(keys[mid] >> shift) < p) lo = mid + 1; else hi = mid;
        }
        dir[p] = lo;
    }
}

__global__ __launch_bounds__(256) void k_counter_lookup(GkiCounterView c, const uint64_t *__restrict__ queries, int64_t q,
                                                        int64_t *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < q; i += stride)
        out[i] = gki_counter_frequency(c, queries[i]);
}

__global__ __launch_bounds__(256) void k_sv_probe_counter(const int32_t *__restrict__ cand, const int64_t *__restrict__ word_start,
                                                          int64_t n_cand, int64_t n_words, const int32_t *__restrict__ node_size,
                                                          const int64_t *__restrict__ seq_start,
                                                          const uint64_t *__restrict__ seq2, int k, int64_t max_frequency,
                                                          GkiCounterSource src, uint64_t *__restrict__ bitmap) {
    sv_probe_body(cand, word_start, n_cand, n_words, node_size, seq_start, seq2, k, max_frequency, src, bitmap);
}

__global__ __launch_bounds__(256) void k_uvk_summarize_counter(
    const int64_t *__restrict__ rec_start, int64_t n_pos, int P, const int64_t *__restrict__ hashes,
    const int32_t *__restrict__ start_nodes, const int16_t *__restrict__ start_offsets, const int32_t *__restrict__ nodes,
    const int32_t *__restrict__ ref_nodes, const int32_t *__restrict__ alt_nodes, GkiCounterSource src,
    gki_uvk_summary *__restrict__ out) {
    uvk_summarize_body(rec_start, n_pos, P, hashes, start_nodes, start_offsets, nodes, ref_nodes, alt_nodes, src, out);
}

int check_counter_device(const gki_counter *c, const char *who) {
    if (c == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "%s: no counter", who);
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != c->device)
        return gki_set_error(GKI_ERR_BAD_ARG, "%s: the counter lives on device %d, the current device is %d", who, c->device, dev);
    return GKI_OK;
}

}  // namespace

int gki_launch_sv_probe_counter(const gki_counter *c, const int32_t *cand, const int64_t *word_start, int64_t n_cand,
                                int64_t n_words, const DevGraph &d, int k, int64_t max_frequency, uint64_t *bitmap) {
    GKI_TRY(check_counter_device(c, "gki_sv_sample_count_counter"));
    GkiCounterSource src;
    src.c = c->v;
    hipLaunchKernelGGL(k_sv_probe_counter, dim3(stream_grid(ceil_div(n_words, SV_CHUNK) * 64, 256)), dim3(256), 0, 0, cand,
                       word_start, n_cand, n_words, d.node_size, d.seq_start, d.seq2, k, max_frequency, src, bitmap);
    HIP_TRY(hipGetLastError());
    return GKI_OK;
}

int gki_launch_uvk_summarize_counter(const gki_counter *c, const int64_t *rec_start, int64_t n_pos, int P,
                                     const int64_t *hashes, const int32_t *start_nodes, const int16_t *start_offsets,
                                     const int32_t *nodes, const int32_t *ref_nodes, const int32_t *alt_nodes,
                                     gki_uvk_summary *out) {
    GKI_TRY(check_counter_device(c, "gki_uvk_summarize_counter"));
    GkiCounterSource src;
    src.c = c->v;
    hipLaunchKernelGGL(k_uvk_summarize_counter, dim3(stream_grid(n_pos, 256)), dim3(256), 0, 0, rec_start, n_pos, P, hashes,
                       start_nodes, start_offsets, nodes, ref_nodes, alt_nodes, src, out);
    HIP_TRY(hipGetLastError());
    return GKI_OK;
}

extern "C" {

int gki_unique_counts_count(const void *d_kmers, int64_t n, int64_t stride, int key_bits, int64_t *n_unique,
                            gki_unique_plan **plan_out, float *kernel_ms) {
    *n_unique = 0;
    *plan_out = nullptr;
    if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.f;
    if (n < 0 || n > (1ll << 33)) return gki_set_error(GKI_ERR_BAD_ARG, "gki_unique_counts_count: n must be in 0..2^33");
    if (stride < 1) return gki_set_error(GKI_ERR_BAD_ARG, "gki_unique_counts_count: stride must be at least 1");
    if (key_bits < 1 || key_bits > 64) return gki_set_error(GKI_ERR_BAD_ARG, "gki_unique_counts_count: key_bits must be in 1..64");
    std::unique_ptr<gki_unique_plan> p(new gki_unique_plan());
    const int64_t m = ceil_div(n, stride);               // kmers[::stride]
    p->m = m;
    if (m == 0) { *plan_out = p.release(); return GKI_OK; }
    if (d_kmers == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "gki_unique_counts_count: no keys");
    const int64_t n_tiles = ceil_div(m, CT), hist_n = (int64_t)CBINS * n_tiles;
    p->n_tiles = n_tiles;
    const int64_t tmp_bytes = gki_scan_tmp_bytes(hist_n);
    TimerEvents ev, ev2;
    if (kernel_ms) {
        HIP_TRY(hipEventCreate(&ev.e0)); HIP_TRY(hipEventCreate(&ev.e1));
        HIP_TRY(hipEventCreate(&ev2.e0)); HIP_TRY(hipEventCreate(&ev2.e1));
    }
    DevBuf buf[2], hist, offs, tmp, bad;
    HIP_TRY(buf[0].alloc((size_t)m * 8));
    HIP_TRY(buf[1].alloc((size_t)m * 8));
    HIP_TRY(hist.alloc((size_t)hist_n * 4));
    HIP_TRY(offs.alloc((size_t)(hist_n + 1) * 8));
    HIP_TRY(tmp.alloc((size_t)tmp_bytes));
    HIP_TRY(bad.alloc(sizeof(int)));
    HIP_TRY(hipMemsetAsync(bad.get(), 0, sizeof(int), 0));
    // 1. the sort: the first pass reads the caller's array at its stride, later ones ping-pong between the two buffers
    if (kernel_ms) HIP_TRY(hipEventRecord(ev.e0, 0));
    const uint64_t *src = (const uint64_t *)d_kmers;
    int64_t src_stride = stride;
    int cur = 1;                                         // the buffer the next pass reads once it is no longer the input
    for (int shift = 0; shift < key_bits; shift += 8) {
        uint64_t *dst = buf[1 - cur].get<uint64_t>();
        hipLaunchKernelGGL(k_count_hist, dim3((unsigned)n_tiles), dim3(CB), 0, 0, src, m, src_stride, shift,
                           shift == 0 ? key_bits : 0, hist.get<uint32_t>(), n_tiles, bad.get<int>());
        HIP_TRY(hipGetLastError());
        GKI_TRY(gki_scan_u32_to_i64(hist.get<const uint32_t>(), hist_n, offs.get<int64_t>(), tmp.get(), tmp_bytes, 0));
        if (shift == 0) {                                // a key outside key_bits ends the call before anything is scattered
            int h_bad = 0;
            HIP_TRY(hipMemcpy(&h_bad, bad.get(), sizeof(int), hipMemcpyDeviceToHost));
            if (h_bad) return gki_set_error(GKI_ERR_BAD_ARG, "gki_unique_counts_count: a key does not fit key_bits = %d", key_bits);
        }
        hipLaunchKernelGGL(k_count_scatter, dim3((unsigned)n_tiles), dim3(CB), 0, 0, src, m, src_stride, shift,
                           offs.get<const int64_t>(), n_tiles, dst);
        HIP_TRY(hipGetLastError());
        cur = 1 - cur;
        src = dst;
        src_stride = 1;
    }
    if (kernel_ms) { HIP_TRY(hipEventRecord(ev.e1, 0)); HIP_TRY(hipEventRecord(ev2.e0, 0)); }
    // 2. run heads per tile and their scan (the histogram buffer is free again: n_tiles <= hist_n)
    HIP_TRY(p->tile_start.alloc((size_t)(n_tiles + 1) * 8));
    hipLaunchKernelGGL(k_run_count, dim3((unsigned)n_tiles), dim3(CB), 0, 0, src, m, hist.get<uint32_t>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(gki_scan_u32_to_i64(hist.get<const uint32_t>(), n_tiles, p->tile_start.get<int64_t>(), tmp.get(), tmp_bytes, 0));
    if (kernel_ms) HIP_TRY(hipEventRecord(ev2.e1, 0));
    HIP_TRY(hipMemcpy(&p->n_unique, p->tile_start.get<const int64_t>() + n_tiles, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipStreamSynchronize(0));
    if (kernel_ms) {
        HIP_TRY(hipEventElapsedTime(&kernel_ms[0], ev.e0, ev.e1));
        HIP_TRY(hipEventElapsedTime(&kernel_ms[1], ev2.e0, ev2.e1));
    }
    p->sorted.swap(buf[cur]);
    *n_unique = p->n_unique;
    *plan_out = p.release();
    return GKI_OK;
}

int gki_unique_counts_emit(gki_unique_plan *p, void *d_unique, void *d_counts, float *kernel_ms) {
    if (kernel_ms) kernel_ms[0] = 0.f;
    if (p == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "gki_unique_counts_emit: no plan");
    const int64_t nu = p->n_unique;
    if (nu == 0) return GKI_OK;
    if (d_unique == nullptr || d_counts == nullptr)
        return gki_set_error(GKI_ERR_BAD_ARG, "gki_unique_counts_emit: the keys and counts columns are required");
    TimerEvents ev;
    if (kernel_ms) { HIP_TRY(hipEventCreate(&ev.e0)); HIP_TRY(hipEventCreate(&ev.e1)); }
    DevBuf head_pos;
    HIP_TRY(head_pos.alloc((size_t)nu * 8));
    if (kernel_ms) HIP_TRY(hipEventRecord(ev.e0, 0));
    hipLaunchKernelGGL(k_run_emit, dim3((unsigned)p->n_tiles), dim3(CB), 0, 0, p->sorted.get<const uint64_t>(), p->m,
                       p->tile_start.get<const int64_t>(), nu, (uint64_t *)d_unique, head_pos.get<int64_t>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_run_lengths, dim3(stream_grid(nu, 256)), dim3(256), 0, 0, head_pos.get<const int64_t>(), nu, p->m,
                       (int64_t *)d_counts);
    HIP_TRY(hipGetLastError());
    if (kernel_ms) HIP_TRY(hipEventRecord(ev.e1, 0));
    HIP_TRY(hipStreamSynchronize(0));
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(&kernel_ms[0], ev.e0, ev.e1));
    return GKI_OK;
}

int gki_unique_counts_destroy(gki_unique_plan *p) {
    delete p;
    return GKI_OK;
}

int gki_counter_create(const void *d_unique, const void *d_counts, int64_t n_unique, int key_bits, gki_counter **out) {
    *out = nullptr;
    if (n_unique < 0) return gki_set_error(GKI_ERR_BAD_ARG, "gki_counter_create: negative number of keys");
    if (key_bits < 1 || key_bits > 64) return gki_set_error(GKI_ERR_BAD_ARG, "gki_counter_create: key_bits must be in 1..64");
    if (n_unique > 0 && (d_unique == nullptr || d_counts == nullptr))
        return gki_set_error(GKI_ERR_BAD_ARG, "gki_counter_create: no keys or no counts");
    std::unique_ptr<gki_counter> c(new gki_counter());
    HIP_TRY(hipGetDevice(&c->device));
    // 2^dir_bits in (n / 4, n / 2]: two to four keys per bucket on evenly spread keys, a directory of a quarter to a half
    // of the keys' bytes; at most 2^28 entries (2 GiB)
    int log2n = 0;
    while (log2n < 62 && (1ll << log2n) < n_unique) ++log2n;
    int dir_bits = log2n - 2;
    if (dir_bits < 0) dir_bits = 0;
    if (dir_bits > 28) dir_bits = 28;
    if (dir_bits > key_bits) dir_bits = key_bits;
    const int64_t n_dir = 1ll << dir_bits;
    HIP_TRY(c->dir.alloc((size_t)(n_dir + 1) * 8));
    c->v.keys = (const uint64_t *)d_unique;
    c->v.counts = (const int64_t *)d_counts;
    c->v.dir = c->dir.get<const int64_t>();
    c->v.n = n_unique;
    c->v.key_bits = key_bits;
    c->v.dir_bits = dir_bits;
    // dir_bits == 0: shift would be key_bits (64 at most, not a valid shift); the one bucket is [0, n)
    const int shift = dir_bits ? key_bits - dir_bits : 0;
    if (dir_bits == 0) {
        const int64_t h_dir[2] = {0, n_unique};
        HIP_TRY(hipMemcpy(c->dir.get(), h_dir, sizeof(h_dir), hipMemcpyHostToDevice));
    } else {
        hipLaunchKernelGGL(k_counter_directory, dim3(stream_grid(n_dir + 1, 256)), dim3(256), 0, 0, c->v.keys, n_unique, shift,
                           n_dir, c->dir.get<int64_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(0));
    }
    *out = c.release();
    return GKI_OK;
}

int gki_counter_lookup(gki_counter *c, const void *d_queries, int64_t q, void *d_out) {
    GKI_TRY(check_counter_device(c, "gki_counter_lookup"));
    if (q < 0) return gki_set_error(GKI_ERR_BAD_ARG, "gki_counter_lookup: negative number of queries");
    if (q == 0) return GKI_OK;
    if (d_queries == nullptr || d_out == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "gki_counter_lookup: no queries or no output");
    hipLaunchKernelGGL(k_counter_lookup, dim3(stream_grid(q, 256)), dim3(256), 0, 0, c->v, (const uint64_t *)d_queries, q,
                       (int64_t *)d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

int gki_counter_destroy(gki_counter *c) {
    delete c;
    return GKI_OK;
}

}  // extern "C"
