// sample_kmers_from_structural_variants on the device (structural_variants.py:6-43 of the reference): for every
// candidate node longer than k + 5 bases, the windows of the node's own sequence whose get_frequency in the index is
// below max_frequency, thinned greedily from the left so that no two chosen windows overlap.
//
//   k_sv_words    one lane per candidate: its number of 64-window bitmap words (0 when the size test fails)
//   k_sv_probe    one wave per bitmap word, one lane per window: the k-mer is a bit-field of the packed sequence, two
//                 probes (the k-mer, its 31-mer reverse complement), a ballot of f < max_frequency is the word
//   k_sv_greedy   one wave per candidate: 64 bitmap words per load, then "first set bit at or after prev + k" as a
//                 ballot over the masked words -- O(size / k) uniform steps.  Runs twice: the count pass leaves the number
//                 chosen per candidate, after the scan the emit pass leaves every chosen window's position and node
//   k_sv_records  one lane per record: the hash read again from the position, the node, offset 0, allele frequency 1
//
// Every output is sized by an exact count.  Every per-lane quantity is a scalar in registers.
#include "gki_frequency.h"
#include <memory>

// What the count call leaves for the emit call.  The graph must outlive the plan.
struct gki_sv_plan {
    gki_graph *g = nullptr;
    int64_t n_cand = 0, n_words = 0, n_records = 0;
    int k = 0;
    DevBuf cand;             // int32[n_cand]: the caller's candidates
    DevBuf word_start;       // int64[n_cand + 1]: first bitmap word of every candidate
    DevBuf bitmap;           // uint64[n_words]: bit j % 64 of word word_start[i] + j / 64 = window j of candidate i is valid
    DevBuf rec_start;        // int64[n_cand + 1]: first record of every candidate
};

namespace {

__global__ __launch_bounds__(256) void k_sv_words(const int32_t *__restrict__ cand, int64_t n_cand,
                                                  const int32_t *__restrict__ node_size, int64_t n_nodes, int k,
                                                  uint32_t *__restrict__ words, unsigned long long *__restrict__ first_bad) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cand; i += stride) {
        const int32_t node = cand[i];
        uint32_t w = 0;
        if (node < 0 || node >= n_nodes) atomicMin(first_bad, (unsigned long long)i);
        else {
            const int32_t size = node_size[node];
            if (size > k + 5) w = (uint32_t)(((int64_t)size - k + 1 + 63) >> 6);       // structural_variants.py:18
        }
        words[i] = w;
    }
}

__global__ __launch_bounds__(256) void k_sv_probe(const int32_t *__restrict__ cand, const int64_t *__restrict__ word_start,
                                                  int64_t n_cand, int64_t n_words, const int32_t *__restrict__ node_size,
                                                  const int64_t *__restrict__ seq_start, const uint64_t *__restrict__ seq2,
                                                  int k, int64_t max_frequency, GkiIndexSource ix, uint64_t *__restrict__ bitmap) {
    sv_probe_body(cand, word_start, n_cand, n_words, node_size, seq_start, seq2, k, max_frequency, ix, bitmap);
}

// the value lane l (uniform) holds, in scalar registers
__device__ __forceinline__ uint64_t sv_lane_value(uint64_t v, int l) {
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// structural_variants.py:24-30: in ascending order a valid window is chosen iff it lies at or after prev + k.  `pos` is
// the first window that may be chosen next (0 at the start: prev = -10000).  EMIT: the j-th chosen window of candidate i
// goes to record rec_start[i] + j, never past rec_start[i + 1].
template <bool EMIT>
__global__ __launch_bounds__(256) void k_sv_greedy(const int32_t *__restrict__ cand, const int64_t *__restrict__ word_start,
                                                   int64_t n_cand, const uint64_t *__restrict__ bitmap, int k,
                                                   uint32_t *__restrict__ count, const int64_t *__restrict__ rec_start,
                                                   const int64_t *__restrict__ seq_start, int64_t *__restrict__ rec_pos,
                                                   uint32_t *__restrict__ rec_node) {
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i = sv_wave(); i < n_cand; i += n_waves) {
        const int64_t ws = word_start[i], nw = word_start[i + 1] - ws;
        const int32_t node = cand[i];
        int64_t o = 0, o_end = 0, base = 0;
        if (EMIT) { o = rec_start[i]; o_end = rec_start[i + 1]; base = seq_start[node]; }
        int64_t pos = 0;
        uint32_t cnt = 0;
        for (int64_t cb = 0; cb < nw; cb += 64) {            // 64 words = 4096 windows per load
            const uint64_t word = cb + lane < nw ? bitmap[ws + cb + lane] : 0ull;
            while (true) {
                int64_t rel = pos - cb * 64;
                if (rel < 0) rel = 0;
                if (rel >= 4096) break;
                const int pw = (int)(rel >> 6), pb = (int)(rel & 63);
                const uint64_t m = lane < pw ? 0ull : lane == pw ? (word & (~0ull << pb)) : word;
                const uint64_t has = __ballot(m != 0ull);
                if (has == 0ull) break;
                const int l = __builtin_amdgcn_readfirstlane(__builtin_ctzll(has));
                const int64_t j = (cb + l) * 64 + __builtin_ctzll(sv_lane_value(m, l));
                if (EMIT && lane == 0 && o + cnt < o_end) {
                    rec_pos[o + cnt] = base + j;
                    rec_node[o + cnt] = (uint32_t)node;
                }
                ++cnt;
                pos = j + k;
            }
        }
        if (!EMIT && lane == 0) count[i] = cnt;
    }
}

__global__ __launch_bounds__(256) void k_sv_records(const int64_t *__restrict__ rec_pos, const uint32_t *__restrict__ rec_node,
                                                    int64_t n, const uint64_t *__restrict__ seq2, int k,
                                                    uint64_t *__restrict__ hashes, uint32_t *__restrict__ nodes,
                                                    uint64_t *__restrict__ ref_offsets, float *__restrict__ af) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < n; o += stride) {
        hashes[o] = gki_extract(seq2, rec_pos[o], k);
        nodes[o] = rec_node[o];
        if (ref_offsets) ref_offsets[o] = 0ull;              // structural_variants.py:38
        if (af) af[o] = 1.0f;                                // FlatKmers' default
    }
}

// gki_sv_sample_count with either frequency source: the index, or the counter when there is one
int sv_sample_count(gki_graph *g, const gki_index_view *ix, const gki_counter *counter, const void *d_cand_nodes,
                    int64_t n_cand, int k, int64_t max_frequency, void *d_rec_start, int64_t *n_records,
                    gki_sv_plan **plan_out, float *kernel_ms) {
    *n_records = 0;
    *plan_out = nullptr;
    if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.f;
    if (k < 1 || k > GKI_MAX_K) return gki_set_error(GKI_ERR_BAD_ARG, "k must be in 1..31");
    if (max_frequency < 0) return gki_set_error(GKI_ERR_BAD_ARG, "gki_sv_sample_count: max_frequency must not be negative");
    if (n_cand < 0 || n_cand > (1ll << 31)) return gki_set_error(GKI_ERR_BAD_ARG, "gki_sv_sample_count: bad candidate count");
    if (counter == nullptr && (ix == nullptr || ix->modulo == 0))
        return gki_set_error(GKI_ERR_BAD_ARG, "gki_sv_sample_count: no frequency index");
    GKI_TRY(gki_check_graph_device(g, "gki_sv_sample_count"));
    std::unique_ptr<gki_sv_plan> p(new gki_sv_plan());
    p->g = g;
    p->n_cand = n_cand;
    p->k = k;
    HIP_TRY(p->rec_start.alloc((size_t)(n_cand + 1) * 8));
    if (n_cand == 0) {
        HIP_TRY(hipMemset(p->rec_start.get(), 0, 8));
        if (d_rec_start) HIP_TRY(hipMemset(d_rec_start, 0, 8));
        *plan_out = p.release();
        return GKI_OK;
    }
    TimerEvents ev, ev2;
    if (kernel_ms) {
        HIP_TRY(hipEventCreate(&ev.e0)); HIP_TRY(hipEventCreate(&ev.e1));
        HIP_TRY(hipEventCreate(&ev2.e0)); HIP_TRY(hipEventCreate(&ev2.e1));
    }
    const int64_t tmp_bytes = gki_scan_tmp_bytes(n_cand);
    DevBuf cnt, tmp, bad;
    HIP_TRY(p->cand.alloc((size_t)n_cand * 4));
    HIP_TRY(p->word_start.alloc((size_t)(n_cand + 1) * 8));
    HIP_TRY(cnt.alloc((size_t)n_cand * 4));
    HIP_TRY(tmp.alloc((size_t)tmp_bytes));
    HIP_TRY(bad.alloc(8));
    HIP_TRY(hipMemcpyAsync(p->cand.get(), d_cand_nodes, (size_t)n_cand * 4, hipMemcpyDeviceToDevice, 0));
    HIP_TRY(hipMemsetAsync(bad.get(), 0xFF, 8, 0));
    const DevGraph &d = g->d;
    const int32_t *cand = p->cand.get<const int32_t>();
    // 1. bitmap words per candidate; a node id outside the graph ends the call before anything is read through it
    hipLaunchKernelGGL(k_sv_words, dim3(stream_grid(n_cand, 256)), dim3(256), 0, 0, cand, n_cand, d.node_size, d.n_nodes, k,
                       cnt.get<uint32_t>(), bad.get<unsigned long long>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(gki_scan_u32_to_i64(cnt.get<const uint32_t>(), n_cand, p->word_start.get<int64_t>(), tmp.get(), tmp_bytes, 0));
    unsigned long long h_bad = ~0ull;
    HIP_TRY(hipMemcpy(&h_bad, bad.get(), 8, hipMemcpyDeviceToHost));
    if (h_bad != ~0ull)
        return gki_set_error(GKI_ERR_BAD_ARG, "gki_sv_sample_count: candidate %lld is not a node of the graph (%lld nodes)",
                             (long long)h_bad, (long long)d.n_nodes);
    HIP_TRY(hipMemcpy(&p->n_words, p->word_start.get<const int64_t>() + n_cand, 8, hipMemcpyDeviceToHost));
    HIP_TRY(p->bitmap.alloc((size_t)(p->n_words > 0 ? p->n_words : 1) * 8));
    // 2. the valid bitmap: every word of it is written
    if (kernel_ms) HIP_TRY(hipEventRecord(ev.e0, 0));
    if (p->n_words > 0 && counter != nullptr) {
        GKI_TRY(gki_launch_sv_probe_counter(counter, cand, p->word_start.get<const int64_t>(), n_cand, p->n_words, d, k,
                                            max_frequency, p->bitmap.get<uint64_t>()));
    } else if (p->n_words > 0) {
        hipLaunchKernelGGL(k_sv_probe, dim3(stream_grid(ceil_div(p->n_words, SV_CHUNK) * 64, 256)), dim3(256), 0, 0, cand,
                           p->word_start.get<const int64_t>(), n_cand, p->n_words, d.node_size, d.seq_start, d.seq2, k,
                           max_frequency, gki_index_source(ix), p->bitmap.get<uint64_t>());
        HIP_TRY(hipGetLastError());
    }
    if (kernel_ms) { HIP_TRY(hipEventRecord(ev.e1, 0)); HIP_TRY(hipEventRecord(ev2.e0, 0)); }
    // 3. the number chosen per candidate, and its scan
    hipLaunchKernelGGL(k_sv_greedy<false>, dim3(stream_grid(n_cand * 64, 256)), dim3(256), 0, 0, cand,
                       p->word_start.get<const int64_t>(), n_cand, p->bitmap.get<const uint64_t>(), k, cnt.get<uint32_t>(),
                       (const int64_t *)nullptr, (const int64_t *)nullptr, (int64_t *)nullptr, (uint32_t *)nullptr);
    HIP_TRY(hipGetLastError());
    GKI_TRY(gki_scan_u32_to_i64(cnt.get<const uint32_t>(), n_cand, p->rec_start.get<int64_t>(), tmp.get(), tmp_bytes, 0));
    if (kernel_ms) HIP_TRY(hipEventRecord(ev2.e1, 0));
    HIP_TRY(hipMemcpy(&p->n_records, p->rec_start.get<const int64_t>() + n_cand, 8, hipMemcpyDeviceToHost));
    if (d_rec_start)
        HIP_TRY(hipMemcpy(d_rec_start, p->rec_start.get(), (size_t)(n_cand + 1) * 8, hipMemcpyDeviceToDevice));
    HIP_TRY(hipStreamSynchronize(0));
    if (kernel_ms) {
        HIP_TRY(hipEventElapsedTime(&kernel_ms[0], ev.e0, ev.e1));
        HIP_TRY(hipEventElapsedTime(&kernel_ms[1], ev2.e0, ev2.e1));
    }
    *n_records = p->n_records;
    *plan_out = p.release();
    return GKI_OK;
}

}  // namespace

extern "C" {

int gki_sv_sample_count(gki_graph *g, const gki_index_view *ix, const void *d_cand_nodes, int64_t n_cand, int k,
                        int64_t max_frequency, void *d_rec_start, int64_t *n_records, gki_sv_plan **plan_out,
                        float *kernel_ms) {
    return sv_sample_count(g, ix, nullptr, d_cand_nodes, n_cand, k, max_frequency, d_rec_start, n_records, plan_out, kernel_ms);
}

int gki_sv_sample_count_counter(gki_graph *g, const gki_counter *counter, const void *d_cand_nodes, int64_t n_cand, int k,
                                int64_t max_frequency, void *d_rec_start, int64_t *n_records, gki_sv_plan **plan_out,
                                float *kernel_ms) {
    if (counter == nullptr) {
        *n_records = 0;
        *plan_out = nullptr;
        return gki_set_error(GKI_ERR_BAD_ARG, "gki_sv_sample_count_counter: no counter");
    }
    return sv_sample_count(g, nullptr, counter, d_cand_nodes, n_cand, k, max_frequency, d_rec_start, n_records, plan_out,
                           kernel_ms);
}

int gki_sv_sample_emit(gki_sv_plan *p, void *d_hashes, void *d_nodes, void *d_ref_offsets, void *d_af32, float *kernel_ms) {
    if (kernel_ms) kernel_ms[0] = 0.f;
    if (p == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "gki_sv_sample_emit: no plan");
    GKI_TRY(gki_check_graph_device(p->g, "gki_sv_sample_emit"));
    const int64_t n = p->n_records;
    if (n == 0) return GKI_OK;
    if (d_hashes == nullptr || d_nodes == nullptr)
        return gki_set_error(GKI_ERR_BAD_ARG, "gki_sv_sample_emit: the hashes and nodes columns are required");
    TimerEvents ev;
    if (kernel_ms) { HIP_TRY(hipEventCreate(&ev.e0)); HIP_TRY(hipEventCreate(&ev.e1)); }
    DevBuf rec_pos, rec_node;
    HIP_TRY(rec_pos.alloc((size_t)n * 8));
    HIP_TRY(rec_node.alloc((size_t)n * 4));
    const DevGraph &d = p->g->d;
    if (kernel_ms) HIP_TRY(hipEventRecord(ev.e0, 0));
    hipLaunchKernelGGL(k_sv_greedy<true>, dim3(stream_grid(p->n_cand * 64, 256)), dim3(256), 0, 0, p->cand.get<const int32_t>(),
                       p->word_start.get<const int64_t>(), p->n_cand, p->bitmap.get<const uint64_t>(), p->k,
                       (uint32_t *)nullptr, p->rec_start.get<const int64_t>(), d.seq_start, rec_pos.get<int64_t>(),
                       rec_node.get<uint32_t>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sv_records, dim3(stream_grid(n, 256)), dim3(256), 0, 0, rec_pos.get<const int64_t>(),
                       rec_node.get<const uint32_t>(), n, d.seq2, p->k, (uint64_t *)d_hashes, (uint32_t *)d_nodes,
                       (uint64_t *)d_ref_offsets, (float *)d_af32);
    HIP_TRY(hipGetLastError());
    if (kernel_ms) HIP_TRY(hipEventRecord(ev.e1, 0));
    HIP_TRY(hipStreamSynchronize(0));
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(&kernel_ms[0], ev.e0, ev.e1));
    return GKI_OK;
}

int gki_sv_sample_destroy(gki_sv_plan *p) {
    delete p;
    return GKI_OK;
}

}  // extern "C"
