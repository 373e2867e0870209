// Node counts of a sample haplotype by its difference from the all-ref path, and the count model over many samples.  The
// rules are those of include/gki.h ("haplotype segments", "node count model") and DESIGN.md 4.20.
//
// A window of a slot's sequence that touches no alt allele the slot takes occurs in the all-ref path too, so only the
// windows around the taken lines are probed: those of the all-ref path are taken away, those of the slot's sequence added
// (k_probe_segments, gki_probe.hip).  This file lists them.  With the kept lines j = 0 .. K - 1 and a spell count call of the
// slot behind us (its before / cut / bounds are the plan's):
//   (scan of alt_size), k_seg_ref_bounds   once per plan: before and bounds of the all-ref path, which drops every alt
//   k_seg_taken_flags  one lane per kept line: does the slot take its alt allele
//   (exclusive scan)   rank[j]; k_seg_taken_emit compacts: taken[rank[j]] = j
//   k_seg_runs<false>  one lane per taken line: its run of dirty windows in either sequence; 1 or 0 segments each, and the
//                      windows of both summed
//   (two scans)        where a taken line's segment goes in either list
//   k_seg_runs<true>   the same run again, written: seg_start, seg_windows
// The count model: k_model_row_start makes an individual's row ploidy x the base row, for its slots' passes to change;
// k_model_accumulate, one lane per kept line, adds the finished row to the line's two histograms.
#include "gki_haplotype_plan.h"
#include "gki_seq_gather.h"

namespace {

constexpr int SEG_BLOCK = 256;

// bounds[c] of the all-ref path, c = 0 .. n_chrom, as k_hap_cuts forms a slot's
__global__ __launch_bounds__(SEG_BLOCK) void k_seg_ref_bounds(int n_chrom, const int64_t *__restrict__ chrom_seq_start,
                                                              const int64_t *__restrict__ chrom_first_kept,
                                                              const int64_t *__restrict__ ref_before,
                                                              int64_t *__restrict__ ref_bounds) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c <= n_chrom; c += stride)
        ref_bounds[c] = chrom_seq_start[c] - ref_before[chrom_first_kept[c]];
}

__global__ __launch_bounds__(SEG_BLOCK) void k_seg_taken_flags(int64_t K, const int64_t *__restrict__ kline,
                                                               const uint64_t *__restrict__ slot_bits,
                                                               uint32_t *__restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < K; j += stride) {
        const int64_t line = kline[j];
        flag[j] = (uint32_t)((slot_bits[line >> 6] >> (line & 63)) & 1ull);
    }
}

__global__ __launch_bounds__(SEG_BLOCK) void k_seg_taken_emit(int64_t K, const uint32_t *__restrict__ flag,
                                                              const int64_t *__restrict__ rank, int64_t *__restrict__ taken) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < K; j += stride)
        if (flag[j]) taken[rank[j]] = j;
}

struct SegPlan {
    const int64_t *ref_start;
    const int32_t *ref_size, *alt_size;
    const int64_t *ref_before, *ref_bounds;                // the all-ref path
    const int64_t *cut, *bounds;                           // the slot's sequence
    const int64_t *chrom_first_kept;
    int n_chrom, k;
};

// the dirty windows of the interval [a, b) that no earlier taken line owns, inside the chromosome [c_lo, c_hi)
__device__ __forceinline__ void seg_run(int64_t a, int64_t b, int64_t b_prev, int64_t c_lo, int64_t c_hi, int k, int64_t *lo,
                                        int64_t *n) {
    int64_t l = a - k + 1, h = b - 1;
    if (l < b_prev) l = b_prev;
    if (l < c_lo) l = c_lo;
    if (h > c_hi - k) h = c_hi - k;
    *lo = l;
    *n = h >= l ? h - l + 1 : 0;
}

// One lane per taken line r; the trip count is the same for every lane of a wave, for wave_add64.  !EMIT: has_ref[r] and
// has_slot[r] are 1 where the line's run in that sequence is not empty, windows[0 / 1] += the runs' lengths.  EMIT: the
// runs are written where ref_at / slot_at say.
template <bool EMIT>
__global__ __launch_bounds__(SEG_BLOCK) void k_seg_runs(SegPlan p, int64_t n_taken, const int64_t *__restrict__ taken,
                                                        uint32_t *__restrict__ has_ref, uint32_t *__restrict__ has_slot,
                                                        unsigned long long *__restrict__ windows,
                                                        const int64_t *__restrict__ ref_at, const int64_t *__restrict__ slot_at,
                                                        int64_t *__restrict__ ref_seg_start, int64_t *__restrict__ ref_seg_windows,
                                                        int64_t *__restrict__ slot_seg_start,
                                                        int64_t *__restrict__ slot_seg_windows) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint64_t w_ref = 0, w_slot = 0;
    for (int64_t r0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); r0 < n_taken; r0 += stride) {
        const int64_t r = r0 + (threadIdx.x & 63);
        if (r >= n_taken) continue;
        const int64_t j = taken[r], jp = r > 0 ? taken[r - 1] : -1;
        // chromosome c holds the kept lines chrom_first_kept[c] .. chrom_first_kept[c + 1] - 1
        int64_t c = first_site_after(p.chrom_first_kept, 0, (int64_t)p.n_chrom + 1, j) - 1;
        c = c < 0 ? 0 : c >= p.n_chrom ? p.n_chrom - 1 : c;
        int64_t lo, n;
        {                                                  // the all-ref path: the line's ref allele
            const int64_t a = p.ref_start[j] - p.ref_before[j];
            const int64_t b_prev = jp >= 0 ? p.ref_start[jp] - p.ref_before[jp] + p.ref_size[jp] : 0;
            seg_run(a, a + p.ref_size[j], b_prev, p.ref_bounds[c], p.ref_bounds[c + 1], p.k, &lo, &n);
            if (EMIT) {
                if (n > 0) { const int64_t o = ref_at[r]; ref_seg_start[o] = lo; ref_seg_windows[o] = n; }
            } else {
                has_ref[r] = n > 0;
                w_ref += (uint64_t)n;
            }
        }
        {                                                  // the slot's sequence: the line's alt allele, at its cut
            const int64_t a = p.cut[j];
            const int64_t b_prev = jp >= 0 ? p.cut[jp] + p.alt_size[jp] : 0;
            seg_run(a, a + p.alt_size[j], b_prev, p.bounds[c], p.bounds[c + 1], p.k, &lo, &n);
            if (EMIT) {
                if (n > 0) { const int64_t o = slot_at[r]; slot_seg_start[o] = lo; slot_seg_windows[o] = n; }
            } else {
                has_slot[r] = n > 0;
                w_slot += (uint64_t)n;
            }
        }
    }
    if (!EMIT) {
        wave_add64(&windows[0], w_ref);
        wave_add64(&windows[1], w_slot);
    }
}

// row[i] = copies * base[i], modulo 2^32 as every count
__global__ __launch_bounds__(SEG_BLOCK) void k_model_row_start(int64_t n, const uint32_t *__restrict__ base, uint32_t copies,
                                                               uint32_t *__restrict__ row) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) row[i] = copies * base[i];
}

// One lane per kept line, which owns the line's entries: no atomics.  c_alt of the individual's `ploidy` slots take the alt
// allele; the row's count of the ref node goes to entry (line, 0, ploidy - c_alt), that of the var node to (line, 1, c_alt).
__global__ __launch_bounds__(SEG_BLOCK) void k_model_accumulate(int64_t K, const int64_t *__restrict__ kline,
                                                                const uint32_t *__restrict__ var_nodes,
                                                                const uint64_t *__restrict__ alt_bits, int64_t W,
                                                                int64_t first_slot, int ploidy,
                                                                const uint32_t *__restrict__ row, int64_t n_nodes, int n_bins,
                                                                uint32_t *__restrict__ histogram,
                                                                unsigned long long *__restrict__ count_sum) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < K; j += stride) {
        const int64_t line = kline[j];
        int c_alt = 0;
        for (int i = 0; i < ploidy; i++) c_alt += (int)((alt_bits[(first_slot + i) * W + (line >> 6)] >> (line & 63)) & 1ull);
        const int64_t var = var_nodes[line], ref = var - 1;               // a bubble: the two allele nodes side by side
        const uint32_t count[2] = {ref < n_nodes ? row[ref] : 0u, var < n_nodes ? row[var] : 0u};
        const int copies[2] = {ploidy - c_alt, c_alt};
#pragma unroll
        for (int allele = 0; allele < 2; allele++) {
            const int64_t e = (line * 2 + allele) * (ploidy + 1) + copies[allele];
            const uint32_t bin = count[allele] < (uint32_t)(n_bins - 1) ? count[allele] : (uint32_t)(n_bins - 1);
            histogram[e * n_bins + bin] += 1u;
            count_sum[e] += count[allele];
        }
    }
}

// before and bounds of the all-ref path, once per plan
int ensure_ref_path(gki_haplotype_paths &g) {
    if (g.has_ref_path) return GKI_OK;
    const int64_t K = g.K;
    DevBuf before, bounds, tmp;
    HIP_TRY(before.alloc((size_t)(K + 1) * 8));
    HIP_TRY(bounds.alloc((size_t)(g.n_chrom + 1) * 8));
    HIP_TRY(hipMemsetAsync(before.get(), 0, (size_t)(K + 1) * 8, 0));      // K == 0: before = [0], no scan runs
    if (K > 0) {
        const int64_t tmp_bytes = gki_scan_tmp_bytes(K);
        HIP_TRY(tmp.alloc((size_t)tmp_bytes));
        GKI_TRY(gki_scan_i32_to_i64(g.alt_size.get<const int32_t>(), K, before.get<int64_t>(), tmp.get(), tmp_bytes, 0));
    }
    hipLaunchKernelGGL(k_seg_ref_bounds, dim3(stream_grid(g.n_chrom + 1, SEG_BLOCK)), dim3(SEG_BLOCK), 0, 0, g.n_chrom,
                       g.chrom_seq_start.get<const int64_t>(), g.chrom_first_kept.get<const int64_t>(),
                       before.get<const int64_t>(), bounds.get<int64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    g.ref_before.swap(before);
    g.ref_bounds.swap(bounds);
    g.has_ref_path = true;
    return GKI_OK;
}

SegPlan seg_plan_of(const gki_haplotype_paths &g, int k) {
    SegPlan p;
    p.ref_start = g.ref_start.get<const int64_t>();
    p.ref_size = g.ref_size.get<const int32_t>();
    p.alt_size = g.alt_size.get<const int32_t>();
    p.ref_before = g.ref_before.get<const int64_t>();
    p.ref_bounds = g.ref_bounds.get<const int64_t>();
    p.cut = g.cut.get<const int64_t>();
    p.bounds = g.bounds.get<const int64_t>();
    p.chrom_first_kept = g.chrom_first_kept.get<const int64_t>();
    p.n_chrom = g.n_chrom;
    p.k = k;
    return p;
}

// what a segments count call leaves in the plan goes back unless the call succeeds
void drop_segments(gki_haplotype_paths &g) {
    g.seg_taken.reset();
    g.seg_ref_at.reset();
    g.seg_slot_at.reset();
    g.seg_n_taken = -1;
}

int segments_count(gki_haplotype_paths &g, const void *d_alt_bits, int64_t slot, int k, int64_t *totals, float *kernel_ms) {
    GKI_TRY(ensure_ref_path(g));
    const int64_t K = g.K;
    int64_t n_taken = 0;
    TimerEvents ev;
    float ms = 0.0f;
    if (K > 0) {
        DevBuf flag, rank, tmp;
        const int64_t tmp_bytes = gki_scan_tmp_bytes(K);
        HIP_TRY(flag.alloc((size_t)K * 4));
        HIP_TRY(rank.alloc((size_t)(K + 1) * 8));
        HIP_TRY(tmp.alloc((size_t)tmp_bytes));
        GKI_TRY(ev.start(0));
        hipLaunchKernelGGL(k_seg_taken_flags, dim3(stream_grid(K, SEG_BLOCK)), dim3(SEG_BLOCK), 0, 0, K,
                           g.kline.get<const int64_t>(), (const uint64_t *)d_alt_bits + slot * g.W, flag.get<uint32_t>());
        HIP_TRY(hipGetLastError());
        GKI_TRY(gki_scan_u32_to_i64(flag.get<const uint32_t>(), K, rank.get<int64_t>(), tmp.get(), tmp_bytes, 0));
        GKI_TRY(ev.stop(0, &ms));
        if (kernel_ms) *kernel_ms += ms;
        HIP_TRY(hipMemcpy(&n_taken, rank.get<const int64_t>() + K, 8, hipMemcpyDeviceToHost));
        if (n_taken < 0 || n_taken > K)
            return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_segments_count: %lld taken lines of %lld (internal)", (long long)n_taken, (long long)K);
        if (n_taken > 0) {
            HIP_TRY(g.seg_taken.alloc((size_t)n_taken * 8));
            GKI_TRY(ev.start(0));
            hipLaunchKernelGGL(k_seg_taken_emit, dim3(stream_grid(K, SEG_BLOCK)), dim3(SEG_BLOCK), 0, 0, K,
                               flag.get<const uint32_t>(), rank.get<const int64_t>(), g.seg_taken.get<int64_t>());
            HIP_TRY(hipGetLastError());
            GKI_TRY(ev.stop(0, &ms));
            if (kernel_ms) *kernel_ms += ms;
        }
    }
    totals[0] = n_taken;
    if (n_taken > 0) {
        DevBuf has_ref, has_slot, windows, tmp;
        const int64_t tmp_bytes = gki_scan_tmp_bytes(n_taken);
        HIP_TRY(has_ref.alloc((size_t)n_taken * 4));
        HIP_TRY(has_slot.alloc((size_t)n_taken * 4));
        HIP_TRY(windows.alloc(16));
        HIP_TRY(tmp.alloc((size_t)tmp_bytes));
        HIP_TRY(g.seg_ref_at.alloc((size_t)(n_taken + 1) * 8));
        HIP_TRY(g.seg_slot_at.alloc((size_t)(n_taken + 1) * 8));
        HIP_TRY(hipMemsetAsync(windows.get(), 0, 16, 0));
        GKI_TRY(ev.start(0));
        hipLaunchKernelGGL(k_seg_runs<false>, dim3(stream_grid(n_taken, SEG_BLOCK)), dim3(SEG_BLOCK), 0, 0, seg_plan_of(g, k),
                           n_taken, g.seg_taken.get<const int64_t>(), has_ref.get<uint32_t>(), has_slot.get<uint32_t>(),
                           windows.get<unsigned long long>(), (const int64_t *)nullptr, (const int64_t *)nullptr,
                           (int64_t *)nullptr, (int64_t *)nullptr, (int64_t *)nullptr, (int64_t *)nullptr);
        HIP_TRY(hipGetLastError());
        GKI_TRY(gki_scan_u32_to_i64(has_ref.get<const uint32_t>(), n_taken, g.seg_ref_at.get<int64_t>(), tmp.get(), tmp_bytes, 0));
        GKI_TRY(gki_scan_u32_to_i64(has_slot.get<const uint32_t>(), n_taken, g.seg_slot_at.get<int64_t>(), tmp.get(), tmp_bytes, 0));
        GKI_TRY(ev.stop(0, &ms));
        if (kernel_ms) *kernel_ms += ms;
        unsigned long long w[2] = {0, 0};
        HIP_TRY(hipMemcpy(&totals[1], g.seg_ref_at.get<const int64_t>() + n_taken, 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&totals[3], g.seg_slot_at.get<const int64_t>() + n_taken, 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(w, windows.get(), 16, hipMemcpyDeviceToHost));
        totals[2] = (int64_t)w[0];
        totals[4] = (int64_t)w[1];
    }
    return GKI_OK;
}

}  // namespace

extern "C" {

int gki_haplotype_segments_count(gki_haplotype_paths *plan, const void *d_alt_bits, int64_t n_slots, int64_t slot, int k,
                                 int64_t *n_taken, int64_t *n_ref_segs, int64_t *n_ref_windows, int64_t *n_slot_segs,
                                 int64_t *n_slot_windows, float *kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    int64_t *outs[5] = {n_taken, n_ref_segs, n_ref_windows, n_slot_segs, n_slot_windows};
    for (int64_t *o : outs) if (o) *o = 0;
    GKI_TRY(gki_check_haplotype_plan(plan, "haplotype_segments_count"));
    gki_haplotype_paths &g = *plan;
    drop_segments(g);
    for (int64_t *o : outs)
        if (o == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_segments_count: a total's pointer is NULL");
    if (k < 1 || k > GKI_MAX_K) return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_segments_count: k must be in 1..31");
    if (slot < 0 || slot >= n_slots || (g.W > 0 && d_alt_bits == nullptr))
        return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_segments_count: slot %lld of %lld, or the plane is NULL", (long long)slot,
                             (long long)n_slots);
    if (g.spelled_slot != slot || g.spelled_plane != d_alt_bits)
        return gki_set_error(GKI_ERR_STATE, "haplotype_segments_count: the last spell count call was not of slot %lld of this plane",
                             (long long)slot);
    int64_t totals[5] = {0, 0, 0, 0, 0};
    const int rc = segments_count(g, d_alt_bits, slot, k, totals, kernel_ms);
    if (rc != GKI_OK) { drop_segments(g); return rc; }
    g.seg_n_taken = totals[0];
    g.seg_n_ref = totals[1];
    g.seg_n_slot = totals[3];
    g.seg_k = k;
    g.seg_slot = slot;
    g.seg_plane = d_alt_bits;
    for (int i = 0; i < 5; i++) *outs[i] = totals[i];
    return GKI_OK;
}

int gki_haplotype_segments_emit(gki_haplotype_paths *plan, void *d_ref_seg_start, void *d_ref_seg_windows,
                                void *d_slot_seg_start, void *d_slot_seg_windows, float *kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    GKI_TRY(gki_check_haplotype_plan(plan, "haplotype_segments_emit"));
    gki_haplotype_paths &g = *plan;
    if (g.seg_n_taken < 0) return gki_set_error(GKI_ERR_STATE, "haplotype_segments_emit: no segments count call came before");
    DevBuf taken, ref_at, slot_at;                         // the plan's go back to the pool when the call returns
    taken.swap(g.seg_taken);
    ref_at.swap(g.seg_ref_at);
    slot_at.swap(g.seg_slot_at);
    const int64_t n_taken = g.seg_n_taken;
    g.seg_n_taken = -1;
    if (g.spelled_slot != g.seg_slot || g.spelled_plane != g.seg_plane)
        return gki_set_error(GKI_ERR_STATE, "haplotype_segments_emit: another slot or plane was spelled since the count call");
    if (n_taken == 0 || (g.seg_n_ref == 0 && g.seg_n_slot == 0)) return GKI_OK;
    if ((g.seg_n_ref > 0 && (d_ref_seg_start == nullptr || d_ref_seg_windows == nullptr)) ||
        (g.seg_n_slot > 0 && (d_slot_seg_start == nullptr || d_slot_seg_windows == nullptr)))
        return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_segments_emit: an output is NULL");
    TimerEvents ev;
    GKI_TRY(ev.start(0));
    hipLaunchKernelGGL(k_seg_runs<true>, dim3(stream_grid(n_taken, SEG_BLOCK)), dim3(SEG_BLOCK), 0, 0, seg_plan_of(g, g.seg_k),
                       n_taken, taken.get<const int64_t>(), (uint32_t *)nullptr, (uint32_t *)nullptr,
                       (unsigned long long *)nullptr, ref_at.get<const int64_t>(), slot_at.get<const int64_t>(),
                       (int64_t *)d_ref_seg_start, (int64_t *)d_ref_seg_windows, (int64_t *)d_slot_seg_start,
                       (int64_t *)d_slot_seg_windows);
    HIP_TRY(hipGetLastError());
    return ev.stop(0, kernel_ms);
}

int gki_node_count_model_row_start(const void *d_base, int64_t n_nodes, int ploidy, void *d_row) {
    if (ploidy < 1 || ploidy > 8) return gki_set_error(GKI_ERR_BAD_ARG, "node_count_model_row_start: ploidy must be in 1..8");
    if (n_nodes < 0 || (n_nodes > 0 && (d_base == nullptr || d_row == nullptr)))
        return gki_set_error(GKI_ERR_BAD_ARG, "node_count_model_row_start: n_nodes is negative or a row is NULL");
    if (n_nodes == 0) return GKI_OK;
    hipLaunchKernelGGL(k_model_row_start, dim3(stream_grid(n_nodes, SEG_BLOCK)), dim3(SEG_BLOCK), 0, 0, n_nodes,
                       (const uint32_t *)d_base, (uint32_t)ploidy, (uint32_t *)d_row);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

int gki_node_count_model_accumulate(gki_haplotype_paths *plan, const void *d_alt_bits, int64_t n_slots, int64_t first_slot,
                                    int ploidy, const void *d_row, int64_t n_nodes, int n_bins, void *d_histogram,
                                    void *d_count_sum, float *kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    GKI_TRY(gki_check_haplotype_plan(plan, "node_count_model_accumulate"));
    gki_haplotype_paths &g = *plan;
    if (ploidy < 1 || ploidy > 8) return gki_set_error(GKI_ERR_BAD_ARG, "node_count_model_accumulate: ploidy must be in 1..8");
    if (n_bins < 2 || n_bins > 65536) return gki_set_error(GKI_ERR_BAD_ARG, "node_count_model_accumulate: n_bins must be in 2..65536");
    if (first_slot < 0 || n_slots < ploidy || first_slot > n_slots - ploidy || n_nodes < 0 || (n_nodes > 0 && d_row == nullptr) ||
        (g.W > 0 && d_alt_bits == nullptr) || (g.n_lines > 0 && (d_histogram == nullptr || d_count_sum == nullptr)))
        return gki_set_error(GKI_ERR_BAD_ARG, "node_count_model_accumulate: slots %lld .. of %lld, or a pointer is NULL",
                             (long long)first_slot, (long long)n_slots);
    if (g.K == 0) return GKI_OK;
    TimerEvents ev;
    GKI_TRY(ev.start(0));
    hipLaunchKernelGGL(k_model_accumulate, dim3(stream_grid(g.K, SEG_BLOCK)), dim3(SEG_BLOCK), 0, 0, g.K,
                       g.kline.get<const int64_t>(), g.var_nodes.get<const uint32_t>(), (const uint64_t *)d_alt_bits, g.W,
                       first_slot, ploidy, (const uint32_t *)d_row, n_nodes, n_bins, (uint32_t *)d_histogram,
                       (unsigned long long *)d_count_sum);
    HIP_TRY(hipGetLastError());
    return ev.stop(0, kernel_ms);
}

}  // extern "C"
