// Node counts of a sample haplotype by its difference from the all-ref path, and the count model over many samples.  The
// rules are those of include/gki.h ("haplotype segments", "node count model") and DESIGN.md 4.20.
//
// A window of a slot's sequence that touches no alt allele the slot takes occurs in the all-ref path too, so only the
// windows around the taken lines are probed: those of the all-ref path are taken away, those of the slot's sequence added
// (k_probe_segments, gki_probe.hip).  This file lists them.  With the kept lines j = 0 .. K - 1 and a spell count call of the
// slot behind us (the plan's slot_path is its path; ref_path, the all-ref path, is built once per plan by the same builder):
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

__global__ __launch_bounds__(SEG_BLOCK) void k_seg_taken_flags(int64_t K, const int64_t *__restrict__ kline,
                                                               const uint64_t *__restrict__ slot_bits,
                                                               uint32_t *__restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < K; j += stride)
        flag[j] = hap_alt_bit(slot_bits, kline[j]);
}

__global__ __launch_bounds__(SEG_BLOCK) void k_seg_taken_emit(int64_t K, const uint32_t *__restrict__ flag,
                                                              const int64_t *__restrict__ rank, int64_t *__restrict__ taken) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < K; j += stride)
        if (flag[j]) taken[rank[j]] = j;
}

// A path as k_seg_runs sees it at a taken line j: `size` is that of the allele the path keeps there.  It begins at cut[j],
// or, with in_front, ends there.  The slot's path drops the ref allele of a taken line and its alt allele stands at the
// cut.  The all-ref path drops the alt allele, cut[j] = alt_start[j] - before[j], and create holds alt_start[j] ==
// ref_start[j] + ref_size[j]: its ref allele lies in front of the cut, at ref_start[j] - before[j].
struct SegView {
    const int64_t *cut, *bounds;
    const int32_t *size;
    bool in_front;
};

struct SegPlan {
    SegView ref, slot;                                     // the all-ref path, the slot's path
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

// where the allele that path v keeps at taken line j ends
__device__ __forceinline__ int64_t seg_allele_end(const SegView &v, int64_t j) {
    return v.in_front ? v.cut[j] : v.cut[j] + v.size[j];
}

// the run of taken line j in path v, jp the taken line before it (-1: none), c its chromosome
__device__ __forceinline__ void seg_line_run(const SegView &v, int64_t j, int64_t jp, int64_t c, int k, int64_t *lo,
                                             int64_t *n) {
    const int64_t b = seg_allele_end(v, j);
    seg_run(b - v.size[j], b, jp < 0 ? 0 : seg_allele_end(v, jp), v.bounds[c], v.bounds[c + 1], k, lo, n);
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
        seg_line_run(p.ref, j, jp, c, p.k, &lo, &n);       // the all-ref path: the line's ref allele
        if (EMIT) {
            if (n > 0) { const int64_t o = ref_at[r]; ref_seg_start[o] = lo; ref_seg_windows[o] = n; }
        } else {
            has_ref[r] = n > 0;
            w_ref += (uint64_t)n;
        }
        seg_line_run(p.slot, j, jp, c, p.k, &lo, &n);      // the slot's sequence: the line's alt allele
        if (EMIT) {
            if (n > 0) { const int64_t o = slot_at[r]; slot_seg_start[o] = lo; slot_seg_windows[o] = n; }
        } else {
            has_slot[r] = n > 0;
            w_slot += (uint64_t)n;
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
        for (int i = 0; i < ploidy; i++) c_alt += (int)hap_alt_bit(alt_bits + (first_slot + i) * W, line);
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

SegView seg_view_of(const HapPath &path, const DevBuf &size, bool in_front) {
    return {path.cut.get<const int64_t>(), path.bounds.get<const int64_t>(), size.get<const int32_t>(), in_front};
}

SegPlan seg_plan_of(const gki_haplotype_paths &g, int k) {
    return {seg_view_of(g.ref_path, g.ref_size, true), seg_view_of(g.slot_path, g.alt_size, false),
            g.chrom_first_kept.get<const int64_t>(), g.n_chrom, k};
}

// what a segments count call leaves in the plan goes back unless the call succeeds
void drop_segments(gki_haplotype_paths &g) {
    g.seg.taken.reset();
    g.seg.ref_at.reset();
    g.seg.slot_at.reset();
    g.seg.of = HapKey();
}

int segments_count(gki_haplotype_paths &g, const void *d_alt_bits, int64_t slot, int k, int64_t *totals, float *kernel_ms) {
    const int64_t K = g.K;
    if (g.ref_path.of != HapKey::all_ref()) {              // once per plan; the null stream puts it in front of k_seg_runs
        HIP_TRY(g.ref_path.alloc(K, g.n_chrom));
        GKI_TRY(gki_haplotype_build_path(g, nullptr, g.ref_path));
        g.ref_path.of = HapKey::all_ref();
    }
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
            HIP_TRY(g.seg.taken.alloc((size_t)n_taken * 8));
            GKI_TRY(ev.start(0));
            hipLaunchKernelGGL(k_seg_taken_emit, dim3(stream_grid(K, SEG_BLOCK)), dim3(SEG_BLOCK), 0, 0, K,
                               flag.get<const uint32_t>(), rank.get<const int64_t>(), g.seg.taken.get<int64_t>());
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
        HIP_TRY(g.seg.ref_at.alloc((size_t)(n_taken + 1) * 8));
        HIP_TRY(g.seg.slot_at.alloc((size_t)(n_taken + 1) * 8));
        HIP_TRY(hipMemsetAsync(windows.get(), 0, 16, 0));
        GKI_TRY(ev.start(0));
        hipLaunchKernelGGL(k_seg_runs<false>, dim3(stream_grid(n_taken, SEG_BLOCK)), dim3(SEG_BLOCK), 0, 0, seg_plan_of(g, k),
                           n_taken, g.seg.taken.get<const int64_t>(), has_ref.get<uint32_t>(), has_slot.get<uint32_t>(),
                           windows.get<unsigned long long>(), (const int64_t *)nullptr, (const int64_t *)nullptr,
                           (int64_t *)nullptr, (int64_t *)nullptr, (int64_t *)nullptr, (int64_t *)nullptr);
        HIP_TRY(hipGetLastError());
        GKI_TRY(gki_scan_u32_to_i64(has_ref.get<const uint32_t>(), n_taken, g.seg.ref_at.get<int64_t>(), tmp.get(), tmp_bytes, 0));
        GKI_TRY(gki_scan_u32_to_i64(has_slot.get<const uint32_t>(), n_taken, g.seg.slot_at.get<int64_t>(), tmp.get(), tmp_bytes, 0));
        GKI_TRY(ev.stop(0, &ms));
        if (kernel_ms) *kernel_ms += ms;
        unsigned long long w[2] = {0, 0};
        HIP_TRY(hipMemcpy(&totals[1], g.seg.ref_at.get<const int64_t>() + n_taken, 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&totals[3], g.seg.slot_at.get<const int64_t>() + n_taken, 8, hipMemcpyDeviceToHost));
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
    if (g.slot_path.of != HapKey{slot, d_alt_bits})
        return gki_set_error(GKI_ERR_STATE, "haplotype_segments_count: the last spell count call was not of slot %lld of this plane",
                             (long long)slot);
    int64_t totals[5] = {0, 0, 0, 0, 0};
    const int rc = segments_count(g, d_alt_bits, slot, k, totals, kernel_ms);
    if (rc != GKI_OK) { drop_segments(g); return rc; }
    g.seg.n_taken = totals[0]; g.seg.n_ref = totals[1]; g.seg.n_slot = totals[3]; g.seg.k = k;
    g.seg.of = g.slot_path.of;
    for (int i = 0; i < 5; i++) *outs[i] = totals[i];
    return GKI_OK;
}

int gki_haplotype_segments_emit(gki_haplotype_paths *plan, void *d_ref_seg_start, void *d_ref_seg_windows,
                                void *d_slot_seg_start, void *d_slot_seg_windows, float *kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    GKI_TRY(gki_check_haplotype_plan(plan, "haplotype_segments_emit"));
    gki_haplotype_paths &g = *plan;
    if (g.seg.of == HapKey()) return gki_set_error(GKI_ERR_STATE, "haplotype_segments_emit: no segments count call came before");
    DevBuf taken, ref_at, slot_at;                         // the plan's go back to the pool when the call returns
    taken.swap(g.seg.taken);
    ref_at.swap(g.seg.ref_at);
    slot_at.swap(g.seg.slot_at);
    const int64_t n_taken = g.seg.n_taken;
    const HapKey of = g.seg.of;
    g.seg.of = HapKey();
    if (g.slot_path.of != of)
        return gki_set_error(GKI_ERR_STATE, "haplotype_segments_emit: another slot or plane was spelled since the count call");
    if (n_taken == 0 || (g.seg.n_ref == 0 && g.seg.n_slot == 0)) return GKI_OK;
    if ((g.seg.n_ref > 0 && (d_ref_seg_start == nullptr || d_ref_seg_windows == nullptr)) ||
        (g.seg.n_slot > 0 && (d_slot_seg_start == nullptr || d_slot_seg_windows == nullptr)))
        return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_segments_emit: an output is NULL");
    TimerEvents ev;
    GKI_TRY(ev.start(0));
    hipLaunchKernelGGL(k_seg_runs<true>, dim3(stream_grid(n_taken, SEG_BLOCK)), dim3(SEG_BLOCK), 0, 0, seg_plan_of(g, g.seg.k),
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
