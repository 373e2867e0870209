// UniqueVariantKmersFinder on the device (unique_variant_kmers.py:114-270 of the reference, dense path): for every variant
// the k-mers that stand for its ref and alt allele, chosen among its P = len(range(2, k-2)[::4]) start positions.
//
//   gki_uvk_starts     one lane per (variant, start): linear-ref offset -> (node, offset) by binary search
//   (gki_forward_count / gki_forward_emit over all starts at once, no store filter)
//   gki_uvk_summarize  one lane per start: its records of the variant's ref and alt node, their maximum frequency in the
//                      index (first hit of h plus first hit of its 31-mer reverse complement, get_frequency's defaults),
//                      and whether a hash is shared by a ref window and an alt window among the first 500 windows
//   gki_uvk_select     one lane per variant: rules 5-6 over its summaries for a given store set, record counts, scan
//   gki_uvk_emit       one lane per variant: the chosen start's records of the stored nodes, in emission order
//
// Simple selection (find_kmers_over_variant, :66-111): gki_uvk_simple_starts, one lane per (variant, allele), then the
// per-node search gki_forward_node_count / gki_forward_node_emit (csrc/gki_forward.hip), which writes the output itself.
//
// Every per-lane quantity is a scalar in registers: no arrays, no scratch.
#include "gki_frequency.h"

namespace {

// (node, offset) at graph ref offset x: the last linear-ref node of nonzero size whose first base is at or before x.
// false: x lies before the first node, or past the end of the node found (past the linear path, or in a gap of it).
__device__ __forceinline__ bool lin_locate(const int64_t *__restrict__ lin_start, const int32_t *__restrict__ lin_node,
                                           const int32_t *__restrict__ node_size, int64_t n_lin, int64_t x, int32_t *node, int32_t *off) {
    int64_t lo = 0, hi = n_lin;                      // answer in [lo, hi): lin_start[lo] <= x < lin_start[hi]
    *node = 0; *off = 0;
    if (!(n_lin > 0 && x >= lin_start[0])) return false;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (lin_start[mid] <= x) lo = mid; else hi = mid;
    }
    *node = lin_node[lo];
    const int64_t d = x - lin_start[lo];
    *off = (int32_t)d;
    return d < (int64_t)node_size[*node];
}

__global__ __launch_bounds__(256) void k_uvk_starts(const int64_t *__restrict__ lin_start, const int32_t *__restrict__ lin_node,
                                                    const int32_t *__restrict__ node_size, int64_t n_lin,
                                                    const int64_t *__restrict__ var_ref_offset, int64_t n_var, int P,
                                                    int32_t *__restrict__ out_nodes, int32_t *__restrict__ out_offsets,
                                                    int32_t *__restrict__ out_variant, unsigned long long *__restrict__ first_bad) {
    const int64_t n = n_var * P;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t v = i / P;
        const int j = (int)(i - v * P);
        const int64_t x = var_ref_offset[v] - (2 + 4 * (P - 1 - j));     // [POS - i for i in range(2, k-2)][::4][::-1]
        int32_t node, off;
        if (!lin_locate(lin_start, lin_node, node_size, n_lin, x, &node, &off)) { atomicMin(first_bad, (unsigned long long)v); node = 0; off = 0; }
        out_nodes[i] = node;
        out_offsets[i] = off;
        out_variant[i] = (int32_t)v;
    }
}

// Simple selection, unique_variant_kmers.py:72-89: search 2 v + a of variant v is for its ref (a = 0) or alt (a = 1) node.
// A SNP starts at (node, 0) of a node with bases; an indel, and a SNP's empty node, at the linear-ref position 8 bases before
// P, with P = POS for an indel and POS - 1 for a SNP as 0-based chromosome offsets (var_ref_offset holds the chromosome's
// graph ref offset + the 1-based VCF POS, as for k_uvk_starts).
__global__ __launch_bounds__(256) void k_uvk_simple_starts(const int64_t *__restrict__ lin_start, const int32_t *__restrict__ lin_node,
                                                           const int32_t *__restrict__ node_size, int64_t n_nodes, int64_t n_lin,
                                                           const int64_t *__restrict__ var_ref_offset, const uint8_t *__restrict__ is_snp,
                                                           const int32_t *__restrict__ ref_nodes, const int32_t *__restrict__ alt_nodes, int64_t n_var,
                                                           int32_t *__restrict__ out_nodes, int32_t *__restrict__ out_offsets,
                                                           int32_t *__restrict__ out_targets, unsigned long long *__restrict__ first_bad) {
    const int64_t n = n_var * 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t v = i >> 1;
        const int32_t target = (i & 1) ? alt_nodes[v] : ref_nodes[v];
        const bool snp = is_snp[v] != 0;
        int32_t node = 0, off = 0;
        bool ok = target >= 0 && (int64_t)target < n_nodes;
        if (ok && snp && node_size[target] > 0) node = target;
        else if (ok) ok = lin_locate(lin_start, lin_node, node_size, n_lin, var_ref_offset[v] - (snp ? 9 : 8), &node, &off);
        if (!ok) { atomicMin(first_bad, (unsigned long long)v); node = 0; off = 0; }
        out_nodes[i] = node;
        out_offsets[i] = off;
        out_targets[i] = target;
    }
}

__global__ __launch_bounds__(256) void k_uvk_summarize(
    const int64_t *__restrict__ rec_start, int64_t n_pos, int P, const int64_t *__restrict__ hashes,
    const int32_t *__restrict__ start_nodes, const int16_t *__restrict__ start_offsets, const int32_t *__restrict__ nodes,
    const int32_t *__restrict__ ref_nodes, const int32_t *__restrict__ alt_nodes, GkiIndexSource ix,
    gki_uvk_summary *__restrict__ out) {
    uvk_summarize_body(rec_start, n_pos, P, hashes, start_nodes, start_offsets, nodes, ref_nodes, alt_nodes, ix, out);
}

__global__ __launch_bounds__(256) void k_uvk_select(const gki_uvk_summary *__restrict__ summ, int64_t n_var, int P, int lowest,
                                                    const uint8_t *__restrict__ store_mask, int32_t *__restrict__ choice,
                                                    uint32_t *__restrict__ count) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_var; v += stride) {
        const uint32_t m = store_mask ? store_mask[v] : 3u;
        int best = P - 1, first = -1;
        uint32_t best_score = 0xFFFFFFFFu;
        for (int j = 0; j < P; ++j) {
            const gki_uvk_summary s = summ[v * P + j];
            const bool shared = (s.flags & 1u) && (m & 1u) && ((m & 2u) || (s.flags & 2u));
            if (shared && j != P - 1) continue;                       // rule 5; the last position is always valid
            uint32_t score = 0;
            if (m & 1u) score = s.f_ref;
            if ((m & 2u) && s.f_alt > score) score = s.f_alt;
            if (first < 0) first = j;
            if (score < best_score) { best_score = score; best = j; }  // stable sort: the first of the lowest
            if (score <= 1) break;                                    // rule 6: no later position is looked at
        }
        const int c = lowest ? best : first;
        const gki_uvk_summary s = summ[v * P + c];
        choice[v] = c;
        count[v] = ((m & 1u) ? s.n_ref : 0u) + ((m & 2u) ? s.n_alt : 0u);
    }
}

__global__ __launch_bounds__(256) void k_uvk_emit(
    const int64_t *__restrict__ rec_start, int64_t n_var, int P, const int32_t *__restrict__ choice,
    const uint8_t *__restrict__ store_mask, const int32_t *__restrict__ ref_nodes, const int32_t *__restrict__ alt_nodes,
    const int64_t *__restrict__ out_start, const int64_t *__restrict__ hashes, const int32_t *__restrict__ start_nodes,
    const int16_t *__restrict__ start_offsets, const int32_t *__restrict__ nodes, const double *__restrict__ af64,
    const int64_t *__restrict__ pos_base, uint64_t *__restrict__ o_hashes, uint32_t *__restrict__ o_nodes,
    uint64_t *__restrict__ o_ref_offsets, float *__restrict__ o_af) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_var; v += stride) {
        const uint32_t m = store_mask ? store_mask[v] : 3u;
        const int32_t ref = ref_nodes[v], alt = alt_nodes[v];
        const int64_t i = v * P + choice[v];
        const int64_t re = rec_start[i + 1];
        int64_t o = out_start[v];
        const int64_t o_end = out_start[v + 1];
        for (int64_t r = rec_start[i]; r < re && o < o_end; ++r) {
            const int32_t nd = nodes[r];
            if (!(((m & 1u) && nd == ref) || ((m & 2u) && nd == alt && alt != ref))) continue;
            o_hashes[o] = (uint64_t)hashes[r];
            o_nodes[o] = (uint32_t)nd;
            o_ref_offsets[o] = (uint64_t)(pos_base[start_nodes[r]] + (int64_t)start_offsets[r]);   // PositionId.get
            o_af[o] = (float)af64[r];
            ++o;
        }
    }
}

}  // namespace

extern "C" {

int gki_uvk_starts(gki_graph *g, const void *d_lin_start, const void *d_lin_node, int64_t n_lin,
                   const void *d_var_ref_offset, int64_t n_var, int n_starts_per_variant, void *d_nodes, void *d_offsets,
                   void *d_variant, int64_t *first_bad_variant) {
    *first_bad_variant = -1;
    if (n_starts_per_variant < 1) return gki_set_error(GKI_ERR_BAD_ARG, "gki_uvk_starts: no start position per variant");
    GKI_TRY(gki_check_graph_device(g, "gki_uvk_starts"));
    if (n_var <= 0) return GKI_OK;
    DevBuf bad;
    HIP_TRY(bad.alloc(8));
    HIP_TRY(hipMemset(bad.get(), 0xFF, 8));
    const int64_t n = n_var * n_starts_per_variant;
    hipLaunchKernelGGL(k_uvk_starts, dim3(stream_grid(n, 256)), dim3(256), 0, 0, (const int64_t *)d_lin_start,
                       (const int32_t *)d_lin_node, g->d.node_size, n_lin, (const int64_t *)d_var_ref_offset, n_var,
                       n_starts_per_variant, (int32_t *)d_nodes, (int32_t *)d_offsets, (int32_t *)d_variant, bad.get<unsigned long long>());
    HIP_TRY(hipGetLastError());
    unsigned long long h = ~0ull;
    HIP_TRY(hipMemcpy(&h, bad.get(), 8, hipMemcpyDeviceToHost));
    if (h != ~0ull) *first_bad_variant = (int64_t)h;
    return GKI_OK;
}

int gki_uvk_simple_starts(gki_graph *g, const void *d_lin_start, const void *d_lin_node, int64_t n_lin, const void *d_var_ref_offset,
                          const void *d_is_snp, const void *d_ref_nodes, const void *d_alt_nodes, int64_t n_var, void *d_nodes,
                          void *d_offsets, void *d_targets, int64_t *first_bad_variant) {
    *first_bad_variant = -1;
    GKI_TRY(gki_check_graph_device(g, "gki_uvk_simple_starts"));
    if (n_var <= 0) return GKI_OK;
    DevBuf bad;
    HIP_TRY(bad.alloc(8));
    HIP_TRY(hipMemset(bad.get(), 0xFF, 8));
    hipLaunchKernelGGL(k_uvk_simple_starts, dim3(stream_grid(n_var * 2, 256)), dim3(256), 0, 0, (const int64_t *)d_lin_start,
                       (const int32_t *)d_lin_node, g->d.node_size, g->d.n_nodes, n_lin, (const int64_t *)d_var_ref_offset,
                       (const uint8_t *)d_is_snp, (const int32_t *)d_ref_nodes, (const int32_t *)d_alt_nodes, n_var, (int32_t *)d_nodes,
                       (int32_t *)d_offsets, (int32_t *)d_targets, bad.get<unsigned long long>());
    HIP_TRY(hipGetLastError());
    unsigned long long h = ~0ull;
    HIP_TRY(hipMemcpy(&h, bad.get(), 8, hipMemcpyDeviceToHost));
    if (h != ~0ull) *first_bad_variant = (int64_t)h;
    return GKI_OK;
}

int gki_uvk_summarize(gki_graph *g, const gki_index_view *ix, const void *d_rec_start, int64_t n_var,
                      int n_starts_per_variant, const void *d_hashes, const void *d_start_nodes, const void *d_start_offsets,
                      const void *d_nodes, const void *d_ref_nodes, const void *d_alt_nodes, void *d_summary) {
    if (n_starts_per_variant < 1) return gki_set_error(GKI_ERR_BAD_ARG, "gki_uvk_summarize: no start position per variant");
    if (ix == nullptr || ix->modulo == 0) return gki_set_error(GKI_ERR_BAD_ARG, "gki_uvk_summarize: no frequency index");
    GKI_TRY(gki_check_graph_device(g, "gki_uvk_summarize"));
    const int64_t n_pos = n_var * n_starts_per_variant;
    if (n_pos <= 0) return GKI_OK;
    hipLaunchKernelGGL(k_uvk_summarize, dim3(stream_grid(n_pos, 256)), dim3(256), 0, 0, (const int64_t *)d_rec_start, n_pos,
                       n_starts_per_variant, (const int64_t *)d_hashes, (const int32_t *)d_start_nodes,
                       (const int16_t *)d_start_offsets, (const int32_t *)d_nodes, (const int32_t *)d_ref_nodes,
                       (const int32_t *)d_alt_nodes, gki_index_source(ix), (gki_uvk_summary *)d_summary);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

int gki_uvk_summarize_counter(gki_graph *g, const gki_counter *counter, const void *d_rec_start, int64_t n_var,
                              int n_starts_per_variant, const void *d_hashes, const void *d_start_nodes,
                              const void *d_start_offsets, const void *d_nodes, const void *d_ref_nodes,
                              const void *d_alt_nodes, void *d_summary) {
    if (n_starts_per_variant < 1) return gki_set_error(GKI_ERR_BAD_ARG, "gki_uvk_summarize_counter: no start position per variant");
    if (counter == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "gki_uvk_summarize_counter: no counter");
    GKI_TRY(gki_check_graph_device(g, "gki_uvk_summarize_counter"));
    const int64_t n_pos = n_var * n_starts_per_variant;
    if (n_pos <= 0) return GKI_OK;
    GKI_TRY(gki_launch_uvk_summarize_counter(counter, (const int64_t *)d_rec_start, n_pos, n_starts_per_variant,
                                             (const int64_t *)d_hashes, (const int32_t *)d_start_nodes,
                                             (const int16_t *)d_start_offsets, (const int32_t *)d_nodes,
                                             (const int32_t *)d_ref_nodes, (const int32_t *)d_alt_nodes,
                                             (gki_uvk_summary *)d_summary));
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

int gki_uvk_select(const void *d_summary, int64_t n_var, int n_starts_per_variant, int choose_lowest,
                   const void *d_store_mask, void *d_choice, void *d_out_start, int64_t *n_records) {
    *n_records = 0;
    if (n_starts_per_variant < 1) return gki_set_error(GKI_ERR_BAD_ARG, "gki_uvk_select: no start position per variant");
    if (n_var <= 0) { HIP_TRY(hipMemset(d_out_start, 0, 8)); return GKI_OK; }
    const int64_t tmp_bytes = gki_scan_tmp_bytes(n_var);
    DevBuf cnt, tmp;
    HIP_TRY(cnt.alloc((size_t)n_var * 4));
    HIP_TRY(tmp.alloc((size_t)tmp_bytes));
    hipLaunchKernelGGL(k_uvk_select, dim3(stream_grid(n_var, 256)), dim3(256), 0, 0, (const gki_uvk_summary *)d_summary,
                       n_var, n_starts_per_variant, choose_lowest, (const uint8_t *)d_store_mask, (int32_t *)d_choice, cnt.get<uint32_t>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(gki_scan_u32_to_i64(cnt.get<const uint32_t>(), n_var, (int64_t *)d_out_start, tmp.get(), tmp_bytes, 0));
    int64_t total = 0;
    HIP_TRY(hipMemcpy(&total, (const int64_t *)d_out_start + n_var, 8, hipMemcpyDeviceToHost));
    *n_records = total;
    return GKI_OK;
}

int gki_uvk_emit(gki_graph *g, const void *d_rec_start, int64_t n_var, int n_starts_per_variant, const void *d_choice,
                 const void *d_store_mask, const void *d_ref_nodes, const void *d_alt_nodes, const void *d_out_start,
                 const void *d_hashes, const void *d_start_nodes, const void *d_start_offsets, const void *d_nodes,
                 const void *d_af64, void *d_out_hashes, void *d_out_nodes, void *d_out_ref_offsets, void *d_out_af32) {
    if (n_starts_per_variant < 1) return gki_set_error(GKI_ERR_BAD_ARG, "gki_uvk_emit: no start position per variant");
    GKI_TRY(gki_check_graph_device(g, "gki_uvk_emit"));
    if (n_var <= 0) return GKI_OK;
    hipLaunchKernelGGL(k_uvk_emit, dim3(stream_grid(n_var, 256)), dim3(256), 0, 0, (const int64_t *)d_rec_start, n_var,
                       n_starts_per_variant, (const int32_t *)d_choice, (const uint8_t *)d_store_mask,
                       (const int32_t *)d_ref_nodes, (const int32_t *)d_alt_nodes, (const int64_t *)d_out_start,
                       (const int64_t *)d_hashes, (const int32_t *)d_start_nodes, (const int16_t *)d_start_offsets,
                       (const int32_t *)d_nodes, (const double *)d_af64, g->d.pos_base, (uint64_t *)d_out_hashes,
                       (uint32_t *)d_out_nodes, (uint64_t *)d_out_ref_offsets, (float *)d_out_af32);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

}  // extern "C"
