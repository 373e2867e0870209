// Genotyping a sample from its node counts with the count model: the fit of the model, the sample's coverage and the calls.
// The rules are those of include/gki.h ("genotyping") and DESIGN.md 4.21.
//
//   k_genotype_fit     once per model, one lane per data line: n = the bins' sum and s = count_sum of the line's
//                      2 (P + 1) entries -> the fitted means (s / n, or the nearest populated copy number's mean moved by the
//                      difference in copies) and n_alt; the kept lines' s go to the model total, one integer atomic per wave
//   k_genotype_scale   per row of a batch: S = the counts of the kept lines' two nodes summed, one integer atomic per wave
//   k_genotype_call    per row and data line: the P + 1 log likelihoods, the best and the second best of them in registers;
//                      no atomics
// The fitted table lies entry-major on the device: mean double[2 (P + 1)][V], n_alt uint32[P + 1][V], so that the wave's 64
// lanes read 64 consecutive values of one entry (a record per line would put a lane's reads 16 (P + 1) bytes apart).  The
// line's two node counts are a gather.  An entry's place is a function of a loop counter and no per-lane array is indexed
// by a run-time value: no scratch.
//
// Every floating-point operation here is rounded on its own: the fit is bit-equal to its NumPy statement, and the two
// passes of k_genotype_call over a line's genotypes give the same values.
#pragma clang fp contract(off)
#include "gki_text_lines.h"

namespace {

constexpr int GT_BLOCK = 256;
constexpr int GT_MAX_PLOIDY = 8;

// the fit's totals: the lowest line at fault (LineFault's word) and the model total T
struct FitTotals {
    unsigned long long first_bad = ~0ull, total = 0;
};

__device__ __forceinline__ uint64_t bins_sum(const uint32_t *__restrict__ bins, int n_bins) {
    uint64_t n = 0;
    for (int b = 0; b < n_bins; b++) n += bins[b];
    return n;
}

// histogram uint32[V][2][P + 1][n_bins], count_sum uint64[V][2][P + 1] -> mean, n_alt (entry-major).  A line that is not
// kept gets zeros.  Fault kinds: 1 = an allele of a kept line with no populated entry, 2 = an allele whose entries do not
// hold N individuals.  The trip count is the same for every lane of a wave, for wave_add64.
__global__ __launch_bounds__(GT_BLOCK) void k_genotype_fit(int64_t V, const uint32_t *__restrict__ histogram,
                                                           const unsigned long long *__restrict__ count_sum,
                                                           const uint32_t *__restrict__ var_nodes, int P, int n_bins,
                                                           int64_t N, double *__restrict__ mean, uint32_t *__restrict__ n_alt,
                                                           unsigned long long *__restrict__ totals) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int E = P + 1;
    uint64_t t = 0;
    for (int64_t v0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); v0 < V; v0 += stride) {
        const int64_t v = v0 + (threadIdx.x & 63);
        if (v >= V) continue;
        const bool kept = var_nodes[v] != 0u;
#pragma unroll
        for (int a = 0; a < 2; a++) {
            const int64_t e0 = (v * 2 + a) * E;            // the allele's first entry
            uint32_t populated = 0;                        // bit c: n[v][a][c] > 0
            uint64_t held = 0;
            for (int c = 0; c < E; c++) {
                const uint64_t n = kept ? bins_sum(histogram + (e0 + c) * n_bins, n_bins) : 0ull;
                populated |= (n > 0 ? 1u : 0u) << c;
                held += n;
                if (a == 1) n_alt[(int64_t)c * V + v] = (uint32_t)n;
                if (kept) t += count_sum[e0 + c];
            }
            if (kept && populated == 0u) line_fault(&totals[0], v, 1);
            else if (kept && held != (uint64_t)N) line_fault(&totals[0], v, 2);
            for (int c = 0; c < E; c++) {
                double mu = 0.0;
                if (populated) {
                    int from = c;                          // the populated copy number nearest to c, the lower at a tie
                    for (int d = 1; !((populated >> from) & 1u); d++) {
                        if (c - d >= 0 && ((populated >> (c - d)) & 1u)) from = c - d;
                        else if (c + d <= P && ((populated >> (c + d)) & 1u)) from = c + d;
                    }
                    const uint64_t n = bins_sum(histogram + (e0 + from) * n_bins, n_bins);
                    mu = (double)count_sum[e0 + from] / (double)n;
                    if (from != c) {
                        mu = mu + (double)(c - from);
                        mu = mu > 0.0 ? mu : 0.0;
                    }
                }
                mean[((int64_t)a * E + c) * V + v] = mu;
            }
        }
    }
    wave_add64(&totals[1], t);
}

// sums[row] += the row's counts of the kept lines' ref and var nodes; a node at or beyond n_nodes counts 0.  blockIdx.y is
// the row.  The trip count is the same for every lane of a wave, for wave_add64.
__global__ __launch_bounds__(GT_BLOCK) void k_genotype_scale(int64_t V, const uint32_t *__restrict__ ref_nodes,
                                                             const uint32_t *__restrict__ var_nodes,
                                                             const uint32_t *__restrict__ counts, int64_t n_nodes,
                                                             unsigned long long *__restrict__ sums) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const uint32_t *__restrict__ x = counts + (int64_t)blockIdx.y * n_nodes;
    uint64_t s = 0;
    for (int64_t v0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); v0 < V; v0 += stride) {
        const int64_t v = v0 + (threadIdx.x & 63);
        if (v >= V) continue;
        const int64_t var = var_nodes[v], ref = ref_nodes[v];
        if (var == 0) continue;
        s += (uint64_t)(ref < n_nodes ? x[ref] : 0u) + (uint64_t)(var < n_nodes ? x[var] : 0u);
    }
    wave_add64(&sums[blockIdx.y], s);
}

struct CallRule {
    double error, pseudo_count, prior_total;               // prior_total = N + (P + 1) pseudo_count
    int P;
};

// L[g] of line v, left to right as the rule writes it
__device__ __forceinline__ double genotype_loglik(const double *__restrict__ mean, const uint32_t *__restrict__ n_alt,
                                                  int64_t V, int64_t v, const CallRule &r, double lambda, double x0, double x1,
                                                  int g) {
    const double m0 = lambda * (mean[(int64_t)(r.P - g) * V + v] + r.error);
    const double m1 = lambda * (mean[(int64_t)(r.P + 1 + g) * V + v] + r.error);
    const double prior = ((double)n_alt[(int64_t)g * V + v] + r.pseudo_count) / r.prior_total;
    return x0 * log(m0) - m0 + x1 * log(m1) - m1 + log(prior);
}

// counts uint32[n_samples][n_nodes], coverage double[n_samples] -> call int8[n_samples][V], gq uint8[n_samples][V] and,
// unless it is NULL, loglik double[n_samples][V][P + 1].  blockIdx.y is the row; one lane per line.
__global__ __launch_bounds__(GT_BLOCK) void k_genotype_call(int64_t V, const double *__restrict__ mean,
                                                            const uint32_t *__restrict__ n_alt,
                                                            const uint32_t *__restrict__ ref_nodes,
                                                            const uint32_t *__restrict__ var_nodes,
                                                            const uint32_t *__restrict__ counts, int64_t n_nodes,
                                                            const double *__restrict__ coverage, CallRule r,
                                                            int8_t *__restrict__ call, uint8_t *__restrict__ gq,
                                                            double *__restrict__ loglik) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, row = blockIdx.y;
    const uint32_t *__restrict__ x = counts + row * n_nodes;
    const double lambda = coverage[row];
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += stride) {
        const int64_t var = var_nodes[v], ref = ref_nodes[v];
        double *__restrict__ out = loglik ? loglik + (row * V + v) * (r.P + 1) : nullptr;
        if (var == 0) {
            call[row * V + v] = (int8_t)-1;
            gq[row * V + v] = 0;
            if (out) for (int g = 0; g <= r.P; g++) out[g] = 0.0;
            continue;
        }
        const double x0 = (double)(ref < n_nodes ? x[ref] : 0u), x1 = (double)(var < n_nodes ? x[var] : 0u);
        double best = -__builtin_huge_val(), second = -__builtin_huge_val();
        int best_g = 0;
        for (int g = 0; g <= r.P; g++) {
            const double L = genotype_loglik(mean, n_alt, V, v, r, lambda, x0, x1, g);
            if (L > best) { second = best; best = L; best_g = g; }
            else if (L > second) second = L;
        }
        const double q = 4.342944819032518 * (best - second);
        call[row * V + v] = (int8_t)best_g;
        gq[row * V + v] = q >= 99.0 ? (uint8_t)99 : (uint8_t)floor(q);
        if (out) for (int g = 0; g <= r.P; g++) out[g] = genotype_loglik(mean, n_alt, V, v, r, lambda, x0, x1, g) - best;
    }
}

bool positive_finite(double x) { return x > 0.0 && x <= 1.7976931348623157e308; }

}  // namespace

extern "C" {

int gki_genotype_fit(const void *d_histogram, const void *d_count_sum, const void *d_var_nodes, int64_t n_lines, int ploidy,
                     int n_bins, int64_t n_individuals, void *d_mean, void *d_n_alt, uint64_t *model_total,
                     int64_t *first_bad_line, int *first_bad_kind, float *kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    if (model_total) *model_total = 0;
    if (first_bad_line) *first_bad_line = -1;
    if (first_bad_kind) *first_bad_kind = 0;
    if (ploidy < 1 || ploidy > GT_MAX_PLOIDY) return gki_set_error(GKI_ERR_BAD_ARG, "genotype_fit: ploidy must be in 1..8");
    if (n_bins < 2 || n_bins > 65536) return gki_set_error(GKI_ERR_BAD_ARG, "genotype_fit: n_bins must be in 2..65536");
    if (n_lines < 0 || n_individuals < 0 || model_total == nullptr || first_bad_line == nullptr || first_bad_kind == nullptr)
        return gki_set_error(GKI_ERR_BAD_ARG, "genotype_fit: a negative size or a result's pointer is NULL");
    if (n_lines == 0) return GKI_OK;
    if (d_histogram == nullptr || d_count_sum == nullptr || d_var_nodes == nullptr || d_mean == nullptr || d_n_alt == nullptr)
        return gki_set_error(GKI_ERR_BAD_ARG, "genotype_fit: a buffer is NULL");
    DevBuf totals;
    GKI_TRY(line_fault_init<FitTotals>(totals));
    TimerEvents ev;
    GKI_TRY(ev.start(0));
    hipLaunchKernelGGL(k_genotype_fit, dim3(stream_grid(n_lines, GT_BLOCK)), dim3(GT_BLOCK), 0, 0, n_lines,
                       (const uint32_t *)d_histogram, (const unsigned long long *)d_count_sum, (const uint32_t *)d_var_nodes,
                       ploidy, n_bins, n_individuals, (double *)d_mean, (uint32_t *)d_n_alt,
                       totals.get<unsigned long long>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(ev.stop(0, kernel_ms));
    FitTotals got;
    GKI_TRY(line_fault_read(totals, &got));
    LineFault fault;
    fault.first_bad = got.first_bad;
    *first_bad_line = fault.line();
    *first_bad_kind = fault.kind();
    *model_total = got.total;
    return GKI_OK;
}

int gki_genotype_scale(const void *d_ref_nodes, const void *d_var_nodes, int64_t n_lines, const void *d_counts,
                       int64_t n_samples, int64_t n_nodes, uint64_t *h_sums, float *kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_lines < 0 || n_nodes < 0 || n_samples < 0 || n_samples > 65535 || (n_samples > 0 && h_sums == nullptr))
        return gki_set_error(GKI_ERR_BAD_ARG, "genotype_scale: a size is negative, more than 65535 rows, or the sums are NULL");
    for (int64_t i = 0; i < n_samples; i++) h_sums[i] = 0;
    if (n_samples == 0 || n_lines == 0) return GKI_OK;
    if (d_ref_nodes == nullptr || d_var_nodes == nullptr || (n_nodes > 0 && d_counts == nullptr))
        return gki_set_error(GKI_ERR_BAD_ARG, "genotype_scale: a buffer is NULL");
    DevBuf sums;
    HIP_TRY(sums.alloc((size_t)n_samples * 8));
    HIP_TRY(hipMemsetAsync(sums.get(), 0, (size_t)n_samples * 8, 0));
    TimerEvents ev;
    GKI_TRY(ev.start(0));
    hipLaunchKernelGGL(k_genotype_scale, dim3(stream_grid(n_lines, GT_BLOCK), (unsigned)n_samples), dim3(GT_BLOCK), 0, 0, n_lines,
                       (const uint32_t *)d_ref_nodes, (const uint32_t *)d_var_nodes, (const uint32_t *)d_counts, n_nodes,
                       sums.get<unsigned long long>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(ev.stop(0, kernel_ms));
    HIP_TRY(hipMemcpy(h_sums, sums.get(), (size_t)n_samples * 8, hipMemcpyDeviceToHost));
    return GKI_OK;
}

int gki_genotype_call(const void *d_mean, const void *d_n_alt, const void *d_ref_nodes, const void *d_var_nodes,
                      int64_t n_lines, int ploidy, int64_t n_individuals, const void *d_counts, int64_t n_samples,
                      int64_t n_nodes, const double *h_coverage, double error, double pseudo_count, void *d_call, void *d_gq,
                      void *d_loglik, float *kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    if (ploidy < 1 || ploidy > GT_MAX_PLOIDY) return gki_set_error(GKI_ERR_BAD_ARG, "genotype_call: ploidy must be in 1..8");
    if (n_lines < 0 || n_nodes < 0 || n_individuals < 0 || n_samples < 0 || n_samples > 65535 ||
        (n_samples > 0 && h_coverage == nullptr))
        return gki_set_error(GKI_ERR_BAD_ARG, "genotype_call: a size is negative, more than 65535 rows, or the coverage is NULL");
    if (!positive_finite(error) || !positive_finite(pseudo_count))
        return gki_set_error(GKI_ERR_BAD_ARG, "genotype_call: error and pseudo_count must be positive and finite");
    for (int64_t i = 0; i < n_samples; i++)
        if (!positive_finite(h_coverage[i]))
            return gki_set_error(GKI_ERR_BAD_ARG, "genotype_call: the coverage of row %lld is not positive and finite", (long long)i);
    if (n_samples == 0 || n_lines == 0) return GKI_OK;
    if (d_mean == nullptr || d_n_alt == nullptr || d_ref_nodes == nullptr || d_var_nodes == nullptr || d_call == nullptr ||
        d_gq == nullptr || (n_nodes > 0 && d_counts == nullptr))
        return gki_set_error(GKI_ERR_BAD_ARG, "genotype_call: a buffer is NULL");
    DevBuf coverage;
    HIP_TRY(coverage.alloc((size_t)n_samples * 8));
    HIP_TRY(hipMemcpy(coverage.get(), h_coverage, (size_t)n_samples * 8, hipMemcpyHostToDevice));
    const CallRule rule = {error, pseudo_count, (double)n_individuals + (double)(ploidy + 1) * pseudo_count, ploidy};
    TimerEvents ev;
    GKI_TRY(ev.start(0));
    hipLaunchKernelGGL(k_genotype_call, dim3(stream_grid(n_lines, GT_BLOCK), (unsigned)n_samples), dim3(GT_BLOCK), 0, 0, n_lines,
                       (const double *)d_mean, (const uint32_t *)d_n_alt, (const uint32_t *)d_ref_nodes,
                       (const uint32_t *)d_var_nodes, (const uint32_t *)d_counts, n_nodes, coverage.get<const double>(), rule,
                       (int8_t *)d_call, (uint8_t *)d_gq, (double *)d_loglik);
    HIP_TRY(hipGetLastError());
    return ev.stop(0, kernel_ms);
}

}  // extern "C"
