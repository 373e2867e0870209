// Allele frequencies of VCF text in HBM: per data line (ref_af, alt_af) from INFO's AF= entry or from the GT columns.
// The rules are those of include/gki.h ("VCF allele frequencies") and DESIGN.md 4.17.
//
// per piece of text (gki_vcf_allele_frequencies), beside the unchanged gki_vcf_parse_* and gki_graph_sites_*:
//   (data lines)     gki_vcf_data_lines (gki_text_lines.hip): line ends, header / blank / data, line -> data lines before
//                    it -- the front end of the site pass and the haplotype matrix, so the three number the data lines
//                    alike; the host checks the count
//   k_af_info        source info: one lane per data line walks to the seventh tab and through INFO, which lies before the
//                    sample columns, finds the AF= entry and turns its value text into a double by one exact operation
//   k_af_genotypes   source genotypes: one wave per data line, dense in the bytes, by gki_vcf_gt.h's gt_walk_line.  A
//                    lane whose bytes hold tab number 9 or higher parses the GT behind it straight from memory, eight bytes
//                    in one load (a GT is a few bytes; they may lie in the next lane's or the next step's bytes).  Tab
//                    number 8 opens FORMAT, which its lane checks.  One wave reduction per line gives the three counts;
//                    lane 0 divides and stores.  A wave owns its line: no atomics but that of the lowest line at fault.
// The walk and the GT grammar are gki_vcf_gt.h's, shared with the haplotype matrix (gki_vcf_gt.hip).
#include "gki_vcf_gt.h"

namespace {

constexpr int AF_MAX_MANTISSA_DIGITS = 15, AF_MAX_EXPONENT_DIGITS = 3, AF_MAX_POWER = 22;
constexpr uint8_t ROUTE_DEVICE = 0, ROUTE_ABSENT = 1, ROUTE_HOST = 2;

// the powers of ten a double holds exactly
__device__ const double AF_POW10[AF_MAX_POWER + 1] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                                      1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

// The value text bytes [b, e) under the device grammar  D* [ . D* ] [ (e|E) [+|-] D+ ]: true and *value when the mantissa
// has 1 to 15 digits, the exponent at most 3 and |q| <= 22, q = exponent - fraction digits.  m (below 10^15) and 10^|q| are
// exact doubles, so the one multiplication or division is the correctly rounded value of the text.
__device__ __forceinline__ bool af_value(const uint8_t *__restrict__ bytes, int64_t b, int64_t e, double *value) {
    uint64_t m = 0;
    int digits = 0, fraction = 0, exponent = 0, exponent_digits = 0;
    bool negative = false, ok = true;
    int64_t p = b;
    for (; p < e && is_digit(bytes[p]); p++, digits++)
        if (digits < AF_MAX_MANTISSA_DIGITS) m = m * 10 + (bytes[p] - (uint8_t)'0');
    if (p < e && bytes[p] == (uint8_t)'.') {
        for (p++; p < e && is_digit(bytes[p]); p++, digits++, fraction++)
            if (digits < AF_MAX_MANTISSA_DIGITS) m = m * 10 + (bytes[p] - (uint8_t)'0');
    }
    ok = digits >= 1 && digits <= AF_MAX_MANTISSA_DIGITS;
    if (ok && p < e && (bytes[p] | 0x20) == (uint8_t)'e') {
        p++;
        if (p < e && (bytes[p] == (uint8_t)'+' || bytes[p] == (uint8_t)'-')) { negative = bytes[p] == (uint8_t)'-'; p++; }
        for (; p < e && is_digit(bytes[p]) && exponent_digits <= AF_MAX_EXPONENT_DIGITS; p++, exponent_digits++)
            exponent = exponent * 10 + (bytes[p] - (uint8_t)'0');
        ok = exponent_digits >= 1 && exponent_digits <= AF_MAX_EXPONENT_DIGITS;
    }
    ok = ok && p == e;                                     // a stray byte, a sign, nan, inf: the host's
    const int q = (negative ? -exponent : exponent) - fraction;
    ok = ok && q >= -AF_MAX_POWER && q <= AF_MAX_POWER;
    const double power = AF_POW10[ok ? (q < 0 ? -q : q) : 0];
    *value = q < 0 ? (double)m / power : (double)m * power;
    return ok;
}

// Data line v: INFO is field 7.  route 0 with the value, 1 absent, 2 with the value text's place for the host.
__global__ __launch_bounds__(PARSE_BLOCK) void k_af_info(const uint8_t *__restrict__ bytes,
                                                         const int64_t *__restrict__ line_end, int64_t n_lines,
                                                         const uint32_t *__restrict__ is_data,
                                                         const int64_t *__restrict__ variant_index, int64_t n_variants,
                                                         double *__restrict__ ref_af, double *__restrict__ alt_af,
                                                         uint8_t *__restrict__ route, int64_t *__restrict__ span_begin,
                                                         int32_t *__restrict__ span_len,
                                                         unsigned long long *__restrict__ first_bad) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_lines; i += stride) {
        if (!is_data[i]) continue;
        const int64_t v = variant_index[i];
        if (v >= n_variants) continue;
        const VcfLine l = vcf_line(bytes, line_end, i);
        int64_t p = l.b;
        int tabs = 0;
        for (; p < l.e && tabs < 7; p++) tabs += bytes[p] == (uint8_t)'\t';
        int64_t value_b = -1, value_e = -1;
        if (tabs == 7) {                                   // p is INFO's first byte; its entries end at ';', the field at a tab
            bool entry_begins = true;
            for (; p < l.e && bytes[p] != (uint8_t)'\t'; p++) {
                const uint8_t c = bytes[p];
                if (entry_begins && c == (uint8_t)'A' && p + 2 < l.e && bytes[p + 1] == (uint8_t)'F' && bytes[p + 2] == (uint8_t)'=') {
                    value_b = value_e = p + 3;
                    while (value_e < l.e && bytes[value_e] != (uint8_t)';' && bytes[value_e] != (uint8_t)',' &&
                           bytes[value_e] != (uint8_t)'\t')
                        value_e++;
                    break;
                }
                entry_begins = c == (uint8_t)';';
            }
        }
        const int64_t len = value_e - value_b;
        double value = 0.0;
        uint8_t r = ROUTE_ABSENT;
        if (value_b >= 0 && len > 0 && !(len == 1 && bytes[value_b] == (uint8_t)'.'))
            r = af_value(bytes, value_b, value_e, &value) ? ROUTE_DEVICE : ROUTE_HOST;
        const bool at_fault = r == ROUTE_DEVICE && !(value <= 1.0);   // the grammar has no sign: never negative, never NaN
        if (at_fault) line_fault(first_bad, v, 1);
        const bool parsed = r == ROUTE_DEVICE && !at_fault;
        ref_af[v] = parsed ? 1.0 - value : 1.0;
        alt_af[v] = parsed ? value : 1.0;
        route[v] = r;
        span_begin[v] = r == ROUTE_HOST ? value_b : 0;
        span_len[v] = r == ROUTE_HOST ? (int32_t)(len < 0x7FFFFFFFll ? len : 0x7FFFFFFFll) : 0;
    }
}

// what k_af_genotypes takes from a GT: the numeric alleles, those equal to 0 and those equal to 1
struct GtCounts {
    int called = 0, n_ref = 0, n_alt = 0;
    __device__ __forceinline__ void number(int value) { called += 1; n_ref += value == 0; n_alt += value == 1; }
    __device__ __forceinline__ void missing() {}
    __device__ __forceinline__ void slash() {}
};

// what a lane of k_af_genotypes gathers over its line (gt_walk_line's visitor): the counts of its samples, and what it saw
struct AfLine {
    const uint8_t *__restrict__ bytes;
    int64_t n_bytes, e;
    int &called, &n_ref, &n_alt, &bad_format, &bad_gt;
    __device__ __forceinline__ void format(bool ok) { bad_format |= !ok; }
    __device__ __forceinline__ void sample(int64_t, int64_t p) {
        GtCounts c;
        bad_gt |= !gt_at(bytes, n_bytes, p, e, &c);
        called += c.called;
        n_ref += c.n_ref;
        n_alt += c.n_alt;
    }
};

// One wave per data line.
__global__ __launch_bounds__(PARSE_BLOCK) void k_af_genotypes(const uint8_t *__restrict__ bytes, int64_t n_bytes,
                                                              const int64_t *__restrict__ line_end, int64_t n_lines,
                                                              const uint32_t *__restrict__ is_data,
                                                              const int64_t *__restrict__ variant_index, int64_t n_variants,
                                                              double *__restrict__ ref_af, double *__restrict__ alt_af,
                                                              uint8_t *__restrict__ route,
                                                              unsigned long long *__restrict__ first_bad) {
    const int lane = threadIdx.x & 63;
    const int64_t first = wave_uniform((int64_t)blockIdx.x * (PARSE_BLOCK / 64) + (threadIdx.x >> 6));
    const int64_t stride = (int64_t)gridDim.x * (PARSE_BLOCK / 64);
    for (int64_t i = first; i < n_lines; i += stride) {
        if (!is_data[i]) continue;
        const int64_t v = variant_index[i];
        if (v >= n_variants) continue;
        const VcfLine l = vcf_line(bytes, line_end, i);
        const int64_t b = wave_uniform(l.b), e = wave_uniform(l.e);
        int called = 0, n_ref = 0, n_alt = 0, bad_format = 0, bad_gt = 0;
        const int tabs_before = gt_walk_line(bytes, n_bytes, b, e, lane,
                                             AfLine{bytes, n_bytes, e, called, n_ref, n_alt, bad_format, bad_gt});
        called = wave_sum(called);
        n_ref = wave_sum(n_ref);
        n_alt = wave_sum(n_alt);
        const int kind = tabs_before < 9 ? 0 : wave_sum(bad_format) ? 2 : wave_sum(bad_gt) ? 3 : 0;
        if (lane == 0) {
            const bool counted = tabs_before >= 9 && kind == 0 && called > 0;
            if (kind) line_fault(first_bad, v, kind);
            ref_af[v] = counted ? (double)n_ref / (double)called : 1.0;
            alt_af[v] = counted ? (double)n_alt / (double)called : 1.0;
            route[v] = counted ? ROUTE_DEVICE : ROUTE_ABSENT;
        }
    }
}

}  // namespace

extern "C" int gki_vcf_allele_frequencies(const void *d_text, int64_t n_bytes, int source, int64_t n_variants, void *d_ref_af,
                                          void *d_alt_af, void *d_route, void *d_span_begin, void *d_span_len,
                                          int64_t *n_data_lines, int64_t *first_bad_variant, int *first_bad_kind,
                                          float *kernel_ms) {
    if (n_data_lines) *n_data_lines = 0;
    if (first_bad_variant) *first_bad_variant = -1;
    if (first_bad_kind) *first_bad_kind = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_bytes < 0 || n_variants < 0) return gki_set_error(GKI_ERR_BAD_ARG, "vcf_allele_frequencies: a negative size");
    if (source != GKI_AF_SOURCE_INFO && source != GKI_AF_SOURCE_GENOTYPES)
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_allele_frequencies: source %d is neither INFO nor genotypes", source);
    if (n_bytes > 0 && d_text == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "vcf_allele_frequencies: the text is NULL");
    if (n_variants > 0 && (d_ref_af == nullptr || d_alt_af == nullptr || d_route == nullptr ||
                           (source == GKI_AF_SOURCE_INFO && (d_span_begin == nullptr || d_span_len == nullptr))))
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_allele_frequencies: an output buffer is NULL");
    const uint8_t *bytes = (const uint8_t *)d_text;
    TimerEvents ev;
    VcfDataLines d;
    DevBuf totals;
    if (n_bytes > 0) GKI_TRY(gki_vcf_data_lines(bytes, n_bytes, "vcf_allele_frequencies", d));
    if (n_data_lines) *n_data_lines = d.n_data;
    GKI_TRY(gki_vcf_expect_data_lines("vcf_allele_frequencies", d.n_data, n_variants));
    if (n_variants == 0) return GKI_OK;
    GKI_TRY(line_fault_init(totals));
    GKI_TRY(ev.start(0));
    if (source == GKI_AF_SOURCE_INFO)
        hipLaunchKernelGGL(k_af_info, dim3(stream_grid(d.n_lines, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0, bytes,
                           d.line_end.get<const int64_t>(), d.n_lines, d.is_data.get<const uint32_t>(),
                           d.variant_index.get<const int64_t>(), n_variants, (double *)d_ref_af, (double *)d_alt_af,
                           (uint8_t *)d_route, (int64_t *)d_span_begin, (int32_t *)d_span_len,
                           totals.get<unsigned long long>());
    else
        hipLaunchKernelGGL(k_af_genotypes, dim3(stream_grid(d.n_lines, PARSE_BLOCK / 64)), dim3(PARSE_BLOCK), 0, 0, bytes,
                           n_bytes, d.line_end.get<const int64_t>(), d.n_lines, d.is_data.get<const uint32_t>(),
                           d.variant_index.get<const int64_t>(), n_variants, (double *)d_ref_af, (double *)d_alt_af,
                           (uint8_t *)d_route, totals.get<unsigned long long>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(ev.stop(0, kernel_ms));
    LineFault fault;
    GKI_TRY(line_fault_read(totals, &fault));
    if (first_bad_variant) *first_bad_variant = fault.line();
    if (first_bad_kind) *first_bad_kind = fault.kind();
    return GKI_OK;
}
