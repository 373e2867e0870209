// A genotyped VCF's data lines from VCF text in HBM: per data line its first eight fields and a GT:GQ column for one sample.
// The rules are those of include/gki.h ("genotyped VCF text") and DESIGN.md 4.21.
//
// per piece of text (gki_vcf_genotypes_count and again in gki_vcf_genotypes_emit, which keeps no state):
//   (data lines)        gki_vcf_data_lines (gki_text_lines.hip): line ends, header / blank / data, line -> data lines before it
//   k_vcf_gt_lengths    one lane per data line: the walk to the eighth tab -> where the line begins, the bytes of its first
//                       eight fields and the length of its output line; the lowest line at fault
//   (exclusive scan)    out_start[v] = where data line v's output begins, n_data + 1 entries
//   k_vcf_gt_tile_lines one lane per tile boundary: the first data line whose output ends behind byte t * PARSE_TILE
//   k_vcf_gt_emit       output-dense, the shape of k_hap_spell: a workgroup owns 4096 consecutive output bytes, a lane 16 of
//                       them.  When the 16 lie inside one line's copied fields they move with one unaligned 16-byte load and
//                       one aligned 16-byte store; else they lie in two lines at most, and every byte is chosen between two
//                       unaligned 16-byte loads of the text, one per line, and the generated suffix "\tGT:GQ\t" GT ":" GQ
//                       "\n", which is a function of (call, gq, ploidy, position): one 16-byte store either way.
// A line may be longer than a tile: the tile's lane search then has one candidate.
// The eight-field walk, the suffix's bytes, text16 and k_vcf_gt_tile_lines are gki_vcf_text.h's, shared with the cohort's writer.
#include "gki_vcf_text.h"

namespace {

// Fault kinds: 1 = fewer than eight fields, 2 = a call outside -1 .. P.  Data lines at or beyond n_calls are left alone:
// the host refuses the piece.
__global__ __launch_bounds__(PARSE_BLOCK) void k_vcf_gt_lengths(const uint8_t *__restrict__ bytes,
                                                                const int64_t *__restrict__ line_end, int64_t n_lines,
                                                                const uint32_t *__restrict__ is_data,
                                                                const int64_t *__restrict__ variant_index, int64_t n_calls,
                                                                const int8_t *__restrict__ call,
                                                                const uint8_t *__restrict__ gq, int P,
                                                                int64_t *__restrict__ line_begin,
                                                                uint32_t *__restrict__ prefix_len,
                                                                uint32_t *__restrict__ out_len,
                                                                unsigned long long *__restrict__ first_bad) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_lines; i += stride) {
        if (!is_data[i]) continue;
        const int64_t v = variant_index[i];
        if (v >= n_calls) continue;
        const VcfLine l = vcf_line(bytes, line_end, i);
        int tabs;
        const int64_t p = vcf_eight_fields(bytes, l.b, l.e, &tabs);
        const int c = call[v];
        if (tabs < 7) line_fault(first_bad, v, 1);
        else if (c < -1 || c > P) line_fault(first_bad, v, 2);
        line_begin[v] = l.b;
        prefix_len[v] = (uint32_t)(p - l.b);
        out_len[v] = (uint32_t)(p - l.b) + (uint32_t)suffix_bytes(c, gq[v], P);
    }
}

// out[0, n_out): n_out = out_start[n_data] > 0.  `out` is 16-byte aligned; no byte outside out[0, n_out) is written and no
// byte outside bytes[0, n_bytes) is read.  An output line is at least 18 bytes (eight fields hold seven tabs, the suffix is
// at least 11), so a lane's 16 bytes lie in the line A of its first byte and at most the next one, B.  The text's byte for
// output position p of a line is bytes[line_begin - out_start + p]: the 16 positions of a lane are 16 consecutive bytes of
// the text for A and 16 for B, two unaligned loads that do not wait for one another, and every byte is then a choice between
// A's load, B's load and the generated suffix.  Nothing of this depends on control flow but the first test, for 16 bytes
// inside A's fields, which long lines take.
__global__ __launch_bounds__(PARSE_BLOCK) void k_vcf_gt_emit(const uint8_t *__restrict__ bytes, int64_t n_bytes, int64_t n_data,
                                                             const int64_t *__restrict__ line_begin,
                                                             const uint32_t *__restrict__ prefix_len,
                                                             const int64_t *__restrict__ out_start,
                                                             const int64_t *__restrict__ tile_line,
                                                             const int8_t *__restrict__ call, const uint8_t *__restrict__ gq,
                                                             int P, int64_t n_out, uint8_t *__restrict__ out) {
    const int64_t n_tiles = (n_out + PARSE_TILE - 1) / PARSE_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t v_lo = tile_line[tile];              // the same for every lane
        const int64_t v_hi = tile_line[tile + 1] < n_data ? tile_line[tile + 1] + 1 : n_data;
        const int64_t p0 = tile * PARSE_TILE + (int64_t)threadIdx.x * PARSE_LANE_BYTES;
        if (p0 >= n_out) continue;
        const int64_t v = first_site_after(out_start + 1, v_lo, v_hi, p0);        // line A: v < n_data
        const int64_t vb = v + 1 < n_data ? v + 1 : v;     // line B; A again behind the last line, where no byte is B's
        const int64_t begin_a = out_start[v], end_a = out_start[v + 1];
        const int64_t from_a = line_begin[v], from_b = line_begin[vb], pre_a = prefix_len[v], pre_b = prefix_len[vb];
        if (p0 + PARSE_LANE_BYTES <= n_out && p0 - begin_a + PARSE_LANE_BYTES <= pre_a) {
            Letters16 in;                                  // 16 bytes of A's fields
            __builtin_memcpy(&in, bytes + (from_a + (p0 - begin_a)), PARSE_LANE_BYTES);
            *reinterpret_cast<uint4 *>(out + p0) = make_uint4(in.w[0], in.w[1], in.w[2], in.w[3]);
            continue;
        }
        const int call_a = call[v], call_b = call[vb];
        const uint32_t gq_a = gq[v], gq_b = gq[vb];
        const Letters16 text_a = text16(bytes, n_bytes, from_a - begin_a + p0);
        const Letters16 text_b = text16(bytes, n_bytes, from_b - end_a + p0);
        uint32_t w[4];                                     // indexed by unrolled loops only: registers
#pragma unroll
        for (int j = 0; j < 4; j++) {
            w[j] = 0u;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int64_t p = p0 + 4 * j + i;
                const bool in_a = p < end_a;
                const int64_t at = p - (in_a ? begin_a : end_a), pre = in_a ? pre_a : pre_b;
                uint32_t byte = ((in_a ? text_a.w[j] : text_b.w[j]) >> (8 * i)) & 0xFFu;
                if (at >= pre) byte = suffix_byte((int)(at - pre), in_a ? call_a : call_b, in_a ? gq_a : gq_b, P);
                w[j] |= byte << (8 * i);
            }
        }
        if (p0 + PARSE_LANE_BYTES <= n_out)
            *reinterpret_cast<uint4 *>(out + p0) = make_uint4(w[0], w[1], w[2], w[3]);
        else {                                             // the output's last bytes
#pragma unroll
            for (int b = 0; b < PARSE_LANE_BYTES - 1; b++)
                if (p0 + b < n_out) out[p0 + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
        }
    }
}

// what both calls make of a piece: the data lines, per data line its begin / prefix / output length, the scan, the fault
struct WritePlan {
    VcfDataLines d;
    DevBuf line_begin, prefix_len, out_len, out_start;
    int64_t n_out = 0;
    LineFault fault;
};

int check_arguments(const char *who, const void *d_text, int64_t n_bytes, const void *d_call, const void *d_gq, int64_t n_calls,
                    int ploidy) {
    if (n_bytes < 0 || n_calls < 0) return gki_set_error(GKI_ERR_BAD_ARG, "%s: a negative size", who);
    if (n_bytes > VCF_WRITE_MAX_BYTES)
        return gki_set_error(GKI_ERR_BAD_ARG, "%s: a piece of %lld bytes is beyond 4 GiB", who, (long long)n_bytes);
    if (ploidy < 1 || ploidy > 8) return gki_set_error(GKI_ERR_BAD_ARG, "%s: ploidy must be in 1..8", who);
    if ((n_bytes > 0 && d_text == nullptr) || (n_calls > 0 && (d_call == nullptr || d_gq == nullptr)))
        return gki_set_error(GKI_ERR_BAD_ARG, "%s: the text, the calls or the qualities are NULL", who);
    return GKI_OK;
}

// n_bytes > 0.  *ms += the device time of the lengths kernel and the scan.
int make_plan(const char *who, const uint8_t *bytes, int64_t n_bytes, const void *d_call, const void *d_gq, int64_t n_calls,
              int ploidy, WritePlan &w, float *ms) {
    GKI_TRY(gki_vcf_data_lines(bytes, n_bytes, who, w.d));
    const int64_t n_data = w.d.n_data;
    if (n_data > n_calls)
        return gki_set_error(GKI_ERR_BAD_ARG, "%s: the text has %lld data lines, the caller has calls for %lld", who,
                             (long long)n_data, (long long)n_calls);
    if (n_data == 0) return GKI_OK;
    DevBuf totals, tmp;
    const int64_t tmp_bytes = gki_scan_tmp_bytes(n_data);
    GKI_TRY(line_fault_init(totals));
    HIP_TRY(w.line_begin.alloc((size_t)n_data * 8));
    HIP_TRY(w.prefix_len.alloc((size_t)n_data * 4));
    HIP_TRY(w.out_len.alloc((size_t)n_data * 4));
    HIP_TRY(w.out_start.alloc((size_t)(n_data + 1) * 8));
    HIP_TRY(tmp.alloc((size_t)tmp_bytes));
    TimerEvents ev;
    float t = 0.0f;
    GKI_TRY(ev.start(0));
    hipLaunchKernelGGL(k_vcf_gt_lengths, dim3(stream_grid(w.d.n_lines, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0, bytes,
                       w.d.line_end.get<const int64_t>(), w.d.n_lines, w.d.is_data.get<const uint32_t>(),
                       w.d.variant_index.get<const int64_t>(), n_calls, (const int8_t *)d_call, (const uint8_t *)d_gq, ploidy,
                       w.line_begin.get<int64_t>(), w.prefix_len.get<uint32_t>(), w.out_len.get<uint32_t>(),
                       totals.get<unsigned long long>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(gki_scan_u32_to_i64(w.out_len.get<const uint32_t>(), n_data, w.out_start.get<int64_t>(), tmp.get(), tmp_bytes, 0));
    GKI_TRY(ev.stop(0, &t));
    if (ms) *ms += t;
    GKI_TRY(gki_scan_total(w.out_start, n_data, &w.n_out));
    return line_fault_read(totals, &w.fault);
}

}  // namespace

extern "C" {

int gki_vcf_genotypes_count(const void *d_text, int64_t n_bytes, const void *d_call, const void *d_gq, int64_t n_calls,
                            int ploidy, int64_t *n_data_lines, int64_t *n_out_bytes, int64_t *first_bad_line,
                            int *first_bad_kind, float *kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_data_lines) *n_data_lines = 0;
    if (n_out_bytes) *n_out_bytes = 0;
    if (first_bad_line) *first_bad_line = -1;
    if (first_bad_kind) *first_bad_kind = 0;
    GKI_TRY(check_arguments("vcf_genotypes_count", d_text, n_bytes, d_call, d_gq, n_calls, ploidy));
    if (n_data_lines == nullptr || n_out_bytes == nullptr || first_bad_line == nullptr || first_bad_kind == nullptr)
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_genotypes_count: a result's pointer is NULL");
    if (n_bytes == 0) return GKI_OK;
    WritePlan w;
    const int rc = make_plan("vcf_genotypes_count", (const uint8_t *)d_text, n_bytes, d_call, d_gq, n_calls, ploidy, w, kernel_ms);
    *n_data_lines = w.d.n_data;                            // known before the piece is refused for having too many
    GKI_TRY(rc);
    *n_out_bytes = w.n_out;
    *first_bad_line = w.fault.line();
    *first_bad_kind = w.fault.kind();
    return GKI_OK;
}

int gki_vcf_genotypes_emit(const void *d_text, int64_t n_bytes, const void *d_call, const void *d_gq, int64_t n_calls,
                           int ploidy, void *d_out, int64_t out_capacity, int64_t *n_out_bytes, float *kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_out_bytes) *n_out_bytes = 0;
    GKI_TRY(check_arguments("vcf_genotypes_emit", d_text, n_bytes, d_call, d_gq, n_calls, ploidy));
    if (out_capacity < 0) return gki_set_error(GKI_ERR_BAD_ARG, "vcf_genotypes_emit: a negative capacity");
    if (n_bytes == 0) return GKI_OK;
    WritePlan w;
    GKI_TRY(make_plan("vcf_genotypes_emit", (const uint8_t *)d_text, n_bytes, d_call, d_gq, n_calls, ploidy, w, kernel_ms));
    if (w.fault.kind())
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_genotypes_emit: data line %lld is at fault (kind %d); nothing is written",
                             (long long)w.fault.line(), w.fault.kind());
    if (w.n_out > out_capacity)
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_genotypes_emit: the output needs %lld bytes, the buffer holds %lld",
                             (long long)w.n_out, (long long)out_capacity);
    if (w.n_out == 0) return GKI_OK;
    if (d_out == nullptr || ((uintptr_t)d_out & 15u))
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_genotypes_emit: the output is NULL or not 16-byte aligned");
    const int64_t n_tiles = ceil_div(w.n_out, PARSE_TILE);
    DevBuf tile_line;
    HIP_TRY(tile_line.alloc((size_t)(n_tiles + 1) * 8));
    TimerEvents ev;
    float t = 0.0f;
    GKI_TRY(ev.start(0));
    hipLaunchKernelGGL(k_vcf_gt_tile_lines, dim3(stream_grid(n_tiles + 1, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0,
                       w.out_start.get<const int64_t>(), w.d.n_data, n_tiles, tile_line.get<int64_t>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_vcf_gt_emit, dim3((unsigned)(n_tiles < 256 * 8 ? n_tiles : 256 * 8)), dim3(PARSE_BLOCK), 0, 0,
                       (const uint8_t *)d_text, n_bytes, w.d.n_data, w.line_begin.get<const int64_t>(),
                       w.prefix_len.get<const uint32_t>(), w.out_start.get<const int64_t>(), tile_line.get<const int64_t>(),
                       (const int8_t *)d_call, (const uint8_t *)d_gq, ploidy, w.n_out, (uint8_t *)d_out);
    HIP_TRY(hipGetLastError());
    GKI_TRY(ev.stop(0, &t));
    if (kernel_ms) *kernel_ms += t;
    if (n_out_bytes) *n_out_bytes = w.n_out;
    return GKI_OK;
}

}  // extern "C"
