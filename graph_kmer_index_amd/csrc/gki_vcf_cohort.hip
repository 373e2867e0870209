// A genotyped cohort VCF's data lines from VCF text in HBM: per data line its first eight fields, "\tGT:GQ" and one GT:GQ
// column per sample.  The rules are those of include/gki.h ("genotyped cohort VCF text") and DESIGN.md 4.23.
//
// per piece of text (gki_vcf_cohort_count and again in gki_vcf_cohort_emit, which keeps no state):
//   (data lines)          gki_vcf_data_lines (gki_text_lines.hip)
//   k_vcf_cohort_pack     a workgroup owns 64 data lines x 64 samples of the batch, which is sample-major ([S][row_stride]):
//                         it reads them along the lines, turns them through LDS and writes the line-major record
//                         uint16[lines][S] (gq | (call + 1) << 8; only for the lines to be emitted), with __ballot the
//                         wide-column mask uint64[V][W] (W = ceil(S / 64); wide = call >= 0 and gq >= 10), and keeps the
//                         lowest line with a call outside -1 .. P (one atomic-min per wave)
//   k_vcf_cohort_lengths  one lane per data line: the walk to the eighth tab, the running count of wide columns in front
//                         of each mask word (__popcll), the output length; the lowest line with fewer than eight fields
//   (exclusive scan)      where each data line's output begins
//   k_vcf_gt_tile_lines   gki_vcf_text.h: the first line of every 4096-byte output tile
//   k_vcf_cohort_emit     output-dense: a workgroup owns 4096 consecutive output bytes, a lane 16 of them, stored as one
//                         aligned 16-byte word.  16 bytes inside a line's copied fields move with one unaligned 16-byte
//                         load.  A lane in a line's columns finds its column from the width identity -- column s begins
//                         (2P + 2) s + (wide columns below s) bytes behind "\tGT:GQ" -- by a search over the running counts
//                         of the mask words its offset admits and six register steps inside the word, loads the records of
//                         the at most five columns its bytes touch with one 12-byte load, and makes its bytes in registers.
// A line's columns may span many tiles: such a tile's search has one candidate.
#include "gki_vcf_text.h"

namespace {

constexpr int COHORT_TILE = 64;                            // lines and samples per workgroup of the pack pass
constexpr int64_t COHORT_MAX_SAMPLES = 1 << 20;
constexpr int FORMAT_BYTES = FORMAT_COLUMN_BYTES - 1;      // "\tGT:GQ": the column's own tab follows

// the device times of the calling thread's last call, apart (gki_vcf_cohort_kernel_ms)
thread_local float g_pack_ms = 0.0f, g_lengths_ms = 0.0f, g_emit_ms = 0.0f;

// The pack pass.  call / gq point at the batch's entry [0][first data line of the piece]; record (may be NULL) receives the
// lines [rec_from, rec_to) at record[(v - rec_from) * S + s].  Lines at or beyond n_data are not read.
__global__ __launch_bounds__(PARSE_BLOCK) void k_vcf_cohort_pack(const int8_t *__restrict__ call, const uint8_t *__restrict__ gq,
                                                                 int64_t row_stride, int64_t n_data, int S, int W, int P,
                                                                 int64_t rec_from, int64_t rec_to,
                                                                 uint16_t *__restrict__ record,
                                                                 unsigned long long *__restrict__ mask,
                                                                 unsigned long long *__restrict__ first_bad) {
    __shared__ uint16_t tile[COHORT_TILE][COHORT_TILE + 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int word = blockIdx.y;
    const int s0 = word * COHORT_TILE;
    const int64_t n_groups = (n_data + COHORT_TILE - 1) / COHORT_TILE;
    for (int64_t group = blockIdx.x; group < n_groups; group += gridDim.x) {
        const int64_t v0 = group * COHORT_TILE;
        int64_t bad = -1;
#pragma unroll 4
        for (int r = 0; r < COHORT_TILE / 4; r++) {        // a wave reads 64 consecutive lines of one sample
            const int j = wave * (COHORT_TILE / 4) + r, s = s0 + j;
            const int64_t v = v0 + lane;
            uint32_t rec = 0u;
            if (s < S && v < n_data) {
                const int c = call[(int64_t)s * row_stride + v];
                const uint32_t q = gq[(int64_t)s * row_stride + v];
                if (c < -1 || c > P) bad = v;
                rec = (q < 99u ? q : 99u) | (uint32_t)((c + 1) & 0xFF) << 8;
            }
            tile[lane][j] = (uint16_t)rec;
        }
        if (__any(bad >= 0)) {                              // the lowest such line of the wave, one atomic
            unsigned long long key = bad >= 0 ? (unsigned long long)bad : ~0ull;
#pragma unroll
            for (int d = 32; d; d >>= 1) {
                const unsigned long long other = __shfl_xor(key, d);
                key = other < key ? other : key;
            }
            if (lane == 0) line_fault(first_bad, (int64_t)key, 2);
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < COHORT_TILE / 4; r++) {        // a wave writes 64 consecutive samples of one line
            const int i = wave * (COHORT_TILE / 4) + r, s = s0 + lane;
            const int64_t v = v0 + i;
            const uint32_t rec = tile[i][lane];
            const bool live = s < S && v < n_data;
            const unsigned long long wide = __ballot(live && (rec >> 8) != 0u && (rec & 0xFFu) >= 10u);
            if (v < n_data && lane == 0) mask[v * W + word] = wide;
            if (live && record != nullptr && v >= rec_from && v < rec_to) record[(v - rec_from) * S + s] = (uint16_t)rec;
        }
        __syncthreads();
    }
}

// Per data line v < n_calls: where the line begins, the bytes of its first eight fields, wide_before[v][w] = the wide
// columns in front of mask word w, and the output length = fields + "\tGT:GQ" + (2P + 2) S + wide columns + '\n'.
__global__ __launch_bounds__(PARSE_BLOCK) void k_vcf_cohort_lengths(const uint8_t *__restrict__ bytes,
                                                                    const int64_t *__restrict__ line_end, int64_t n_lines,
                                                                    const uint32_t *__restrict__ is_data,
                                                                    const int64_t *__restrict__ variant_index, int64_t n_calls,
                                                                    const unsigned long long *__restrict__ mask, int S, int W,
                                                                    int P, int64_t *__restrict__ line_begin,
                                                                    uint32_t *__restrict__ prefix_len,
                                                                    uint32_t *__restrict__ wide_before,
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
        if (tabs < 7) line_fault(first_bad, v, 1);
        uint32_t wide = 0u;
        for (int w = 0; w < W; w++) {
            wide_before[v * W + w] = wide;
            wide += (uint32_t)__popcll(mask[v * W + w]);
        }
        line_begin[v] = l.b;
        prefix_len[v] = (uint32_t)(p - l.b);
        out_len[v] = (uint32_t)(p - l.b) + (uint32_t)FORMAT_BYTES + (uint32_t)(2 * P + 2) * (uint32_t)S + wide + 1u;
    }
}

// byte o of a column whose record is rec: '\t', the P alleles joined by '/', ':', the quality's one or two digits
__device__ __forceinline__ uint32_t column_byte(int o, uint32_t rec, int P) {
    const int call = (int)((rec >> 8) & 0xFFu) - 1;
    const uint32_t q = rec & 0xFFu;
    if (o == 0) return (uint32_t)'\t';
    o -= 1;
    if (o < 2 * P - 1) return (o & 1) ? (uint32_t)'/' : call < 0 ? (uint32_t)'.' : (o >> 1) < P - call ? (uint32_t)'0' : (uint32_t)'1';
    if (o == 2 * P - 1) return (uint32_t)':';
    if (call < 0) return (uint32_t)'.';
    const uint32_t tens = (q * 205u) >> 11;                // q / 10 for q < 1029
    return (uint32_t)'0' + ((q >= 10u && o == 2 * P) ? tens : q - 10u * tens);
}

// out[0, n_out), 16-byte aligned: the output of n_data lines whose arrays begin at the first of them (out_start from 0).
// An output line is at least 18 bytes (seven tabs, "\tGT:GQ", a column of at least four bytes, '\n'), so a lane's 16 bytes
// lie in the line A of its first byte and at most the next one, B; of B's columns they can hold the first two bytes of
// column 0 alone.  record holds 16 bytes more than its lines' columns, so that the 12-byte load of a line's last column
// stays inside it.  No byte outside out[0, n_out) is written and no byte outside bytes[0, n_bytes) is read.
__global__ __launch_bounds__(PARSE_BLOCK) void k_vcf_cohort_emit(const uint8_t *__restrict__ bytes, int64_t n_bytes, int64_t n_data,
                                                                 const int64_t *__restrict__ line_begin,
                                                                 const uint32_t *__restrict__ prefix_len,
                                                                 const int64_t *__restrict__ out_start,
                                                                 const int64_t *__restrict__ tile_line,
                                                                 const uint16_t *__restrict__ record,
                                                                 const unsigned long long *__restrict__ mask,
                                                                 const uint32_t *__restrict__ wide_before, int S, int W, int P,
                                                                 int64_t n_out, uint8_t *__restrict__ out) {
    const int64_t n_tiles = (n_out + PARSE_TILE - 1) / PARSE_TILE;
    const int B = 2 * P + 2;                               // a narrow column's bytes
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t v_lo = tile_line[tile];              // the same for every lane
        const int64_t v_hi = tile_line[tile + 1] < n_data ? tile_line[tile + 1] + 1 : n_data;
        const int64_t p0 = tile * PARSE_TILE + (int64_t)threadIdx.x * PARSE_LANE_BYTES;
        if (p0 >= n_out) continue;
        const int64_t v = first_site_after(out_start + 1, v_lo, v_hi, p0);        // line A: v < n_data
        const int64_t begin_a = out_start[v], end_a = out_start[v + 1];
        const int64_t from_a = line_begin[v], pre_a = prefix_len[v];
        const int64_t at0 = p0 - begin_a;                  // the lane's first byte in A
        if (p0 + PARSE_LANE_BYTES <= n_out && at0 + PARSE_LANE_BYTES <= pre_a) {
            Letters16 in;                                  // 16 bytes of A's fields
            __builtin_memcpy(&in, bytes + (from_a + at0), PARSE_LANE_BYTES);
            *reinterpret_cast<uint4 *>(out + p0) = make_uint4(in.w[0], in.w[1], in.w[2], in.w[3]);
            continue;
        }
        // A's columns: the column of the lane's first byte among them, by the width identity
        const int64_t cols_a = end_a - begin_a - pre_a - FORMAT_BYTES - 1;       // the bytes of A's columns
        int64_t k0 = at0 - pre_a - FORMAT_BYTES;           // the lane's first byte, counted from the columns' first
        k0 = k0 < 0 ? 0 : k0 >= cols_a ? cols_a - 1 : k0;
        const unsigned long long *mask_a = mask + v * W;
        const uint32_t *before_a = wide_before + v * W;
        int w_lo = (int)(k0 / ((B + 1) * 64)), w_hi = (int)(k0 / (B * 64));      // word w begins at 64 B w + before[w]
        w_hi = w_hi < W - 1 ? w_hi : W - 1;
        while (w_lo < w_hi) {                              // the last word that begins at or before k0
            const int mid = (w_lo + w_hi + 1) >> 1;
            if ((int64_t)64 * B * mid + before_a[mid] <= k0) w_lo = mid; else w_hi = mid - 1;
        }
        const unsigned long long m = mask_a[w_lo];
        const unsigned long long m_next = mask_a[w_lo + 1 < W ? w_lo + 1 : w_lo];
        const int64_t word_begin = (int64_t)64 * B * w_lo + (w_lo ? before_a[w_lo] : 0u);
        const int kw = (int)(k0 - word_begin);             // < 64 (B + 1)
        int i = 0;
#pragma unroll
        for (int step = 32; step; step >>= 1) {            // the last column of the word that begins at or before kw
            const int t = i + step;
            if (B * t + __popcll(m & ((1ull << t) - 1ull)) <= kw) i = t;
        }
        int o = kw - (B * i + __popcll(m & ((1ull << i) - 1ull)));               // the byte of that column
        const int64_t s_first = (int64_t)w_lo * 64 + i < S ? (int64_t)w_lo * 64 + i : S - 1;    // < S by the identity
        uint32_t wide = (uint32_t)(m >> i) | (i > 58 ? (uint32_t)(m_next << (64 - i)) : 0u);   // of that column and the next
        uint32_t r[3];                                     // their records: indexed by unrolled code only
        __builtin_memcpy(r, reinterpret_cast<const uint8_t *>(record + (v * S + s_first)), 12);
        uint64_t recs = (uint64_t)r[0] | (uint64_t)r[1] << 32;
        uint32_t recs_hi = r[2];
        // the rest: the text of A's fields, and B
        const int64_t vb = v + 1 < n_data ? v + 1 : v;     // line B; A again behind the last line, where no byte is B's
        Letters16 text_a, text_b;
        text_a.w[0] = text_a.w[1] = text_a.w[2] = text_a.w[3] = 0u;
        text_b = text_a;
        int64_t pre_b = 0;
        uint32_t rec_b = 0u;
        if (at0 < pre_a) text_a = text16(bytes, n_bytes, from_a + at0);
        if (end_a < p0 + PARSE_LANE_BYTES) {
            pre_b = prefix_len[vb];
            text_b = text16(bytes, n_bytes, line_begin[vb] - end_a + p0);
            rec_b = record[vb * S];
        }
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            w[j] = 0u;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int64_t p = p0 + 4 * j + b;
                const bool in_a = p < end_a;
                const int64_t at = p - (in_a ? begin_a : end_a), pre = in_a ? pre_a : pre_b;
                uint32_t byte = ((in_a ? text_a.w[j] : text_b.w[j]) >> (8 * b)) & 0xFFu;
                if (at >= pre) {
                    const int64_t k = at - pre;
                    if (k < FORMAT_BYTES) byte = (uint32_t)(FORMAT_COLUMN >> (8 * (int)k)) & 0xFFu;
                    else if (!in_a) byte = column_byte((int)(k - FORMAT_BYTES), rec_b, P);
                    else if (p == end_a - 1) byte = (uint32_t)'\n';
                    else {                                 // the next byte of A's columns
                        byte = column_byte(o, (uint32_t)recs & 0xFFFFu, P);
                        if (++o == B + (int)(wide & 1u)) {
                            o = 0;
                            wide >>= 1;
                            recs = recs >> 16 | (uint64_t)recs_hi << 48;
                            recs_hi >>= 16;
                        }
                    }
                }
                w[j] |= byte << (8 * b);
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

struct Batch {
    const int8_t *call;                                    // entry [0][the piece's first data line]
    const uint8_t *gq;
    int64_t row_stride, n_calls;
    int S, W, P;
};

// what both calls make of a piece: the data lines, the masks and running counts, per data line its begin / fields / output
// length, the fault; and for the lines [rec_from, rec_to) the records
struct CohortPlan {
    VcfDataLines d;
    DevBuf record, mask, wide_before, line_begin, prefix_len, out_len;
    LineFault fault;
};

int check_arguments(const char *who, const void *d_text, int64_t n_bytes, const void *d_call, const void *d_gq, int64_t row_stride,
                    int64_t first, int64_t n_samples, int64_t n_calls, int ploidy, Batch &b) {
    if (n_bytes < 0 || n_calls < 0 || first < 0 || row_stride < 0) return gki_set_error(GKI_ERR_BAD_ARG, "%s: a negative size", who);
    if (n_samples < 1 || n_samples > COHORT_MAX_SAMPLES)
        return gki_set_error(GKI_ERR_BAD_ARG, "%s: n_samples must be in 1..%lld", who, (long long)COHORT_MAX_SAMPLES);
    if (ploidy < 1 || ploidy > 8) return gki_set_error(GKI_ERR_BAD_ARG, "%s: ploidy must be in 1..8", who);
    if (first + n_calls > row_stride)
        return gki_set_error(GKI_ERR_BAD_ARG, "%s: %lld calls from entry %lld do not lie in a row of %lld", who, (long long)n_calls,
                             (long long)first, (long long)row_stride);
    if (n_bytes + FORMAT_BYTES + 1 + (2 * ploidy + 3) * n_samples > VCF_WRITE_MAX_BYTES)
        return gki_set_error(GKI_ERR_BAD_ARG, "%s: a piece of %lld bytes with %lld columns is beyond 4 GiB a line", who,
                             (long long)n_bytes, (long long)n_samples);
    if ((n_bytes > 0 && d_text == nullptr) || (n_calls > 0 && (d_call == nullptr || d_gq == nullptr)))
        return gki_set_error(GKI_ERR_BAD_ARG, "%s: the text, the calls or the qualities are NULL", who);
    b.call = (const int8_t *)d_call + first;
    b.gq = (const uint8_t *)d_gq + first;
    b.row_stride = row_stride;
    b.n_calls = n_calls;
    b.S = (int)n_samples;
    b.W = (int)ceil_div(n_samples, 64);
    b.P = ploidy;
    return GKI_OK;
}

// n_bytes > 0.  The records of the lines [rec_from, rec_to) are made (none when the range is empty).  *ms += the device
// time of the pack pass and of the lengths kernel.
int make_plan(const char *who, const uint8_t *bytes, int64_t n_bytes, const Batch &b, int64_t rec_from, int64_t rec_to,
              CohortPlan &c, float *ms) {
    GKI_TRY(gki_vcf_data_lines(bytes, n_bytes, who, c.d));
    const int64_t n_data = c.d.n_data;
    if (n_data > b.n_calls)
        return gki_set_error(GKI_ERR_BAD_ARG, "%s: the text has %lld data lines, the caller has calls for %lld", who,
                             (long long)n_data, (long long)b.n_calls);
    if (n_data == 0) return GKI_OK;
    if (rec_to > n_data) rec_to = n_data;
    DevBuf totals;
    GKI_TRY(line_fault_init(totals));
    if (rec_to > rec_from) HIP_TRY(c.record.alloc((size_t)(rec_to - rec_from) * b.S * 2 + 16));
    HIP_TRY(c.mask.alloc((size_t)n_data * b.W * 8));
    HIP_TRY(c.wide_before.alloc((size_t)n_data * b.W * 4));
    HIP_TRY(c.line_begin.alloc((size_t)n_data * 8));
    HIP_TRY(c.prefix_len.alloc((size_t)n_data * 4));
    HIP_TRY(c.out_len.alloc((size_t)n_data * 4));
    TimerEvents ev;
    float t = 0.0f;
    GKI_TRY(ev.start(0));
    const int64_t groups = ceil_div(n_data, COHORT_TILE);
    hipLaunchKernelGGL(k_vcf_cohort_pack, dim3((unsigned)(groups < 65536 ? groups : 65536), (unsigned)b.W), dim3(PARSE_BLOCK), 0,
                       0, b.call, b.gq, b.row_stride, n_data, b.S, b.W, b.P, rec_from, rec_to, c.record.get<uint16_t>(),
                       c.mask.get<unsigned long long>(), totals.get<unsigned long long>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(ev.stop(0, &g_pack_ms));
    GKI_TRY(ev.start(0));
    hipLaunchKernelGGL(k_vcf_cohort_lengths, dim3(stream_grid(c.d.n_lines, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0, bytes,
                       c.d.line_end.get<const int64_t>(), c.d.n_lines, c.d.is_data.get<const uint32_t>(),
                       c.d.variant_index.get<const int64_t>(), b.n_calls, c.mask.get<const unsigned long long>(), b.S, b.W, b.P,
                       c.line_begin.get<int64_t>(), c.prefix_len.get<uint32_t>(), c.wide_before.get<uint32_t>(),
                       c.out_len.get<uint32_t>(), totals.get<unsigned long long>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(ev.stop(0, &t));
    g_lengths_ms = t;
    if (ms) *ms += g_pack_ms + t;
    return line_fault_read(totals, &c.fault);
}

// out_start[0 .. n] = the exclusive scan of out_len[from, from + n), *total its last entry.  *ms += the scan's device time.
int scan_lengths(const CohortPlan &c, int64_t from, int64_t n, DevBuf &out_start, int64_t *total, float *ms) {
    DevBuf tmp;
    const int64_t tmp_bytes = gki_scan_tmp_bytes(n);
    HIP_TRY(out_start.alloc((size_t)(n + 1) * 8));
    HIP_TRY(tmp.alloc((size_t)tmp_bytes));
    TimerEvents ev;
    float t = 0.0f;
    GKI_TRY(ev.start(0));
    GKI_TRY(gki_scan_u32_to_i64(c.out_len.get<const uint32_t>() + from, n, out_start.get<int64_t>(), tmp.get(), tmp_bytes, 0));
    GKI_TRY(ev.stop(0, &t));
    g_lengths_ms += t;
    if (ms) *ms += t;
    return gki_scan_total(out_start, n, total);
}

}  // namespace

extern "C" {

int gki_vcf_cohort_count(const void *d_text, int64_t n_bytes, const void *d_call, const void *d_gq, int64_t row_stride,
                         int64_t first, int64_t n_samples, int64_t n_calls, int ploidy, int64_t *n_data_lines,
                         int64_t *n_out_bytes, int64_t *first_bad_line, int *first_bad_kind, void *d_line_start,
                         int64_t line_start_capacity, float *kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_data_lines) *n_data_lines = 0;
    if (n_out_bytes) *n_out_bytes = 0;
    if (first_bad_line) *first_bad_line = -1;
    if (first_bad_kind) *first_bad_kind = 0;
    g_pack_ms = g_lengths_ms = g_emit_ms = 0.0f;
    Batch b;
    GKI_TRY(check_arguments("vcf_cohort_count", d_text, n_bytes, d_call, d_gq, row_stride, first, n_samples, n_calls, ploidy, b));
    if (n_data_lines == nullptr || n_out_bytes == nullptr || first_bad_line == nullptr || first_bad_kind == nullptr)
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_cohort_count: a result's pointer is NULL");
    if (n_bytes == 0) return GKI_OK;
    CohortPlan c;
    const int rc = make_plan("vcf_cohort_count", (const uint8_t *)d_text, n_bytes, b, 0, 0, c, kernel_ms);
    *n_data_lines = c.d.n_data;                            // known before the piece is refused for having too many
    GKI_TRY(rc);
    *first_bad_line = c.fault.line();
    *first_bad_kind = c.fault.kind();
    if (c.d.n_data == 0) return GKI_OK;
    if (d_line_start != nullptr && line_start_capacity < c.d.n_data + 1)
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_cohort_count: the line starts need %lld entries, the buffer holds %lld",
                             (long long)(c.d.n_data + 1), (long long)line_start_capacity);
    DevBuf out_start;
    GKI_TRY(scan_lengths(c, 0, c.d.n_data, out_start, n_out_bytes, kernel_ms));
    if (d_line_start != nullptr)
        HIP_TRY(hipMemcpy(d_line_start, out_start.get(), (size_t)(c.d.n_data + 1) * 8, hipMemcpyDeviceToDevice));
    return GKI_OK;
}

int gki_vcf_cohort_emit(const void *d_text, int64_t n_bytes, const void *d_call, const void *d_gq, int64_t row_stride,
                        int64_t first, int64_t n_samples, int64_t n_calls, int ploidy, int64_t line_from, int64_t line_to,
                        void *d_out, int64_t out_capacity, int64_t *n_out_bytes, float *kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_out_bytes) *n_out_bytes = 0;
    g_pack_ms = g_lengths_ms = g_emit_ms = 0.0f;
    Batch b;
    GKI_TRY(check_arguments("vcf_cohort_emit", d_text, n_bytes, d_call, d_gq, row_stride, first, n_samples, n_calls, ploidy, b));
    if (out_capacity < 0) return gki_set_error(GKI_ERR_BAD_ARG, "vcf_cohort_emit: a negative capacity");
    if (line_from < 0 || line_to < line_from) return gki_set_error(GKI_ERR_BAD_ARG, "vcf_cohort_emit: not a range of lines");
    if (n_bytes == 0) {
        if (line_to > 0) return gki_set_error(GKI_ERR_BAD_ARG, "vcf_cohort_emit: the lines end at %lld, the text has none", (long long)line_to);
        return GKI_OK;
    }
    CohortPlan c;
    GKI_TRY(make_plan("vcf_cohort_emit", (const uint8_t *)d_text, n_bytes, b, line_from, line_to, c, kernel_ms));
    if (line_to > c.d.n_data)
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_cohort_emit: the lines end at %lld, the text has %lld", (long long)line_to,
                             (long long)c.d.n_data);
    if (c.fault.kind())
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_cohort_emit: data line %lld is at fault (kind %d); nothing is written",
                             (long long)c.fault.line(), c.fault.kind());
    const int64_t n = line_to - line_from;
    if (n == 0) return GKI_OK;
    DevBuf out_start, tile_line;
    int64_t n_out = 0;
    GKI_TRY(scan_lengths(c, line_from, n, out_start, &n_out, kernel_ms));
    if (n_out > out_capacity)
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_cohort_emit: the output needs %lld bytes, the buffer holds %lld",
                             (long long)n_out, (long long)out_capacity);
    if (d_out == nullptr || ((uintptr_t)d_out & 15u))
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_cohort_emit: the output is NULL or not 16-byte aligned");
    const int64_t n_tiles = ceil_div(n_out, PARSE_TILE);
    HIP_TRY(tile_line.alloc((size_t)(n_tiles + 1) * 8));
    TimerEvents ev;
    float t = 0.0f;
    GKI_TRY(ev.start(0));
    hipLaunchKernelGGL(k_vcf_gt_tile_lines, dim3(stream_grid(n_tiles + 1, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0,
                       out_start.get<const int64_t>(), n, n_tiles, tile_line.get<int64_t>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_vcf_cohort_emit, dim3((unsigned)(n_tiles < 256 * 8 ? n_tiles : 256 * 8)), dim3(PARSE_BLOCK), 0, 0,
                       (const uint8_t *)d_text, n_bytes, n, c.line_begin.get<const int64_t>() + line_from,
                       c.prefix_len.get<const uint32_t>() + line_from, out_start.get<const int64_t>(),
                       tile_line.get<const int64_t>(), c.record.get<const uint16_t>(),
                       c.mask.get<const unsigned long long>() + line_from * b.W,
                       c.wide_before.get<const uint32_t>() + line_from * b.W, b.S, b.W, b.P, n_out, (uint8_t *)d_out);
    HIP_TRY(hipGetLastError());
    GKI_TRY(ev.stop(0, &t));
    g_emit_ms = t;
    if (kernel_ms) *kernel_ms += t;
    if (n_out_bytes) *n_out_bytes = n_out;
    return GKI_OK;
}

int gki_vcf_cohort_kernel_ms(float *pack_ms, float *lengths_ms, float *emit_ms) {
    if (pack_ms) *pack_ms = g_pack_ms;
    if (lengths_ms) *lengths_ms = g_lengths_ms;
    if (emit_ms) *emit_ms = g_emit_ms;
    return GKI_OK;
}

}  // extern "C"
