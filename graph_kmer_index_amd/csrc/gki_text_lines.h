// Lines of ASCII text in HBM: what the six parsers of text files share -- reads (gki_reads_parse.hip), VCF
// (gki_vcf_parse.hip), the graph build's site pass (gki_graph_build.hip), the VCF's allele frequencies (gki_vcf_af.hip), its
// haplotype matrix (gki_vcf_gt.hip) and the reference FASTA (gki_fasta_parse.hip).
// The tile geometry, the SWAR byte test, the block prefix and the wave copy serve the dense kernels; the line-end pass
// (kernels in gki_text_lines.hip) serves all but the FASTA parser; the VCF line rules (vcf_line, vcf_fields, vcf_pos_value)
// and the record of the lowest line at fault (LineFault) serve the four VCF passes.  The site pass, the allele frequencies
// and the haplotype matrix number the data lines through one front end, gki_vcf_data_lines (k_vcf_is_data, the scan, the
// total), and check the caller's count with gki_vcf_expect_data_lines; the VCF parser applies the same vcf_line in its
// fused k_vcf_classify, which makes the fields in the same walk.
#pragma once
#include "gki_common.h"

constexpr int PARSE_BLOCK = 256;                          // threads per workgroup
constexpr int PARSE_LANE_BYTES = 16;                      // one 16-byte load per lane
constexpr int PARSE_TILE = PARSE_BLOCK * PARSE_LANE_BYTES; // 4096 bytes per workgroup

// str.strip() of ASCII text removes 0x09-0x0D, 0x1C-0x1F and the blank
__device__ __forceinline__ bool is_strip_byte(uint8_t c) {
    return c == 0x20 || (c >= 0x09 && c <= 0x0D) || (c >= 0x1C && c <= 0x1F);
}

// bit j set where byte j of the word equals C: x = w ^ CCCCCCCC has a zero byte there; (x & 0x7F) + 0x7F carries into
// bit 7 of a byte exactly when its low seven bits are not all zero, and never beyond the byte, so the test is exact per byte
template <uint32_t C> __device__ __forceinline__ uint32_t equal_bits4(uint32_t w) {
    const uint32_t x = w ^ (C * 0x01010101u);
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    const uint32_t z = ~(t | x | 0x7F7F7F7Fu) >> 7;       // bit 0, 8, 16, 24 = byte 0..3 equals C
    return (z * 0x01020408u) >> 24;                       // gathered into bits 0..3 (no two partial products meet)
}
template <uint32_t C> __device__ __forceinline__ uint32_t equal_mask16(const uint4 &v) {
    return equal_bits4<C>(v.x) | equal_bits4<C>(v.y) << 4 | equal_bits4<C>(v.z) << 8 | equal_bits4<C>(v.w) << 12;
}

// The lanes' counts summed over the workgroup's four waves, in lane order: returns the sum of the lanes before this one,
// *total = the sum of all.  Every lane calls it; lds holds one int per wave and serves one call.  A count may pack two
// fields (high and low half) that do not overflow over the workgroup.  64 bits wide as its users add it to a tile's 64-bit
// offset: formed in 32 bits, `incl - cnt` is folded back into the scan's six partial sums, all live across the barrier.
__device__ __forceinline__ int64_t block_excl_sum(int cnt, int *lds, int *total) {
    const int incl = gki_wave_incl_sum(cnt);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) lds[wave] = incl;       // lane 63's inclusive sum is its wave's total
    __syncthreads();
    int b = 0, t = 0;
#pragma unroll
    for (int w = 0; w < PARSE_BLOCK / 64; w++) {
        const int v = lds[w];
        if (w < wave) b += v;
        t += v;
    }
    *total = t;
    return (int64_t)b + (incl - cnt);
}

// one wave copies len bytes, 64 a step
__device__ __forceinline__ void wave_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, int64_t len, int lane) {
    for (int64_t j = lane; j < len; j += 64) dst[j] = src[j];
}

// Line i is bytes [b, e) = [line_end[i - 1] + 1, line_end[i]), its '\n' excluded
struct TextLine { int64_t b, e; };
__device__ __forceinline__ TextLine text_line(const int64_t *line_end, int64_t i) {
    return {i ? line_end[i - 1] + 1 : 0, line_end[i]};
}

constexpr int VCF_MAX_POS_DIGITS = 18;                     // 10^18 - 1 fits int64
constexpr int VCF_FIELDS = 5;                              // CHROM POS ID REF ALT: no kernel walks beyond them

// Line i of VCF text: every '\r' at its end is dropped; a data line is not empty, does not begin with '#' and is not blank
// (nothing but strip bytes).  One function: a kernel drops what it does not use, two helpers cost k_vcf_is_data a register.
struct VcfLine { int64_t b, e; bool data; };
__device__ __forceinline__ VcfLine vcf_line(const uint8_t *bytes, const int64_t *line_end, int64_t i) {
    auto [b, e] = text_line(line_end, i);
    while (e > b && bytes[e - 1] == (uint8_t)'\r') e--;
    bool data = b < e && bytes[b] != (uint8_t)'#';
    if (data) {                                            // ends at the first byte that is no strip byte
        int64_t p = b;
        while (p < e && is_strip_byte(bytes[p])) p++;
        data = p < e;
    }
    return {b, e, data};
}

// Fields 0..4 of the data line [b, e): field f is closed by tab number f + 1, or by the line's end.  n = how many of them
// the line has (1..5); field f < n is bytes [begin(f), end[f]).  The walk never goes beyond the fifth tab.
struct VcfFields {
    int64_t b, end[VCF_FIELDS];
    int n;
    __device__ __forceinline__ int64_t begin(int f) const { return f ? end[f - 1] + 1 : b; }
    __device__ __forceinline__ int64_t len(int f) const { return end[f] - begin(f); }
};
__device__ __forceinline__ VcfFields vcf_fields(const uint8_t *__restrict__ bytes, int64_t b, int64_t e) {
    VcfFields f;
    f.b = b;
    f.n = 0;
#pragma unroll
    for (int k = 0; k < VCF_FIELDS; k++) f.end[k] = e;
    for (int64_t p = b; f.n < VCF_FIELDS; p++) {
        const bool last = p == e;
        if (last || bytes[p] == (uint8_t)'\t') {
#pragma unroll
            for (int k = 0; k < VCF_FIELDS; k++) f.end[k] = k == f.n ? p : f.end[k];
            f.n++;
            if (last) break;
        }
    }
    return f;
}

// POS is 1 to 18 plain digits: bytes [b, e) -> *value; false otherwise, and *value is then of no meaning
__device__ __forceinline__ bool vcf_pos_value(const uint8_t *__restrict__ bytes, int64_t b, int64_t e, int64_t *value) {
    int64_t v = 0;
    bool ok = e > b && e - b <= VCF_MAX_POS_DIGITS;
    for (int64_t p = b; ok && p < e; p++) {
        const uint8_t c = bytes[p];
        ok = c >= (uint8_t)'0' && c <= (uint8_t)'9';
        v = v * 10 + (c - (uint8_t)'0');
    }
    *value = v;
    return ok;
}

// bytes[0, n) on the device (n > 0) -> line_end, int64[*n_lines]: line i is bytes [line_end[i - 1] + 1, line_end[i]),
// its '\n' excluded; a last line without '\n' ends at n.  *n_lines = number of '\n' + (the last byte is not '\n').
// The kernels are k_parse_count_newlines and k_parse_line_ends of gki_text_lines.hip; `who` begins the error messages.
int gki_text_line_ends(const uint8_t *bytes, int64_t n, const char *who, DevBuf &line_end, int64_t *n_lines);

// the total of an exclusive scan of n inputs (gki_scan_u32_to_i64): its entry n, read back; waits for the scan
static inline int gki_scan_total(const DevBuf &scan, int64_t n, int64_t *total) {
    HIP_TRY(hipMemcpy(total, scan.get<const int64_t>() + n, 8, hipMemcpyDeviceToHost));
    return GKI_OK;
}

// The data lines of VCF text, numbered: is_data uint32[n_lines] by vcf_line (k_vcf_is_data of gki_text_lines.hip),
// variant_index int64[n_lines + 1] its exclusive scan -- the data lines before line i -- and n_data the scan's total.
struct VcfDataLines {
    DevBuf line_end, is_data, variant_index;
    int64_t n_lines = 0, n_data = 0;
};
// bytes[0, n) on the device (n > 0) -> out; waits for the device (gki_scan_total).  `who` begins the error messages.
int gki_vcf_data_lines(const uint8_t *bytes, int64_t n, const char *who, VcfDataLines &out);
// GKI_ERR_BAD_ARG unless the text has the data lines its caller counted before (through `counted_by`)
int gki_vcf_expect_data_lines(const char *who, int64_t found, int64_t expected, const char *counted_by = "the caller expects");

// The lowest line at fault of a pass and its kind (1..7), in one word for atomicMin: line << 3 | kind, all ones when there
// is none.  A pass with flag words of its own derives its totals from LineFault, so that one copy brings all of them back.
struct LineFault {
    unsigned long long first_bad = ~0ull;
    int64_t line() const { return first_bad == ~0ull ? -1 : (int64_t)(first_bad >> 3); }
    int kind() const { return first_bad == ~0ull ? 0 : (int)(first_bad & 7); }
};
__device__ __forceinline__ void line_fault(unsigned long long *first_bad, int64_t line, int kind) {
    atomicMin(first_bad, (unsigned long long)line << 3 | (unsigned long long)kind);
}
// host side: a pass's totals T (LineFault or derived from it) in their first state on the device, and read back
template <class T = LineFault> static inline int line_fault_init(DevBuf &totals) {
    const T none;
    HIP_TRY(totals.alloc(sizeof(T)));
    HIP_TRY(hipMemcpy(totals.get(), &none, sizeof(T), hipMemcpyHostToDevice));
    return GKI_OK;
}
template <class T> static inline int line_fault_read(const DevBuf &totals, T *out) {
    HIP_TRY(hipMemcpy(out, totals.get(), sizeof(T), hipMemcpyDeviceToHost));
    return GKI_OK;
}
