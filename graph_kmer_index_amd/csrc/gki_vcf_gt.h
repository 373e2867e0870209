// The GT columns of VCF text in HBM: what the two kernels that walk them share -- k_af_genotypes (gki_vcf_af.hip, allele
// frequencies) and k_gt_matrix (gki_vcf_gt.hip, the haplotype matrix).  One wave takes a data line GT_STEP bytes a step,
// 16 per lane; the lane that holds a sample's tab parses the GT behind it.  The walk is stated once, in gt_walk_line, and
// the GT grammar of include/gki.h ("VCF allele frequencies") once, in gt_parse; what a kernel does with a field is its
// visitor's, what it does with the alleles its sink's.
#pragma once
#include "gki_text_lines.h"

constexpr int GT_STEP = 64 * PARSE_LANE_BYTES;             // bytes a wave takes per step
constexpr int GT_MAX_ALLELE_DIGITS = 9;
constexpr int GT_WINDOW = 8;                               // bytes of a GT and what closes it that one load holds

__device__ __forceinline__ bool is_digit(uint8_t c) { return c >= (uint8_t)'0' && c <= (uint8_t)'9'; }

__device__ __forceinline__ int64_t wave_uniform(int64_t x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)x >> 32));
    return (int64_t)((uint64_t)hi << 32 | lo);
}
__device__ __forceinline__ int wave_sum(int x) { return gki_lane_value(gki_wave_incl_sum(x), 63); }

// The 16 bytes at p0 of the line that ends at e, at any alignment; bytes at and behind e read as zero.  One load where
// 16 bytes lie inside the piece, else byte by byte: none behind n_bytes is read.
struct alignas(4) Bytes16 { uint32_t w[4]; };
__device__ __forceinline__ uint4 line_bytes16(const uint8_t *__restrict__ bytes, int64_t n_bytes, int64_t p0, int64_t e) {
    uint4 in = {0u, 0u, 0u, 0u};
    if (p0 + PARSE_LANE_BYTES <= n_bytes) {                // bytes behind e are masked by the caller
        if (p0 < e) {
            Bytes16 raw;
            __builtin_memcpy(&raw, bytes + p0, PARSE_LANE_BYTES);
            in = {raw.w[0], raw.w[1], raw.w[2], raw.w[3]};
        }
    } else {                                               // the piece's last bytes
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < PARSE_LANE_BYTES; j++)
            if (p0 + j < e) w[j >> 2] |= (uint32_t)bytes[p0 + j] << (8 * (j & 3));
        in = {w[0], w[1], w[2], w[3]};
    }
    return in;
}

// bit j set where byte p0 + j is a tab of the line that ends at e
__device__ __forceinline__ uint32_t line_tabs16(const uint4 &in, int64_t p0, int64_t e) {
    const int64_t left = e - p0;                           // bytes of the line from p0 on
    const uint32_t inside = left >= PARSE_LANE_BYTES ? 0xFFFFu : left > 0 ? (1u << (int)left) - 1u : 0u;
    return equal_mask16<'\t'>(in) & inside;
}

// FORMAT at bytes[p ..] of the line that ends at e begins with GT followed by ':' or its end
__device__ __forceinline__ bool format_begins_with_gt(const uint8_t *__restrict__ bytes, int64_t p, int64_t e) {
    return p + 2 <= e && bytes[p] == (uint8_t)'G' && bytes[p + 1] == (uint8_t)'T' &&
           (p + 2 == e || bytes[p + 2] == (uint8_t)':' || bytes[p + 2] == (uint8_t)'\t');
}

// A GT of `len` bytes at most, byte i of it at(i): alleles separated by '/' or '|', each '.' or 1 to 9 digits, closed by
// ':', a tab, or the end of the bytes when they reach the line's end (`whole`).  The sink is told of every allele in text
// order -- number(value) or missing() -- and of every slash().  1: closed; 0: an empty GT, an empty allele or any other
// byte; 2: the bytes ended first (never when `whole`).  Unless it returns 1 the sink holds a part of the GT: reset it.
template <class At, class Sink> __device__ __forceinline__ int gt_parse(At at, int64_t len, bool whole, Sink *sink) {
    for (int64_t i = 0;;) {
        if (i < len && at(i) == (uint8_t)'.') {
            i++;
            sink->missing();
        } else {
            int value = 0, digits = 0;
            for (; i < len && is_digit(at(i)) && digits <= GT_MAX_ALLELE_DIGITS; i++, digits++)
                value = value * 10 + (at(i) - (uint8_t)'0');
            if (i >= len && !whole) return 2;
            if (digits < 1 || digits > GT_MAX_ALLELE_DIGITS) return 0;
            sink->number(value);
        }
        if (i >= len) return whole ? 1 : 2;
        const uint8_t sep = at(i);
        if (sep == (uint8_t)':' || sep == (uint8_t)'\t') return 1;
        if (sep != (uint8_t)'/' && sep != (uint8_t)'|') return 0;
        if (sep == (uint8_t)'/') sink->slash();
        i++;
    }
}

// The GT at bytes[p ..] of the line that ends at e into a sink made by Sink(); false when it is at fault.  Eight bytes in
// one load hold a GT and what closes it in all but rare lines ("0|1" and a tab are four), so the parse reads registers:
// one load per GT instead of one per byte, which is what the kernels' rate hangs on.  A GT that is
// longer, and one within eight bytes of the piece's end, goes byte by byte from memory.
struct alignas(4) Bytes8 { uint32_t w[2]; };
template <class Sink> __device__ __forceinline__ bool gt_at(const uint8_t *__restrict__ bytes, int64_t n_bytes, int64_t p,
                                                            int64_t e, Sink *sink) {
    int state = 2;
    if (p + GT_WINDOW <= n_bytes) {
        Bytes8 raw;
        __builtin_memcpy(&raw, bytes + p, GT_WINDOW);
        const uint64_t window = (uint64_t)raw.w[1] << 32 | raw.w[0];
        *sink = Sink();
        state = gt_parse([window](int64_t i) { return (uint8_t)(window >> (8 * (int)i)); },
                         e - p < GT_WINDOW ? e - p : GT_WINDOW, e - p <= GT_WINDOW, sink);
    }
    if (state == 2) {
        *sink = Sink();
        state = gt_parse([bytes, p](int64_t i) { return bytes[p + i]; }, e - p, true, sink);
    }
    return state == 1;
}

// One wave walks the data line [b, e) (both wave-uniform), GT_STEP bytes a step: the lanes find the tabs of their 16 bytes
// and number them with a wave prefix sum on top of the line's running count, which the wave carries in a scalar.  FORMAT is
// field 8 (opened by tab number 8), sample s is field 9 + s.  The lane that holds tab 8 calls visit.format(ok), ok = FORMAT
// begins with GT; the lane that holds tab 9 + s calls visit.sample(s, p), p the sample field's first byte, where the kernel
// calls gt_at with its own sink.  Returns the line's tab count, wave-uniform.  Every lane of the wave must be active.
// The visitor is taken by value and refers to what the lane gathers in the kernel's own locals: with the state inside a
// visitor passed by reference k_af_genotypes needs a 59th register.
template <class Visitor> __device__ __forceinline__ int gt_walk_line(const uint8_t *__restrict__ bytes, int64_t n_bytes, int64_t b,
                                                                     int64_t e, int lane, Visitor visit) {
    int tabs_before = 0;
    for (int64_t base = b; base < e; base += GT_STEP) {
        const int64_t p0 = base + (int64_t)lane * PARSE_LANE_BYTES;
        const uint4 in = line_bytes16(bytes, n_bytes, p0, e);
        uint32_t tabs = line_tabs16(in, p0, e);
        const int mine = __popc(tabs);
        const int incl = gki_wave_incl_sum(mine);
        int number = tabs_before + incl - mine;            // tabs of the line before this lane's first
        tabs_before += gki_lane_value(incl, 63);
        while (tabs) {
            const int j = __ffs(tabs) - 1;
            tabs &= tabs - 1;
            number++;
            const int64_t p = p0 + j + 1;                  // the field tab `number` opens
            if (number == 8)
                visit.format(format_begins_with_gt(bytes, p, e));
            else if (number >= 9)
                visit.sample((int64_t)(number - 9), p);
        }
    }
    return tabs_before;
}
