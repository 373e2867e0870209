// What the two writers of genotyped VCF text share -- one sample column (gki_vcf_write.hip) and a cohort's columns
// (gki_vcf_cohort.hip): the walk to a data line's eighth tab, the bytes of one sample column, an unaligned 16-byte read of
// the text, and the search of every output tile's first line.  The rules are those of include/gki.h ("genotyped VCF text",
// "genotyped cohort VCF text").
#pragma once
#include "gki_seq_gather.h"
#include "gki_text_lines.h"

constexpr int64_t VCF_WRITE_MAX_BYTES = 0xFFFFFFFFll - 64;   // a line's output length fits uint32 with its suffix
constexpr uint64_t FORMAT_COLUMN = 0x0951473A544709ull;       // "\tGT:GQ\t", the first byte the lowest
constexpr int FORMAT_COLUMN_BYTES = 7;

__device__ __forceinline__ int gq_digits(int call, uint32_t gq) { return call < 0 ? 1 : gq >= 100u ? 3 : gq >= 10u ? 2 : 1; }

// bytes a data line's suffix has: the FORMAT column, P alleles and P - 1 slashes, ':', the GQ, '\n'
__device__ __forceinline__ int suffix_bytes(int call, uint32_t gq, int P) {
    return FORMAT_COLUMN_BYTES + (2 * P - 1) + 1 + gq_digits(call, gq) + 1;
}

// byte k of that suffix
__device__ __forceinline__ uint32_t suffix_byte(int k, int call, uint32_t gq, int P) {
    if (k < FORMAT_COLUMN_BYTES) return (uint32_t)(FORMAT_COLUMN >> (8 * k)) & 0xFFu;
    k -= FORMAT_COLUMN_BYTES;
    if (k < 2 * P - 1) return (k & 1) ? (uint32_t)'/' : call < 0 ? (uint32_t)'.' : (k >> 1) < P - call ? (uint32_t)'0' : (uint32_t)'1';
    k -= 2 * P - 1;
    if (k == 0) return (uint32_t)':';
    k -= 1;
    const int nd = gq_digits(call, gq);
    if (k >= nd) return (uint32_t)'\n';
    if (call < 0) return (uint32_t)'.';
    const uint32_t digit = k == nd - 1 ? gq % 10u : k == nd - 2 ? (gq / 10u) % 10u : gq / 100u;
    return (uint32_t)'0' + digit;
}

// The first eight fields of the data line [b, e): returns where they end -- the eighth tab, or e -- and *tabs = the tabs
// met on the way (8 at the eighth tab; fewer than 7: the line has fewer than eight fields)
__device__ __forceinline__ int64_t vcf_eight_fields(const uint8_t *__restrict__ bytes, int64_t b, int64_t e, int *tabs) {
    int t = 0;
    int64_t p = b;
    for (; p < e; p++)
        if (bytes[p] == (uint8_t)'\t' && ++t == 8) break;
    *tabs = t;
    return p;
}

// 16 bytes of the text at src .. src + 15, at any alignment; a byte outside [0, n) reads as 0
__device__ __forceinline__ Letters16 text16(const uint8_t *__restrict__ bytes, int64_t n, int64_t src) {
    Letters16 r;
    if (src >= 0 && src + PARSE_LANE_BYTES <= n) {
        __builtin_memcpy(&r, bytes + src, PARSE_LANE_BYTES);
        return r;
    }
    r.w[0] = r.w[1] = r.w[2] = r.w[3] = 0u;                 // the text's first or last bytes: one by one
#pragma unroll
    for (int j = 0; j < PARSE_LANE_BYTES; j++)
        if (src + j >= 0 && src + j < n) r.w[j >> 2] |= (uint32_t)bytes[src + j] << (8 * (j & 3));
    return r;
}

namespace {

// tile_line[t] = the first data line whose output ends behind byte t * PARSE_TILE (n_data when there is none), t = 0 .. n_tiles
__global__ __launch_bounds__(PARSE_BLOCK) void k_vcf_gt_tile_lines(const int64_t *__restrict__ out_start, int64_t n_data,
                                                                   int64_t n_tiles, int64_t *__restrict__ tile_line) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t <= n_tiles; t += stride)
        tile_line[t] = first_site_after(out_start + 1, 0, n_data, t * PARSE_TILE);
}

}  // namespace
