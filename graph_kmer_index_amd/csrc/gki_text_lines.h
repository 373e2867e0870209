// Lines of ASCII text in HBM, shared by the parsers of text files (gki_reads_parse.hip, gki_vcf_parse.hip): the tile
// geometry of the line-end pass, its host-side driver, and the small device helpers both parsers use.
#pragma once
#include "gki_common.h"

constexpr int PARSE_BLOCK = 256;                          // threads per workgroup
constexpr int PARSE_LANE_BYTES = 16;                      // one 16-byte load per lane
constexpr int PARSE_TILE = PARSE_BLOCK * PARSE_LANE_BYTES; // 4096 bytes per workgroup

// str.strip() of ASCII text removes 0x09-0x0D, 0x1C-0x1F and the blank
__device__ __forceinline__ bool is_strip_byte(uint8_t c) {
    return c == 0x20 || (c >= 0x09 && c <= 0x0D) || (c >= 0x1C && c <= 0x1F);
}

// the lanes' values summed over the workgroup's four waves: (sum of the waves before this one, sum of all)
__device__ __forceinline__ void block_wave_offsets(int wave_total, int *lds, int *before, int *total) {
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) lds[wave] = wave_total;
    __syncthreads();
    int b = 0, t = 0;
#pragma unroll
    for (int w = 0; w < PARSE_BLOCK / 64; w++) {
        const int v = lds[w];
        if (w < wave) b += v;
        t += v;
    }
    *before = b;
    *total = t;
}

// bytes[0, n) on the device (n > 0) -> line_end, int64[*n_lines]: line i is bytes [line_end[i - 1] + 1, line_end[i]),
// its '\n' excluded; a last line without '\n' ends at n.  *n_lines = number of '\n' + (the last byte is not '\n').
// The kernels are k_parse_count_newlines and k_parse_line_ends of gki_reads_parse.hip; `who` begins the error messages.
int gki_text_line_ends(const uint8_t *bytes, int64_t n, const char *who, DevBuf &line_end, int64_t *n_lines);
