// The line-end pass of gki_text_lines.h: where every line of a buffer ends.  The only whole-buffer work of the reads parser
// and the VCF passes.  Behind it the numbering of VCF data lines that the graph build's site pass, the allele frequencies
// and the haplotype matrix share (gki_vcf_data_lines).
//   k_parse_count_newlines   a workgroup counts the '\n' of its PARSE_TILE bytes: one 16-byte load per lane, a SWAR
//                            compare per word, popcounts, a wave and a workgroup sum
//   (exclusive scan)         tile -> number of line ends before it
//   k_parse_line_ends        the same loads again; a wave prefix sum of the lanes' popcounts numbers every '\n', and its
//                            byte position goes to line_end[its number]
//   k_vcf_is_data            one lane per line: header / blank / data by gki_text_lines.h's vcf_line, the rule k_vcf_classify
//                            applies too
//   (exclusive scan)         line -> data lines before it
#include "gki_text_lines.h"

namespace {

// 16-bit mask of the '\n' among bytes [pos, pos + 16) of the buffer; bytes at or past n are not read and are no line ends.
// A mask only: the FASTA parser's load_lane16 also hands the bytes on, which costs registers on the slow path.
__device__ __forceinline__ uint32_t newline_mask16(const uint8_t *__restrict__ bytes, int64_t pos, int64_t n) {
    if (pos >= n) return 0u;
    if (pos + PARSE_LANE_BYTES <= n && (reinterpret_cast<uintptr_t>(bytes + pos) & 15) == 0)
        return equal_mask16<10u>(*reinterpret_cast<const uint4 *>(bytes + pos));
    uint32_t m = 0;                                        // the buffer's last bytes, or a buffer that is not 16-byte aligned
#pragma unroll
    for (int j = 0; j < PARSE_LANE_BYTES; j++)
        if (pos + j < n && bytes[pos + j] == (uint8_t)'\n') m |= 1u << j;
    return m;
}

__global__ __launch_bounds__(PARSE_BLOCK) void k_parse_count_newlines(const uint8_t *__restrict__ bytes, int64_t n,
                                                                      uint32_t *__restrict__ tile_newlines) {
    __shared__ int lds[PARSE_BLOCK / 64];
    const int64_t pos = (int64_t)blockIdx.x * PARSE_TILE + (int64_t)threadIdx.x * PARSE_LANE_BYTES;
    int total;
    block_excl_sum(__popc(newline_mask16(bytes, pos, n)), lds, &total);   // every lane is active here
    if (threadIdx.x == 0) tile_newlines[blockIdx.x] = (uint32_t)total;
}

// line_end[i] = the byte position of the i-th '\n' (i < n_newlines: the count the first kernel made over the same bytes)
__global__ __launch_bounds__(PARSE_BLOCK) void k_parse_line_ends(const uint8_t *__restrict__ bytes, int64_t n,
                                                                 const int64_t *__restrict__ tile_first_line,
                                                                 int64_t n_newlines, int64_t *__restrict__ line_end) {
    __shared__ int lds[PARSE_BLOCK / 64];
    const int64_t pos = (int64_t)blockIdx.x * PARSE_TILE + (int64_t)threadIdx.x * PARSE_LANE_BYTES;
    uint32_t m = newline_mask16(bytes, pos, n);
    int total;
    int64_t line = tile_first_line[blockIdx.x] + block_excl_sum(__popc(m), lds, &total);
    while (m) {
        const int j = __ffs(m) - 1;
        m &= m - 1u;
        if (line < n_newlines) line_end[line] = pos + j;
        line++;
    }
}

__global__ __launch_bounds__(PARSE_BLOCK) void k_vcf_is_data(const uint8_t *__restrict__ bytes,
                                                             const int64_t *__restrict__ line_end, int64_t n_lines,
                                                             uint32_t *__restrict__ is_data) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_lines; i += stride)
        is_data[i] = vcf_line(bytes, line_end, i).data ? 1u : 0u;
}

}  // namespace

int gki_text_line_ends(const uint8_t *bytes, int64_t n, const char *who, DevBuf &line_end, int64_t *n_lines) {
    const int64_t n_tiles = ceil_div(n, PARSE_TILE);
    if (n_tiles > 0x7FFFFFFFll) return gki_set_error(GKI_ERR_BAD_ARG, "%s: buffer of %lld bytes is too large", who, (long long)n);
    DevBuf tile_newlines, tile_first_line, tmp;
    const int64_t tile_tmp_bytes = gki_scan_tmp_bytes(n_tiles);
    HIP_TRY(tile_newlines.alloc((size_t)n_tiles * 4));
    HIP_TRY(tile_first_line.alloc((size_t)(n_tiles + 1) * 8));
    HIP_TRY(tmp.alloc((size_t)tile_tmp_bytes));
    hipLaunchKernelGGL(k_parse_count_newlines, dim3((unsigned)n_tiles), dim3(PARSE_BLOCK), 0, 0, bytes, n,
                       tile_newlines.get<uint32_t>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(gki_scan_u32_to_i64(tile_newlines.get<const uint32_t>(), n_tiles, tile_first_line.get<int64_t>(), tmp.get(),
                                tile_tmp_bytes, 0));
    int64_t n_newlines = 0;
    uint8_t last = 0;
    GKI_TRY(gki_scan_total(tile_first_line, n_tiles, &n_newlines));
    HIP_TRY(hipMemcpy(&last, bytes + n - 1, 1, hipMemcpyDeviceToHost));
    const bool open_end = last != (uint8_t)'\n';           // the last line has no terminator
    *n_lines = n_newlines + (open_end ? 1 : 0);
    HIP_TRY(line_end.alloc((size_t)*n_lines * 8));
    hipLaunchKernelGGL(k_parse_line_ends, dim3((unsigned)n_tiles), dim3(PARSE_BLOCK), 0, 0, bytes, n,
                       tile_first_line.get<const int64_t>(), n_newlines, line_end.get<int64_t>());
    HIP_TRY(hipGetLastError());
    if (open_end) HIP_TRY(hipMemcpy(line_end.get<int64_t>() + n_newlines, &n, 8, hipMemcpyHostToDevice));
    return GKI_OK;
}

int gki_vcf_data_lines(const uint8_t *bytes, int64_t n, const char *who, VcfDataLines &out) {
    GKI_TRY(gki_text_line_ends(bytes, n, who, out.line_end, &out.n_lines));
    const int64_t n_lines = out.n_lines, tmp_bytes = gki_scan_tmp_bytes(n_lines);
    DevBuf tmp;                                            // the scan's scratch: gki_scan_total has waited when it is freed
    HIP_TRY(out.is_data.alloc((size_t)n_lines * 4));
    HIP_TRY(out.variant_index.alloc((size_t)(n_lines + 1) * 8));
    HIP_TRY(tmp.alloc((size_t)tmp_bytes));
    hipLaunchKernelGGL(k_vcf_is_data, dim3(stream_grid(n_lines, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0, bytes,
                       out.line_end.get<const int64_t>(), n_lines, out.is_data.get<uint32_t>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(gki_scan_u32_to_i64(out.is_data.get<const uint32_t>(), n_lines, out.variant_index.get<int64_t>(), tmp.get(),
                                tmp_bytes, 0));
    return gki_scan_total(out.variant_index, n_lines, &out.n_data);
}

int gki_vcf_expect_data_lines(const char *who, int64_t found, int64_t expected, const char *counted_by) {
    if (found == expected) return GKI_OK;
    return gki_set_error(GKI_ERR_BAD_ARG, "%s: the text has %lld data lines, %s %lld", who, (long long)found, counted_by,
                         (long long)expected);
}
