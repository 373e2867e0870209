// FASTA / FASTQ text parsed in HBM: the raw bytes of a reads file (or of a piece of one that ends at a line end) become
// the layout the read-side kernels take -- the letters of all reads back to back, uint8, and int64 read_start[n_reads + 1]
// (gki_hash_reads, gki_probe_reads_count_nodes).  The rules are those of include/gki.h ("reads files"); the FASTA one is
// the reference's (read_kmers.py:18-25: every line that does not start with '>' is one read, stripped).
//
//   k_parse_count_newlines   a workgroup counts the '\n' of its PARSE_TILE bytes: one 16-byte load per lane, a SWAR
//                            compare per word, popcounts, a wave and a workgroup sum
//   (exclusive scan)         tile -> number of line ends before it
//   k_parse_line_ends        the same loads again; a wave prefix sum of the lanes' popcounts numbers every '\n', and its
//                            byte position goes to line_end[its number]
//   k_parse_classify         one lane per line: header / read / FASTQ role by position, the record-shape check, the strip;
//                            writes whether the line is a read, where its letters begin and how many there are
//   (two exclusive scans)    line -> number of reads before it, line -> letters before it
//   k_parse_emit             one wave per line: read_start[read] and the letters, copied 64 bytes per step
//
// A line may be of any length: nothing here holds a line in a workgroup.  Lines of 2^32 letters or more after the strip
// are refused (GKI_ERR_BAD_ARG): a read's length passes through the 32-bit input of the scan.
#include "gki_text_lines.h"

namespace {

// bit j set where byte j of the word is '\n': x = w ^ 0x0A.. has a zero byte there; (x & 0x7F) + 0x7F carries into bit 7
// of a byte exactly when its low seven bits are not all zero, and never beyond the byte, so the test is exact per byte
__device__ __forceinline__ uint32_t newline_bits4(uint32_t w) {
    const uint32_t x = w ^ 0x0A0A0A0Au;
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    const uint32_t z = ~(t | x | 0x7F7F7F7Fu) >> 7;       // bit 0, 8, 16, 24 = byte 0..3 is '\n'
    return (z * 0x01020408u) >> 24;                       // gathered into bits 0..3 (no two partial products meet)
}

// 16-bit mask of the '\n' among bytes [pos, pos + 16) of the buffer; bytes at or past n are not read and are no line ends
__device__ __forceinline__ uint32_t newline_mask16(const uint8_t *__restrict__ bytes, int64_t pos, int64_t n) {
    if (pos >= n) return 0u;
    if (pos + PARSE_LANE_BYTES <= n && (reinterpret_cast<uintptr_t>(bytes + pos) & 15) == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(bytes + pos);
        return newline_bits4(v.x) | newline_bits4(v.y) << 4 | newline_bits4(v.z) << 8 | newline_bits4(v.w) << 12;
    }
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
    const int cnt = __popc(newline_mask16(bytes, pos, n));
    const int incl = gki_wave_incl_sum(cnt);               // every lane is active here
    int before, total;
    block_wave_offsets(incl, lds, &before, &total);        // lane 63's inclusive sum is its wave's total
    if (threadIdx.x == 0) tile_newlines[blockIdx.x] = (uint32_t)total;
}

// line_end[i] = the byte position of the i-th '\n' (i < n_newlines: the count the first kernel made over the same bytes)
__global__ __launch_bounds__(PARSE_BLOCK) void k_parse_line_ends(const uint8_t *__restrict__ bytes, int64_t n,
                                                                 const int64_t *__restrict__ tile_first_line,
                                                                 int64_t n_newlines, int64_t *__restrict__ line_end) {
    __shared__ int lds[PARSE_BLOCK / 64];
    const int64_t pos = (int64_t)blockIdx.x * PARSE_TILE + (int64_t)threadIdx.x * PARSE_LANE_BYTES;
    uint32_t m = newline_mask16(bytes, pos, n);
    const int cnt = __popc(m);
    const int incl = gki_wave_incl_sum(cnt);
    int before, total;
    block_wave_offsets(incl, lds, &before, &total);
    int64_t line = tile_first_line[blockIdx.x] + before + (incl - cnt);
    while (m) {
        const int j = __ffs(m) - 1;
        m &= m - 1u;
        if (line < n_newlines) line_end[line] = pos + j;
        line++;
    }
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
    HIP_TRY(hipMemcpy(&n_newlines, tile_first_line.get<const int64_t>() + n_tiles, 8, hipMemcpyDeviceToHost));
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

namespace {

struct ParseTotals { unsigned long long n_bad; unsigned int too_long; unsigned int pad; };

// Line i is bytes [line_end[i - 1] + 1, line_end[i]) -- its terminator excluded; the last line of a buffer that does not
// end in '\n' ends at n (the host stores that line_end).  fastq == 0: a line whose first raw byte is '>' is a header and
// every other line a read.  fastq != 0: with g = (i + line_phase) % 4, line g == 1 is a read, a line g == 0 that does not
// begin with '@' and a line g == 2 that does not begin with '+' are counted in n_bad.  The first raw byte of an empty line
// is its '\n'.
__global__ __launch_bounds__(PARSE_BLOCK) void k_parse_classify(const uint8_t *__restrict__ bytes,
                                                                const int64_t *__restrict__ line_end, int64_t n_lines,
                                                                int fastq, int line_phase, uint32_t *__restrict__ is_read,
                                                                uint32_t *__restrict__ read_len,
                                                                int64_t *__restrict__ letters_begin,
                                                                ParseTotals *__restrict__ totals) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_lines; i += stride) {
        int64_t b = i ? line_end[i - 1] + 1 : 0;
        int64_t e = line_end[i];
        const uint8_t first = b < e ? bytes[b] : (uint8_t)'\n';
        bool read;
        if (fastq) {
            const int g = (int)((i + line_phase) & 3);
            read = g == 1;
            if ((g == 0 && first != (uint8_t)'@') || (g == 2 && first != (uint8_t)'+')) atomicAdd(&totals->n_bad, 1ull);
        } else {
            read = first != (uint8_t)'>';
        }
        int64_t len = 0;
        if (read) {
            while (b < e && is_strip_byte(bytes[b])) b++;
            while (e > b && is_strip_byte(bytes[e - 1])) e--;
            len = e - b;
            if (len > 0xFFFFFFFFll) { atomicOr(&totals->too_long, 1u); len = 0; }
        }
        is_read[i] = read ? 1u : 0u;
        read_len[i] = (uint32_t)len;
        letters_begin[i] = b;
    }
}

// One wave per line that is a read: read_start[its number] and its letters.  Thread 0 of the grid closes read_start.
__global__ __launch_bounds__(PARSE_BLOCK) void k_parse_emit(const uint8_t *__restrict__ bytes, int64_t n_lines,
                                                            const uint32_t *__restrict__ is_read,
                                                            const uint32_t *__restrict__ read_len,
                                                            const int64_t *__restrict__ letters_begin,
                                                            const int64_t *__restrict__ read_index,
                                                            const int64_t *__restrict__ letter_offset, int64_t n_reads,
                                                            int64_t n_letters, uint8_t *__restrict__ letters,
                                                            int64_t *__restrict__ read_start) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) read_start[n_reads] = n_letters;
    for (int64_t i = wave; i < n_lines; i += n_waves) {
        if (!is_read[i]) continue;
        const int64_t r = read_index[i], off = letter_offset[i], src = letters_begin[i];
        const int64_t len = read_len[i];
        if (r >= n_reads || off + len > n_letters) continue;   // totals of another run of the same buffer: write nothing
        if (lane == 0) read_start[r] = off;
        for (int64_t j = lane; j < len; j += 64) letters[off + j] = bytes[src + j];
    }
}

// What one parse of a buffer leaves on the device, and its totals.  Both entry points build it; neither keeps it.
struct ParsePlan {
    DevBuf line_end, is_read, read_len, letters_begin, read_index, letter_offset, tmp, totals;
    int64_t n_lines = 0, n_reads = 0, n_letters = 0, n_bad = 0;
};

int parse_lines(const uint8_t *bytes, int64_t n, int format, int line_phase, ParsePlan &p) {
    if (n < 0) return gki_set_error(GKI_ERR_BAD_ARG, "reads_parse: n_bytes must be >= 0");
    if (format != GKI_READS_FASTA && format != GKI_READS_FASTQ)
        return gki_set_error(GKI_ERR_BAD_ARG, "reads_parse: format must be GKI_READS_FASTA or GKI_READS_FASTQ");
    if (line_phase < 0 || line_phase > 3) return gki_set_error(GKI_ERR_BAD_ARG, "reads_parse: line_phase must be in 0..3");
    if (n == 0) return GKI_OK;
    if (bytes == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "reads_parse: d_bytes is NULL");
    int64_t n_lines = 0;
    GKI_TRY(gki_text_line_ends(bytes, n, "reads_parse", p.line_end, &n_lines));

    // lines -> reads
    const int64_t line_tmp_bytes = gki_scan_tmp_bytes(n_lines);
    HIP_TRY(p.tmp.alloc((size_t)line_tmp_bytes));
    HIP_TRY(p.is_read.alloc((size_t)n_lines * 4));
    HIP_TRY(p.read_len.alloc((size_t)n_lines * 4));
    HIP_TRY(p.letters_begin.alloc((size_t)n_lines * 8));
    HIP_TRY(p.read_index.alloc((size_t)(n_lines + 1) * 8));
    HIP_TRY(p.letter_offset.alloc((size_t)(n_lines + 1) * 8));
    HIP_TRY(p.totals.alloc(sizeof(ParseTotals)));
    HIP_TRY(hipMemsetAsync(p.totals.get(), 0, sizeof(ParseTotals), 0));
    hipLaunchKernelGGL(k_parse_classify, dim3(stream_grid(n_lines, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0, bytes,
                       p.line_end.get<const int64_t>(), n_lines, format == GKI_READS_FASTQ ? 1 : 0, line_phase,
                       p.is_read.get<uint32_t>(), p.read_len.get<uint32_t>(), p.letters_begin.get<int64_t>(),
                       p.totals.get<ParseTotals>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(gki_scan_u32_to_i64(p.is_read.get<const uint32_t>(), n_lines, p.read_index.get<int64_t>(), p.tmp.get(),
                                line_tmp_bytes, 0));
    GKI_TRY(gki_scan_u32_to_i64(p.read_len.get<const uint32_t>(), n_lines, p.letter_offset.get<int64_t>(), p.tmp.get(),
                                line_tmp_bytes, 0));
    ParseTotals totals;
    HIP_TRY(hipMemcpy(&p.n_reads, p.read_index.get<const int64_t>() + n_lines, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&p.n_letters, p.letter_offset.get<const int64_t>() + n_lines, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&totals, p.totals.get(), sizeof(ParseTotals), hipMemcpyDeviceToHost));
    if (totals.too_long) return gki_set_error(GKI_ERR_BAD_ARG, "reads_parse: a read of 2^32 letters or more");
    p.n_lines = n_lines;
    p.n_bad = (int64_t)totals.n_bad;
    return GKI_OK;
}

}  // namespace

extern "C" {

int gki_reads_parse_count(const void *d_bytes, int64_t n_bytes, int format, int line_phase, int64_t *n_lines,
                          int64_t *n_reads, int64_t *n_letters, int64_t *n_bad_lines) {
    if (n_lines) *n_lines = 0;
    if (n_reads) *n_reads = 0;
    if (n_letters) *n_letters = 0;
    if (n_bad_lines) *n_bad_lines = 0;
    ParsePlan p;
    GKI_TRY(parse_lines((const uint8_t *)d_bytes, n_bytes, format, line_phase, p));
    if (n_lines) *n_lines = p.n_lines;
    if (n_reads) *n_reads = p.n_reads;
    if (n_letters) *n_letters = p.n_letters;
    if (n_bad_lines) *n_bad_lines = p.n_bad;
    return GKI_OK;
}

int gki_reads_parse_emit(const void *d_bytes, int64_t n_bytes, int format, int line_phase, void *d_letters,
                         int64_t letters_capacity, void *d_read_start, int64_t read_start_capacity) {
    if (d_read_start == nullptr || read_start_capacity < 1)
        return gki_set_error(GKI_ERR_BAD_ARG, "reads_parse_emit: d_read_start needs at least one entry");
    ParsePlan p;
    GKI_TRY(parse_lines((const uint8_t *)d_bytes, n_bytes, format, line_phase, p));
    if (p.n_reads + 1 > read_start_capacity || p.n_letters > letters_capacity)
        return gki_set_error(GKI_ERR_BAD_ARG, "reads_parse_emit: %lld reads and %lld letters, capacity %lld and %lld",
                             (long long)p.n_reads, (long long)p.n_letters, (long long)read_start_capacity - 1,
                             (long long)letters_capacity);
    if (p.n_letters > 0 && d_letters == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "reads_parse_emit: d_letters is NULL");
    if (p.n_lines == 0) {                                  // an empty buffer: read_start = [0]
        HIP_TRY(hipMemset(d_read_start, 0, 8));
        return GKI_OK;
    }
    int64_t blocks = ceil_div(p.n_lines, PARSE_BLOCK / 64);
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(k_parse_emit, dim3((unsigned)blocks), dim3(PARSE_BLOCK), 0, 0, (const uint8_t *)d_bytes, p.n_lines,
                       p.is_read.get<const uint32_t>(), p.read_len.get<const uint32_t>(), p.letters_begin.get<const int64_t>(),
                       p.read_index.get<const int64_t>(), p.letter_offset.get<const int64_t>(), p.n_reads, p.n_letters,
                       (uint8_t *)d_letters, (int64_t *)d_read_start);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

}  // extern "C"
