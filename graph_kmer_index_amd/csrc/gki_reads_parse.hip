// FASTA / FASTQ text parsed in HBM: the raw bytes of a reads file (or of a piece of one that ends at a line end) become
// the layout the read-side kernels take -- the letters of all reads back to back, uint8, and int64 read_start[n_reads + 1]
// (gki_hash_reads, gki_probe_reads_count_nodes).  The rules are those of include/gki.h ("reads files"); the FASTA one is
// the reference's (read_kmers.py:18-25: every line that does not start with '>' is one read, stripped).
//
//   (line ends)              gki_text_line_ends: the coalesced 16-byte pass of gki_text_lines.hip, the only whole-buffer work
//   k_parse_classify        one lane per line: header / read / FASTQ role by position, the record-shape check, the strip;
//                            writes whether the line is a read, where its letters begin and how many there are
//   (two exclusive scans)    line -> number of reads before it, line -> letters before it
//   k_parse_emit             one wave per line: read_start[read] and the letters, copied 64 bytes per step
//
// A line may be of any length: nothing here holds a line in a workgroup.  Lines of 2^32 letters or more after the strip
// are refused (GKI_ERR_BAD_ARG): a read's length passes through the 32-bit input of the scan.
#include "gki_text_lines.h"

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
        auto [b, e] = text_line(line_end, i);
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
        wave_copy(letters + off, bytes + src, len, lane);
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
    GKI_TRY(gki_scan_total(p.read_index, n_lines, &p.n_reads));
    GKI_TRY(gki_scan_total(p.letter_offset, n_lines, &p.n_letters));
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
