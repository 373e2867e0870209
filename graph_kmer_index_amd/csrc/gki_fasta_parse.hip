// Reference FASTA text parsed in HBM: the raw bytes of a FASTA file (or of a piece of one that ends at a line end) become
// the names of its records and the letters of the records the host wants, line ends removed.  The rules are those of
// include/gki.h ("FASTA files"), which are snp_kmer_finder.read_fasta_records' own, byte for byte.
//
//   k_fasta_count_tiles      dense: a workgroup counts, in its PARSE_TILE bytes, the headers ('>' at byte 0 or behind a
//                            '\n') and the plain bytes (neither '\n' nor '\r'); one 16-byte load per lane, SWAR compares
//   (two exclusive scans)    tile -> headers before it, tile -> plain bytes before it
//   k_fasta_header_positions dense, the same loads again: header h's byte position and the plain bytes before it
//   k_fasta_header_lines     one wave per header, 64 bytes a step: where its line ends, its name (the first word), the
//                            plain bytes of the header line; with the plain bytes before the next header that is the
//                            record's letter count in this buffer -- no pass over the body is needed for it
//   (exclusive scan)         header -> name bytes before it
//   k_fasta_names            one wave per header: the name's bytes
//   k_fasta_keep_tiles       dense: a lane's record is the number of headers before its bytes, so its 16-bit mask of bytes
//                            to keep needs the wanted flag and the body's first byte of that record only; per-tile count
//   (exclusive scan)         tile -> kept bytes before it
//   k_fasta_emit             dense: the kept bytes go through LDS at the alignment of their place in the output and leave
//                            as 16-byte stores
//
// A lane owns 16 input bytes in every dense pass, whatever the line length: a body of one 250 MB line and one wrapped at
// 60 letters are the same work.  Only a header line is walked by one wave.  Every offset and count is 64-bit; an output
// offset comes from a scan, never from an atomic.  A name of 2^32 bytes or more is refused (GKI_ERR_BAD_ARG): a name's
// length passes through the 32-bit input of the scan.
#include "gki_text_lines.h"

namespace {

constexpr int FASTA_STAGE_CHUNKS = PARSE_BLOCK + 1;       // 16-byte chunks of the emit kernel's LDS stage: a tile + the shift

// bytes [pos, pos + 16) of the buffer in *v, zero where there are none; returns the 16-bit mask of the bytes that exist
// (the line-end pass of gki_text_lines.hip needs a mask only and has a leaner loader of its own)
__device__ __forceinline__ uint32_t load_lane16(const uint8_t *__restrict__ bytes, int64_t pos, int64_t n, uint4 *v) {
    *v = make_uint4(0u, 0u, 0u, 0u);
    if (pos >= n) return 0u;
    if (pos + PARSE_LANE_BYTES <= n && (reinterpret_cast<uintptr_t>(bytes + pos) & 15) == 0) {
        *v = *reinterpret_cast<const uint4 *>(bytes + pos);
        return 0xFFFFu;
    }
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;              // the buffer's last bytes, or a buffer that is not 16-byte aligned
#pragma unroll
    for (int j = 0; j < PARSE_LANE_BYTES; j++) {
        const uint32_t c = pos + j < n ? (uint32_t)bytes[pos + j] << (8 * (j & 3)) : 0u;
        if (j < 4) w0 |= c; else if (j < 8) w1 |= c; else if (j < 12) w2 |= c; else w3 |= c;
    }
    *v = make_uint4(w0, w1, w2, w3);
    return pos + PARSE_LANE_BYTES <= n ? 0xFFFFu : (1u << (int)(n - pos)) - 1u;
}

// What a lane knows of its 16 bytes: which begin a header, which are plain (exist and are neither '\n' nor '\r')
struct FastaLane { uint4 v; uint32_t header, plain; };

__device__ __forceinline__ FastaLane fasta_lane(const uint8_t *__restrict__ bytes, int64_t pos, int64_t n) {
    FastaLane m;
    const uint32_t valid = load_lane16(bytes, pos, n, &m.v);
    const uint32_t nl = equal_mask16<10u>(m.v) & valid, cr = equal_mask16<13u>(m.v) & valid;
    const uint32_t gt = equal_mask16<62u>(m.v) & valid;
    uint32_t line_start = nl << 1;                        // the byte behind a '\n' begins a line
    if (valid && (pos == 0 || bytes[pos - 1] == (uint8_t)'\n')) line_start |= 1u;
    m.header = gt & line_start & 0xFFFFu;
    m.plain = valid & ~(nl | cr);
    return m;
}

// headers in the high half, plain bytes in the low half: a tile has at most 4096 of each, so one wave sum serves both
__device__ __forceinline__ int packed_counts(const FastaLane &m) { return __popc(m.header) << 16 | __popc(m.plain); }

__global__ __launch_bounds__(PARSE_BLOCK) void k_fasta_count_tiles(const uint8_t *__restrict__ bytes, int64_t n,
                                                                   uint32_t *__restrict__ tile_headers,
                                                                   uint32_t *__restrict__ tile_plain) {
    __shared__ int lds[PARSE_BLOCK / 64];
    const int64_t pos = (int64_t)blockIdx.x * PARSE_TILE + (int64_t)threadIdx.x * PARSE_LANE_BYTES;
    const FastaLane m = fasta_lane(bytes, pos, n);
    int total;
    block_excl_sum(packed_counts(m), lds, &total);         // every lane is active here
    if (threadIdx.x == 0) {
        tile_headers[blockIdx.x] = (uint32_t)total >> 16;
        tile_plain[blockIdx.x] = (uint32_t)total & 0xFFFFu;
    }
}

// header_pos[h] = the byte position of header h's '>', plain_before[h] = the plain bytes of the buffer before it
__global__ __launch_bounds__(PARSE_BLOCK) void k_fasta_header_positions(const uint8_t *__restrict__ bytes, int64_t n,
                                                                        const int64_t *__restrict__ tile_first_header,
                                                                        const int64_t *__restrict__ tile_plain_before,
                                                                        int64_t n_headers, int64_t *__restrict__ header_pos,
                                                                        int64_t *__restrict__ plain_before) {
    __shared__ int lds[PARSE_BLOCK / 64];
    const int64_t pos = (int64_t)blockIdx.x * PARSE_TILE + (int64_t)threadIdx.x * PARSE_LANE_BYTES;
    const FastaLane m = fasta_lane(bytes, pos, n);
    int total;
    const int excl = (int)block_excl_sum(packed_counts(m), lds, &total);   // no field borrows: each counts what lies before the lane
    int64_t h = tile_first_header[blockIdx.x] + (excl >> 16);
    const int64_t plain = tile_plain_before[blockIdx.x] + (excl & 0xFFFF);
    uint32_t hm = m.header;
    while (hm) {
        const int j = __ffs(hm) - 1;
        hm &= hm - 1u;
        if (h < n_headers) {
            header_pos[h] = pos + j;
            plain_before[h] = plain + __popc(m.plain & ((1u << j) - 1u));
        }
        h++;
    }
}

// bytes.split()'s separators
__device__ __forceinline__ bool is_split_byte(uint8_t c) { return c == 0x20 || (c >= 0x09 && c <= 0x0D); }

// One wave per header.  Its line is bytes [g, eol), eol its '\n' or n.  body_begin = min(eol + 1, n); the name is the first
// run of bytes that are no separators in (g, eol), empty when there is none; body_len = the plain bytes between this
// header and the next (or the buffer's end) less those of the header line itself.
__global__ __launch_bounds__(PARSE_BLOCK) void k_fasta_header_lines(const uint8_t *__restrict__ bytes, int64_t n,
                                                                    const int64_t *__restrict__ header_pos,
                                                                    const int64_t *__restrict__ plain_before,
                                                                    int64_t n_headers, int64_t n_plain,
                                                                    int64_t *__restrict__ body_begin,
                                                                    int64_t *__restrict__ name_begin,
                                                                    uint32_t *__restrict__ name_len,
                                                                    int64_t *__restrict__ body_len,
                                                                    uint32_t *__restrict__ too_long) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t h = wave; h < n_headers; h += n_waves) {
        const int64_t g = header_pos[h];
        int64_t name_b = -1, name_e = -1, eol = n, line_plain = 0;
        for (int64_t p = g; p < n; p += 64) {              // every value that steers the loop is the same in all lanes
            const int64_t q = p + lane;
            const bool valid = q < n;
            const uint8_t c = valid ? bytes[q] : (uint8_t)0;
            const unsigned long long nl = __ballot(valid && c == (uint8_t)'\n');
            const int at = nl ? __ffsll(nl) - 1 : 64;      // lanes below `at` are inside the line
            const unsigned long long inside = at == 64 ? ~0ull : (1ull << at) - 1ull;
            const unsigned long long through = at == 64 ? ~0ull : inside | 1ull << at;
            line_plain += __popcll(__ballot(valid && c != (uint8_t)'\n' && c != (uint8_t)'\r') & inside);
            const unsigned long long word = __ballot(valid && q > g && !is_split_byte(c)) & inside;
            if (name_b < 0 && word) name_b = p + (__ffsll(word) - 1);
            const unsigned long long gap = __ballot(valid && q > name_b && is_split_byte(c)) & through;
            if (name_b >= 0 && name_e < 0 && gap) name_e = p + (__ffsll(gap) - 1);
            if (nl) { eol = p + at; break; }
        }
        if (name_b < 0) name_b = name_e = eol;
        else if (name_e < 0) name_e = eol;
        if (lane == 0) {
            int64_t len = name_e - name_b;
            if (len > 0xFFFFFFFFll) { atomicOr(too_long, 1u); len = 0; }
            body_begin[h] = eol + 1 < n ? eol + 1 : n;
            name_begin[h] = name_b;
            name_len[h] = (uint32_t)len;
            body_len[h] = (h + 1 < n_headers ? plain_before[h + 1] : n_plain) - plain_before[h] - line_plain;
        }
    }
}

// One wave per header: name_start[h] and the name's bytes.  Thread 0 of the grid closes name_start.
__global__ __launch_bounds__(PARSE_BLOCK) void k_fasta_names(const uint8_t *__restrict__ bytes,
                                                             const int64_t *__restrict__ name_begin,
                                                             const uint32_t *__restrict__ name_len,
                                                             const int64_t *__restrict__ name_offset, int64_t n_headers,
                                                             int64_t n_name_bytes, int64_t *__restrict__ name_start,
                                                             uint8_t *__restrict__ names) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) name_start[n_headers] = n_name_bytes;
    for (int64_t h = wave; h < n_headers; h += n_waves) {
        const int64_t off = name_offset[h], src = name_begin[h], len = name_len[h];
        if (off + len > n_name_bytes) continue;
        if (lane == 0) name_start[h] = off;
        wave_copy(names + off, bytes + src, len, lane);
    }
}

// The 16-bit mask of the lane's bytes that go to the output.  `before` headers lie before the lane's first byte, so that
// byte belongs to record before - 1 (-1: the record carried in from the piece before); every header bit in the lane moves
// on to the next record.  A record's bytes are kept when it is wanted, from body_begin on, where they are plain.
__device__ __forceinline__ uint32_t fasta_keep_mask(const FastaLane &m, int64_t pos, int64_t before, int64_t n_headers,
                                                    const uint8_t *__restrict__ wanted, int carry_wanted,
                                                    const int64_t *__restrict__ body_begin) {
    int64_t cur = before - 1;
    uint32_t keep = 0, hm = m.header;
    int lo = 0;
    for (;;) {
        const int j = hm ? __ffs(hm) - 1 : PARSE_LANE_BYTES;
        if (j > lo && (cur < 0 ? carry_wanted != 0 : (cur < n_headers && wanted[cur] != 0))) {
            const int64_t bb = cur < 0 ? 0 : body_begin[cur];
            const int from = bb <= pos + lo ? lo : bb >= pos + j ? j : (int)(bb - pos);
            keep |= ((1u << j) - 1u) & ~((1u << from) - 1u);
        }
        if (j == PARSE_LANE_BYTES) break;
        cur++;
        lo = j;
        hm &= hm - 1u;
    }
    return keep & m.plain;
}

// The two passes over the kept bytes: the lane's 16 bytes and their keep mask, *at = the tile's kept bytes before the lane's,
// *total = the tile's kept bytes.  Every lane of the workgroup calls it, once.
__device__ __forceinline__ uint32_t fasta_lane_keep(const uint8_t *__restrict__ bytes, int64_t n, int64_t pos,
                                                    const int64_t *__restrict__ tile_first_header, int64_t n_headers,
                                                    const uint8_t *__restrict__ wanted, int carry_wanted,
                                                    const int64_t *__restrict__ body_begin, FastaLane *m, int *at,
                                                    int *total) {
    __shared__ int lds[2][PARSE_BLOCK / 64];
    *m = fasta_lane(bytes, pos, n);
    int htotal;
    const int64_t before = tile_first_header[blockIdx.x] + block_excl_sum(__popc(m->header), lds[0], &htotal);
    const uint32_t keep = fasta_keep_mask(*m, pos, before, n_headers, wanted, carry_wanted, body_begin);
    *at = (int)block_excl_sum(__popc(keep), lds[1], total);
    return keep;
}

__global__ __launch_bounds__(PARSE_BLOCK) void k_fasta_keep_tiles(const uint8_t *__restrict__ bytes, int64_t n,
                                                                  const int64_t *__restrict__ tile_first_header,
                                                                  int64_t n_headers, const uint8_t *__restrict__ wanted,
                                                                  int carry_wanted, const int64_t *__restrict__ body_begin,
                                                                  uint32_t *__restrict__ tile_kept) {
    const int64_t pos = (int64_t)blockIdx.x * PARSE_TILE + (int64_t)threadIdx.x * PARSE_LANE_BYTES;
    FastaLane m;
    int at, total;
    fasta_lane_keep(bytes, n, pos, tile_first_header, n_headers, wanted, carry_wanted, body_begin, &m, &at, &total);
    if (threadIdx.x == 0) tile_kept[blockIdx.x] = (uint32_t)total;
}

// The tile's kept bytes, in order, to letters[tile_out[tile], ..).  They are staged in LDS shifted by the low four bits of
// their destination, so that a 16-byte chunk of the stage is a 16-byte aligned chunk of the output: whole chunks leave as
// one store per lane, the two ragged ends byte by byte.
__global__ __launch_bounds__(PARSE_BLOCK) void k_fasta_emit(const uint8_t *__restrict__ bytes, int64_t n,
                                                            const int64_t *__restrict__ tile_first_header,
                                                            int64_t n_headers, const uint8_t *__restrict__ wanted,
                                                            int carry_wanted, const int64_t *__restrict__ body_begin,
                                                            const int64_t *__restrict__ tile_out, int64_t n_kept,
                                                            uint8_t *__restrict__ letters) {
    __shared__ uint4 stage4[FASTA_STAGE_CHUNKS];
    uint8_t *stage = reinterpret_cast<uint8_t *>(stage4);
    const int64_t pos = (int64_t)blockIdx.x * PARSE_TILE + (int64_t)threadIdx.x * PARSE_LANE_BYTES;
    FastaLane m;
    int at, total;
    const uint32_t keep = fasta_lane_keep(bytes, n, pos, tile_first_header, n_headers, wanted, carry_wanted, body_begin, &m,
                                          &at, &total);
    const int64_t out = tile_out[blockIdx.x];
    if (total == 0 || out + total > n_kept) return;        // the same in every lane; totals of another run: write nothing
    const int shift = (int)((reinterpret_cast<uintptr_t>(letters) + (uint64_t)out) & 15);
    at += shift;
    const uint32_t w[4] = {m.v.x, m.v.y, m.v.z, m.v.w};
#pragma unroll
    for (int j = 0; j < PARSE_LANE_BYTES; j++)
        if (keep >> j & 1u) stage[at++] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    __syncthreads();
    uint8_t *const base = letters + out - shift;           // 16-byte aligned; stage[i] goes to base[i], shift <= i < end
    const int end = shift + total;
    for (int c = threadIdx.x; c * PARSE_LANE_BYTES < end; c += PARSE_BLOCK) {
        const int lo = c * PARSE_LANE_BYTES, hi = lo + PARSE_LANE_BYTES;
        if (lo >= shift && hi <= end) {
            *reinterpret_cast<uint4 *>(base + lo) = stage4[c];
        } else {
            for (int i = lo < shift ? shift : lo; i < (hi < end ? hi : end); i++) base[i] = stage[i];
        }
    }
}

// What the header passes leave on the device for one buffer, and its totals.  Every entry point builds it; none keeps it.
struct FastaPlan {
    DevBuf tile_headers, tile_plain, tile_first_header, tile_plain_before, tmp, header_pos, plain_before, body_begin,
        name_begin, name_len, body_len, name_offset, too_long;
    int64_t n_tiles = 0, n_headers = 0, n_plain = 0, n_name_bytes = 0, n_lead = 0;
};

// the clock of one entry point's device work: from its first kernel to its last
struct FastaClock {
    TimerEvents ev;
    float *ms;
    explicit FastaClock(float *kernel_ms) : ms(kernel_ms) { if (ms) *ms = 0.0f; }
    int start() {
        if (!ms) return GKI_OK;
        HIP_TRY(hipEventCreate(&ev.e0));
        HIP_TRY(hipEventCreate(&ev.e1));
        HIP_TRY(hipEventRecord(ev.e0, 0));
        return GKI_OK;
    }
    int stop() {
        if (!ms || !ev.e0) return GKI_OK;
        HIP_TRY(hipEventRecord(ev.e1, 0));
        HIP_TRY(hipEventSynchronize(ev.e1));
        HIP_TRY(hipEventElapsedTime(ms, ev.e0, ev.e1));
        return GKI_OK;
    }
};

int fasta_plan(const uint8_t *bytes, int64_t n, FastaPlan &p, FastaClock &clock) {
    if (n < 0) return gki_set_error(GKI_ERR_BAD_ARG, "fasta_parse: n_bytes must be >= 0");
    if (n == 0) return GKI_OK;
    if (bytes == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "fasta_parse: d_bytes is NULL");
    const int64_t n_tiles = ceil_div(n, PARSE_TILE);
    if (n_tiles > 0x7FFFFFFFll) return gki_set_error(GKI_ERR_BAD_ARG, "fasta_parse: buffer of %lld bytes is too large", (long long)n);
    p.n_tiles = n_tiles;
    const int64_t tile_tmp_bytes = gki_scan_tmp_bytes(n_tiles);
    HIP_TRY(p.tile_headers.alloc((size_t)n_tiles * 4));
    HIP_TRY(p.tile_plain.alloc((size_t)n_tiles * 4));
    HIP_TRY(p.tile_first_header.alloc((size_t)(n_tiles + 1) * 8));
    HIP_TRY(p.tile_plain_before.alloc((size_t)(n_tiles + 1) * 8));
    HIP_TRY(p.tmp.alloc((size_t)tile_tmp_bytes));
    GKI_TRY(clock.start());
    hipLaunchKernelGGL(k_fasta_count_tiles, dim3((unsigned)n_tiles), dim3(PARSE_BLOCK), 0, 0, bytes, n,
                       p.tile_headers.get<uint32_t>(), p.tile_plain.get<uint32_t>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(gki_scan_u32_to_i64(p.tile_headers.get<const uint32_t>(), n_tiles, p.tile_first_header.get<int64_t>(),
                                p.tmp.get(), tile_tmp_bytes, 0));
    GKI_TRY(gki_scan_u32_to_i64(p.tile_plain.get<const uint32_t>(), n_tiles, p.tile_plain_before.get<int64_t>(),
                                p.tmp.get(), tile_tmp_bytes, 0));
    GKI_TRY(gki_scan_total(p.tile_first_header, n_tiles, &p.n_headers));
    GKI_TRY(gki_scan_total(p.tile_plain_before, n_tiles, &p.n_plain));
    p.tile_headers.reset();
    p.tile_plain.reset();
    p.n_lead = p.n_plain;
    if (p.n_headers == 0) return GKI_OK;

    const int64_t nh = p.n_headers, header_tmp_bytes = gki_scan_tmp_bytes(nh);
    HIP_TRY(p.header_pos.alloc((size_t)nh * 8));
    HIP_TRY(p.plain_before.alloc((size_t)nh * 8));
    HIP_TRY(p.body_begin.alloc((size_t)nh * 8));
    HIP_TRY(p.name_begin.alloc((size_t)nh * 8));
    HIP_TRY(p.name_len.alloc((size_t)nh * 4));
    HIP_TRY(p.body_len.alloc((size_t)nh * 8));
    HIP_TRY(p.name_offset.alloc((size_t)(nh + 1) * 8));
    HIP_TRY(p.too_long.alloc(4));
    HIP_TRY(p.tmp.alloc((size_t)header_tmp_bytes));
    HIP_TRY(hipMemsetAsync(p.too_long.get(), 0, 4, 0));
    hipLaunchKernelGGL(k_fasta_header_positions, dim3((unsigned)n_tiles), dim3(PARSE_BLOCK), 0, 0, bytes, n,
                       p.tile_first_header.get<const int64_t>(), p.tile_plain_before.get<const int64_t>(), nh,
                       p.header_pos.get<int64_t>(), p.plain_before.get<int64_t>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_fasta_header_lines, dim3(stream_grid(nh * 64, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0, bytes, n,
                       p.header_pos.get<const int64_t>(), p.plain_before.get<const int64_t>(), nh, p.n_plain,
                       p.body_begin.get<int64_t>(), p.name_begin.get<int64_t>(), p.name_len.get<uint32_t>(),
                       p.body_len.get<int64_t>(), p.too_long.get<uint32_t>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(gki_scan_u32_to_i64(p.name_len.get<const uint32_t>(), nh, p.name_offset.get<int64_t>(), p.tmp.get(),
                                header_tmp_bytes, 0));
    uint32_t too_long = 0;
    GKI_TRY(gki_scan_total(p.name_offset, nh, &p.n_name_bytes));
    HIP_TRY(hipMemcpy(&p.n_lead, p.plain_before.get<const int64_t>(), 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&too_long, p.too_long.get(), 4, hipMemcpyDeviceToHost));
    p.tile_plain_before.reset();
    p.header_pos.reset();
    p.plain_before.reset();
    if (too_long) return gki_set_error(GKI_ERR_BAD_ARG, "fasta_parse: a record name of 2^32 bytes or more");
    return GKI_OK;
}

}  // namespace

extern "C" {

int gki_fasta_parse_count(const void *d_bytes, int64_t n_bytes, int64_t *n_headers, int64_t *n_name_bytes,
                          int64_t *n_lead_letters, float *kernel_ms) {
    if (n_headers) *n_headers = 0;
    if (n_name_bytes) *n_name_bytes = 0;
    if (n_lead_letters) *n_lead_letters = 0;
    FastaClock clock(kernel_ms);
    FastaPlan p;
    GKI_TRY(fasta_plan((const uint8_t *)d_bytes, n_bytes, p, clock));
    GKI_TRY(clock.stop());
    if (n_headers) *n_headers = p.n_headers;
    if (n_name_bytes) *n_name_bytes = p.n_name_bytes;
    if (n_lead_letters) *n_lead_letters = p.n_lead;
    return GKI_OK;
}

int gki_fasta_parse_names(const void *d_bytes, int64_t n_bytes, void *d_name_start, void *d_body_letters,
                          int64_t header_capacity, void *d_names, int64_t name_capacity, float *kernel_ms) {
    if (d_name_start == nullptr || header_capacity < 0)
        return gki_set_error(GKI_ERR_BAD_ARG, "fasta_parse_names: d_name_start needs at least one entry");
    FastaClock clock(kernel_ms);
    FastaPlan p;
    GKI_TRY(fasta_plan((const uint8_t *)d_bytes, n_bytes, p, clock));
    if (p.n_headers > header_capacity || p.n_name_bytes > name_capacity)
        return gki_set_error(GKI_ERR_BAD_ARG, "fasta_parse_names: %lld headers and %lld name bytes, capacity %lld and %lld",
                             (long long)p.n_headers, (long long)p.n_name_bytes, (long long)header_capacity,
                             (long long)name_capacity);
    if (p.n_headers == 0) {                                // no header: name_start = [0]
        HIP_TRY(hipMemset(d_name_start, 0, 8));
        return clock.stop();
    }
    if (d_body_letters == nullptr || (p.n_name_bytes > 0 && d_names == nullptr))
        return gki_set_error(GKI_ERR_BAD_ARG, "fasta_parse_names: an output buffer is NULL");
    hipLaunchKernelGGL(k_fasta_names, dim3(stream_grid(p.n_headers * 64, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0,
                       (const uint8_t *)d_bytes, p.name_begin.get<const int64_t>(), p.name_len.get<const uint32_t>(),
                       p.name_offset.get<const int64_t>(), p.n_headers, p.n_name_bytes, (int64_t *)d_name_start,
                       (uint8_t *)d_names);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(d_body_letters, p.body_len.get(), (size_t)p.n_headers * 8, hipMemcpyDeviceToDevice, 0));
    GKI_TRY(clock.stop());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

int gki_fasta_parse_emit(const void *d_bytes, int64_t n_bytes, int carry_wanted, const void *d_wanted, int64_t n_wanted,
                         void *d_letters, int64_t letters_capacity, int64_t *n_letters, float *kernel_ms) {
    if (n_letters) *n_letters = 0;
    if (n_wanted < 0 || letters_capacity < 0)
        return gki_set_error(GKI_ERR_BAD_ARG, "fasta_parse_emit: n_wanted and letters_capacity must be >= 0");
    FastaClock clock(kernel_ms);
    FastaPlan p;
    GKI_TRY(fasta_plan((const uint8_t *)d_bytes, n_bytes, p, clock));
    if (p.n_headers != n_wanted)
        return gki_set_error(GKI_ERR_BAD_ARG, "fasta_parse_emit: %lld wanted flags for %lld headers", (long long)n_wanted,
                             (long long)p.n_headers);
    if (p.n_headers > 0 && d_wanted == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "fasta_parse_emit: d_wanted is NULL");
    if (p.n_tiles == 0) return clock.stop();
    DevBuf tile_kept, tile_out;
    const int64_t tile_tmp_bytes = gki_scan_tmp_bytes(p.n_tiles);
    HIP_TRY(tile_kept.alloc((size_t)p.n_tiles * 4));
    HIP_TRY(tile_out.alloc((size_t)(p.n_tiles + 1) * 8));
    HIP_TRY(p.tmp.alloc((size_t)tile_tmp_bytes));
    hipLaunchKernelGGL(k_fasta_keep_tiles, dim3((unsigned)p.n_tiles), dim3(PARSE_BLOCK), 0, 0, (const uint8_t *)d_bytes,
                       n_bytes, p.tile_first_header.get<const int64_t>(), p.n_headers, (const uint8_t *)d_wanted,
                       carry_wanted, p.body_begin.get<const int64_t>(), tile_kept.get<uint32_t>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(gki_scan_u32_to_i64(tile_kept.get<const uint32_t>(), p.n_tiles, tile_out.get<int64_t>(), p.tmp.get(),
                                tile_tmp_bytes, 0));
    int64_t n_kept = 0;
    GKI_TRY(gki_scan_total(tile_out, p.n_tiles, &n_kept));
    if (n_kept > letters_capacity)
        return gki_set_error(GKI_ERR_BAD_ARG, "fasta_parse_emit: %lld letters, capacity %lld", (long long)n_kept,
                             (long long)letters_capacity);
    if (n_kept > 0 && d_letters == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "fasta_parse_emit: d_letters is NULL");
    if (n_kept > 0) {
        hipLaunchKernelGGL(k_fasta_emit, dim3((unsigned)p.n_tiles), dim3(PARSE_BLOCK), 0, 0, (const uint8_t *)d_bytes,
                           n_bytes, p.tile_first_header.get<const int64_t>(), p.n_headers, (const uint8_t *)d_wanted,
                           carry_wanted, p.body_begin.get<const int64_t>(), tile_out.get<const int64_t>(), n_kept,
                           (uint8_t *)d_letters);
        HIP_TRY(hipGetLastError());
    }
    GKI_TRY(clock.stop());
    HIP_TRY(hipStreamSynchronize(0));
    if (n_letters) *n_letters = n_kept;
    return GKI_OK;
}

}  // extern "C"
