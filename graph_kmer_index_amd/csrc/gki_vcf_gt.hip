// The haplotype matrix of VCF text in HBM: which allele every sample haplotype carries at every data line, as one byte a
// slot, and the same as two bit planes.  The rules are those of include/gki.h ("VCF haplotype matrix") and DESIGN.md 4.18.
//
// per piece of text (gki_vcf_haplotype_matrix), beside the unchanged gki_vcf_parse_* and gki_vcf_allele_frequencies:
//   (data lines)        gki_vcf_data_lines (gki_text_lines.hip): line ends, header / blank / data, line -> data lines
//                       before it; the host checks the count
//   k_gt_matrix         the walk of k_af_genotypes (gki_vcf_gt.h's gt_walk_line) with stores in place of counts: one wave
//                       per data line.  The lane that holds tab 9 + s parses sample s and stores its P codes at
//                       codes[v][s P ..]; a good line has exactly S samples, so its lanes write the whole row between
//                       them.  Whether the line is at fault is known after its last step: the wave then writes the row
//                       again, all 3 (a wave-uniform branch behind a wait for the stores above).  Lane 0 stores
//                       phased[v].  No atomics but that of the lowest line at fault.
// once, over the rows of all pieces (gki_haplotype_planes):
//   k_haplotype_planes  a workgroup takes a tile of 64 lines x PLANES_T slots: coalesced row reads, 16 bytes a lane, into
//                       LDS rows padded by one dword (an odd number of dwords, so the 64 lanes that then read one dword
//                       column, a lane a line, hit each bank twice at most -- once per half wave, which is free); four
//                       slots a dword, two __ballot each (== 0, == 1); the lane whose number is the slot's keeps the two
//                       words and stores them.  Lines at and beyond V and slots at and beyond H are 0xFF in LDS: no bit.
#include "gki_vcf_gt.h"

namespace {

constexpr int GT_MAX_PLOIDY = 8;                           // a sample's codes are the bytes of one uint64
constexpr uint64_t GT_ALL_MISSING = 0x0303030303030303ull;
constexpr int PLANES_LINES = 64;                           // a tile's lines: one word of each plane per slot
constexpr int PLANES_T = 256;                              // a tile's slots (vcf_files.PLANES_TILE_SLOTS)
constexpr int PLANES_ROW = PLANES_T + 4;                   // bytes of an LDS row: 65 dwords
constexpr int PLANES_BLOCK = 256;
constexpr uint32_t PLANES_NO_BIT = 0xFFFFFFFFu;

// what k_gt_matrix takes from a GT: the codes of its first eight alleles in text order, a byte each (0, 1, 2: any other
// number, 3: '.'), how many alleles it has and whether a '/' separates two of them
struct GtCodes {
    uint64_t codes = 0;
    int n = 0, slashes = 0;
    __device__ __forceinline__ void put(uint64_t code) {
        if (n < GT_MAX_PLOIDY) codes |= code << (8 * n);
        n++;
    }
    __device__ __forceinline__ void number(int value) { put(value == 0 ? 0u : value == 1 ? 1u : 2u); }
    __device__ __forceinline__ void missing() { put(3u); }
    __device__ __forceinline__ void slash() { slashes = 1; }
    // the slots the GT does not fill hold 3
    __device__ __forceinline__ uint64_t filled() const { return n < GT_MAX_PLOIDY ? codes | GT_ALL_MISSING << (8 * n) : codes; }
};

constexpr int BAD_FORMAT = 1, BAD_GT = 2, TOO_MANY = 4, SLASH = 8;   // what a lane saw in its line, as bits

// what a lane of k_gt_matrix does with its line's fields (gt_walk_line's visitor): sample s goes to row[s P ..], and what
// the lane saw is kept as bits
struct MatrixLine {
    const uint8_t *__restrict__ bytes;
    int64_t n_bytes, e, n_samples;
    int ploidy;
    uint8_t *__restrict__ row;
    int &seen;
    __device__ __forceinline__ void format(bool ok) { seen |= ok ? 0 : BAD_FORMAT; }
    __device__ __forceinline__ void sample(int64_t s, int64_t p) {
        GtCodes c;
        seen |= gt_at(bytes, n_bytes, p, e, &c) ? 0 : BAD_GT;
        seen |= (c.n > ploidy ? TOO_MANY : 0) | (c.slashes ? SLASH : 0);
        if (s < n_samples) {                               // a sample beyond S stores nothing: the line is at fault, kind 4
            const uint64_t filled = c.filled();
            uint8_t *__restrict__ at = row + s * ploidy;
            switch (ploidy) {                              // one store a sample where P is a power of two, at any alignment
            case 1: at[0] = (uint8_t)filled; break;
            case 2: { const uint16_t two = (uint16_t)filled; __builtin_memcpy(at, &two, 2); } break;
            case 4: { const uint32_t four = (uint32_t)filled; __builtin_memcpy(at, &four, 4); } break;
            case 8: __builtin_memcpy(at, &filled, 8); break;
            default:
                for (int a = 0; a < ploidy; a++) at[a] = (uint8_t)(filled >> (8 * a));
            }
        }
    }
};

// One wave per data line.  codes: uint8[n_variants][H], H = n_samples * ploidy; the row's offset is formed in 64 bits.
__global__ __launch_bounds__(PARSE_BLOCK) void k_gt_matrix(const uint8_t *__restrict__ bytes, int64_t n_bytes,
                                                           const int64_t *__restrict__ line_end, int64_t n_lines,
                                                           const uint32_t *__restrict__ is_data,
                                                           const int64_t *__restrict__ variant_index, int64_t n_variants,
                                                           int64_t n_samples, int ploidy, uint8_t *__restrict__ codes,
                                                           uint8_t *__restrict__ phased,
                                                           unsigned long long *__restrict__ first_bad) {
    const int lane = threadIdx.x & 63;
    const int64_t first = wave_uniform((int64_t)blockIdx.x * (PARSE_BLOCK / 64) + (threadIdx.x >> 6));
    const int64_t stride = (int64_t)gridDim.x * (PARSE_BLOCK / 64);
    const int64_t row_bytes = n_samples * (int64_t)ploidy;
    for (int64_t i = first; i < n_lines; i += stride) {
        if (!is_data[i]) continue;
        const int64_t v = variant_index[i];
        if (v >= n_variants) continue;
        const VcfLine l = vcf_line(bytes, line_end, i);
        const int64_t b = wave_uniform(l.b), e = wave_uniform(l.e);
        uint8_t *__restrict__ row = codes + v * row_bytes;
        int seen = 0;
        const int tabs_before = gt_walk_line(bytes, n_bytes, b, e, lane, MatrixLine{bytes, n_bytes, e, n_samples, ploidy, row, seen});
        // a line of fewer than 10 fields has no samples: at fault unless none is expected, and its FORMAT is not looked at
        seen = (__ballot(seen & BAD_FORMAT) ? BAD_FORMAT : 0) | (__ballot(seen & BAD_GT) ? BAD_GT : 0) |
               (__ballot(seen & TOO_MANY) ? TOO_MANY : 0) | (__ballot(seen & SLASH) ? SLASH : 0);
        const int64_t samples = tabs_before < 9 ? 0 : tabs_before - 8;
        const int kind = tabs_before < 9 ? (n_samples > 0 ? 4 : 0)
                         : (seen & BAD_FORMAT) ? 2 : (seen & BAD_GT) ? 3 : samples != n_samples ? 4 : (seen & TOO_MANY) ? 5 : 0;
        if (kind) {                                        // wave-uniform; the stores above have landed before the row is written again
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            for (int64_t h = lane; h < row_bytes; h += 64) row[h] = 3;
        }
        if (lane == 0) {
            if (kind) line_fault(first_bad, v, kind);
            phased[v] = kind == 0 && !(seen & SLASH) ? 1 : 0;
        }
    }
}

// codes uint8[n_variants][n_slots] -> ref_bits, alt_bits uint64[n_slots][n_words], n_words = ceil(n_variants / 64): bit
// v % 64 of word [h][v / 64] is set in ref_bits where codes[v][h] == 0, in alt_bits where it is 1.  A tile is 64 lines x
// PLANES_T slots; the tiles of one word column are consecutive, and a workgroup takes tiles grid-stride.  Offsets v * n_slots
// and h * n_words are formed in 64 bits.  No byte of a slot at or beyond n_slots is read, no word of one is written.
__global__ __launch_bounds__(PLANES_BLOCK) void k_haplotype_planes(const uint8_t *__restrict__ codes, int64_t n_variants,
                                                                   int64_t n_slots, int64_t n_words, int64_t slot_tiles,
                                                                   uint64_t *__restrict__ ref_bits, uint64_t *__restrict__ alt_bits) {
    __shared__ uint32_t tile[PLANES_LINES * PLANES_ROW / 4];
    constexpr int ROW_LANES = PLANES_T / PARSE_LANE_BYTES;              // 16 lanes read one row of the tile
    constexpr int ROWS_A_PASS = PLANES_BLOCK / ROW_LANES;               // 16 rows per pass of the workgroup
    constexpr int WAVE_DWORDS = PLANES_T / 4 / (PLANES_BLOCK / 64);     // 16 dword columns = 64 slots per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_tiles = n_words * slot_tiles;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t word = t / slot_tiles, h0 = (t - word * slot_tiles) * PLANES_T, v0 = word * PLANES_LINES;
        const int in_row = (threadIdx.x % ROW_LANES) * PARSE_LANE_BYTES;
#pragma unroll
        for (int pass = 0; pass < PLANES_LINES / ROWS_A_PASS; pass++) {
            const int r = pass * ROWS_A_PASS + threadIdx.x / ROW_LANES;
            const int64_t v = v0 + r, h = h0 + in_row;
            uint32_t w[4] = {PLANES_NO_BIT, PLANES_NO_BIT, PLANES_NO_BIT, PLANES_NO_BIT};
            if (v < n_variants && h < n_slots) {
                const uint8_t *__restrict__ from = codes + v * n_slots + h;
                if (h + PARSE_LANE_BYTES <= n_slots) {
                    Bytes16 raw;
                    __builtin_memcpy(&raw, from, PARSE_LANE_BYTES);
#pragma unroll
                    for (int k = 0; k < 4; k++) w[k] = raw.w[k];
                } else {                                   // the row's last slots: one by one
#pragma unroll
                    for (int j = 0; j < PARSE_LANE_BYTES; j++)
                        if (h + j < n_slots) w[j >> 2] = (w[j >> 2] & ~(0xFFu << (8 * (j & 3)))) | (uint32_t)from[j] << (8 * (j & 3));
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) tile[(r * PLANES_ROW + in_row) / 4 + k] = w[k];
        }
        __syncthreads();
        uint64_t ref_word = 0, alt_word = 0;               // of slot h0 + 64 wave + lane
#pragma unroll
        for (int c = 0; c < WAVE_DWORDS; c++) {
            const uint32_t four = tile[lane * (PLANES_ROW / 4) + wave * WAVE_DWORDS + c];   // line `lane`, four slots
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t code = (four >> (8 * k)) & 0xFFu;
                const uint64_t is_ref = __ballot(code == 0u), is_alt = __ballot(code == 1u);
                if (lane == 4 * c + k) { ref_word = is_ref; alt_word = is_alt; }
            }
        }
        const int64_t h = h0 + wave * 64 + lane;
        if (h < n_slots) {
            ref_bits[h * n_words + word] = ref_word;
            alt_bits[h * n_words + word] = alt_word;
        }
        __syncthreads();                                   // the tile is read before the next one is loaded
    }
}

}  // namespace

extern "C" int gki_vcf_haplotype_matrix(const void *d_text, int64_t n_bytes, int64_t n_variants, int64_t n_samples, int ploidy,
                                        void *d_codes, void *d_phased, int64_t *n_data_lines, int64_t *first_bad_variant,
                                        int *first_bad_kind, float *kernel_ms) {
    if (n_data_lines) *n_data_lines = 0;
    if (first_bad_variant) *first_bad_variant = -1;
    if (first_bad_kind) *first_bad_kind = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_bytes < 0 || n_variants < 0 || n_samples < 0)
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_haplotype_matrix: a negative size");
    if (ploidy < 1 || ploidy > GT_MAX_PLOIDY)
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_haplotype_matrix: ploidy %d is not in 1..%d", ploidy, GT_MAX_PLOIDY);
    if (n_samples > INT64_MAX / GT_MAX_PLOIDY / (n_variants > 0 ? n_variants : 1))
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_haplotype_matrix: the matrix is beyond 2^63 bytes");
    if (n_bytes > 0 && d_text == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "vcf_haplotype_matrix: the text is NULL");
    if (n_variants > 0 && (d_phased == nullptr || (n_samples > 0 && d_codes == nullptr)))
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_haplotype_matrix: an output buffer is NULL");
    const uint8_t *bytes = (const uint8_t *)d_text;
    TimerEvents ev;
    VcfDataLines d;
    DevBuf totals;
    if (n_bytes > 0) GKI_TRY(gki_vcf_data_lines(bytes, n_bytes, "vcf_haplotype_matrix", d));
    if (n_data_lines) *n_data_lines = d.n_data;
    GKI_TRY(gki_vcf_expect_data_lines("vcf_haplotype_matrix", d.n_data, n_variants));
    if (n_variants == 0) return GKI_OK;
    GKI_TRY(line_fault_init(totals));
    GKI_TRY(ev.start(0));
    hipLaunchKernelGGL(k_gt_matrix, dim3(stream_grid(d.n_lines, PARSE_BLOCK / 64)), dim3(PARSE_BLOCK), 0, 0, bytes, n_bytes,
                       d.line_end.get<const int64_t>(), d.n_lines, d.is_data.get<const uint32_t>(),
                       d.variant_index.get<const int64_t>(), n_variants, n_samples, ploidy, (uint8_t *)d_codes,
                       (uint8_t *)d_phased, totals.get<unsigned long long>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(ev.stop(0, kernel_ms));
    LineFault fault;
    GKI_TRY(line_fault_read(totals, &fault));
    if (first_bad_variant) *first_bad_variant = fault.line();
    if (first_bad_kind) *first_bad_kind = fault.kind();
    return GKI_OK;
}

extern "C" int gki_haplotype_planes(const void *d_codes, int64_t n_variants, int64_t n_slots, void *d_ref_bits,
                                    void *d_alt_bits, float *kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_variants < 0 || n_slots < 0) return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_planes: a negative size");
    if (n_slots > INT64_MAX / (n_variants > 0 ? n_variants : 1))
        return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_planes: the matrix is beyond 2^63 bytes");
    if (n_variants == 0 || n_slots == 0) return GKI_OK;    // no word to write
    if (d_codes == nullptr || d_ref_bits == nullptr || d_alt_bits == nullptr)
        return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_planes: a buffer is NULL");
    const int64_t n_words = ceil_div(n_variants, PLANES_LINES), slot_tiles = ceil_div(n_slots, PLANES_T);
    TimerEvents ev;
    GKI_TRY(ev.start(0));
    hipLaunchKernelGGL(k_haplotype_planes, dim3(stream_grid(n_words * slot_tiles, 1)), dim3(PLANES_BLOCK), 0, 0,
                       (const uint8_t *)d_codes, n_variants, n_slots, n_words, slot_tiles, (uint64_t *)d_ref_bits,
                       (uint64_t *)d_alt_bits);
    HIP_TRY(hipGetLastError());
    return ev.stop(0, kernel_ms);
}
