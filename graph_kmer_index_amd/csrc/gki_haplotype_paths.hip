// Sample haplotypes through a bubble-chain graph: a slot's sequence and the alt nodes of every slot.  The rules are those
// of include/gki.h ("haplotype paths") and DESIGN.md 4.19.
//
// In a bubble chain node ids ascend along every path and a kept line's two allele nodes lie side by side in `seq`, so a
// haplotype's sequence is `seq` with one allele node per kept line cut out.  With the kept lines numbered j = 0 .. K - 1:
//   k_hap_drops        one lane per kept line: the slot's alt bit -> the allele not taken: drop_len[j], drop_start[j]
//   (exclusive scan)   before[j] = letters dropped in front of kept line j, K + 1 entries
//   k_hap_cuts         cut[j] = drop_start[j] - before[j], the output position at which drop j is skipped (non-decreasing);
//                      and the chromosome bounds of the output
//   k_hap_tile_sites   one lane per tile boundary: the first j with cut[j] > t * HAP_TILE
//   k_hap_spell        output-dense: a workgroup owns 4096 consecutive output letters, a lane 16 of them.
//                      out[p] = "ACGT"[seq[p + before[J(p)]]], J(p) = the number of j with cut[j] <= p; when no cut falls
//                      among the lane's 16 bytes they come from 16 consecutive codes of seq (one unaligned 16-byte load,
//                      one aligned 16-byte store), else piece by piece with all loads in flight.
// The alt nodes of all slots at once:
//   k_hap_alt_count    per (slot, tile of 1024 plane words): the set bits of alt_bits & kept_bits
//   (exclusive scan)   tile_before; k_hap_alt_starts picks start[h] = tile_before[h * T] out of it
//   k_hap_alt_emit     per (slot, tile): var_nodes[64 w + b] for every set bit, behind a block prefix of the lanes' counts
#include "gki_haplotype_plan.h"
#include "gki_seq_gather.h"
#include "gki_text_lines.h"

namespace {

constexpr int HAP_TILE = PARSE_BLOCK * 16;                 // 4096 output letters per workgroup
constexpr int HAP_LANE_WORDS = 4;                          // plane words per lane in the alt-node kernels
constexpr int HAP_WORD_TILE = PARSE_BLOCK * HAP_LANE_WORDS; // 1024 plane words per workgroup

// the allele kept line j does not take: the ref allele when the slot's alt bit of its line is set, else the alt allele; a
// NULL bit row has no bit set (the same for every lane)
__global__ __launch_bounds__(PARSE_BLOCK) void k_hap_drops(int64_t K, const int64_t *__restrict__ kline,
                                                           const int64_t *__restrict__ ref_start,
                                                           const int32_t *__restrict__ ref_size,
                                                           const int64_t *__restrict__ alt_start,
                                                           const int32_t *__restrict__ alt_size,
                                                           const uint64_t *__restrict__ slot_bits,
                                                           int32_t *__restrict__ drop_len, int64_t *__restrict__ drop_start) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < K; j += stride) {
        const bool alt = slot_bits != nullptr && hap_alt_bit(slot_bits, kline[j]);
        drop_len[j] = alt ? ref_size[j] : alt_size[j];
        drop_start[j] = alt ? ref_start[j] : alt_start[j];
    }
}

// i < K: cut[i]; i = K + c, c = 0 .. n_chrom: bounds[c] = where chromosome c begins in the output, bounds[n_chrom] = n_out
// (chrom_seq_start[n_chrom] = n_bases, chrom_first_kept[n_chrom] = K)
__global__ __launch_bounds__(PARSE_BLOCK) void k_hap_cuts(int64_t K, const int64_t *__restrict__ drop_start,
                                                          const int64_t *__restrict__ before, int64_t *__restrict__ cut,
                                                          const int64_t *__restrict__ chrom_seq_start,
                                                          const int64_t *__restrict__ chrom_first_kept, int n_chrom,
                                                          int64_t *__restrict__ bounds) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < K + n_chrom + 1; i += stride) {
        if (i < K) cut[i] = drop_start[i] - before[i];
        else bounds[i - K] = chrom_seq_start[i - K] - before[chrom_first_kept[i - K]];
    }
}

// tile_site[t] = the first kept line whose cut lies behind output byte t * HAP_TILE (K when there is none), t = 0 .. n_tiles
__global__ __launch_bounds__(PARSE_BLOCK) void k_hap_tile_sites(const int64_t *__restrict__ cut, int64_t K, int64_t n_tiles,
                                                                int64_t *__restrict__ tile_site) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t <= n_tiles; t += stride)
        tile_site[t] = first_site_after(cut, 0, K, t * HAP_TILE);
}

// four codes 0..3, a byte each -> four of "ACGT": 'A' + 2 b0 + 6 b1 + 11 b0 b1 per byte, no carry leaves a byte
__device__ __forceinline__ uint32_t letters4(uint32_t w) {
    const uint32_t b0 = w & 0x01010101u, b1 = (w >> 1) & 0x01010101u;
    return 0x41414141u + 2u * b0 + 6u * b1 + 11u * (b0 & b1);
}

__global__ __launch_bounds__(PARSE_BLOCK) void k_hap_spell(const uint8_t *__restrict__ seq, int64_t K,
                                                           const int64_t *__restrict__ cut,
                                                           const int64_t *__restrict__ before,
                                                           const int64_t *__restrict__ tile_site, int64_t n_out,
                                                           uint8_t *__restrict__ out) {
    const int64_t n_tiles = (n_out + HAP_TILE - 1) / HAP_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t j_lo = tile_site[tile], j_hi = tile_site[tile + 1];         // the same for every lane
        const int64_t p0 = tile * HAP_TILE + (int64_t)threadIdx.x * 16;
        if (p0 >= n_out) continue;
        int64_t j = first_site_after(cut, j_lo, j_hi, p0);                        // cut[j] > p0, or j == K
        const int64_t next_cut = j < K ? cut[j] : n_out;
        if (p0 + 16 <= n_out && p0 + 16 <= next_cut) {     // 16 codes in a row, at any alignment; the store is aligned
            Letters16 in;
            __builtin_memcpy(&in, seq + (p0 + before[j]), 16);
            uint4 o;
            o.x = letters4(in.w[0]);
            o.y = letters4(in.w[1]);
            o.z = letters4(in.w[2]);
            o.w = letters4(in.w[3]);
            *reinterpret_cast<uint4 *>(out + p0) = o;
            continue;
        }
        // a cut among the 16, or the end of the output: piece by piece -- the letters up to the next cut share one shift --
        // so that a piece's byte loads do not wait for one another
        uint64_t low = 0, high = 0;
        const int count = n_out - p0 < 16 ? (int)(n_out - p0) : 16;
        const int64_t p_end = p0 + count;
        int64_t p = p0;
        while (p < p_end) {
            while (j < K && cut[j] <= p) j++;              // zero-length drops and drops that touch are skipped together
            const int64_t shift = before[j];
            const int64_t stop = j < K && cut[j] < p_end ? cut[j] : p_end;
            // all 16 loads are issued whatever the piece covers (a byte outside it reads seq[0])
            uint32_t code[16];                             // indexed by unrolled loops only: registers
#pragma unroll
            for (int b = 0; b < 16; b++) {
                const int64_t q = p0 + b;
                code[b] = seq[q >= p && q < stop ? q + shift : 0];
            }
#pragma unroll
            for (int b = 0; b < 16; b++) {
                const int64_t q = p0 + b;
                const uint64_t c = q >= p && q < stop ? (uint64_t)(code[b] & 3u) : 0ull;
                if (b < 8) low |= c << (8 * b); else high |= c << (8 * (b - 8));
            }
            p = stop;
        }
        uint4 o;
        o.x = letters4((uint32_t)low); o.y = letters4((uint32_t)(low >> 32));
        o.z = letters4((uint32_t)high); o.w = letters4((uint32_t)(high >> 32));
        if (count == 16)
            *reinterpret_cast<uint4 *>(out + p0) = o;
        else {
            const uint32_t w[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
            for (int b = 0; b < 15; b++)
                if (b < count) out[p0 + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
        }
    }
}

// ------------------------------------------------------------------------------------------------ alt nodes of all slots

// the lane's words of tile t of slot h, masked: alt_bits & kept_bits (the planes' tail bits are never relied on); 0 past W
__device__ __forceinline__ void hap_lane_masks(const uint64_t *__restrict__ alt_bits, const uint64_t *__restrict__ kept_bits,
                                               int64_t W, int64_t h, int64_t t, uint64_t m[HAP_LANE_WORDS], int64_t *w0) {
    *w0 = t * HAP_WORD_TILE + (int64_t)threadIdx.x * HAP_LANE_WORDS;
#pragma unroll
    for (int i = 0; i < HAP_LANE_WORDS; i++) {
        const int64_t w = *w0 + i;
        m[i] = w < W ? alt_bits[h * W + w] & kept_bits[w] : 0ull;
    }
}

__global__ __launch_bounds__(PARSE_BLOCK) void k_hap_alt_count(const uint64_t *__restrict__ alt_bits,
                                                               const uint64_t *__restrict__ kept_bits, int64_t W, int64_t T,
                                                               int64_t n_slots, uint32_t *__restrict__ tile_cnt) {
    __shared__ int lds[PARSE_BLOCK / 64];
    for (int64_t b = blockIdx.x; b < n_slots * T; b += gridDim.x) {
        uint64_t m[HAP_LANE_WORDS];
        int64_t w0;
        hap_lane_masks(alt_bits, kept_bits, W, b / T, b % T, m, &w0);
        int cnt = 0, total = 0;
#pragma unroll
        for (int i = 0; i < HAP_LANE_WORDS; i++) cnt += __popcll(m[i]);
        (void)block_excl_sum(cnt, lds, &total);
        if (threadIdx.x == 0) tile_cnt[b] = (uint32_t)total;
        __syncthreads();                                   // lds serves the next tile
    }
}

__global__ __launch_bounds__(PARSE_BLOCK) void k_hap_alt_starts(const int64_t *__restrict__ tile_before, int64_t T,
                                                                int64_t n_slots, int64_t *__restrict__ start) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; h <= n_slots; h += stride) start[h] = tile_before[h * T];
}

__global__ __launch_bounds__(PARSE_BLOCK) void k_hap_alt_emit(const uint64_t *__restrict__ alt_bits,
                                                              const uint64_t *__restrict__ kept_bits, int64_t W, int64_t T,
                                                              int64_t n_slots, const int64_t *__restrict__ tile_before,
                                                              const uint32_t *__restrict__ var_nodes,
                                                              uint32_t *__restrict__ nodes) {
    __shared__ int lds[PARSE_BLOCK / 64];
    for (int64_t b = blockIdx.x; b < n_slots * T; b += gridDim.x) {
        uint64_t m[HAP_LANE_WORDS];
        int64_t w0;
        hap_lane_masks(alt_bits, kept_bits, W, b / T, b % T, m, &w0);
        int cnt = 0, total = 0;
#pragma unroll
        for (int i = 0; i < HAP_LANE_WORDS; i++) cnt += __popcll(m[i]);
        int64_t o = tile_before[b] + block_excl_sum(cnt, lds, &total);
#pragma unroll
        for (int i = 0; i < HAP_LANE_WORDS; i++)
            for (uint64_t rest = m[i]; rest; rest &= rest - 1)             // a set bit is a kept line: below n_lines
                nodes[o++] = var_nodes[(w0 + i) * 64 + (__ffsll((unsigned long long)rest) - 1)];
        __syncthreads();                                   // lds serves the next tile
    }
}

int upload(DevBuf &dst, const void *h_src, size_t bytes) {
    HIP_TRY(dst.alloc(bytes ? bytes : 8));
    if (bytes) HIP_TRY(hipMemcpy(dst.get(), h_src, bytes, hipMemcpyHostToDevice));
    return GKI_OK;
}

}  // namespace

int gki_haplotype_build_path(gki_haplotype_paths &g, const uint64_t *slot_bits, HapPath &path) {
    const int64_t K = g.K;
    path.of = HapKey();
    if (K > 0) {
        hipLaunchKernelGGL(k_hap_drops, dim3(stream_grid(K, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0, K,
                           g.kline.get<const int64_t>(), g.ref_start.get<const int64_t>(), g.ref_size.get<const int32_t>(),
                           g.alt_start.get<const int64_t>(), g.alt_size.get<const int32_t>(), slot_bits,
                           g.drop_len.get<int32_t>(), g.drop_start.get<int64_t>());
        HIP_TRY(hipGetLastError());
        GKI_TRY(gki_scan_i32_to_i64(g.drop_len.get<const int32_t>(), K, path.before.get<int64_t>(), g.scan_tmp.get(),
                                    g.scan_tmp_bytes, 0));
    } else
        HIP_TRY(hipMemsetAsync(path.before.get(), 0, 8, 0));              // no kept line: before = [0], no scan runs
    hipLaunchKernelGGL(k_hap_cuts, dim3(stream_grid(K + g.n_chrom + 1, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0, K,
                       g.drop_start.get<const int64_t>(), path.before.get<const int64_t>(), path.cut.get<int64_t>(),
                       g.chrom_seq_start.get<const int64_t>(), g.chrom_first_kept.get<const int64_t>(), g.n_chrom,
                       path.bounds.get<int64_t>());
    HIP_TRY(hipGetLastError());
    return GKI_OK;
}

extern "C" {

int gki_haplotype_paths_destroy(gki_haplotype_paths *plan) {
    delete plan;
    return GKI_OK;
}

int gki_haplotype_paths_create(const uint8_t *h_seq, int64_t n_bases, int64_t n_lines, const uint32_t *h_var_nodes,
                               const uint64_t *h_kept_bits, int64_t n_kept, const int64_t *h_kept_line,
                               const int64_t *h_ref_start, const int32_t *h_ref_size, const int64_t *h_alt_start,
                               const int32_t *h_alt_size, int64_t n_chromosomes, const int64_t *h_chrom_seq_start,
                               const int64_t *h_chrom_first_kept, gki_haplotype_paths **plan_out) {
    if (plan_out == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_paths_create: plan is NULL");
    *plan_out = nullptr;
    const int64_t K = n_kept, C = n_chromosomes;
    if (n_bases < 0 || n_lines < 0 || K < 0 || K > n_lines || C < 1 || C > 0x7FFFFFFFll / 2 ||
        (n_bases > 0 && h_seq == nullptr) || (n_lines > 0 && (h_var_nodes == nullptr || h_kept_bits == nullptr)) ||
        (K > 0 && (h_kept_line == nullptr || h_ref_start == nullptr || h_ref_size == nullptr || h_alt_start == nullptr ||
                   h_alt_size == nullptr)) || h_chrom_seq_start == nullptr || h_chrom_first_kept == nullptr)
        return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_paths_create: a size is out of range or an array is NULL");
    // what keeps every read of the gather inside seq: the kept lines ascend, a line's two alleles lie side by side and the
    // next line's begin behind them; every kept line has its bit
    for (int64_t j = 0; j < K; j++) {
        const int64_t line = h_kept_line[j], end = h_alt_start[j] + h_alt_size[j];
        if (line < 0 || line >= n_lines || (j > 0 && line <= h_kept_line[j - 1]) || !((h_kept_bits[line >> 6] >> (line & 63)) & 1ull) ||
            h_ref_start[j] < 0 || h_ref_size[j] < 0 || h_alt_size[j] < 0 || h_alt_start[j] != h_ref_start[j] + h_ref_size[j] ||
            end > (j + 1 < K ? h_ref_start[j + 1] : n_bases))
            return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_paths_create: kept line %lld is not a bubble of the chain", (long long)j);
    }
    const int64_t W = ceil_div(n_lines, 64);
    int64_t bits = 0;
    for (int64_t w = 0; w < W; w++) bits += __builtin_popcountll(h_kept_bits[w]);
    if (bits != K) return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_paths_create: kept_bits has %lld bits for %lld kept lines", (long long)bits, (long long)K);
    for (int64_t c = 0; c <= C; c++) {
        const int64_t s = h_chrom_seq_start[c], f = h_chrom_first_kept[c];
        if (s < 0 || s > n_bases || f < 0 || f > K || (c > 0 && (s < h_chrom_seq_start[c - 1] || f < h_chrom_first_kept[c - 1])) ||
            (c == C && (s != n_bases || f != K)))
            return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_paths_create: chromosome %lld's start is out of order", (long long)c);
    }
    gki_haplotype_paths *raw = new gki_haplotype_paths;
    struct Guard { gki_haplotype_paths *p; ~Guard() { delete p; } } guard{raw};
    gki_haplotype_paths &g = *raw;
    g.n_bases = n_bases; g.n_lines = n_lines; g.K = K; g.W = W; g.n_chrom = (int)C;
    HIP_TRY(hipGetDevice(&g.device));
    GKI_TRY(upload(g.seq, h_seq, (size_t)n_bases));
    GKI_TRY(upload(g.var_nodes, h_var_nodes, (size_t)n_lines * 4));
    GKI_TRY(upload(g.kept_bits, h_kept_bits, (size_t)W * 8));
    GKI_TRY(upload(g.kline, h_kept_line, (size_t)K * 8));
    GKI_TRY(upload(g.ref_start, h_ref_start, (size_t)K * 8));
    GKI_TRY(upload(g.ref_size, h_ref_size, (size_t)K * 4));
    GKI_TRY(upload(g.alt_start, h_alt_start, (size_t)K * 8));
    GKI_TRY(upload(g.alt_size, h_alt_size, (size_t)K * 4));
    GKI_TRY(upload(g.chrom_seq_start, h_chrom_seq_start, (size_t)(C + 1) * 8));
    GKI_TRY(upload(g.chrom_first_kept, h_chrom_first_kept, (size_t)(C + 1) * 8));
    g.scan_tmp_bytes = gki_scan_tmp_bytes(K > 0 ? K : 1);
    HIP_TRY(g.drop_len.alloc((size_t)(K + 1) * 4));
    HIP_TRY(g.drop_start.alloc((size_t)(K + 1) * 8));
    HIP_TRY(g.scan_tmp.alloc((size_t)g.scan_tmp_bytes));
    HIP_TRY(g.slot_path.alloc(K, g.n_chrom));
    HIP_TRY(g.tile_site.alloc((size_t)(ceil_div(n_bases, HAP_TILE) + 1) * 8));
    *plan_out = raw;
    guard.p = nullptr;
    return GKI_OK;
}

int gki_haplotype_spell_count(gki_haplotype_paths *plan, const void *d_alt_bits, int64_t n_slots, int64_t slot,
                              int64_t *n_out, int64_t *h_bounds, float *count_ms) {
    if (count_ms) *count_ms = 0.0f;
    if (n_out) *n_out = 0;
    GKI_TRY(gki_check_haplotype_plan(plan, "haplotype_spell_count"));
    gki_haplotype_paths &g = *plan;
    g.n_out = -1;
    g.slot_path.of = HapKey();
    if (n_out == nullptr || h_bounds == nullptr || slot < 0 || slot >= n_slots || (g.W > 0 && d_alt_bits == nullptr))
        return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_spell_count: slot %lld of %lld, or a pointer is NULL", (long long)slot,
                             (long long)n_slots);
    HapPath &path = g.slot_path;
    TimerEvents ev;
    float ms_a = 0.0f, ms_b = 0.0f;
    GKI_TRY(ev.start(0));
    GKI_TRY(gki_haplotype_build_path(g, (const uint64_t *)d_alt_bits + slot * g.W, path));
    GKI_TRY(ev.stop(0, &ms_a));
    HIP_TRY(hipMemcpy(h_bounds, path.bounds.get(), (size_t)(g.n_chrom + 1) * 8, hipMemcpyDeviceToHost));
    const int64_t total = h_bounds[g.n_chrom];
    if (total < 0 || total > g.n_bases)
        return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_spell_count: %lld letters out of %lld (internal)", (long long)total,
                             (long long)g.n_bases);
    const int64_t n_tiles = ceil_div(total, HAP_TILE);
    GKI_TRY(ev.start(0));
    hipLaunchKernelGGL(k_hap_tile_sites, dim3(stream_grid(n_tiles + 1, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0,
                       path.cut.get<const int64_t>(), g.K, n_tiles, g.tile_site.get<int64_t>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(ev.stop(0, &ms_b));
    if (count_ms) *count_ms = ms_a + ms_b;
    g.n_out = total;
    path.of = {slot, d_alt_bits};
    *n_out = total;
    return GKI_OK;
}

int gki_haplotype_spell_emit(gki_haplotype_paths *plan, void *d_letters, float *spell_ms) {
    if (spell_ms) *spell_ms = 0.0f;
    GKI_TRY(gki_check_haplotype_plan(plan, "haplotype_spell_emit"));
    gki_haplotype_paths &g = *plan;
    if (g.n_out < 0) return gki_set_error(GKI_ERR_STATE, "haplotype_spell_emit: no spell count call came before");
    const int64_t total = g.n_out;
    g.n_out = -1;
    if (total == 0) return GKI_OK;
    if (d_letters == nullptr || ((uintptr_t)d_letters & 15u))
        return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_spell_emit: the output is NULL or not 16-byte aligned");
    const int64_t n_tiles = ceil_div(total, HAP_TILE);
    TimerEvents ev;
    GKI_TRY(ev.start(0));
    hipLaunchKernelGGL(k_hap_spell, dim3((unsigned)(n_tiles < 256 * 8 ? n_tiles : 256 * 8)), dim3(PARSE_BLOCK), 0, 0,
                       g.seq.get<const uint8_t>(), g.K, g.slot_path.cut.get<const int64_t>(),
                       g.slot_path.before.get<const int64_t>(),
                       g.tile_site.get<const int64_t>(), total, (uint8_t *)d_letters);
    HIP_TRY(hipGetLastError());
    return ev.stop(0, spell_ms);
}

int gki_haplotype_alt_nodes_count(gki_haplotype_paths *plan, const void *d_alt_bits, int64_t n_slots, void *d_start,
                                  int64_t *n_nodes, float *kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_nodes) *n_nodes = 0;
    GKI_TRY(gki_check_haplotype_plan(plan, "haplotype_alt_nodes_count"));
    gki_haplotype_paths &g = *plan;
    g.alt.of = HapKey();
    g.alt.tile_before.reset();
    if (n_nodes == nullptr || d_start == nullptr || n_slots < 0 || (n_slots > 0 && g.W > 0 && d_alt_bits == nullptr))
        return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_alt_nodes_count: n_slots %lld, or a pointer is NULL", (long long)n_slots);
    const int64_t T = ceil_div(g.W, HAP_WORD_TILE), n_tiles = n_slots * T;
    if (n_slots > 0 && T > 0 && n_tiles / T != n_slots)
        return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_alt_nodes_count: %lld slots are too many", (long long)n_slots);
    DevBuf tile_cnt, tmp;
    const int64_t tmp_bytes = gki_scan_tmp_bytes(n_tiles > 0 ? n_tiles : 1);
    HIP_TRY(g.alt.tile_before.alloc((size_t)(n_tiles + 1) * 8));
    HIP_TRY(hipMemset(g.alt.tile_before.get(), 0, 8));     // no tile: [0]
    HIP_TRY(tile_cnt.alloc((size_t)(n_tiles + 1) * 4));
    HIP_TRY(tmp.alloc((size_t)tmp_bytes));
    TimerEvents ev;
    GKI_TRY(ev.start(0));
    if (n_tiles > 0) {
        hipLaunchKernelGGL(k_hap_alt_count, dim3((unsigned)(n_tiles < 256 * 8 ? n_tiles : 256 * 8)), dim3(PARSE_BLOCK), 0, 0,
                           (const uint64_t *)d_alt_bits, g.kept_bits.get<const uint64_t>(), g.W, T, n_slots,
                           tile_cnt.get<uint32_t>());
        HIP_TRY(hipGetLastError());
        GKI_TRY(gki_scan_u32_to_i64(tile_cnt.get<const uint32_t>(), n_tiles, g.alt.tile_before.get<int64_t>(), tmp.get(),
                                    tmp_bytes, 0));
    }
    hipLaunchKernelGGL(k_hap_alt_starts, dim3(stream_grid(n_slots + 1, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0,
                       g.alt.tile_before.get<const int64_t>(), T, n_slots, (int64_t *)d_start);
    HIP_TRY(hipGetLastError());
    GKI_TRY(ev.stop(0, kernel_ms));
    HIP_TRY(hipMemcpy(&g.alt.total, g.alt.tile_before.get<const int64_t>() + n_tiles, 8, hipMemcpyDeviceToHost));
    g.alt.of = {n_slots, d_alt_bits};
    *n_nodes = g.alt.total;
    return GKI_OK;
}

int gki_haplotype_alt_nodes_emit(gki_haplotype_paths *plan, const void *d_alt_bits, int64_t n_slots, void *d_nodes,
                                 float *kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    GKI_TRY(gki_check_haplotype_plan(plan, "haplotype_alt_nodes_emit"));
    gki_haplotype_paths &g = *plan;
    if (g.alt.of == HapKey()) return gki_set_error(GKI_ERR_STATE, "haplotype_alt_nodes_emit: no alt-nodes count call came before");
    if (g.alt.of != HapKey{n_slots, d_alt_bits})
        return gki_set_error(GKI_ERR_STATE, "haplotype_alt_nodes_emit: the count call was given another plane");
    DevBuf tile_before;                                    // the plan's goes back to the pool when the call returns
    tile_before.swap(g.alt.tile_before);
    g.alt.of = HapKey();
    if (g.alt.total == 0) return GKI_OK;
    if (d_nodes == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "haplotype_alt_nodes_emit: the output is NULL");
    const int64_t T = ceil_div(g.W, HAP_WORD_TILE), n_tiles = n_slots * T;
    TimerEvents ev;
    GKI_TRY(ev.start(0));
    hipLaunchKernelGGL(k_hap_alt_emit, dim3((unsigned)(n_tiles < 256 * 8 ? n_tiles : 256 * 8)), dim3(PARSE_BLOCK), 0, 0,
                       (const uint64_t *)d_alt_bits, g.kept_bits.get<const uint64_t>(), g.W, T, n_slots,
                       tile_before.get<const int64_t>(), g.var_nodes.get<const uint32_t>(), (uint32_t *)d_nodes);
    HIP_TRY(hipGetLastError());
    return ev.stop(0, kernel_ms);
}

}  // extern "C"
