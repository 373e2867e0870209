// K-mers of a linear reference (snp_kmer_finder.py:298-312, command_line_interface.py:105-153): every record is a pure
// function of its position in the sequence, so the kernel is a store stream.  The caller describes the output as
// SEGMENTS (first position, record count): record j of a segment is the k-mer at first + j * spacing; with reverse
// complements a segment's forward records are followed by as many records with the reverse-complemented hash.  Here
// each half of a segment is a SPAN (first output record, first position, strand), and the output is cut into blocks of
// 4096 records, a wave per block, as in k_emit_interior_dense: every store covers 64 consecutive records
// of one column, whole and line-aligned, whatever the segments' sizes.
#include "gki_read_windows.h"
#include <vector>

namespace {

constexpr int LIN_BLOCK = 4096;                  // output records of one wave-owned block: 64 groups of 64

// ASCII letters -> 2-bit stream, 16 letters per lane, by the read side's letter rule (letter_code, gki_read_windows.h)
__global__ __launch_bounds__(256) void k_pack_letters(const uint8_t *__restrict__ letters, int64_t n, int aligned16,
                                                      uint32_t *__restrict__ seq2_u32, int64_t n_u32) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_u32; i += stride) {
        const int64_t b = i * 16;
        uint32_t r = 0;
        if (aligned16 && b + 16 <= n) {
            const uint4 v = *reinterpret_cast<const uint4 *>(letters + b);         // 16 B per lane, coalesced
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 16; j++) r |= letter_code((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) << (2 * j);
        } else {
            for (int j = 0; j < 16; j++)
                if (b + j < n) r |= letter_code(letters[b + j]) << (2 * j);
        }
        seq2_u32[i] = r;
    }
}

struct LinArgs {
    int64_t n_words;             // words of the 2-bit stream (zero beyond the sequence)
    int n_spans;
    int rc_pairs;                // spans come in (forward, reverse complement) pairs: the odd ones are reverse complements
    int k;
    int64_t spacing;
    int64_t n_out;
    uint64_t *hashes;
    uint32_t *nodes;
    uint64_t *ref_offsets;
    float *af;
};

// the last span that begins at or before output record o (empty spans share their begin with the next one and lose)
__device__ __forceinline__ int lin_span_of(const int64_t *__restrict__ span_out, int n_spans, int64_t o) {
    int lo = 0, hi = n_spans;                            // span_out[lo] <= o < span_out[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (span_out[mid] <= o) lo = mid; else hi = mid;
    }
    return lo;
}

// A block is DENSE when all its 4096 records lie in one span at spacing 1: its bases are then 130 consecutive words at
// most.  k_linear_emit_dense writes those blocks, k_linear_emit_rest every other one.
__device__ __forceinline__ bool lin_is_dense(const LinArgs &a, const int64_t *__restrict__ span_out, int64_t block, int *span) {
    *span = lin_span_of(span_out, a.n_spans, block * LIN_BLOCK);
    return a.spacing == 1 && (block + 1) * LIN_BLOCK <= span_out[*span + 1];
}

// the first dense block among b, b + step, b + 2 * step, ... (n_blocks if there is none); wave-uniform, scalar loads only
__device__ __forceinline__ int64_t lin_next_dense(const LinArgs &a, const int64_t *__restrict__ span_out, int64_t b, int64_t step,
                                                  int64_t n_blocks, int *span) {
    while (b < n_blocks && !lin_is_dense(a, span_out, b, span)) b += step;
    return b < n_blocks ? b : n_blocks;
}

// The words of a dense block's bases, word 64 * i + lane in w<i>: 3 * 64 words hold the 4096 + 31 + 30 bases a block can
// touch (named, not an array: they must stay in registers)
struct LinWords { uint64_t w0, w1, w2; };

__device__ __forceinline__ LinWords lin_load_words(const uint64_t *__restrict__ seq2, int64_t n_words, int64_t pos0, int lane) {
    LinWords w;
    w.w0 = w.w1 = w.w2 = 0;
    const int64_t i = (pos0 >> 5) + lane;
    if (i < n_words) w.w0 = seq2[i];
    if (i + 64 < n_words) w.w1 = seq2[i + 64];
    if (i + 128 < n_words) w.w2 = seq2[i + 128];
    return w;
}

// word j (a constant) of the block's bases, in scalar registers
__device__ __forceinline__ uint64_t lin_word(const LinWords &w, int j) {
    const uint64_t v = j < 64 ? w.w0 : j < 128 ? w.w1 : w.w2;
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, j & 63);
    const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), j & 63);
    return ((uint64_t)hi << 32) | lo;
}

// A wave per dense block.  The words of the wave's NEXT dense block are loaded before the current block's stores (64
// groups x 4 columns, one straight line) are issued, so the only wait of the loop is a counted one that leaves the
// stores in flight.
template <bool COLUMNS>
__global__ __launch_bounds__(256) void k_linear_emit_dense(LinArgs a, const uint64_t *__restrict__ seq2,
                                                           const int64_t *__restrict__ span_out,
                                                           const int64_t *__restrict__ span_pos) {
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t n_blocks = (a.n_out + LIN_BLOCK - 1) / LIN_BLOCK;
    const uint64_t mask = (1ull << (2 * a.k)) - 1ull;
    // the wave's number: uniform, fits 32 bits (the grid has at most 2048 * 4 waves)
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    int span, span_next = 0;
    int64_t b = lin_next_dense(a, span_out, wave, n_waves, n_blocks, &span);
    if (b >= n_blocks) return;
    int64_t pos0 = span_pos[span] + (b * LIN_BLOCK - span_out[span]);
    LinWords cur = lin_load_words(seq2, a.n_words, pos0, lane);
    // the first block's words are waited for HERE: left to the loop, that wait would sit in its body and drain every
    // later block's stores as well
    asm volatile("" : "+v"(cur.w0), "+v"(cur.w1), "+v"(cur.w2));
    while (true) {
        const int64_t nb = lin_next_dense(a, span_out, b + n_waves, n_waves, n_blocks, &span_next);
        int64_t pos0_next = 0;
        LinWords nxt = {0, 0, 0};
        if (nb < n_blocks) {
            pos0_next = span_pos[span_next] + (nb * LIN_BLOCK - span_out[span_next]);
            nxt = lin_load_words(seq2, a.n_words, pos0_next, lane);
        }
        const bool rc = a.rc_pairs && (span & 1);
        const int rel0 = (int)(pos0 & 31) + lane;        // base of this lane's first record, counted from the block's first word
        uint64_t *__restrict__ ph = a.hashes + b * LIN_BLOCK + lane;
        uint32_t *__restrict__ pn = a.nodes + b * LIN_BLOCK + lane;
        uint64_t *__restrict__ pr = a.ref_offsets + b * LIN_BLOCK + lane;
        float *__restrict__ pa = a.af + b * LIN_BLOCK + lane;
        const uint64_t r0 = (uint64_t)(pos0 + lane);
#pragma unroll
        for (int u = 0; u < 64; u++) {
            const int d = rel0 >> 5;                     // the record's word is 2u + d, d = 0, 1 or 2
            const uint64_t s0 = lin_word(cur, 2 * u), s1 = lin_word(cur, 2 * u + 1), s2 = lin_word(cur, 2 * u + 2),
                           s3 = lin_word(cur, 2 * u + 3);
            const uint64_t lo = d == 0 ? s0 : d == 1 ? s1 : s2;
            const uint64_t hi = d == 0 ? s1 : d == 1 ? s2 : s3;
            const int sh = (rel0 & 31) * 2;
            const uint64_t h = ((lo >> sh) | ((hi << 1) << (63 - sh))) & mask;
            const uint64_t hr = gki_revcomp(h, a.k);
            ph[u * 64] = rc ? hr : h;
            if (COLUMNS) {
                pn[u * 64] = 1u;
                pr[u * 64] = r0 + (uint64_t)(u * 64);
                pa[u * 64] = 1.0f;
            }
            __builtin_amdgcn_sched_barrier(0);           // group by group: 64 groups of arithmetic above the stores cost 200 VGPRs
        }
        if (nb >= n_blocks) break;
        cur = nxt;
        b = nb; span = span_next; pos0 = pos0_next;
    }
}

// Every block that is not dense, a wave per block: each lane finds the span of its own record, starting from the span
// of the group's first one, and reads its k-mer from global memory.
template <bool COLUMNS>
__global__ __launch_bounds__(256) void k_linear_emit_rest(LinArgs a, const uint64_t *__restrict__ seq2,
                                                          const int64_t *__restrict__ span_out,
                                                          const int64_t *__restrict__ span_pos) {
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t n_blocks = (a.n_out + LIN_BLOCK - 1) / LIN_BLOCK;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    for (int64_t b = wave; b < n_blocks; b += n_waves) {
        int t;
        if (lin_is_dense(a, span_out, b, &t)) continue;
        for (int u = 0; u < 64; u++) {
            const int64_t o0 = b * LIN_BLOCK + u * 64;
            if (o0 >= a.n_out) break;
            while (span_out[t + 1] <= o0) t++;           // uniform; o0 < n_out = span_out[n_spans] ends it
            const int64_t o = o0 + lane;
            if (o < a.n_out) {
                int tl = t;
                while (span_out[tl + 1] <= o) tl++;
                const int64_t pos = span_pos[tl] + (o - span_out[tl]) * a.spacing;
                uint64_t h = gki_extract(seq2, pos, a.k);
                if (a.rc_pairs && (tl & 1)) h = gki_revcomp(h, a.k);
                a.hashes[o] = h;
                if (COLUMNS) {
                    a.nodes[o] = 1u;
                    a.ref_offsets[o] = (uint64_t)pos;
                    a.af[o] = 1.0f;
                }
            }
        }
    }
}

}  // namespace

extern "C" {

int gki_linear_kmers(const void *d_letters, int64_t n_letters, int k, int64_t spacing, const int64_t *h_seg_first,
                     const int64_t *h_seg_count, int64_t n_segments, int with_reverse_complement, void *d_hashes,
                     void *d_nodes, void *d_ref_offsets, void *d_af32, int64_t out_capacity, int64_t *n_out,
                     float *kernel_ms) {
    *n_out = 0;
    if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.f;
    if (k < 1 || k > GKI_MAX_K) return gki_set_error(GKI_ERR_BAD_ARG, "k must be in 1..31");
    if (spacing < 1) return gki_set_error(GKI_ERR_BAD_ARG, "linear_kmers: spacing must be at least 1");
    if (n_letters < 0 || n_segments < 0 || n_segments > (1 << 28))
        return gki_set_error(GKI_ERR_BAD_ARG, "linear_kmers: bad sequence length or segment count");
    const int per = with_reverse_complement ? 2 : 1;
    const int64_t n_spans = n_segments * per;
    std::vector<int64_t> span_out((size_t)n_spans + 1), span_pos((size_t)n_spans + 1);      // before the DevBufs
    int64_t total = 0;
    for (int64_t s = 0; s < n_segments; s++) {
        const int64_t first = h_seg_first[s], cnt = h_seg_count[s];
        if (first < 0 || cnt < 0) return gki_set_error(GKI_ERR_BAD_ARG, "linear_kmers: segment %lld has a negative field", (long long)s);
        // the last record's k-mer must end inside the sequence (no clipping here: the caller sizes its segments)
        if (cnt > 0 && (cnt - 1 > (n_letters - k - first) / spacing || first + k > n_letters))
            return gki_set_error(GKI_ERR_BAD_ARG, "linear_kmers: segment %lld (first %lld, %lld records, spacing %lld, k %d) "
                                 "runs past the sequence of %lld letters", (long long)s, (long long)first, (long long)cnt,
                                 (long long)spacing, k, (long long)n_letters);
        if (cnt > (INT64_MAX / 4 - total) / per) return gki_set_error(GKI_ERR_BAD_ARG, "linear_kmers: record count overflows");
        for (int h = 0; h < per; h++) {
            span_out[(size_t)(s * per + h)] = total;
            span_pos[(size_t)(s * per + h)] = first;
            total += cnt;
        }
    }
    span_out[(size_t)n_spans] = total;
    span_pos[(size_t)n_spans] = 0;
    *n_out = total;
    if (d_hashes == nullptr) return GKI_OK;               // count only
    if (total > out_capacity) return gki_set_error(GKI_ERR_BAD_ARG, "linear_kmers: output needs %lld records, capacity %lld",
                                                   (long long)total, (long long)out_capacity);
    const bool columns = d_nodes != nullptr;
    if (columns && (d_ref_offsets == nullptr || d_af32 == nullptr))
        return gki_set_error(GKI_ERR_BAD_ARG, "linear_kmers: nodes, ref_offsets and allele_frequencies go together");
    if (total == 0) return GKI_OK;

    TimerEvents ev, ev2;
    if (kernel_ms) {
        HIP_TRY(hipEventCreate(&ev.e0)); HIP_TRY(hipEventCreate(&ev.e1));
        HIP_TRY(hipEventCreate(&ev2.e0)); HIP_TRY(hipEventCreate(&ev2.e1));
    }
    // the dense path loads whole words up to 3 * 64 past a block's first one, guarded by n_words; gki_extract reads one
    // word past a k-mer's first
    const int64_t n_u32 = ceil_div(n_letters, 16);
    const int64_t n_words = ceil_div(n_letters, 32) + 2;
    DevBuf seq2, spans;
    HIP_TRY(seq2.alloc((size_t)n_words * 8));
    HIP_TRY(spans.alloc((size_t)(2 * n_spans + 2) * 8));
    HIP_TRY(hipMemsetAsync(seq2.get(), 0, (size_t)n_words * 8, 0));
    HIP_TRY(hipMemcpyAsync(spans.get(), span_out.data(), (size_t)(n_spans + 1) * 8, hipMemcpyHostToDevice, 0));
    HIP_TRY(hipMemcpyAsync(spans.get<int64_t>() + n_spans + 1, span_pos.data(), (size_t)(n_spans + 1) * 8, hipMemcpyHostToDevice, 0));
    if (kernel_ms) HIP_TRY(hipEventRecord(ev.e0, 0));
    hipLaunchKernelGGL(k_pack_letters, dim3(stream_grid(n_u32, 256)), dim3(256), 0, 0, (const uint8_t *)d_letters, n_letters,
                       (int)(((uintptr_t)d_letters & 15) == 0), seq2.get<uint32_t>(), n_u32);
    HIP_TRY(hipGetLastError());
    if (kernel_ms) { HIP_TRY(hipEventRecord(ev.e1, 0)); HIP_TRY(hipEventRecord(ev2.e0, 0)); }

    LinArgs a;
    a.n_words = n_words;
    a.n_spans = (int)n_spans;
    a.rc_pairs = with_reverse_complement ? 1 : 0;
    a.k = k;
    a.spacing = spacing;
    a.n_out = total;
    a.hashes = (uint64_t *)d_hashes;
    a.nodes = (uint32_t *)d_nodes;
    a.ref_offsets = (uint64_t *)d_ref_offsets;
    a.af = (float *)d_af32;
    const uint64_t *d_seq2 = seq2.get<const uint64_t>();
    const int64_t *d_span_out = spans.get<const int64_t>();            // span_out[n_spans + 1], then span_pos[n_spans + 1]
    const int64_t *d_span_pos = d_span_out + n_spans + 1;
    const int grid = stream_grid(ceil_div(total, LIN_BLOCK) * 64, 256);
    if (spacing == 1 && total >= LIN_BLOCK) {
        if (columns) hipLaunchKernelGGL(k_linear_emit_dense<true>, dim3(grid), dim3(256), 0, 0, a, d_seq2, d_span_out, d_span_pos);
        else hipLaunchKernelGGL(k_linear_emit_dense<false>, dim3(grid), dim3(256), 0, 0, a, d_seq2, d_span_out, d_span_pos);
        HIP_TRY(hipGetLastError());
    }
    if (columns) hipLaunchKernelGGL(k_linear_emit_rest<true>, dim3(grid), dim3(256), 0, 0, a, d_seq2, d_span_out, d_span_pos);
    else hipLaunchKernelGGL(k_linear_emit_rest<false>, dim3(grid), dim3(256), 0, 0, a, d_seq2, d_span_out, d_span_pos);
    HIP_TRY(hipGetLastError());
    if (kernel_ms) HIP_TRY(hipEventRecord(ev2.e1, 0));
    HIP_TRY(hipStreamSynchronize(0));
    if (kernel_ms) {
        HIP_TRY(hipEventElapsedTime(&kernel_ms[0], ev.e0, ev.e1));
        HIP_TRY(hipEventElapsedTime(&kernel_ms[1], ev2.e0, ev2.e1));
    }
    return GKI_OK;
}

}  // extern "C"
