// Text in HBM deflated into BGZF members in HBM (include/gki.h, "BGZF deflate"): the way out of what gki_inflate.hip is
// the way in of.  Only the compressed bytes cross to the host.
//
//   k_bgzf_deflate   one workgroup of 256 lanes (four waves) per member, all of them on it: the pieces of
//                    csrc/gki_deflate_core.h under the schedule that header lists -- the CRC-32 per 256-byte segment, the
//                    candidates in rounds of 256 positions (one lane each) with the round's own earlier positions looked
//                    at too, a greedy walk per segment (one lane each) for the counts, the codes (the two rank sorts
//                    across the lanes, the two code constructions on one lane of two different waves, the header on one
//                    lane), the walk again for the segments' bits, and once more to emit them at their bit offsets.
//                    Workgroups take members grid-stride.
//                      LDS: one gki_def_state, static, below 64 KiB (tests/test_deflate_codegen.py pins it).  The member's
//                    input is read from global memory (64 KiB that stay in the cache), its per-position match words pm live
//                    in a global scratch of 0xff00 words per WORKGROUP, and its output goes straight to its slot of the
//                    staging buffer.
//                      Output: a dynamic member's words are zeroed, then a word that one emitter fills is stored and a
//                    word shared between emitters is or-ed with atomics only; a stored member is written in bytes.
//   k_bgzf_pack      members from their fixed stride to back to back: a lane owns 16 output bytes, finds their member by a
//                    search of the scanned sizes, and moves them with one 16-byte load and store when they lie in one
//                    member.
//
// Bounds: a member's slot is stride >= its input + 31 bytes rounded up to 16, which no member exceeds (a dynamic payload is
// taken only when it is smaller than the stored one); the emitter writes no word at or above the slot's end; pm is indexed
// by positions below the member's length.
#include "gki_common.h"
#include "gki_deflate_core.h"
#include "gki_seq_gather.h"

namespace {

constexpr int DEFLATE_BLOCK = GKI_DEF_SEG;                // one lane per position of a round and per segment
constexpr int DEFLATE_MAX_GRID = 512;                     // workgroups, and scratches of 0xff00 words

__global__ __launch_bounds__(DEFLATE_BLOCK) void k_bgzf_deflate(const uint8_t *__restrict__ in, int64_t n_in, int block_size,
                                                                int64_t n_members, uint8_t *__restrict__ stage, int64_t stride,
                                                                uint32_t *__restrict__ pm_all, int32_t *__restrict__ sizes) {
    __shared__ gki_def_state st;
    const int t = threadIdx.x;
    st.crc_table[t] = gki_crc32_table_entry((uint32_t)t);
    uint32_t *pm = pm_all + (int64_t)blockIdx.x * GKI_DEF_MAX_IN;
    for (int64_t m = blockIdx.x; m < n_members; m += gridDim.x) {
        const int64_t a = m * block_size;
        const int n = (int)(n_in - a < block_size ? n_in - a : (int64_t)block_size);
        const uint8_t *src = in + a;
        uint32_t *words = reinterpret_cast<uint32_t *>(stage + m * stride);
        const int n_seg = (n + GKI_DEF_SEG - 1) / GKI_DEF_SEG;
        const int begin = t * GKI_DEF_SEG, end = begin + GKI_DEF_SEG < n ? begin + GKI_DEF_SEG : n;   // begin < n: the lane has a segment
        for (int i = t; i < GKI_DEF_HASH_SIZE; i += DEFLATE_BLOCK) st.head[i] = 0;
        for (int i = t; i < 288; i += DEFLATE_BLOCK) st.lfreq[i] = 0;
        if (t < 32) st.dfreq[t] = 0;
        st.seg_bits[t] = 0;
        if (t == 0) st.crc = 0;
        __syncthreads();
        if (begin < n) gki_def_crc_add_segment(st, src, n, begin, end);
        for (int r = 0; r < n_seg; r++) {
            const int p = r * GKI_DEF_SEG + t;
            const uint32_t cand1 = gki_def_round_begin(st, src, n, p, t);
            __syncthreads();
            gki_def_round_end(st, src, n, p, t, cand1, pm);
            __syncthreads();
        }
        if (begin < n) gki_def_count_segment(st, src, pm, begin, end);
        __syncthreads();
        if (t == 0) gki_def_counts_finish(st);
        __syncthreads();
        for (int s = t; s < GKI_DEF_LCODES; s += DEFLATE_BLOCK) gki_def_rank_symbol(st.lfreq, GKI_DEF_LCODES, s, st.lorder);
        if (t < GKI_DEF_DCODES) gki_def_rank_symbol(st.dfreq, GKI_DEF_DCODES, t, st.dorder);
        __syncthreads();
        if (t == 0) gki_def_build_code(st.lfreq, GKI_DEF_LCODES, 15, st.lorder, st.lwork, st.llen, st.lcode);
        if (t == GKI_WAVE) gki_def_build_code(st.dfreq, GKI_DEF_DCODES, 15, st.dorder, st.dwork, st.dlen, st.dcode);
        __syncthreads();
        if (t == 0) gki_def_header_plan(st);
        __syncthreads();
        if (begin < n) st.seg_bits[t] = gki_def_segment_bits(st, src, pm, begin, end);
        __syncthreads();
        if (t == 0) gki_def_layout(st, n);
        __syncthreads();
        if (st.stored) {
            gki_def_stored_bytes(reinterpret_cast<uint8_t *>(words), src, t, n, DEFLATE_BLOCK);
            if (t == 0) gki_def_stored_frame(reinterpret_cast<uint8_t *>(words), gki_def_crc_finish(st.crc, n), n);
        } else {
            const int member_words = (int)((st.member_bytes + 3u) / 4u);
            for (int i = t; i < member_words; i += DEFLATE_BLOCK) words[i] = 0u;
            __syncthreads();
            gki_def_bits b;
            if (begin < n) {
                gki_def_bits_begin(b, words, member_words, st.seg_bits[t]);
                gki_def_emit_segment(st, src, pm, begin, end, b);
                gki_def_bits_end(b);
            }
            if (t == 0) {
                gki_def_bits_begin(b, words, member_words, 0u);
                gki_def_emit_member_head(b, st.member_bytes);
                gki_def_emit_header(st, b);
                gki_def_bits_end(b);
            }
            if (t == GKI_WAVE) {
                gki_def_bits_begin(b, words, member_words, st.end_bit - st.llen[256]);
                gki_def_emit_tail(st, b, gki_def_crc_finish(st.crc, n), n);
                gki_def_bits_end(b);
            }
        }
        if (t == 0) sizes[m] = (int32_t)st.member_bytes;
        __syncthreads();                                   // st and pm are the next member's from here
    }
}

// member_start: int64[n_members + 1], the scan of the sizes
__global__ __launch_bounds__(256) void k_bgzf_pack(const uint8_t *__restrict__ stage, int64_t stride,
                                                   const int64_t *__restrict__ member_start, int64_t n_members,
                                                   uint8_t *__restrict__ out, int64_t n_out) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c * 16 < n_out; c += step) {
        const int64_t p = c * 16, e = p + 16 < n_out ? p + 16 : n_out;
        int64_t m = first_site_after(member_start + 1, 0, n_members, p);       // below n_members: p < n_out
        if (e - p == 16 && member_start[m + 1] >= e) {
            *reinterpret_cast<Letters16 *>(out + p) =
                *reinterpret_cast<const Letters16 *>(stage + m * stride + (p - member_start[m]));
        } else {
            for (int64_t q = p; q < e; q++) {
                while (m + 1 < n_members && member_start[m + 1] <= q) m++;
                out[q] = stage[m * stride + (q - member_start[m])];
            }
        }
    }
}

thread_local float g_deflate_kernel_ms = 0.0f;            // the kernels of this thread's last gki_bgzf_deflate

int deflate_check(int64_t n_in, int block_size, const char *who) {
    if (n_in < 0) return gki_set_error(GKI_ERR_BAD_ARG, "%s: a negative size", who);
    if (block_size < 1 || block_size > GKI_DEF_MAX_IN)
        return gki_set_error(GKI_ERR_BAD_ARG, "%s: block_size %d is outside 1..65280", who, block_size);
    return GKI_OK;
}

}  // namespace

extern "C" {

int gki_bgzf_deflate_bound(int64_t n_in, int block_size, int64_t *bytes) {
    if (bytes == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "bgzf_deflate_bound: bytes is NULL");
    *bytes = 0;
    GKI_TRY(deflate_check(n_in, block_size, "bgzf_deflate_bound"));
    *bytes = n_in + GKI_DEF_MEMBER_EXTRA * ceil_div(n_in, block_size);
    return GKI_OK;
}

int gki_bgzf_deflate(const void *d_in, int64_t n_in, int block_size, void *d_out, int64_t out_capacity, int64_t *n_out,
                     int64_t *n_members, void *d_member_end) {
    if (n_out) *n_out = 0;
    if (n_members) *n_members = 0;
    g_deflate_kernel_ms = 0.0f;
    if (n_out == nullptr || n_members == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "bgzf_deflate: n_out or n_members is NULL");
    GKI_TRY(deflate_check(n_in, block_size, "bgzf_deflate"));
    if (out_capacity < 0) return gki_set_error(GKI_ERR_BAD_ARG, "bgzf_deflate: a negative size");
    const int64_t members = ceil_div(n_in, block_size), bound = n_in + GKI_DEF_MEMBER_EXTRA * members;
    if ((n_in > 0 && d_in == nullptr) || (out_capacity > 0 && d_out == nullptr))
        return gki_set_error(GKI_ERR_BAD_ARG, "bgzf_deflate: a NULL buffer");
    if (out_capacity < bound)
        return gki_set_error(GKI_ERR_BAD_ARG, "bgzf_deflate: a capacity of %lld bytes is below the bound of %lld", (long long)out_capacity,
                             (long long)bound);
    if (members > 0x7FFFFFFFll) return gki_set_error(GKI_ERR_BAD_ARG, "bgzf_deflate: %lld members are too many", (long long)members);
    if (members == 0) return GKI_OK;
    const int64_t stride = (block_size + GKI_DEF_MEMBER_EXTRA + 15) / 16 * 16, tmp_bytes = gki_scan_tmp_bytes(members);
    const int grid = (int)(members < DEFLATE_MAX_GRID ? members : DEFLATE_MAX_GRID);
    TimerEvents ev;
    DevBuf stage, pm, sizes, start, tmp;
    HIP_TRY(stage.alloc((size_t)(members * stride)));
    HIP_TRY(pm.alloc((size_t)grid * GKI_DEF_MAX_IN * sizeof(uint32_t)));
    HIP_TRY(sizes.alloc((size_t)members * sizeof(int32_t)));
    HIP_TRY(start.alloc((size_t)(members + 1) * sizeof(int64_t)));
    HIP_TRY(tmp.alloc((size_t)tmp_bytes));
    GKI_TRY(ev.start(0));
    hipLaunchKernelGGL(k_bgzf_deflate, dim3(grid), dim3(DEFLATE_BLOCK), 0, 0, (const uint8_t *)d_in, n_in, block_size, members,
                       stage.get<uint8_t>(), stride, pm.get<uint32_t>(), sizes.get<int32_t>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(gki_scan_i32_to_i64(sizes.get<const int32_t>(), members, start.get<int64_t>(), tmp.get(), tmp_bytes, 0));
    int64_t total = 0;
    HIP_TRY(hipMemcpy(&total, start.get<const int64_t>() + members, sizeof(total), hipMemcpyDeviceToHost));
    if (total < 0 || total > bound) return gki_set_error(GKI_ERR_STATE,"bgzf_deflate: %lld bytes of members, above the bound", (long long)total);
    hipLaunchKernelGGL(k_bgzf_pack, dim3(stream_grid(ceil_div(total, 16), 256)), dim3(256), 0, 0, stage.get<const uint8_t>(), stride,
                       start.get<const int64_t>(), members, (uint8_t *)d_out, total);
    HIP_TRY(hipGetLastError());
    GKI_TRY(ev.stop(0, &g_deflate_kernel_ms));
    if (d_member_end)
        HIP_TRY(hipMemcpy(d_member_end, start.get<const int64_t>() + 1, (size_t)members * sizeof(int64_t), hipMemcpyDeviceToDevice));
    *n_out = total;
    *n_members = members;
    return GKI_OK;
}

int gki_bgzf_deflate_kernel_ms(float *ms) {
    if (ms == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "bgzf_deflate_kernel_ms: ms is NULL");
    *ms = g_deflate_kernel_ms;
    return GKI_OK;
}

}  // extern "C"
