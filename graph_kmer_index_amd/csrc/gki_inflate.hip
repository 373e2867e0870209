// BGZF members inflated in HBM (include/gki.h, "BGZF"): the compressed bytes of a piece of a .gz reads file go in, the
// text the parse kernels take (csrc/gki_reads_parse.hip) comes out, with no host pass over either.
//
//   k_bgzf_inflate        one lane per member, and one member per wave: lane 0 of a one-wave workgroup runs
//                         gki_inflate_member (csrc/gki_inflate_core.h) over the member's payload with the Huffman tables in
//                         its private memory, then the CRC-32 of what it wrote against the member's trailer, through a
//                         256-entry table in LDS that the wave builds.  Members differ in length and in content, so lanes
//                         that share a wave diverge at every symbol and the wave pays for all their paths; a piece holds a
//                         few thousand members, fewer than the device has SIMDs.  Measured: 1 member per wave against 4,
//                         8, 16 and 64 (profiles/r11_bgzf_reads.txt).  A member that fails leaves its status; the others'
//                         output is whole.
//   k_bgzf_first_bad      the lowest member with a status, and that status
//   k_last_byte           the last position of a byte value in a window of a buffer (the line cut of the streaming route)
//
// Bounds: gki_bgzf_inflate checks on the device, before the inflate is launched, that every payload lies inside the input
// and every output range inside the output and is at most 64 KiB; the core reads and writes only inside the two ranges it
// is given.
#include "gki_common.h"
#include "gki_inflate_core.h"

namespace {

constexpr int INFLATE_BLOCK = 64;                         // one wave per workgroup, one member per workgroup
constexpr int64_t BGZF_MAX_OUT = 65536;                   // a member's ISIZE limit

struct InflateReport { unsigned long long first_bad; int invalid; int pad; };

// block b is valid when its payload lies in [0, n_in) and its output in [0, out_capacity), at most 64 KiB, not negative
__global__ __launch_bounds__(256) void k_bgzf_validate(const int64_t *__restrict__ payload_start,
                                                       const int32_t *__restrict__ payload_len,
                                                       const int64_t *__restrict__ out_start, int64_t n_blocks, int64_t n_in,
                                                       int64_t out_capacity, InflateReport *__restrict__ report) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_blocks; b += stride) {
        const int64_t ps = payload_start[b], pl = payload_len[b], o0 = out_start[b], o1 = out_start[b + 1];
        const bool ok = ps >= 0 && pl >= 0 && ps <= n_in && pl <= n_in - ps && o0 >= 0 && o1 >= o0 && o1 - o0 <= BGZF_MAX_OUT &&
                        o1 <= out_capacity;
        if (!ok) atomicOr(&report->invalid, 1);
    }
}

__global__ __launch_bounds__(INFLATE_BLOCK) void k_bgzf_inflate(const uint8_t *__restrict__ in,
                                                                const int64_t *__restrict__ payload_start,
                                                                const int32_t *__restrict__ payload_len,
                                                                const uint32_t *__restrict__ crc32,
                                                                const int64_t *__restrict__ out_start, int64_t n_blocks,
                                                                uint8_t *__restrict__ out, uint8_t *__restrict__ status) {
    __shared__ uint32_t crc_table[256];
    for (int i = threadIdx.x; i < 256; i += INFLATE_BLOCK) crc_table[i] = gki_crc32_table_entry((uint32_t)i);
    __syncthreads();
    const int64_t b = blockIdx.x;
    if (threadIdx.x != 0 || b >= n_blocks) return;
    gki_inf_tables tables;
    int64_t n_out;
    const int64_t o0 = out_start[b];
    status[b] = (uint8_t)gki_inflate_member(in + payload_start[b], payload_len[b], out + o0, out_start[b + 1] - o0, crc32[b],
                                            crc_table, tables, &n_out);
}

__global__ __launch_bounds__(256) void k_bgzf_first_bad(const uint8_t *__restrict__ status, int64_t n_blocks,
                                                        InflateReport *__restrict__ report) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_blocks; b += stride)
        if (status[b]) atomicMin(&report->first_bad, (unsigned long long)b);
}

// the greatest position p in [begin, end) with bytes[p] == value, as p + 1 in *best (0: none)
__global__ __launch_bounds__(256) void k_last_byte(const uint8_t *__restrict__ bytes, int64_t begin, int64_t end, int value,
                                                   unsigned long long *__restrict__ best) {
    __shared__ unsigned long long block_best;
    if (threadIdx.x == 0) block_best = 0ull;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long mine = 0ull;
    for (int64_t p = begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < end; p += stride)
        if (bytes[p] == (uint8_t)value) mine = (unsigned long long)p + 1ull;
    if (mine) atomicMax(&block_best, mine);
    __syncthreads();
    if (threadIdx.x == 0 && block_best) atomicMax(best, block_best);
}

thread_local float g_inflate_kernel_ms = 0.0f;            // k_bgzf_inflate of this thread's last gki_bgzf_inflate

}  // namespace

extern "C" {

int gki_bgzf_inflate(const void *d_in, int64_t n_in, const void *d_payload_start, const void *d_payload_len,
                     const void *d_crc32, const void *d_out_start, int64_t n_blocks, void *d_out, int64_t out_capacity,
                     int64_t *first_bad_block, int *first_bad_status) {
    if (first_bad_block) *first_bad_block = -1;
    if (first_bad_status) *first_bad_status = 0;
    if (n_blocks < 0 || n_in < 0 || out_capacity < 0) return gki_set_error(GKI_ERR_BAD_ARG, "bgzf_inflate: a negative size");
    if (n_blocks == 0) return GKI_OK;
    if (n_blocks > 0x7FFFFFFFll) return gki_set_error(GKI_ERR_BAD_ARG, "bgzf_inflate: %lld blocks are too many", (long long)n_blocks);
    if (!d_payload_start || !d_payload_len || !d_crc32 || !d_out_start || (n_in > 0 && !d_in) || (out_capacity > 0 && !d_out))
        return gki_set_error(GKI_ERR_BAD_ARG, "bgzf_inflate: a NULL array");
    InflateReport rep;
    TimerEvents ev;
    DevBuf report, status;
    g_inflate_kernel_ms = 0.0f;
    HIP_TRY(hipEventCreate(&ev.e0));
    HIP_TRY(hipEventCreate(&ev.e1));
    HIP_TRY(report.alloc(sizeof(InflateReport)));
    HIP_TRY(status.alloc((size_t)n_blocks));
    rep.first_bad = ~0ull; rep.invalid = 0; rep.pad = 0;
    HIP_TRY(hipMemcpy(report.get(), &rep, sizeof(rep), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_bgzf_validate, dim3(stream_grid(n_blocks, 256)), dim3(256), 0, 0, (const int64_t *)d_payload_start,
                       (const int32_t *)d_payload_len, (const int64_t *)d_out_start, n_blocks, n_in, out_capacity,
                       report.get<InflateReport>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&rep, report.get(), sizeof(rep), hipMemcpyDeviceToHost));
    if (rep.invalid)
        return gki_set_error(GKI_ERR_BAD_ARG, "bgzf_inflate: a payload outside the %lld input bytes, or an output range that is "
                             "decreasing, above 65536 bytes or outside the capacity of %lld", (long long)n_in, (long long)out_capacity);
    HIP_TRY(hipMemsetAsync(status.get(), 0, (size_t)n_blocks, 0));
    HIP_TRY(hipEventRecord(ev.e0, 0));
    hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)n_blocks), dim3(INFLATE_BLOCK), 0, 0,
                       (const uint8_t *)d_in, (const int64_t *)d_payload_start, (const int32_t *)d_payload_len,
                       (const uint32_t *)d_crc32, (const int64_t *)d_out_start, n_blocks, (uint8_t *)d_out, status.get<uint8_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e1, 0));
    hipLaunchKernelGGL(k_bgzf_first_bad, dim3(stream_grid(n_blocks, 256)), dim3(256), 0, 0, status.get<const uint8_t>(), n_blocks,
                       report.get<InflateReport>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&rep, report.get(), sizeof(rep), hipMemcpyDeviceToHost));
    HIP_TRY(hipEventElapsedTime(&g_inflate_kernel_ms, ev.e0, ev.e1));
    if (rep.first_bad == ~0ull) return GKI_OK;
    uint8_t st = 0;
    HIP_TRY(hipMemcpy(&st, status.get<const uint8_t>() + rep.first_bad, 1, hipMemcpyDeviceToHost));
    if (first_bad_block) *first_bad_block = (int64_t)rep.first_bad;
    if (first_bad_status) *first_bad_status = (int)st;
    return gki_set_error(GKI_ERR_INFLATE, "bgzf_inflate: block %lld does not inflate (status %d)", (long long)rep.first_bad, (int)st);
}

int gki_bgzf_inflate_kernel_ms(float *ms) {
    if (ms == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "bgzf_inflate_kernel_ms: ms is NULL");
    *ms = g_inflate_kernel_ms;
    return GKI_OK;
}

int gki_last_byte_position(const void *d_bytes, int64_t n_bytes, int value, int64_t *position) {
    if (position == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "last_byte_position: position is NULL");
    *position = -1;
    if (n_bytes < 0 || value < 0 || value > 255) return gki_set_error(GKI_ERR_BAD_ARG, "last_byte_position: n_bytes or value out of range");
    if (n_bytes == 0) return GKI_OK;
    if (d_bytes == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "last_byte_position: d_bytes is NULL");
    DevBuf best;
    HIP_TRY(best.alloc(8));
    HIP_TRY(hipMemset(best.get(), 0, 8));
    // windows from the end, each four times the last: the byte looked for is a line end, so the first window has one
    int64_t end = n_bytes, window = 1 << 20;
    while (end > 0) {
        const int64_t begin = end > window ? end - window : 0;
        unsigned long long found = 0ull;
        hipLaunchKernelGGL(k_last_byte, dim3(stream_grid(end - begin, 256)), dim3(256), 0, 0, (const uint8_t *)d_bytes, begin, end,
                           value, best.get<unsigned long long>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(&found, best.get(), 8, hipMemcpyDeviceToHost));
        if (found) { *position = (int64_t)found - 1; break; }
        end = begin;
        window *= 4;
    }
    return GKI_OK;
}

}  // extern "C"
