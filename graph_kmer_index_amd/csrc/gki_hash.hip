// Hash kernels outside the graph walk: k-windows of a plain sequence (A1/A4), read k-mers (A10),
// reverse complement / complement of hashes (A8).
// Launches: k_hash_windows; k_read_counts, then k_hash_reads<STRAND> -- the walk of gki_read_windows.h with HashSink as
// its sink, the same walk k_probe_reads probes from; k_complement<REVERSE>.
#include "gki_read_windows.h"

namespace {

__global__ __launch_bounds__(256) void k_hash_windows(const uint64_t *__restrict__ seq2, int64_t n_out, int k,
                                                      uint64_t *__restrict__ out) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += stride)
        out[i] = gki_extract(seq2, i, k);
}

template <bool REVERSE>
__global__ __launch_bounds__(256) void k_complement(const uint64_t *__restrict__ in, int64_t n, int k,
                                                    uint64_t *__restrict__ out) {
    const uint64_t mask = (1ull << (2 * k)) - 1ull;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint64_t x = in[i];
        out[i] = REVERSE ? gki_revcomp(x & mask, k) : (~x & mask);
    }
}

// cnt is 32 bits wide: a read with more k-mers than that is flagged (as k_parse_classify flags a line of 2^32 letters)
// and the call refused, instead of its count stored modulo 2^32
__global__ __launch_bounds__(256) void k_read_counts(const int64_t *__restrict__ read_start, int64_t n_reads, int k,
                                                     uint32_t *__restrict__ cnt, unsigned int *__restrict__ too_long) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        int64_t len = read_start[r + 1] - read_start[r];
        int64_t c = len >= k ? len - k + 1 : 0;
        if (c > 0xFFFFFFFFll) { atomicOr(too_long, 1u); c = 0; }
        cnt[r] = (uint32_t)c;
    }
}

// The walk's sink that stores: strand 0 writes window j's forward k-mer at o[j]; strand 1 hashes
// str(Seq(read).reverse_complement()) (read_kmers.py:23-26), whose window n_out - 1 - j is the reverse complement of
// forward window j, other letters than ACGT staying 0 -- the walk's rc word.
template <int STRAND>
struct HashSink {
    static constexpr bool NEEDS_FW = STRAND == 0, NEEDS_RC = STRAND == 1;
    const int64_t *__restrict__ out_start;
    uint64_t *__restrict__ out;
    uint64_t *o = nullptr;
    __device__ __forceinline__ void begin(int64_t r) { o = out + out_start[r]; }
    __device__ __forceinline__ void window(bool active, int64_t j, int64_t n_out, uint64_t fw, uint64_t rc) {
        if (active) o[STRAND ? n_out - 1 - j : j] = STRAND ? rc : fw;
    }
    __device__ __forceinline__ void finish() {}
};

template <int STRAND>
__global__ __launch_bounds__(256) void k_hash_reads(const uint8_t *__restrict__ reads,
                                                    const int64_t *__restrict__ read_start, int64_t n_reads, int k,
                                                    const int64_t *__restrict__ out_start,
                                                    uint64_t *__restrict__ out) {
    HashSink<STRAND> sink{out_start, out};
    walk_span_windows(reads, ReadSpans{read_start}, n_reads, k, sink);
}

}  // namespace

extern "C" {

int gki_hash_sequence(const void *d_codes, int64_t n, int k, void *d_out) {
    GKI_TRY(gki_check_k(k));
    if (n < k) return GKI_OK;
    int64_t n_u64 = ceil_div(n, 32) + 2;
    DevBuf seq2;
    HIP_TRY(seq2.alloc((size_t)n_u64 * 8));
    HIP_TRY(hipMemsetAsync(seq2.get(), 0, (size_t)n_u64 * 8, 0));
    GKI_TRY(gki_launch_pack((const uint8_t *)d_codes, n, seq2.get<uint32_t>(), 0));
    int64_t n_out = n - k + 1;
    hipLaunchKernelGGL(k_hash_windows, dim3(stream_grid(n_out, 256)), dim3(256), 0, 0, seq2.get<const uint64_t>(), n_out, k,
                       (uint64_t *)d_out);
    if (hipGetLastError() != hipSuccess) return gki_set_error(GKI_ERR_HIP, "k_hash_windows launch failed");
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

int gki_hash_reads(const void *d_reads, const void *d_read_start, int64_t n_reads, int k, int strand,
                   void *d_out_start, void *d_out, int64_t out_capacity, int64_t *n_out) {
    *n_out = 0;
    GKI_TRY(gki_check_k(k));
    if (strand != 0 && strand != 1) return gki_set_error(GKI_ERR_BAD_ARG, "strand must be 0 or 1");
    if (n_reads <= 0) { HIP_TRY(hipMemset(d_out_start, 0, 8)); return GKI_OK; }
    int64_t total = 0;
    {
        DevBuf cnt, tmp, flag;                         // freed before the hashing pass
        int64_t tmp_bytes = gki_scan_tmp_bytes(n_reads);
        unsigned int too_long = 0;
        HIP_TRY(cnt.alloc((size_t)n_reads * 4));
        HIP_TRY(tmp.alloc((size_t)tmp_bytes));
        HIP_TRY(flag.alloc(4));
        HIP_TRY(hipMemsetAsync(flag.get(), 0, 4, 0));
        hipLaunchKernelGGL(k_read_counts, dim3(stream_grid(n_reads, 256)), dim3(256), 0, 0, (const int64_t *)d_read_start,
                           n_reads, k, cnt.get<uint32_t>(), flag.get<unsigned int>());
        HIP_TRY(hipGetLastError());
        GKI_TRY(gki_scan_u32_to_i64(cnt.get<const uint32_t>(), n_reads, (int64_t *)d_out_start, tmp.get(), tmp_bytes, 0));
        HIP_TRY(hipMemcpy(&total, (const int64_t *)d_out_start + n_reads, 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&too_long, flag.get(), 4, hipMemcpyDeviceToHost));
        if (too_long) return gki_set_error(GKI_ERR_BAD_ARG, "hash_reads: a read of more than 2^32 - 1 k-mers");
    }
    *n_out = total;
    if (d_out == nullptr) return GKI_OK;               // count only
    if (total > out_capacity) return gki_set_error(GKI_ERR_BAD_ARG, "hash_reads: output needs %lld entries, capacity %lld",
                                                   (long long)total, (long long)out_capacity);
    auto *kernel = strand == 0 ? k_hash_reads<0> : k_hash_reads<1>;
    hipLaunchKernelGGL(kernel, dim3(span_grid(n_reads)), dim3(256), 0, 0, (const uint8_t *)d_reads,
                       (const int64_t *)d_read_start, n_reads, k, (const int64_t *)d_out_start, (uint64_t *)d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

int gki_reverse_complement(const void *d_in, int64_t n, int k, void *d_out) {
    GKI_TRY(gki_check_k(k));                           // kmer_hashing.py:25
    if (n <= 0) return GKI_OK;
    hipLaunchKernelGGL(k_complement<true>, dim3(stream_grid(n, 256)), dim3(256), 0, 0, (const uint64_t *)d_in, n, k,
                       (uint64_t *)d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

int gki_complement(const void *d_in, int64_t n, int k, void *d_out) {
    GKI_TRY(gki_check_k(k));
    if (n <= 0) return GKI_OK;
    hipLaunchKernelGGL(k_complement<false>, dim3(stream_grid(n, 256)), dim3(256), 0, 0, (const uint64_t *)d_in, n, k,
                       (uint64_t *)d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

}  // extern "C"
