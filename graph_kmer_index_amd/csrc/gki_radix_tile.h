// The tile ranking core of the stable radix passes, and one LSD pass over 8-byte items built on it.  Device-only.
//
//   same_digit_lanes, wave_rank, block_excl, rank_tile, tile_slot
//                         every row's slot in its tile sorted stably by digit.  Users: the partition passes and the finish of
//                         the row-carrying index build (gki_index_rows.hip, up to 1024 digits) and the pass below
//   radix_tile_hist, radix_tile_scatter
//                         the two launches of one 8-bit pass over a tile of THREADS * RI 8-byte items.  What an item is lives
//                         in a traits type: the (key, index) pairs of the pair-sorting index build (gki_index.hip) and the
//                         64-bit keys of the k-mer counter (gki_count.hip)
//
// Everything is __forceinline__ and takes its pointers by value: a struct of pointers that a kernel hands on by reference
// escapes to memory and every load through it becomes a FLAT load (gki_finder.hip, WalkSrc).
#pragma once
#include "gki_common.h"

// The lanes of the wave that are valid and hold the same `bits`-bit digit as this lane (a ballot per bit).  An invalid lane
// is in nobody's mask whatever its digit; its own result means nothing.
__device__ __forceinline__ uint64_t same_digit_lanes(uint32_t dig, int bits, bool valid) {
    uint64_t same = __ballot(valid);
    for (int b = 0; b < bits; b++) {
        const uint64_t bit = __ballot((dig >> b) & 1u);
        same &= ((dig >> b) & 1u) ? bit : ~bit;
    }
    return same;
}

// Exclusive scan of v over the THREADS threads of the block (lds: THREADS / 64 + 1 words)
template <int THREADS>
__device__ __forceinline__ uint32_t block_excl(uint32_t v, uint32_t *lds, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t inc = gki_wave_incl_sum(v);
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    uint32_t woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; w++) { const uint32_t c = lds[w]; if (w < wave) woff += c; tot += c; }
    __syncthreads();
    *total = tot;
    return woff + inc - v;
}

// Rank of every element among the earlier elements of its wave with the same digit, and the wave's digit counts.
// Element order inside a tile is (wave, round, lane): wave w owns a contiguous slice, round r its r-th group of 64.
template <int RI>
__device__ __forceinline__ void wave_rank(const uint32_t (&dig)[RI], const bool (&valid)[RI], int bits, uint16_t *wcnt /* this wave's [bins] */,
                                          uint32_t (&rank)[RI]) {
    const int lane = threadIdx.x & 63;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < RI; r++) {
        const uint32_t d = dig[r];
        const uint64_t same = same_digit_lanes(d, bits, valid[r]);
        const uint32_t before = (uint32_t)__popcll(same & lt_mask);
        uint32_t prev = 0;
        if (valid[r]) prev = wcnt[d];                       // all lanes of the group read the same value ...
        rank[r] = prev + before;
        if (valid[r] && before == 0) wcnt[d] = (uint16_t)(prev + (uint32_t)__popcll(same));   // ... then its first lane publishes
        __builtin_amdgcn_wave_barrier();                    // (rounds are sequential per wave)
    }
}

// Ranks inside the wave, digit counts per wave (s_wcnt[W][MAXB], zeroed a barrier ago; MAXB: the most digits a pass of the
// caller has); then per digit: exclusive offsets over the waves (left in s_wcnt), the digit's start in the sorted tile
// (s_dstart) and, by run_to(digit, that start), where its run goes.  Ends on a barrier.
template <int THREADS, int RI, class RunTo, int MAXB>
__device__ __forceinline__ void rank_tile(const uint32_t (&dig)[RI], const bool (&valid)[RI], int bits, uint16_t (*s_wcnt)[MAXB],
                                          uint32_t *s_dstart, uint32_t *s_scan, uint32_t (&rank)[RI], RunTo run_to) {
    constexpr int W = THREADS / 64;
    const int bins = 1 << bits;
    wave_rank<RI>(dig, valid, bits, s_wcnt[threadIdx.x >> 6], rank);
    __syncthreads();
    constexpr int C = MAXB / THREADS > 0 ? MAXB / THREADS : 1;      // digits per thread
    uint32_t tot[C], sum = 0;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int d = threadIdx.x * C + c;
        tot[c] = 0;
        if (d < bins) {
            uint32_t run = 0;
#pragma unroll
            for (int w = 0; w < W; w++) { const uint32_t x = s_wcnt[w][d]; s_wcnt[w][d] = (uint16_t)run; run += x; }
            tot[c] = run;
        }
        sum += tot[c];
    }
    uint32_t total;
    uint32_t ex = block_excl<THREADS>(sum, s_scan, &total);
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int d = threadIdx.x * C + c;
        if (d < bins) {
            s_dstart[d] = ex;
            run_to(d, ex);
            ex += tot[c];
        }
    }
    __syncthreads();
}
// The slot of a row in the sorted tile: the start of its digit, the rows of the digit in earlier waves, its rank in its own
__device__ __forceinline__ uint32_t tile_slot(const uint32_t *s_dstart, const uint16_t *wcnt /* this wave's */, uint32_t dig, uint32_t rank) {
    return s_dstart[dig] + wcnt[dig] + rank;
}

// ------------------------------------------------------------------------------------ one LSD pass over 8-byte items
// A pass sorts stably on one 8-bit digit: tile histograms (bin-major: hist[bin * n_tiles + tile]) -> the caller's exclusive
// scan of them -> scatter.  Items says what is sorted:
//   Offset                        what the scan leaves: uint32_t, or int64_t for more items than 32 bits count
//   uint64_t load_key(int64_t i)  the sort key of item i of the pass's input, alone (the histogram reads nothing else)
//   uint64_t load(int64_t i)      item i
//   void store(int64_t i, item)   an item to position i of the pass's output
//   uint32_t digit(item, shift)   the pass's digit of an item, or of a key alone
constexpr int RADIX_BITS = 8, RADIX_BINS = 1 << RADIX_BITS;

// A tile's digit histogram.  Returns the OR of the keys this thread counted (for a caller that bounds its keys).
template <int THREADS, int RI, class Items>
__device__ __forceinline__ uint64_t radix_tile_hist(const Items in, int64_t n, int shift, uint32_t *__restrict__ hist, int64_t n_tiles) {
    static_assert(THREADS == RADIX_BINS, "one thread per digit");
    __shared__ uint32_t h[RADIX_BINS];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * (THREADS * RI);
    uint64_t acc = 0;
#pragma unroll
    for (int r = 0; r < RI; r++) {
        const int64_t i = base + r * THREADS + threadIdx.x;
        if (i < n) {
            const uint64_t key = in.load_key(i);
            acc |= key;
            atomicAdd(&h[Items::digit(key, shift)], 1u);
        }
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
    return acc;
}

// Stable scatter of one tile: load -> rank_tile -> tile_slot -> the tile sorted by digit in LDS -> every digit's run leaves
// as one contiguous store, to offs[digit * n_tiles + tile] onwards.
template <int THREADS, int RI, class Items>
__device__ __forceinline__ void radix_tile_scatter(const Items io, int64_t n, int shift, const typename Items::Offset *__restrict__ offs,
                                                   int64_t n_tiles) {
    constexpr int TILE = THREADS * RI, W = THREADS / 64, SLICE = TILE / W;
    __shared__ uint16_t s_wcnt[W][RADIX_BINS];  // per wave, per digit: running count (<= SLICE), then exclusive offset
    __shared__ uint32_t s_dstart[RADIX_BINS];   // start of each digit's run in the locally sorted tile
    __shared__ uint32_t s_scan[W + 1];
    __shared__ uint64_t s_items[TILE];
    static_assert(SLICE <= 65535, "a wave's digit counts are 16 bits wide");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < W * RADIX_BINS / 2; i += THREADS) reinterpret_cast<uint32_t *>(s_wcnt)[i] = 0;
    __syncthreads();
    const int64_t tile_base = (int64_t)blockIdx.x * TILE;
    const int n_here = (int)((n - tile_base) < TILE ? (n - tile_base) : TILE);
    uint64_t item[RI];
    uint32_t dig[RI], rank[RI];
    bool valid[RI];
#pragma unroll
    for (int r = 0; r < RI; r++) {
        const int e = wave * SLICE + r * 64 + lane;
        valid[r] = e < n_here;
        item[r] = valid[r] ? io.load(tile_base + e) : 0ull;
        dig[r] = valid[r] ? Items::digit(item[r], shift) : 0u;
    }
    rank_tile<THREADS, RI>(dig, valid, RADIX_BITS, s_wcnt, s_dstart, s_scan, rank, [](int, uint32_t) {});
    // The digit is taken from the item again, and the item made opaque first: left to itself the compiler keeps every
    // round's digit and the address of its count alive across the ranking to save three instructions per item (115 VGPRs
    // against 94)
#pragma unroll
    for (int r = 0; r < RI; r++) {
        asm volatile("" : "+v"(item[r]));
        if (valid[r]) s_items[tile_slot(s_dstart, s_wcnt[wave], Items::digit(item[r], shift), rank[r])] = item[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RI; r++) {
        const int p = r * THREADS + threadIdx.x;
        if (p < n_here) {
            const uint64_t it = s_items[p];
            const uint32_t d = Items::digit(it, shift);
            io.store((int64_t)offs[(int64_t)d * n_tiles + blockIdx.x] + (int64_t)(p - (int)s_dstart[d]), it);
        }
    }
}
