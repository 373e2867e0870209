// The read side's walk, written once: the letters of a span become its forward and reverse-complement k-mers, window by
// window, and a SINK says what happens to them.  k_hash_reads (gki_hash.hip) stores them, k_probe_reads and
// k_probe_segments (gki_probe.hip) probe the index with them; k_pack_letters (gki_linear.hip) shares the letter rule.
#pragma once
#include "gki_common.h"

// ---------------------------------------------------------------------------------- the letter rule
// c/g/t in either case are 1/2/3, every other byte -- a, n, and whatever else a file holds -- is 0
// (flat_kmers.py:134-145, read_kmers.py:67-70)
__device__ __forceinline__ uint32_t letter_code(uint32_t byte) {
    const uint32_t ch = byte | 0x20u;
    return (ch == 'c') + 2u * (ch == 'g') + 3u * (ch == 't');            // a sum, not a chain of ?: -- no branches
}
// only these have a complement: on the reverse strand every other letter stays 0 (Bio.Seq maps N to N)
__device__ __forceinline__ bool letter_is_acgt(uint32_t byte) { return (byte | 0x20u) == 'a' || letter_code(byte) != 0u; }

// Every bit of a wave-uniform x twice: bit i goes to bits 2i and 2i + 1, in ONE scalar instruction.  It turns a bit plane
// of 32 letters into their places in the 2-bit stream; the same spread in shifts and masks is fifteen instructions a plane.
__device__ __forceinline__ uint64_t bits_doubled(uint32_t x) {
    uint64_t y;
    asm("s_bitreplicate_b64_b32 %0, %1" : "=s"(y) : "s"(x));
    return y;
}
// the 2-bit codes of 32 letters from the planes of their low and high bits
__device__ __forceinline__ uint64_t interleaved(uint32_t lo, uint32_t hi) {
    return (bits_doubled(lo) & 0x5555555555555555ull) | (bits_doubled(hi) & 0xAAAAAAAAAAAAAAAAull);
}

// ---------------------------------------------------------------------------------- spans
// `spans` says where span r lies in the letters: spans.at(r, &s, &len).  A read is [read_start[r], read_start[r + 1]); a
// segment is seg_windows[r] windows from seg_start[r] on, and segments may overlap one another in the letters.
struct ReadSpans {
    const int64_t *__restrict__ read_start;
    __device__ __forceinline__ void at(int64_t r, int64_t *s, int64_t *len) const {
        *s = read_start[r];
        *len = read_start[r + 1] - *s;
    }
};

// Whatever the arrays hold, [s, s + len) lies inside [0, n_letters): a segment that does not is cut to what does, and
// *fault is raised for the entry to report.
struct SegmentSpans {
    const int64_t *__restrict__ seg_start, *__restrict__ seg_windows;
    int64_t n_letters;
    int k;
    unsigned long long *__restrict__ fault;
    __device__ __forceinline__ void at(int64_t r, int64_t *s, int64_t *len) const {
        const int64_t a = seg_start[r], w = seg_windows[r];
        const int64_t a_in = a < 0 ? 0 : a > n_letters ? n_letters : a;
        const int64_t w_in = w < 0 ? 0 : w > n_letters ? n_letters : w;      // w_in + k - 1 cannot overflow
        const int64_t want = w_in > 0 ? w_in + (k - 1) : 0, room = n_letters - a_in;
        if (a != a_in || w != w_in || want > room) atomicOr(fault, 1ull);
        *s = a_in;
        *len = want < room ? want : room;
    }
};

// One wave per span: workgroups of 256 threads are 4 waves, at most 256 * 8 of them; the waves stride over the spans.
static inline int span_grid(int64_t n_spans) { return stream_grid(n_spans, 4); }

// The argument checks of every entry that takes k, and of those that take a strand mask as well
static inline int gki_check_k(int k) {
    return k < 1 || k > GKI_MAX_K ? gki_set_error(GKI_ERR_BAD_ARG, "k must be in 1..31") : GKI_OK;
}
static inline int gki_check_k_strands(int k, int strands) {
    GKI_TRY(gki_check_k(k));
    return strands < 1 || strands > 3 ? gki_set_error(GKI_ERR_BAD_ARG, "strands must be 1 (forward), 2 (reverse) or 3 (both)") : GKI_OK;
}

// ---------------------------------------------------------------------------------- the walk
// One wave per span, wave-strided.  Forward k-mer of window j: bases j..j+k-1, first base least significant
// (read_kmers.py:70).  Reverse strand (read_kmers.py:23-26): the k-mers of str(Seq(read).reverse_complement()) are, window
// by window, the reverse complements of the forward windows in reverse order, with non-ACGT letters hashing as 0 on both
// strands: code' = acgt ? 3 - code : 0, window reversed.
//
// The 64 letters of a step become wave-uniform bit planes (__ballot) and are interleaved ONCE per step into the 2-bit
// stream (scalar work): C0,C1 = this step's 64 bases, N0,N1 = the next step's.  A lane's window is then one funnel shift
// of that stream, and its reverse complement a complement + bit reversal of the same word under the ACGT mask.
// Letters are fetched one step ahead (the next 64 letters of this span, or the first 64 of the wave's next span) so that
// their latency hides behind what the sink does with the current step.
//
// The sink:
//   static constexpr bool NEEDS_FW, NEEDS_RC   which of the two words it reads; the other is passed as 0 and costs nothing
//   begin(r)                                   before the first step of a span that has windows
//   window(active, j, n_out, fw, rc)           window j of the span's n_out, active = j < n_out
//   finish()                                   after the wave's last span
// EVERY call is wave-uniform: all 64 lanes make it, the inactive ones too, so a sink may use ballots (the probe sink's
// candidate queue does).
template <class Spans, class Sink>
__device__ __forceinline__ void walk_span_windows(const uint8_t *__restrict__ letters, const Spans &spans, int64_t n_spans, int k,
                                                  Sink &sink) {
    static_assert(Sink::NEEDS_FW || Sink::NEEDS_RC, "a sink reads at least one of the two words");
    const int lane = threadIdx.x & 63;
    // the wave's number in a scalar register (it fits 32 bits: a grid has at most 2048 * 4 waves), so that the span
    // bookkeeping below is scalar work
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t kmask2 = (1ull << (2 * k)) - 1ull;
    int64_t r = wave, s = 0, len = 0;
    if (r < n_spans) spans.at(r, &s, &len);
    unsigned ch_next = lane < len ? letters[s + lane] : 0u;
    while (r < n_spans) {
        const int64_t rn = r + n_waves;
        int64_t sn = 0, lenn = 0;
        if (rn < n_spans) spans.at(rn, &sn, &lenn);
        const int64_t n_out = len - k + 1;
        if (n_out <= 0) {
            ch_next = lane < lenn ? letters[sn + lane] : 0u;
        } else {
            sink.begin(r);
            uint64_t C0 = 0, C1 = 0, Cm0 = 0, Cm1 = 0;
            // step c loads letters [64c, 64c + 64) and puts out windows [64(c - 1), 64c); `left` = n_out - 64(c - 1)
            // windows are not out before it (kept beside c so that the loop's tests compare a scalar with a constant)
            int64_t c = 0;
            for (int64_t left = n_out + 64; left > 0; left -= 64, c++) {
                // this step's letters become bit planes first: `ch` is dead before the next step's are asked for
                const unsigned ch = ch_next;                             // 0 (past the end): code 0, not ACGT
                const unsigned code = letter_code(ch);
                const uint64_t lo = __ballot(code & 1u), hi = __ballot(code & 2u);
                const uint64_t ok = Sink::NEEDS_RC ? __ballot(letter_is_acgt(ch)) : 0ull;
                // ONE load whichever span it reads, asked for before the sink works and first used at the next step's top
                const bool last = left <= 64;                            // no further step for this span
                const int64_t from = last ? sn : s + (c + 1) * 64, room = last ? lenn : len - (c + 1) * 64;
                ch_next = lane < room ? letters[from + lane] : 0u;
                const uint64_t N0 = interleaved((uint32_t)lo, (uint32_t)hi), N1 = interleaved((uint32_t)(lo >> 32), (uint32_t)(hi >> 32));
                const uint64_t Nm0 = bits_doubled((uint32_t)ok), Nm1 = bits_doubled((uint32_t)(ok >> 32));    // 3 where a letter is ACGT
                if (c > 0) {
                    const int64_t j = (c - 1) * 64 + lane;
                    const int sh = (lane & 31) * 2;
                    const bool up = lane >= 32;
                    const uint64_t a = up ? C1 : C0, b = up ? N0 : C1;
                    const uint64_t fw = ((a >> sh) | ((b << 1) << (63 - sh))) & kmask2;
                    uint64_t rc = 0;
                    if (Sink::NEEDS_RC) {
                        const uint64_t am = up ? Cm1 : Cm0, bm = up ? Nm0 : Cm1;
                        const uint64_t m = ((am >> sh) | ((bm << 1) << (63 - sh))) & kmask2;
                        rc = __brevll(~fw & m) >> (64 - 2 * k);          // bases reversed, the two bits of a base swapped
                        rc = ((rc & 0x5555555555555555ull) << 1) | ((rc >> 1) & 0x5555555555555555ull);
                    }
                    sink.window(j < n_out, j, n_out, Sink::NEEDS_FW ? fw : 0ull, rc);
                }
                C0 = N0; C1 = N1; Cm0 = Nm0; Cm1 = Nm1;
            }
        }
        r = rn; s = sn; len = lenn;
    }
    sink.finish();
}
