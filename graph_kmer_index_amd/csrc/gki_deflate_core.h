// Deflate of ONE BGZF member (RFC 1951 / RFC 1952: at most 0xff00 input bytes, no dictionary) as plain C++ pieces: the
// same text is the body of the kernel (csrc/gki_bgzf_deflate.hip), which supplies the parallel schedule and the barriers,
// and of a stand-alone host program (tests/deflate_core_main.cpp), which drives the same pieces over the same rounds and
// segments in the same order and so writes the same bytes.  GKI_DEF_HD is __host__ __device__ under hipcc and nothing
// elsewhere.
//
// The schedule both follow, per member of n bytes (a "segment" and a "round" are both GKI_DEF_SEG = 256 positions):
//   1  CRC-32 per segment from a zero register, each multiplied by x^(8 * bytes behind it) and all of them xor-ed
//   2  candidates in rounds: every position of a round looks its 4-byte hash up in `head` (the most recent position of
//      EARLIER rounds), then -- behind a barrier -- looks among the earlier positions of its own round (their hashes are
//      in `rh`), inserts itself with a max, and measures the match against its one candidate.  The candidate is therefore
//      the most recent earlier position with the same hash, whatever the round size or the schedule; pm[p] = length << 16
//      | distance - 1 (0: no match)
//   3  a greedy walk per segment over pm, matches clipped at the segment's end: symbol counts (sums: order-free)
//   4  length-limited codes from the counts (rank by (count, symbol), Moffat-Katajainen lengths, Kraft repair), the
//      dynamic header (repeat codes 16/17/18, code-length code limited to 7), its size
//   5  the same walk for each segment's bits, a scan of them, dynamic against stored by size
//   6  the same walk once more, emitting at the segment's bit offset into zeroed 32-bit words: a word all of whose bits
//      are one emitter's is stored, a word shared between emitters is or-ed (order-free)
//
// Bounds: every read of the input is below n, every pm access below n, every table index is masked or comes from a value
// the code itself keeps in range (symbols < 286 / 30 / 19), and the emitter writes no word at or above its n_words.  Every
// loop runs over a range fixed by n or by a table's size.
#pragma once
#include <stdint.h>
#include <string.h>

#include "gki_inflate_core.h"

#define GKI_DEF_HD GKI_INFLATE_HD

#define GKI_DEF_SEG 256                 // positions per segment and per round (and the kernel's threads)
#define GKI_DEF_MAX_IN 0xff00           // input bytes of a member, at most
#define GKI_DEF_HASH_BITS 13
#define GKI_DEF_HASH_SIZE (1 << GKI_DEF_HASH_BITS)
#define GKI_DEF_NO_HASH 0xFFFFu
#define GKI_DEF_MIN_MATCH 4             // what a candidate must reach (a clipped match may be 3)
#define GKI_DEF_FAR 4096                // a match of GKI_DEF_MIN_MATCH further away than this is not taken
#define GKI_DEF_MAX_MATCH 258
#define GKI_DEF_MAX_DIST 32768
#define GKI_DEF_LCODES 286
#define GKI_DEF_DCODES 30
#define GKI_DEF_CCODES 19
#define GKI_DEF_MEMBER_HEAD 18          // gzip header with the 'BC' subfield
#define GKI_DEF_MEMBER_EXTRA 31         // a member is at most its input + 18 + 5 (stored block) + 8
#define GKI_DEF_MAX_MEMBER (GKI_DEF_MAX_IN + GKI_DEF_MEMBER_EXTRA)

// sums, maxima and ors that several lanes make into one word: atomics on the device, plain on the host (one thread)
#if defined(__HIP_DEVICE_COMPILE__)
#define GKI_DEF_ADD32(p, v) ((void)atomicAdd((p), (v)))
#define GKI_DEF_MAX32(p, v) ((void)atomicMax((p), (v)))
#define GKI_DEF_OR32(p, v) ((void)atomicOr((p), (v)))
#define GKI_DEF_XOR32(p, v) ((void)atomicXor((p), (v)))
#else
#define GKI_DEF_ADD32(p, v) ((void)(*(p) += (v)))
#define GKI_DEF_MAX32(p, v) ((void)(*(p) = *(p) > (v) ? *(p) : (v)))
#define GKI_DEF_OR32(p, v) ((void)(*(p) |= (v)))
#define GKI_DEF_XOR32(p, v) ((void)(*(p) ^= (v)))
#endif

// a member's working state: LDS in the kernel (about 40 KiB), a heap block on the host
struct gki_def_state {
    uint32_t head[GKI_DEF_HASH_SIZE];             // hash -> position + 1 of its most recent occurrence in earlier rounds
    uint32_t crc_table[256];
    uint32_t lfreq[288], dfreq[32], cfreq[20];    // symbol counts: literal/length, distance, code-length code
    uint32_t lwork[288], dwork[32], cwork[20];    // the counts in rank order, then the lengths in rank order
    uint32_t seg_bits[GKI_DEF_SEG];               // a segment's bits, then the bit of the member its first one goes to
    uint16_t lorder[288], dorder[32], corder[20]; // rank -> symbol
    uint16_t lcode[288], dcode[32], ccode[20];    // the codes, bit-reversed: the first bit to emit lowest
    uint16_t rh[GKI_DEF_SEG];                     // the hashes of the round in progress
    uint8_t llen[288], dlen[32], clen[20];        // code lengths
    uint8_t cl_sym[320], cl_extra[320];           // the header's code-length symbols and their extra bits
    int32_t n_cl, hlit, hdist, hclen;
    uint32_t crc;                                 // the xor of the segments' shifted registers
    uint32_t header_bits;                         // block header and code lengths of the dynamic block
    uint32_t end_bit;                             // the bit of the member behind the end-of-block symbol
    uint32_t member_bytes;
    int32_t stored;
};

// ---------------------------------------------------------------- CRC-32 in segments
// the register after the bytes [begin, end) from a register of 0, with no final complement
static inline GKI_DEF_HD uint32_t gki_def_crc_segment(const uint32_t *table, const uint8_t *in, int begin, int end) {
    uint32_t c = 0;
    for (int i = begin; i < end; i++) c = table[(c ^ in[i]) & 0xFFu] ^ (c >> 8);
    return c;
}

// a * b mod the CRC polynomial, both reflected (bit 31 is x^0)
static inline GKI_DEF_HD uint32_t gki_def_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}

// c * x^(8 * n_bytes): the register c after n_bytes zero bytes
static inline GKI_DEF_HD uint32_t gki_def_crc_shift(uint32_t c, uint32_t n_bytes) {
    uint32_t q = 0x00800000u;                                  // x^8
    for (int i = 0; i < 17 && n_bytes; i++, n_bytes >>= 1) {   // n_bytes <= 0xff00 < 2^17
        if (n_bytes & 1u) c = gki_def_crc_mul(c, q);
        q = gki_def_crc_mul(q, q);
    }
    return c;
}

static inline GKI_DEF_HD void gki_def_crc_add_segment(gki_def_state &st, const uint8_t *in, int n, int begin, int end) {
    const uint32_t c = gki_def_crc_shift(gki_def_crc_segment(st.crc_table, in, begin, end), (uint32_t)(n - end));
    if (c) GKI_DEF_XOR32(&st.crc, c);
}

// gzip's CRC-32 of the n bytes whose segments were added: the initial register of all ones, carried through n bytes
static inline GKI_DEF_HD uint32_t gki_def_crc_finish(uint32_t acc, int n) {
    return acc ^ gki_def_crc_shift(0xFFFFFFFFu, (uint32_t)n) ^ 0xFFFFFFFFu;
}

// ---------------------------------------------------------------- candidates and match lengths, in rounds
static inline GKI_DEF_HD uint32_t gki_def_load32(const uint8_t *p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

static inline GKI_DEF_HD uint32_t gki_def_hash(uint32_t four) { return (four * 2654435761u) >> (32 - GKI_DEF_HASH_BITS); }

// first half of a round for position p = round base + i: its hash goes to rh[i]; returns position + 1 of the most recent
// occurrence of the hash in earlier rounds, 0 when there is none or p has no four bytes left
static inline GKI_DEF_HD uint32_t gki_def_round_begin(gki_def_state &st, const uint8_t *in, int n, int p, int i) {
    uint32_t h = GKI_DEF_NO_HASH, cand1 = 0;
    if (p + 4 <= n) {
        h = gki_def_hash(gki_def_load32(in + p));
        cand1 = st.head[h];
    }
    st.rh[i & (GKI_DEF_SEG - 1)] = (uint16_t)h;
    return cand1;
}

// bytes that in[q..] and in[p..] share, at most max_len (q < p, p + max_len <= n)
static inline GKI_DEF_HD int gki_def_match_length(const uint8_t *in, int q, int p, int max_len) {
    int len = 0;
    while (len + 4 <= max_len) {
        const uint32_t x = gki_def_load32(in + q + len) ^ gki_def_load32(in + p + len);
        if (x) return len + (__builtin_ctz(x) >> 3);
        len += 4;
    }
    while (len < max_len && in[q + len] == in[p + len]) len++;
    return len;
}

// second half, behind a barrier: the nearest earlier position of this round with the hash replaces the candidate; p is
// inserted; the match is measured and pm[p] written
static inline GKI_DEF_HD void gki_def_round_end(gki_def_state &st, const uint8_t *in, int n, int p, int i, uint32_t cand1,
                                                uint32_t *pm) {
    if (p >= n) return;
    i &= GKI_DEF_SEG - 1;
    const uint32_t h = st.rh[i];
    uint32_t word = 0;
    if (h != GKI_DEF_NO_HASH) {
        for (int j = i - 1; j >= 0; j--)
            if (st.rh[j] == h) { cand1 = (uint32_t)(p - i + j) + 1u; break; }
        GKI_DEF_MAX32(&st.head[h & (GKI_DEF_HASH_SIZE - 1)], (uint32_t)p + 1u);
        if (cand1 != 0 && cand1 <= (uint32_t)p) {
            const int q = (int)cand1 - 1, dist = p - q;
            if (dist <= GKI_DEF_MAX_DIST) {
                const int max_len = n - p < GKI_DEF_MAX_MATCH ? n - p : GKI_DEF_MAX_MATCH;
                const int len = gki_def_match_length(in, q, p, max_len);
                if (len > GKI_DEF_MIN_MATCH || (len == GKI_DEF_MIN_MATCH && dist <= GKI_DEF_FAR))
                    word = (uint32_t)len << 16 | (uint32_t)(dist - 1);
            }
        }
    }
    pm[p] = word;
}

// ---------------------------------------------------------------- the token walk
// length 3..258 -> symbol - 257, extra bits and their value
static inline GKI_DEF_HD int gki_def_length_code(int len, int *ebits, uint32_t *extra) {
    if (len == 258) { *ebits = 0; *extra = 0; return 28; }
    const int l = len - 3;
    if (l < 8) { *ebits = 0; *extra = 0; return l; }
    const int e = 29 - __builtin_clz((uint32_t)l);              // floor(log2 l) - 2
    *ebits = e;
    *extra = (uint32_t)l & ((1u << e) - 1u);
    return 4 * e + 4 + ((l >> e) & 3);
}

// distance - 1 (0..32767) -> symbol, extra bits and their value
static inline GKI_DEF_HD int gki_def_dist_code(int d, int *ebits, uint32_t *extra) {
    if (d < 4) { *ebits = 0; *extra = 0; return d; }
    const int e = 30 - __builtin_clz((uint32_t)d);              // floor(log2 d) - 1
    *ebits = e;
    *extra = (uint32_t)d & ((1u << e) - 1u);
    return 2 * e + 2 + ((d >> e) & 1);
}

// The greedy parse of positions [begin, end) given pm: at a position with a match the match is taken, clipped at `end`
// (a rest below 3 is a literal), else the byte is a literal.  lit(byte) and match(length, distance - 1) see the tokens in
// order.  Every pass over a segment is this walk, so the three passes see the same tokens.
template <class L, class M>
static inline GKI_DEF_HD void gki_def_walk(const uint8_t *in, const uint32_t *pm, int begin, int end, L &&lit, M &&match) {
    int p = begin;
    while (p < end) {
        const uint32_t word = pm[p];
        int len = (int)(word >> 16);
        if (len > end - p) len = end - p;
        if (len >= 3) {
            match(len, (int)(word & 0xFFFFu));
            p += len;
        } else {
            lit(in[p]);
            p++;
        }
    }
}

static inline GKI_DEF_HD void gki_def_count_segment(gki_def_state &st, const uint8_t *in, const uint32_t *pm, int begin, int end) {
    gki_def_walk(in, pm, begin, end,
                 [&](uint8_t b) { GKI_DEF_ADD32(&st.lfreq[b], 1u); },
                 [&](int len, int d) {
                     int e; uint32_t x;
                     GKI_DEF_ADD32(&st.lfreq[257 + gki_def_length_code(len, &e, &x)], 1u);
                     GKI_DEF_ADD32(&st.dfreq[gki_def_dist_code(d, &e, &x) & 31], 1u);
                 });
}

// the end-of-block symbol, and a distance code set of at least two codes (what zlib's own deflate writes, and what every
// inflate takes: a complete set even when the block has no match, or one distinct distance)
static inline GKI_DEF_HD void gki_def_counts_finish(gki_def_state &st) {
    st.lfreq[256] += 1u;
    int used = 0, only = 0;
    for (int s = 0; s < GKI_DEF_DCODES; s++)
        if (st.dfreq[s]) { used++; only = s; }
    if (used == 0) { st.dfreq[0] = 1u; st.dfreq[1] = 1u; }
    else if (used == 1) st.dfreq[only == 0 ? 1 : 0] = 1u;
}

// ---------------------------------------------------------------- length-limited codes
// order[rank] = s for a symbol with a count: its rank among those by (count, symbol).  One call per symbol, in any order.
static inline GKI_DEF_HD void gki_def_rank_symbol(const uint32_t *freq, int n, int s, uint16_t *order) {
    const uint32_t f = freq[s];
    if (f == 0) return;
    int rank = 0;
    for (int j = 0; j < n; j++) {
        const uint32_t g = freq[j];
        rank += (g != 0 && (g < f || (g == f && j < s))) ? 1 : 0;
    }
    order[rank] = (uint16_t)s;
}

// Code lengths (at most max_bits) and codes of the n symbols from their counts and their rank order.  The lengths are
// those of a Huffman code (Moffat and Katajainen's in-place computation over the counts in rank order); where its depth
// exceeds max_bits the codes deeper than that are set to max_bits and the Kraft sum is repaired by lengthening the
// deepest code that is shorter, one step per unit of excess.  At least two symbols have counts.
static inline GKI_DEF_HD void gki_def_build_code(const uint32_t *freq, int n, int max_bits, const uint16_t *order,
                                                 uint32_t *a, uint8_t *len, uint16_t *code) {
    int m = 0;
    for (int s = 0; s < n; s++) { m += freq[s] != 0 ? 1 : 0; len[s] = 0; code[s] = 0; }
    if (m < 2) {                                              // not reached through gki_def_counts_finish; one bit each
        for (int s = 0; s < n; s++) if (freq[s]) len[s] = 1;
        return;
    }
    for (int i = 0; i < m; i++) a[i] = freq[order[i]];
    a[0] += a[1];
    int root = 0, leaf = 2, next;
    for (next = 1; next < m - 1; next++) {
        if (leaf >= m || a[root] < a[leaf]) { a[next] = a[root]; a[root++] = (uint32_t)next; } else a[next] = a[leaf++];
        if (leaf >= m || (root < next && a[root] < a[leaf])) { a[next] += a[root]; a[root++] = (uint32_t)next; } else a[next] += a[leaf++];
    }
    a[m - 2] = 0;
    for (next = m - 3; next >= 0; next--) a[next] = a[a[next]] + 1u;
    int avbl = 1, used = 0, dpth = 0;
    root = m - 2; next = m - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)a[root] == dpth) { used++; root--; }
        while (avbl > used) { a[next--] = (uint32_t)dpth; avbl--; }
        avbl = 2 * used; dpth++; used = 0;
    }
    // a[i]: the depth of the symbol of rank i, non-increasing in i.  Codes per length, the deep ones at max_bits:
    uint32_t count[16];
    for (int l = 0; l < 16; l++) count[l] = 0;
    for (int i = 0; i < m; i++) count[a[i] < (uint32_t)max_bits ? a[i] : (uint32_t)max_bits]++;
    uint32_t total = 0;
    for (int l = max_bits; l > 0; l--) total += count[l] << (max_bits - l);
    while (total > (1u << max_bits)) {                        // at most m steps: every step lowers the sum by one
        count[max_bits]--;
        for (int l = max_bits - 1; l > 0; l--)
            if (count[l]) { count[l]--; count[l + 1] += 2; break; }
        total--;
    }
    int j = m;
    for (int l = 1; l <= max_bits; l++)                       // the short codes to the high ranks (the frequent symbols)
        for (uint32_t c = count[l]; c > 0 && j > 0; c--) len[order[--j]] = (uint8_t)l;
    // canonical codes in symbol order, reversed for an emitter that writes the low bit first
    uint32_t next_code[16];
    uint32_t c = 0;
    next_code[0] = 0;
    for (int l = 1; l <= max_bits; l++) { c = (c + (l > 1 ? count[l - 1] : 0u)) << 1; next_code[l] = c; }
    for (int s = 0; s < n; s++) {
        const int l = len[s];
        if (l == 0) continue;
        uint32_t v = next_code[l]++, r = 0;
        for (int b = 0; b < l; b++) { r = r << 1 | (v & 1u); v >>= 1; }
        code[s] = (uint16_t)r;
    }
}

// ---------------------------------------------------------------- the dynamic block's header
// The code lengths of the HLIT + HDIST symbols as code-length symbols (runs of zeros as 17 / 18, repeats of a length as
// 16), the code-length code from their counts, and the header's size in bits.
static inline GKI_DEF_HD void gki_def_header_plan(gki_def_state &st) {
    static const uint8_t order19[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int hlit = GKI_DEF_LCODES, hdist = GKI_DEF_DCODES;
    while (hlit > 257 && st.llen[hlit - 1] == 0) hlit--;
    while (hdist > 1 && st.dlen[hdist - 1] == 0) hdist--;
    const int total = hlit + hdist;
    for (int s = 0; s < 20; s++) st.cfreq[s] = 0;
    int n_cl = 0, i = 0;
    while (i < total) {
        const int l = i < hlit ? st.llen[i] : st.dlen[i - hlit];
        int run = 1;
        while (i + run < total && (i + run < hlit ? st.llen[i + run] : st.dlen[i + run - hlit]) == l) run++;
        i += run;
        while (run > 0 && n_cl < 320) {
            int sym, extra = 0, take;
            if (l == 0 && run >= 11) { take = run < 138 ? run : 138; sym = 18; extra = take - 11; }
            else if (l == 0 && run >= 3) { take = run; sym = 17; extra = take - 3; }
            else { take = 1; sym = l; }
            st.cl_sym[n_cl] = (uint8_t)sym; st.cl_extra[n_cl] = (uint8_t)extra; n_cl++;
            st.cfreq[sym]++;
            run -= take;
            while (l != 0 && run >= 3 && n_cl < 320) {            // the length just written, 3 to 6 more times
                take = run < 6 ? run : 6;
                st.cl_sym[n_cl] = 16; st.cl_extra[n_cl] = (uint8_t)(take - 3); n_cl++;
                st.cfreq[16]++;
                run -= take;
            }
        }
    }
    int used = 0, only = 0;
    for (int s = 0; s < GKI_DEF_CCODES; s++) if (st.cfreq[s]) { used++; only = s; }
    if (used == 1) st.cfreq[only == 0 ? 1 : 0] = 1u;              // a complete code-length code has two codes
    for (int s = 0; s < GKI_DEF_CCODES; s++) gki_def_rank_symbol(st.cfreq, GKI_DEF_CCODES, s, st.corder);
    gki_def_build_code(st.cfreq, GKI_DEF_CCODES, 7, st.corder, st.cwork, st.clen, st.ccode);
    int hclen = GKI_DEF_CCODES;
    while (hclen > 4 && st.clen[order19[hclen - 1]] == 0) hclen--;
    uint32_t bits = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen;
    for (int k = 0; k < n_cl; k++) {
        const int sym = st.cl_sym[k];
        bits += st.clen[sym] + (sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u);
    }
    st.n_cl = n_cl; st.hlit = hlit; st.hdist = hdist; st.hclen = hclen; st.header_bits = bits;
}

// ---------------------------------------------------------------- bits
// An emitter of bits into 32-bit little-endian words that were zeroed: a word that it fills alone is stored, the word it
// starts inside and the word it ends inside may hold another emitter's bits and are or-ed.
struct gki_def_bits {
    uint32_t *w;
    int64_t n_words, idx;
    uint64_t acc;
    int n, shared;
};

static inline GKI_DEF_HD void gki_def_bits_begin(gki_def_bits &b, uint32_t *words, int64_t n_words, uint32_t bit_offset) {
    b.w = words; b.n_words = n_words; b.idx = bit_offset >> 5; b.acc = 0; b.n = (int)(bit_offset & 31u); b.shared = b.n != 0;
}

// nb (0..32) bits of v, the lowest first
static inline GKI_DEF_HD void gki_def_bits_put(gki_def_bits &b, uint32_t v, int nb) {
    b.acc |= (uint64_t)v << b.n;
    b.n += nb;
    if (b.n >= 32) {
        if (b.idx < b.n_words) {
            if (b.shared) GKI_DEF_OR32(&b.w[b.idx], (uint32_t)b.acc); else b.w[b.idx] = (uint32_t)b.acc;
        }
        b.shared = 0; b.idx++; b.acc >>= 32; b.n -= 32;
    }
}

static inline GKI_DEF_HD void gki_def_bits_end(gki_def_bits &b) {
    if (b.n > 0 && b.idx < b.n_words) GKI_DEF_OR32(&b.w[b.idx], (uint32_t)b.acc);
    b.n = 0; b.acc = 0;
}

static inline GKI_DEF_HD uint32_t gki_def_segment_bits(const gki_def_state &st, const uint8_t *in, const uint32_t *pm, int begin, int end) {
    uint32_t bits = 0;
    gki_def_walk(in, pm, begin, end,
                 [&](uint8_t b) { bits += st.llen[b]; },
                 [&](int len, int d) {
                     int e; uint32_t x;
                     bits += st.llen[257 + gki_def_length_code(len, &e, &x)] + (uint32_t)e;
                     bits += st.dlen[gki_def_dist_code(d, &e, &x) & 31] + (uint32_t)e;
                 });
    return bits;
}

// seg_bits[s] becomes the member's bit where segment s starts; dynamic against stored by payload size; the member's size
static inline GKI_DEF_HD void gki_def_layout(gki_def_state &st, int n) {
    const int n_seg = (n + GKI_DEF_SEG - 1) / GKI_DEF_SEG;
    uint32_t at = 8u * GKI_DEF_MEMBER_HEAD + st.header_bits;
    for (int s = 0; s < n_seg; s++) { const uint32_t b = st.seg_bits[s]; st.seg_bits[s] = at; at += b; }
    at += st.llen[256];
    st.end_bit = at;
    const uint32_t dynamic_payload = (at + 7u) / 8u - GKI_DEF_MEMBER_HEAD, stored_payload = (uint32_t)n + 5u;
    st.stored = dynamic_payload >= stored_payload;
    st.member_bytes = GKI_DEF_MEMBER_HEAD + (st.stored ? stored_payload : dynamic_payload) + 8u;
}

// the 18 bytes in front of the payload: MTIME 0, XFL 0, OS 255, 'BC' with BSIZE = the member's size - 1
static inline GKI_DEF_HD void gki_def_emit_member_head(gki_def_bits &b, uint32_t member_bytes) {
    gki_def_bits_put(b, 0x04088B1Fu, 32);                      // ID1 ID2 CM FLG = FEXTRA
    gki_def_bits_put(b, 0u, 32);                               // MTIME
    gki_def_bits_put(b, 0x0006FF00u, 32);                      // XFL 0, OS 255, XLEN 6
    gki_def_bits_put(b, 0x00024342u, 32);                      // 'B' 'C' SLEN 2
    gki_def_bits_put(b, (member_bytes - 1u) & 0xFFFFu, 16);
}

static inline GKI_DEF_HD void gki_def_emit_header(const gki_def_state &st, gki_def_bits &b) {
    static const uint8_t order19[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    gki_def_bits_put(b, 1u | 2u << 1, 3);                      // BFINAL, BTYPE 2
    gki_def_bits_put(b, (uint32_t)(st.hlit - 257), 5);
    gki_def_bits_put(b, (uint32_t)(st.hdist - 1), 5);
    gki_def_bits_put(b, (uint32_t)(st.hclen - 4), 4);
    for (int k = 0; k < st.hclen && k < 19; k++) gki_def_bits_put(b, st.clen[order19[k]], 3);
    for (int k = 0; k < st.n_cl && k < 320; k++) {
        const int sym = st.cl_sym[k] & 31;
        gki_def_bits_put(b, st.ccode[sym < 20 ? sym : 0], st.clen[sym < 20 ? sym : 0]);
        if (sym >= 16) gki_def_bits_put(b, st.cl_extra[k], sym == 16 ? 2 : sym == 17 ? 3 : 7);
    }
}

static inline GKI_DEF_HD void gki_def_emit_segment(const gki_def_state &st, const uint8_t *in, const uint32_t *pm, int begin, int end,
                                                   gki_def_bits &b) {
    gki_def_walk(in, pm, begin, end,
                 [&](uint8_t v) { gki_def_bits_put(b, st.lcode[v], st.llen[v]); },
                 [&](int len, int d) {
                     int e; uint32_t x;
                     const int ls = 257 + gki_def_length_code(len, &e, &x);
                     gki_def_bits_put(b, st.lcode[ls], st.llen[ls]);
                     gki_def_bits_put(b, x, e);
                     const int ds = gki_def_dist_code(d, &e, &x) & 31;
                     gki_def_bits_put(b, st.dcode[ds], st.dlen[ds]);
                     gki_def_bits_put(b, x, e);
                 });
}

// the end-of-block symbol at its bit, zero bits to the byte's end, CRC-32 and ISIZE
static inline GKI_DEF_HD void gki_def_emit_tail(const gki_def_state &st, gki_def_bits &b, uint32_t crc, int n) {
    gki_def_bits_put(b, st.lcode[256], st.llen[256]);
    gki_def_bits_put(b, 0u, (8 - (int)(st.end_bit & 7u)) & 7);
    gki_def_bits_put(b, crc, 32);
    gki_def_bits_put(b, (uint32_t)n, 32);
}

// a stored member, in bytes: the frame (head, block header, LEN, NLEN, trailer) and a range of the data
static inline GKI_DEF_HD void gki_def_stored_frame(uint8_t *out, uint32_t crc, int n) {
    static const uint8_t head[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0};
    const uint32_t bsize = (uint32_t)n + GKI_DEF_MEMBER_EXTRA - 1u;
    for (int i = 0; i < 16; i++) out[i] = head[i];
    out[16] = (uint8_t)bsize; out[17] = (uint8_t)(bsize >> 8);
    out[18] = 1;                                               // BFINAL, BTYPE 0, padding
    out[19] = (uint8_t)n; out[20] = (uint8_t)(n >> 8);
    out[21] = (uint8_t)~n; out[22] = (uint8_t)(~n >> 8);
    uint8_t *t = out + 23 + n;
    for (int i = 0; i < 4; i++) { t[i] = (uint8_t)(crc >> (8 * i)); t[4 + i] = (uint8_t)((uint32_t)n >> (8 * i)); }
}

static inline GKI_DEF_HD void gki_def_stored_bytes(uint8_t *out, const uint8_t *in, int begin, int end, int step) {
    for (int i = begin; i < end; i += step) out[23 + i] = in[i];
}
