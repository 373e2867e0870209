// Inflate of ONE raw DEFLATE stream (RFC 1951) without a dictionary, and the CRC-32 of gzip (RFC 1952), as plain C++:
// the same text is the body of the BGZF kernel (csrc/gki_inflate.hip) and of a stand-alone host program (the sanitizer
// test of tests/test_inflate_core_cpu.py compiles it with the system's compiler).  GKI_INFLATE_HD is __host__ __device__
// under hipcc and nothing elsewhere.
//
// Bounds: every read of the input is behind a test against in_len and every write of the output behind a test against
// out_len; the Huffman tables are indexed by values that construct() and decode() keep inside them (see there).  Every
// loop iteration consumes at least one bit of input, writes at least one byte of output, or returns.
//
// Decoding is the canonical-code walk of zlib's contrib/puff (count of codes per length, symbols in code order; one bit
// per step): two tables of 16 + 288 and 16 + 32 uint16 and 320 code lengths -- about 1 KiB of state per stream.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GKI_INFLATE_HD __host__ __device__
#else
#define GKI_INFLATE_HD
#endif

// status of one stream; 0 is success.  include/gki.h ("BGZF") lists the same numbers for callers of gki_bgzf_inflate.
enum {
    GKI_INF_OK = 0,
    GKI_INF_INPUT_END = 1,       // the input ends before the final block's end-of-block symbol
    GKI_INF_BLOCK_TYPE = 2,      // BTYPE 3
    GKI_INF_STORED_LEN = 3,      // a stored block whose NLEN is not the complement of LEN
    GKI_INF_CODE_LENGTHS = 4,    // an over-subscribed or incomplete code set, more than 286 / 30 codes, a repeat past the
                                 // last length, or no end-of-block code
    GKI_INF_REPEAT_FIRST = 5,    // repeat code 16 with no length before it
    GKI_INF_LITLEN_SYMBOL = 6,   // literal/length symbol 286 or 287
    GKI_INF_DIST_SYMBOL = 7,     // distance symbol 30 or 31
    GKI_INF_DISTANCE = 8,        // a distance that reaches before the start of the output
    GKI_INF_OUTPUT_OVERFLOW = 9, // the stream holds more than out_len bytes
    GKI_INF_OUTPUT_SHORT = 10,   // the stream ends with fewer than out_len bytes
    GKI_INF_TRAILING_INPUT = 11, // whole bytes of input behind the final block
    GKI_INF_CRC = 12,            // the output's CRC-32 is not the one given (set by the callers, not by gki_inflate_raw)
    GKI_INF_INVALID_CODE = 13    // bits that are no code of an incomplete (single-code or empty) set
};

#define GKI_INF_MAXBITS 15
#define GKI_INF_MAXLCODES 286
#define GKI_INF_MAXDCODES 30

struct gki_inf_tables {
    uint16_t lencnt[GKI_INF_MAXBITS + 1], lensym[288];   // literal/length code (and, while a dynamic header is read, the
                                                         // code-length code: 19 symbols)
    uint16_t distcnt[GKI_INF_MAXBITS + 1], distsym[32];  // distance code (32 symbols in a fixed block)
    uint8_t lengths[320];                                // 288 + 32 code lengths
};

struct gki_inf_bits {
    const uint8_t *in;
    int64_t in_len, pos;      // pos: the next byte of the input that has not been loaded
    uint32_t buf;             // the bits loaded and not consumed, the next one lowest
    int cnt;                  // how many; below 8 between calls, so pos is exact: no byte is loaded before a bit of it is needed
};

// n bits (0..16), least significant first; false when the input ends first
static inline GKI_INFLATE_HD bool gki_inf_take(gki_inf_bits &s, int n, uint32_t *v) {
    while (s.cnt < n) {
        if (s.pos >= s.in_len) return false;
        s.buf |= (uint32_t)s.in[s.pos++] << s.cnt;       // cnt < 16 here: at most 24 bits held
        s.cnt += 8;
    }
    *v = s.buf & ((1u << n) - 1u);
    s.buf >>= n;
    s.cnt -= n;
    return true;
}

// One symbol of a canonical code: >= 0 the symbol, -1 the input ended, -2 the bits are no code of the set.  The index
// into sym is below the number of codes: index is the count of codes shorter than len, and code - first < cnt[len].
static inline GKI_INFLATE_HD int gki_inf_decode(gki_inf_bits &s, const uint16_t *cnt, const uint16_t *sym) {
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= GKI_INF_MAXBITS; len++) {
        if (s.cnt == 0) {
            if (s.pos >= s.in_len) return -1;
            s.buf = s.in[s.pos++];
            s.cnt = 8;
        }
        code |= (int)(s.buf & 1u);
        s.buf >>= 1;
        s.cnt--;
        const int count = cnt[len];
        if (code - count < first) return sym[index + (code - first)];
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return -2;
}

// Tables of the canonical code with the n (<= 288) lengths given (0..15 each).  Returns 0 for a complete set and for
// one without any code, > 0 for an incomplete one (how many codes of 15 bits are missing), < 0 for an over-subscribed
// one, whose tables are not to be used.  sym gets one entry per symbol with a code: at most n.
static inline GKI_INFLATE_HD int gki_inf_construct(uint16_t *cnt, uint16_t *sym, const uint8_t *length, int n) {
    uint16_t offs[GKI_INF_MAXBITS + 1];
    for (int len = 0; len <= GKI_INF_MAXBITS; len++) cnt[len] = 0;
    for (int i = 0; i < n; i++) cnt[length[i] & 15]++;
    if (cnt[0] == n) return 0;
    int left = 1;
    for (int len = 1; len <= GKI_INF_MAXBITS; len++) {
        left <<= 1;
        left -= cnt[len];
        if (left < 0) return left;
    }
    offs[1] = 0;
    for (int len = 1; len < GKI_INF_MAXBITS; len++) offs[len + 1] = (uint16_t)(offs[len] + cnt[len]);
    for (int i = 0; i < n; i++)
        if (length[i] & 15) sym[offs[length[i] & 15]++] = (uint16_t)i;
    return left;
}

// zlib's rule for a literal/length or distance set (inflate_table): complete, or empty, or exactly one code of one bit
static inline GKI_INFLATE_HD bool gki_inf_set_ok(int left, const uint16_t *cnt, int n) {
    return left == 0 || (left > 0 && cnt[0] + cnt[1] == n && cnt[1] == 1);
}

// the literals, lengths and distances of one block until its end-of-block symbol
static inline GKI_INFLATE_HD int gki_inf_codes(gki_inf_bits &s, const gki_inf_tables &t, uint8_t *out, int64_t out_len,
                                               int64_t *out_pos) {
    int64_t o = *out_pos;
    for (;;) {
        int sym = gki_inf_decode(s, t.lencnt, t.lensym);
        if (sym < 0) { *out_pos = o; return sym == -1 ? GKI_INF_INPUT_END : GKI_INF_INVALID_CODE; }
        if (sym < 256) {
            if (o >= out_len) { *out_pos = o; return GKI_INF_OUTPUT_OVERFLOW; }
            out[o++] = (uint8_t)sym;
            continue;
        }
        if (sym == 256) break;
        sym -= 257;
        if (sym >= 29) { *out_pos = o; return GKI_INF_LITLEN_SYMBOL; }
        // length: 3..10 for symbols 0..7, then four symbols per number of extra bits, 258 for symbol 28
        uint32_t extra = 0;
        int len;
        if (sym < 8) len = 3 + sym;
        else if (sym == 28) len = 258;
        else {
            const int e = (sym >> 2) - 1;
            if (!gki_inf_take(s, e, &extra)) { *out_pos = o; return GKI_INF_INPUT_END; }
            len = 3 + ((4 + (sym & 3)) << e) + (int)extra;
        }
        const int dsym = gki_inf_decode(s, t.distcnt, t.distsym);
        if (dsym < 0) { *out_pos = o; return dsym == -1 ? GKI_INF_INPUT_END : GKI_INF_INVALID_CODE; }
        if (dsym >= 30) { *out_pos = o; return GKI_INF_DIST_SYMBOL; }
        // distance: 1..4 for symbols 0..3, then two symbols per number of extra bits
        int64_t dist;
        if (dsym < 4) dist = 1 + dsym;
        else {
            const int e = (dsym >> 1) - 1;
            if (!gki_inf_take(s, e, &extra)) { *out_pos = o; return GKI_INF_INPUT_END; }
            dist = 1 + ((int64_t)(2 + (dsym & 1)) << e) + (int64_t)extra;
        }
        if (dist > o) { *out_pos = o; return GKI_INF_DISTANCE; }
        if (o + len > out_len) { *out_pos = o; return GKI_INF_OUTPUT_OVERFLOW; }
        for (int j = 0; j < len; j++, o++) out[o] = out[o - dist];     // in stream order: distance 1 is a run
    }
    *out_pos = o;
    return GKI_INF_OK;
}

static inline GKI_INFLATE_HD int gki_inf_stored(gki_inf_bits &s, uint8_t *out, int64_t out_len, int64_t *out_pos) {
    s.buf = 0;                                            // the rest of the current byte is padding
    s.cnt = 0;
    if (s.pos + 4 > s.in_len) return GKI_INF_INPUT_END;
    const uint32_t len = (uint32_t)s.in[s.pos] | (uint32_t)s.in[s.pos + 1] << 8;
    const uint32_t nlen = (uint32_t)s.in[s.pos + 2] | (uint32_t)s.in[s.pos + 3] << 8;
    s.pos += 4;
    if (len != (~nlen & 0xFFFFu)) return GKI_INF_STORED_LEN;
    if (s.pos + (int64_t)len > s.in_len) return GKI_INF_INPUT_END;
    if (*out_pos + (int64_t)len > out_len) return GKI_INF_OUTPUT_OVERFLOW;
    for (uint32_t j = 0; j < len; j++) out[*out_pos + j] = s.in[s.pos + j];
    s.pos += len;
    *out_pos += len;
    return GKI_INF_OK;
}

static inline GKI_INFLATE_HD void gki_inf_fixed_tables(gki_inf_tables &t) {
    int i = 0;
    for (; i < 144; i++) t.lengths[i] = 8;
    for (; i < 256; i++) t.lengths[i] = 9;
    for (; i < 280; i++) t.lengths[i] = 7;
    for (; i < 288; i++) t.lengths[i] = 8;
    for (; i < 320; i++) t.lengths[i] = 5;
    (void)gki_inf_construct(t.lencnt, t.lensym, t.lengths, 288);        // both complete: symbols 286, 287 and distance
    (void)gki_inf_construct(t.distcnt, t.distsym, t.lengths + 288, 32); // symbols 30, 31 decode and are refused by value
}

static inline GKI_INFLATE_HD int gki_inf_dynamic_tables(gki_inf_bits &s, gki_inf_tables &t) {
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t v;
    if (!gki_inf_take(s, 5, &v)) return GKI_INF_INPUT_END;
    const int nlen = (int)v + 257;
    if (!gki_inf_take(s, 5, &v)) return GKI_INF_INPUT_END;
    const int ndist = (int)v + 1;
    if (!gki_inf_take(s, 4, &v)) return GKI_INF_INPUT_END;
    const int ncode = (int)v + 4;
    if (nlen > GKI_INF_MAXLCODES || ndist > GKI_INF_MAXDCODES) return GKI_INF_CODE_LENGTHS;
    int i = 0;
    for (; i < ncode; i++) {
        if (!gki_inf_take(s, 3, &v)) return GKI_INF_INPUT_END;
        t.lengths[order[i]] = (uint8_t)v;
    }
    for (; i < 19; i++) t.lengths[order[i]] = 0;
    if (gki_inf_construct(t.lencnt, t.lensym, t.lengths, 19) != 0) return GKI_INF_CODE_LENGTHS;   // must be complete
    int index = 0;
    while (index < nlen + ndist) {
        const int sym = gki_inf_decode(s, t.lencnt, t.lensym);
        if (sym < 0) return sym == -1 ? GKI_INF_INPUT_END : GKI_INF_INVALID_CODE;
        if (sym < 16) {
            t.lengths[index++] = (uint8_t)sym;
            continue;
        }
        int len = 0, rep;
        if (sym == 16) {
            if (index == 0) return GKI_INF_REPEAT_FIRST;
            len = t.lengths[index - 1];
            if (!gki_inf_take(s, 2, &v)) return GKI_INF_INPUT_END;
            rep = 3 + (int)v;
        } else if (sym == 17) {
            if (!gki_inf_take(s, 3, &v)) return GKI_INF_INPUT_END;
            rep = 3 + (int)v;
        } else {
            if (!gki_inf_take(s, 7, &v)) return GKI_INF_INPUT_END;
            rep = 11 + (int)v;
        }
        if (index + rep > nlen + ndist) return GKI_INF_CODE_LENGTHS;
        while (rep--) t.lengths[index++] = (uint8_t)len;
    }
    if (t.lengths[256] == 0) return GKI_INF_CODE_LENGTHS;               // no end-of-block code
    // the distance lengths move out of the way of nothing: lensym has its own storage, lengths is only read from here on
    int left = gki_inf_construct(t.lencnt, t.lensym, t.lengths, nlen);
    if (!gki_inf_set_ok(left, t.lencnt, nlen)) return GKI_INF_CODE_LENGTHS;
    left = gki_inf_construct(t.distcnt, t.distsym, t.lengths + nlen, ndist);
    if (!gki_inf_set_ok(left, t.distcnt, ndist)) return GKI_INF_CODE_LENGTHS;
    return GKI_INF_OK;
}

// Inflates in[0, in_len) into out[0, out_len): GKI_INF_OK when the stream is well formed, ends exactly at the end of the
// input (the bits that pad its last byte aside) and gives exactly out_len bytes.  *n_out: the bytes written, at most
// out_len, whatever the status.  `t` is scratch.
static inline GKI_INFLATE_HD int gki_inflate_raw(const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_len,
                                                 gki_inf_tables &t, int64_t *n_out) {
    gki_inf_bits s;
    s.in = in; s.in_len = in_len; s.pos = 0; s.buf = 0; s.cnt = 0;
    int64_t o = 0;
    int status = GKI_INF_OK;
    uint32_t last = 0, type;
    while (!last) {
        if (!gki_inf_take(s, 1, &last) || !gki_inf_take(s, 2, &type)) { status = GKI_INF_INPUT_END; break; }
        if (type == 0) status = gki_inf_stored(s, out, out_len, &o);
        else if (type == 1) {
            gki_inf_fixed_tables(t);
            status = gki_inf_codes(s, t, out, out_len, &o);
        } else if (type == 2) {
            status = gki_inf_dynamic_tables(s, t);
            if (status == GKI_INF_OK) status = gki_inf_codes(s, t, out, out_len, &o);
        } else status = GKI_INF_BLOCK_TYPE;
        if (status != GKI_INF_OK) break;
    }
    *n_out = o;
    if (status != GKI_INF_OK) return status;
    if (s.pos < in_len) return GKI_INF_TRAILING_INPUT;
    if (o < out_len) return GKI_INF_OUTPUT_SHORT;
    return GKI_INF_OK;
}

// ---------------------------------------------------------------- CRC-32 (polynomial 0xEDB88320, as gzip's trailer)
static inline GKI_INFLATE_HD uint32_t gki_crc32_table_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    return c;
}

// table: the 256 entries above
static inline GKI_INFLATE_HD uint32_t gki_crc32(const uint32_t *table, const uint8_t *p, int64_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (int64_t i = 0; i < n; i++) c = table[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

// One gzip member's payload: inflate, then the CRC of what was written when the stream itself was good
static inline GKI_INFLATE_HD int gki_inflate_member(const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_len,
                                                    uint32_t crc, const uint32_t *crc_table, gki_inf_tables &t,
                                                    int64_t *n_out) {
    const int status = gki_inflate_raw(in, in_len, out, out_len, t, n_out);
    if (status != GKI_INF_OK) return status;
    return gki_crc32(crc_table, out, out_len) == crc ? GKI_INF_OK : GKI_INF_CRC;
}
