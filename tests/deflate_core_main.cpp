// Stand-alone host program around csrc/gki_deflate_core.h for tests/test_deflate_core_cpu.py, which builds it with
// -fsanitize=address,undefined, and for tests/test_gpu_bgzf_deflate.py, which compares its bytes with the kernel's.  It
// drives the core's pieces in the order of k_bgzf_deflate (csrc/gki_bgzf_deflate.hip): where the kernel has 256 lanes
// between two barriers, this has a loop over 256 lane numbers.
// Reads a file of vectors -- per vector: uint32 n, uint32 block_size, then n bytes of text, little endian -- and writes,
// per vector: uint32 bytes, then that many bytes of BGZF members (no end-of-file member).  A member's input, its match
// words and its output slot live in heap blocks of exactly their sizes, so a read or write outside them is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../graph_kmer_index_amd/csrc/gki_deflate_core.h"

static const int LANES = GKI_DEF_SEG;

// one member: n (1..block_size) bytes at src into the zero-initialised-by-nobody slot `words`; returns the member's bytes
static uint32_t deflate_member(gki_def_state &st, const uint8_t *src, int n, uint32_t *words, uint32_t *pm) {
    const int n_seg = (n + GKI_DEF_SEG - 1) / GKI_DEF_SEG;
    for (int i = 0; i < GKI_DEF_HASH_SIZE; i++) st.head[i] = 0;
    for (int i = 0; i < 288; i++) st.lfreq[i] = 0;
    for (int i = 0; i < 32; i++) st.dfreq[i] = 0;
    for (int t = 0; t < LANES; t++) st.seg_bits[t] = 0;
    st.crc = 0;
    for (int t = 0; t < n_seg; t++) {
        const int begin = t * GKI_DEF_SEG, end = begin + GKI_DEF_SEG < n ? begin + GKI_DEF_SEG : n;
        gki_def_crc_add_segment(st, src, n, begin, end);
    }
    for (int r = 0; r < n_seg; r++) {
        uint32_t cand1[LANES];
        for (int t = 0; t < LANES; t++) cand1[t] = gki_def_round_begin(st, src, n, r * GKI_DEF_SEG + t, t);
        for (int t = 0; t < LANES; t++) gki_def_round_end(st, src, n, r * GKI_DEF_SEG + t, t, cand1[t], pm);
    }
    for (int t = 0; t < n_seg; t++) {
        const int begin = t * GKI_DEF_SEG, end = begin + GKI_DEF_SEG < n ? begin + GKI_DEF_SEG : n;
        gki_def_count_segment(st, src, pm, begin, end);
    }
    gki_def_counts_finish(st);
    for (int s = 0; s < GKI_DEF_LCODES; s++) gki_def_rank_symbol(st.lfreq, GKI_DEF_LCODES, s, st.lorder);
    for (int s = 0; s < GKI_DEF_DCODES; s++) gki_def_rank_symbol(st.dfreq, GKI_DEF_DCODES, s, st.dorder);
    gki_def_build_code(st.lfreq, GKI_DEF_LCODES, 15, st.lorder, st.lwork, st.llen, st.lcode);
    gki_def_build_code(st.dfreq, GKI_DEF_DCODES, 15, st.dorder, st.dwork, st.dlen, st.dcode);
    gki_def_header_plan(st);
    for (int t = 0; t < n_seg; t++) {
        const int begin = t * GKI_DEF_SEG, end = begin + GKI_DEF_SEG < n ? begin + GKI_DEF_SEG : n;
        st.seg_bits[t] = gki_def_segment_bits(st, src, pm, begin, end);
    }
    gki_def_layout(st, n);
    if (st.stored) {
        for (int t = 0; t < LANES; t++) gki_def_stored_bytes((uint8_t *)words, src, t, n, LANES);
        gki_def_stored_frame((uint8_t *)words, gki_def_crc_finish(st.crc, n), n);
        return st.member_bytes;
    }
    const int member_words = (int)((st.member_bytes + 3u) / 4u);
    for (int i = 0; i < member_words; i++) words[i] = 0u;
    gki_def_bits b;
    for (int t = 0; t < n_seg; t++) {
        const int begin = t * GKI_DEF_SEG, end = begin + GKI_DEF_SEG < n ? begin + GKI_DEF_SEG : n;
        gki_def_bits_begin(b, words, member_words, st.seg_bits[t]);
        gki_def_emit_segment(st, src, pm, begin, end, b);
        gki_def_bits_end(b);
    }
    gki_def_bits_begin(b, words, member_words, 0u);
    gki_def_emit_member_head(b, st.member_bytes);
    gki_def_emit_header(st, b);
    gki_def_bits_end(b);
    gki_def_bits_begin(b, words, member_words, st.end_bit - st.llen[256]);
    gki_def_emit_tail(st, b, gki_def_crc_finish(st.crc, n), n);
    gki_def_bits_end(b);
    return st.member_bytes;
}

// `code max_bits c0 c1 ...`: the code construction alone, from counts given as arguments (at most 286 of them, at least
// two above 0); prints "length code" per symbol
static int code_of_counts(int argc, char **argv) {
    const int max_bits = atoi(argv[2]), n = argc - 3;
    if (n < 2 || n > GKI_DEF_LCODES || max_bits < 1 || max_bits > 15) { fprintf(stderr, "code: 2..286 counts, max_bits 1..15\n"); return 2; }
    uint32_t *freq = (uint32_t *)malloc((size_t)n * 4), *work = (uint32_t *)malloc((size_t)n * 4);
    uint16_t *order = (uint16_t *)malloc((size_t)n * 2), *code = (uint16_t *)malloc((size_t)n * 2);
    uint8_t *len = (uint8_t *)malloc((size_t)n);
    for (int s = 0; s < n; s++) freq[s] = (uint32_t)strtoul(argv[3 + s], NULL, 10);
    for (int s = 0; s < n; s++) gki_def_rank_symbol(freq, n, s, order);
    gki_def_build_code(freq, n, max_bits, order, work, len, code);
    for (int s = 0; s < n; s++) printf("%d %u\n", (int)len[s], (unsigned)code[s]);
    free(freq); free(work); free(order); free(code); free(len);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 3 && strcmp(argv[1], "code") == 0) return code_of_counts(argc, argv);
    if (argc != 3) { fprintf(stderr, "usage: %s vectors.bin members.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) { perror(f ? argv[2] : argv[1]); return 2; }
    gki_def_state *st = (gki_def_state *)malloc(sizeof(gki_def_state));
    uint32_t head[2];
    while (fread(head, 4, 2, f) == 2) {
        const uint32_t n = head[0], block_size = head[1];
        if (block_size < 1 || block_size > GKI_DEF_MAX_IN) { fprintf(stderr, "block_size %u\n", block_size); return 2; }
        uint8_t *text = (uint8_t *)malloc(n);
        if (n && fread(text, 1, n, f) != n) { fprintf(stderr, "short vector file\n"); return 2; }
        const size_t stride = ((size_t)block_size + GKI_DEF_MEMBER_EXTRA + 15) / 16 * 16;
        uint32_t total = 0;
        const long at = ftell(g);
        fwrite(&total, 4, 1, g);
        for (uint32_t a = 0; a < n; a += block_size) {
            const int len = (int)(n - a < block_size ? n - a : block_size);
            uint8_t *src = (uint8_t *)malloc((size_t)len);         // the member alone: it may read nothing of its neighbours
            memcpy(src, text + a, (size_t)len);
            uint32_t *words = (uint32_t *)malloc(stride), *pm = (uint32_t *)malloc((size_t)len * 4);
            memset(st, 0xA5, sizeof(*st));
            for (uint32_t i = 0; i < 256; i++) st->crc_table[i] = gki_crc32_table_entry(i);
            const uint32_t bytes = deflate_member(*st, src, len, words, pm);
            if (bytes > (uint32_t)len + GKI_DEF_MEMBER_EXTRA) { fprintf(stderr, "a member of %u bytes from %d\n", bytes, len); return 3; }
            fwrite(words, 1, bytes, g);
            total += bytes;
            free(src); free(words); free(pm);
        }
        fseek(g, at, SEEK_SET);
        fwrite(&total, 4, 1, g);
        fseek(g, 0, SEEK_END);
        free(text);
    }
    free(st);
    fclose(f);
    if (fclose(g) != 0) { perror(argv[2]); return 2; }
    return 0;
}
