// Stand-alone host program around csrc/gki_inflate_core.h for tests/test_inflate_core_cpu.py, which builds it with
// -fsanitize=address,undefined.  Reads a file of vectors -- per vector: uint32 in_len, uint32 out_len, uint32 crc, then
// in_len payload bytes, little endian -- and prints one line per vector: status, bytes written, CRC-32 of those bytes.
// Input and output live in heap blocks of exactly in_len and out_len bytes, so a read or write outside them is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../graph_kmer_index_amd/csrc/gki_inflate_core.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s vectors.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; i++) table[i] = gki_crc32_table_entry(i);
    gki_inf_tables *tables = (gki_inf_tables *)malloc(sizeof(gki_inf_tables));
    uint32_t head[3];
    while (fread(head, 4, 3, f) == 3) {
        uint8_t *in = (uint8_t *)malloc(head[0]);          // of no bytes: nothing may be read at all
        uint8_t *out = (uint8_t *)malloc(head[1]);
        if (head[0] && fread(in, 1, head[0], f) != head[0]) { fprintf(stderr, "short vector file\n"); return 2; }
        memset(tables, 0xA5, sizeof(*tables));
        int64_t n_out = -1;
        const int status = gki_inflate_member(in, head[0], out, head[1], head[2], table, *tables, &n_out);
        if (n_out < 0 || n_out > (int64_t)head[1]) { fprintf(stderr, "n_out %lld outside [0, %u]\n", (long long)n_out, head[1]); return 3; }
        printf("%d %lld %08x\n", status, (long long)n_out, gki_crc32(table, out, n_out));
        free(in);
        free(out);
    }
    free(tables);
    fclose(f);
    return 0;
}
