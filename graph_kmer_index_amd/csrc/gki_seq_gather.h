// What the two output-dense sequence gathers share -- k_gb_sequence (gki_graph_build.hip: the reference with alt alleles
// put in) and k_hap_spell (gki_haplotype_paths.hip: the graph's seq with one allele per kept line cut out): a lane owns 16
// output bytes, finds the first site behind its first byte by a search bounded by its tile's site range, and when no site
// boundary falls among its 16 bytes moves them with one unaligned 16-byte load and one aligned 16-byte store.
#pragma once
#include "gki_common.h"

// 16 source bytes at any alignment: four-byte alignment keeps the copy one global_load_dwordx4
struct alignas(4) Letters16 { uint32_t w[4]; };

// first k in [a, b) with site_end[k] > p, b when there is none (site_end is non-decreasing)
__device__ __forceinline__ int64_t first_site_after(const int64_t *__restrict__ site_end, int64_t a, int64_t b, int64_t p) {
    while (a < b) {
        const int64_t mid = a + ((b - a) >> 1);
        if (site_end[mid] > p) b = mid; else a = mid + 1;
    }
    return a;
}
