// Frequency sources of the variant-signature kernels, and the kernel bodies that are written once for all of them.
//
// A source answers frequency(h) for a k-mer hash:
//   GkiIndexSource    CollisionFreeKmerIndex.get_frequency with its defaults: the first hit of h plus the first hit of its
//                     31-mer reverse complement (collision_free_kmer_index.py:336-352)
//   GkiCounterSource  KmerCounter.get_frequency: the count of h alone, no reverse complement (kmer_counter.py:72-74)
// k_sv_probe / k_uvk_summarize (gki_sv_kmers.hip, gki_variant_kmers.hip) instantiate the bodies with the index source,
// k_sv_probe_counter / k_uvk_summarize_counter (gki_count.hip) with the counter source.
#pragma once
#include "gki_common.h"

struct GkiIndexSource {
    const int32_t *hashes_to_index;
    const uint32_t *n_kmers;
    const uint64_t *kmers;
    const uint16_t *frequencies;
    int64_t n;
    GkiMod mod;
    uint64_t bucket_begin, n_buckets;
    __device__ __forceinline__ uint32_t frequency(uint64_t h) const {
        return gki_first_hit_frequency(hashes_to_index, n_kmers, kmers, frequencies, n, mod, bucket_begin, n_buckets, h) +
               gki_first_hit_frequency(hashes_to_index, n_kmers, kmers, frequencies, n, mod, bucket_begin, n_buckets,
                                       gki_revcomp(h & ((1ull << 62) - 1ull), 31));
    }
};

struct GkiCounterSource {
    GkiCounterView c;
    __device__ __forceinline__ int64_t frequency(uint64_t h) const { return gki_counter_frequency(c, h); }
};

static inline GkiIndexSource gki_index_source(const gki_index_view *ix) {
    GkiIndexSource s;
    s.hashes_to_index = (const int32_t *)ix->d_hashes_to_index;
    s.n_kmers = (const uint32_t *)ix->d_n_kmers;
    s.kmers = (const uint64_t *)ix->d_kmers;
    s.frequencies = (const uint16_t *)ix->d_frequencies;
    s.n = ix->n;
    s.mod = gki_mod_of(ix->modulo);
    s.bucket_begin = ix->bucket_begin;
    s.n_buckets = ix->n_buckets ? ix->n_buckets : ix->modulo;
    return s;
}

// ---------------------------------------------------------------------------------- structural-variant probe pass
constexpr int SV_CHUNK = 16;                 // consecutive bitmap words a wave takes at a time in the probe pass

// the wave's number: uniform, fits 32 bits (a grid has at most 2048 * 4 waves)
__device__ __forceinline__ int64_t sv_wave() {
    return __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6));
}

// the candidate that owns bitmap word w < word_start[n_cand]: the last one that begins at or before w (candidates
// without words share their begin with the next one and lose)
__device__ __forceinline__ int64_t sv_cand_of(const int64_t *__restrict__ word_start, int64_t n_cand, int64_t w) {
    int64_t lo = 0, hi = n_cand;                         // word_start[lo] <= w < word_start[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (word_start[mid] <= w) lo = mid; else hi = mid;
    }
    return lo;
}

// one wave per bitmap word, one lane per window: bit j of the word = frequency(window j) < max_frequency
template <class Source>
__device__ __forceinline__ void sv_probe_body(const int32_t *__restrict__ cand, const int64_t *__restrict__ word_start,
                                              int64_t n_cand, int64_t n_words, const int32_t *__restrict__ node_size,
                                              const int64_t *__restrict__ seq_start, const uint64_t *__restrict__ seq2,
                                              int k, int64_t max_frequency, const Source &src,
                                              uint64_t *__restrict__ bitmap) {
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t n_chunks = (n_words + SV_CHUNK - 1) / SV_CHUNK;
    for (int64_t c = sv_wave(); c < n_chunks; c += n_waves) {
        int64_t w = c * SV_CHUNK;
        const int64_t w_end = w + SV_CHUNK < n_words ? w + SV_CHUNK : n_words;
        int64_t i = sv_cand_of(word_start, n_cand, w);       // uniform: scalar loads
        for (; w < w_end; ++w) {
            while (word_start[i + 1] <= w) ++i;              // w < n_words = word_start[n_cand] ends it
            const int32_t node = cand[i];
            const int64_t n_win = (int64_t)node_size[node] - k + 1;
            const int64_t j = (w - word_start[i]) * 64 + lane;
            bool valid = false;
            if (j < n_win) {
                const uint64_t h = gki_extract(seq2, seq_start[node] + j, k);
                const auto f = src.frequency(h);
                valid = (int64_t)f < max_frequency;
            }
            const uint64_t word = __ballot(valid);           // windows past the node's last one stay 0
            if (lane == 0) bitmap[w] = word;
        }
    }
}

// ---------------------------------------------------------------------------------- variant k-mer summaries
constexpr int UVK_WINDOW_CAP = 500;          // kmer_finder.py:137-160: kmers_found keeps the first 500 windows

// A new window begins at record r unless r continues the previous record's window: same hash, same end position, a
// larger node (a window's records are its distinct nodes in ascending order, and two windows that end at the same
// position both hold the node they end in, so the next window's first node is never above the previous one's last).
__device__ __forceinline__ bool uvk_new_window(const int64_t *__restrict__ hashes, const int32_t *__restrict__ start_nodes,
                                               const int16_t *__restrict__ start_offsets, const int32_t *__restrict__ nodes,
                                               int64_t r, int64_t rs) {
    return r == rs || hashes[r] != hashes[r - 1] || start_nodes[r] != start_nodes[r - 1] ||
           start_offsets[r] != start_offsets[r - 1] || nodes[r] <= nodes[r - 1];
}

// one lane per start position; a frequency above 2^32 - 1 is stored as 2^32 - 1 (gki_uvk_summary's fields are 32 bits)
template <class Source>
__device__ __forceinline__ void uvk_summarize_body(
    const int64_t *__restrict__ rec_start, int64_t n_pos, int P, const int64_t *__restrict__ hashes,
    const int32_t *__restrict__ start_nodes, const int16_t *__restrict__ start_offsets, const int32_t *__restrict__ nodes,
    const int32_t *__restrict__ ref_nodes, const int32_t *__restrict__ alt_nodes, const Source &src,
    gki_uvk_summary *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pos; i += stride) {
        const int64_t v = i / P;
        const int32_t ref = ref_nodes[v], alt = alt_nodes[v];
        const bool same = ref == alt;
        const int64_t rs = rec_start[i], re = rec_start[i + 1];
        // records inside the first 500 windows: [rs, lim); at most 500 records hold at most 500 windows
        int64_t lim = re;
        if (re - rs > UVK_WINDOW_CAP) {
            int w = 0;
            for (int64_t r = rs; r < re; ++r) {
                if (uvk_new_window(hashes, start_nodes, start_offsets, nodes, r, rs)) {
                    if (w == UVK_WINDOW_CAP) { lim = r; break; }
                    ++w;
                }
            }
        }
        uint32_t n_ref = 0, n_alt = 0, f_ref = 0, f_alt = 0, flags = same ? 2u : 0u;
        for (int64_t r = rs; r < re; ++r) {
            const int32_t nd = nodes[r];
            const bool is_ref = nd == ref, is_alt = !same && nd == alt;
            if (!is_ref && !is_alt) continue;
            const uint64_t h = (uint64_t)hashes[r];
            const auto fw = src.frequency(h);
            const uint32_t f = sizeof(fw) > 4 && (uint64_t)fw > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)fw;
            if (is_ref) { ++n_ref; f_ref = f > f_ref ? f : f_ref; }
            else { ++n_alt; f_alt = f > f_alt ? f : f_alt; }
            if (r < lim && !(flags & 1u)) {
                if (same) flags |= 1u;                  // kmers_ref and kmers_variant are the same non-empty set
                else if (is_alt) {                      // an earlier-or-later ref record of the first 500 windows with h
                    for (int64_t q = rs; q < lim; ++q)
                        if (nodes[q] == ref && hashes[q] == (int64_t)h) { flags |= 1u; break; }
                }
            }
        }
        gki_uvk_summary s;
        s.n_ref = n_ref; s.n_alt = n_alt; s.f_ref = f_ref; s.f_alt = f_alt; s.flags = flags;
        out[i] = s;
    }
}

// ---------------------------------------------------------------------------------- counter variants (gki_count.hip)
// The same passes with a gki_counter as source: launched by gki_sv_sample_count_counter / gki_uvk_summarize_counter.
int gki_launch_sv_probe_counter(const gki_counter *c, const int32_t *cand, const int64_t *word_start, int64_t n_cand,
                                int64_t n_words, const DevGraph &d, int k, int64_t max_frequency, uint64_t *bitmap);
int gki_launch_uvk_summarize_counter(const gki_counter *c, const int64_t *rec_start, int64_t n_pos, int P,
                                     const int64_t *hashes, const int32_t *start_nodes, const int16_t *start_offsets,
                                     const int32_t *nodes, const int32_t *ref_nodes, const int32_t *alt_nodes,
                                     gki_uvk_summary *out);
