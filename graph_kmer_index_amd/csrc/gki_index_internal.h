// What the two files of the index build share: gki_index.hip (the entry points, the pair-sorting form, the frequencies of
// large buckets) and gki_index_rows.hip (the row-carrying form and the bucket-range partition).  Host-side argument
// structs in place of positional lists of untyped pointers; a NULL member is a column the caller does not have or want.
#pragma once
#include "gki_common.h"

constexpr int SMALL_BUCKET = 24;            // buckets of up to this many records count their frequencies one lane per record

static inline int key_bits(uint64_t max_key) {
    int bits = 0;
    while (bits < 32 && (max_key >> bits) != 0) bits++;
    return bits;
}

// the four payload columns of FlatKmers (the allele frequency as its 32 bits: the build only moves it)
template <class U64, class U32> struct RecordColsT {
    U64 *kmers; U32 *nodes; U64 *refs; U32 *af;
    RecordColsT at(int64_t i) const { return {kmers ? kmers + i : kmers, nodes ? nodes + i : nodes, refs ? refs + i : refs, af ? af + i : af}; }
};
using RecordCols = RecordColsT<const uint64_t, const uint32_t>;
using RecordColsOut = RecordColsT<uint64_t, uint32_t>;
static inline RecordCols record_cols(const void *kmers, const void *nodes, const void *refs, const void *af) {
    return {(const uint64_t *)kmers, (const uint32_t *)nodes, (const uint64_t *)refs, (const uint32_t *)af};
}
static inline RecordColsOut record_cols_out(void *kmers, void *nodes, void *refs, void *af) {
    return {(uint64_t *)kmers, (uint32_t *)nodes, (uint64_t *)refs, (uint32_t *)af};
}

// records as 24-byte rows (k-mer, ref offset, node | allele frequency << 32) with their 32-bit keys
template <class U64, class U32> struct RowsT { U64 *rows; U32 *keys; };
using RowsIn = RowsT<const uint64_t, const uint32_t>;
using RowsOut = RowsT<uint64_t, uint32_t>;

struct IndexOut {                           // the directory, the sorted columns, their frequencies, the permutation
    int32_t *h2i; uint32_t *n_kmers;
    RecordColsOut cols;
    uint16_t *freq; uint32_t *perm;
};
struct Slice { uint64_t modulo, bucket_begin, n_buckets; };       // buckets [bucket_begin, +n_buckets) of kmer % modulo
struct Grouping { int group_bits; const int64_t *h_group_start; };   // records grouped by the top group_bits bits of their key
struct PartSpec { uint64_t modulo; int n_parts, sub_bits; int64_t max_rows_per_pass; };

// The row-carrying build (gki_index_rows.hip), from `cols` or -- rows.rows != NULL -- from rows with their keys.  Returns
// GKI_OK when it built the index, GKI_NOT_BUILT when the input is outside its domain (a group too large to stream with one
// workgroup: the caller turns to the pair-sorting form), an error code otherwise.
// by_node: the key of a record is its node id and the "buckets" are the nodes (ReverseKmerIndex.from_flat_kmers,
// reverse_kmer_index.py:47-60: records stably sorted by node): slice.modulo is unused, slice.n_buckets = the number of nodes,
// the allele-frequency, node and frequency output columns may be NULL.
constexpr int GKI_NOT_BUILT = -1;
int gki_index_build_rows(const RecordCols &cols, const RowsIn &rows, int64_t n, const Slice &slice, const Grouping &grouping,
                         int skip_frequencies, int by_node, const IndexOut &out);

// Stable partition of `cols` by owning part (and the top sub_bits bits of the key inside the part) into four columns or --
// out_rows.rows != NULL -- into rows + keys; h_part_start[(n_parts << sub_bits) + 1].
int gki_partition_columns_by_part(const RecordCols &cols, int64_t n, const PartSpec &spec, const RecordColsOut &out_cols,
                                  const RowsOut &out_rows, int64_t *h_part_start);

// Frequencies of the rows in the ranges [d_row_begin[i], d_row_end[i]) of the finished columns, each a whole number of buckets
int gki_frequencies_for_rows(const int64_t *d_row_begin, const int64_t *d_row_end, int n_ranges, const Slice &slice,
                             const IndexOut &out, int64_t n, hipStream_t s);
