/*
 * gki.h -- C ABI of libgki_hip.so, the MI355X (gfx950) implementation of graph_kmer_index's
 * k-mer enumeration + hashing + index hot path.
 *
 * The reference (ivargr/graph_kmer_index v0.0.29) has no FFI seam for this path: it is plain
 * Python/NumPy.  The entry points below are therefore what a ctypes
 * binding inside the reference would call; each one names the reference function it replaces
 * (paths relative to /root/reference/graph_kmer_index/).  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / numpy types.
 *   - every function returns 0 on success or a GKI_ERR_* code; gki_last_error() returns a
 *     thread-local description of the most recent failure.
 *   - "d_" pointers are device (HBM) addresses obtained from gki_malloc(); "h_" pointers are host
 *     memory owned by the caller.  Variable-size results use count -> allocate -> emit.
 *   - one HIP stream per handle; calls on distinct handles may run concurrently, calls on one
 *     handle are serialised by the caller.
 */
#ifndef GKI_H
#define GKI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GKI_OK 0
#define GKI_ERR_HIP 1            /* a HIP runtime call failed (message has the HIP error string) */
#define GKI_ERR_BAD_ARG 2
#define GKI_ERR_NO_DEVICE 3
#define GKI_ERR_WINDOW_TOO_DEEP 4 /* a k-window crosses more nodes than the kernels' stacks hold: GKI_MAX_DEEP_WINDOW_NODES, for
                                     gki_finder_count / emit and for the early-stop search (gki_forward_*) alike -- both
                                     fall back to their slow path above GKI_MAX_WINDOW_NODES.  Also: an emit pass that
                                     had to leave records unwritten (gki_finder_synchronize, gki_forward_emit) */
#define GKI_ERR_STATE 5          /* call order violated (e.g. emit before count) */
#define GKI_ERR_OVERFLOW 6       /* a count does not fit the reference's dtype (e.g. int32 directory) */
#define GKI_ERR_NOT_ONE_REF_SUCC 7 /* the reference's AssertionError kmer_finder.py:402: a reachable window at the
                                     variant limit ends a node that does not have exactly one linear-ref successor */
#define GKI_ERR_OUT_OF_DOMAIN 8  /* gki_index_build_range_from_rows: the records lie outside the row-carrying build's domain (a
                                     group of neighbouring buckets with more than 2^22 records); build that slice from its
                                     columns (gki_index_build_range hands it to the pair-sorting form) */
#define GKI_ERR_INFLATE 9        /* gki_bgzf_inflate: a block's DEFLATE stream is malformed, or its output is not of the size or
                                     the CRC-32 its member states; first_bad_block / first_bad_status say which and how */

#define GKI_MAX_WINDOW_NODES 48        /* stacks of the product kernels (scratch) */
#define GKI_MAX_DEEP_WINDOW_NODES 12288 /* stacks of the slow path (a global-memory arena, grown 192, 384, ... levels): beyond
                                          the ~9 990 nodes at which the reference's own recursion ends in a RecursionError */
#define GKI_MAX_K 31             /* kmer_hashing.py:25 `assert k <= 31` */

/* ---------------------------------------------------------------- runtime */
const char *gki_last_error(void);
int gki_device_count(int *count);
int gki_set_device(int device);
int gki_malloc(void **d_ptr, int64_t bytes);
int gki_free(void *d_ptr);
/* gki_malloc / gki_free and the library's own temporaries go through a cache of freed blocks (a fresh hipMalloc of
 * tens of GB costs up to seconds on this stack); gki_trim returns the cache to the device.  GKI_POOL=0 disables it. */
int gki_trim(void);
/* What the device allocator itself cost this process so far: the calls that reached hipMalloc / hipFree (the pool
 * answers the others), the wall time spent inside them, and the bytes parked now.  hipMalloc / hipFree of tens of GB take
 * from tenths of a second to seconds on this stack; a benchmark that allocates inside its timed phases reports the
 * difference of two calls beside them. */
int gki_pool_stats(int64_t *n_device_mallocs, int64_t *n_device_frees, double *ms_in_malloc, double *ms_in_free,
                   int64_t *bytes_parked);
int gki_memcpy_h2d(void *d_dst, const void *h_src, int64_t bytes);
int gki_memcpy_d2h(void *h_dst, const void *d_src, int64_t bytes);
int gki_memcpy_d2d(void *d_dst, const void *d_src, int64_t bytes);
int gki_memset(void *d_dst, int value, int64_t bytes);
int gki_device_synchronize(void);
/* bytes free / total on the current device */
int gki_mem_info(int64_t *free_bytes, int64_t *total_bytes);
/* Order-independent checksums of a device column of n elements of 1, 2, 4 or 8 bytes (zero-extended): sum mod 2^64 and
 * xor.  Lets a caller check that two layouts / a set of shards hold the same multiset without copying it back. */
int gki_column_checksum(const void *d_column, int64_t n, int elem_bytes, uint64_t *sum, uint64_t *xor_fold);
/* Checking aid: the library's internal exclusive scan run alone, for tests that compare it with a host prefix sum (no
 * feature needs the call).  d_out[i] = d_in[0] + .. + d_in[i - 1] for i = 0..n, so d_out has n + 1 entries and
 * d_out[n] is the total.  kind 0: uint32 -> int64, 1: int32 -> int64, 2: uint32 -> uint32 (modulo 2^32).  Allocates its
 * own temporary, runs on stream 0 and returns when the result is there; n == 0 writes d_out[0] = 0.
 * GKI_ERR_BAD_ARG for another kind or a negative n. */
int gki_exclusive_scan(const void *d_in, int64_t n, int kind, void *d_out);
/* FlatKmers.get_new_without_singletons (flat_kmers.py:98-125): d_flags uint8[n] = 1 for every record whose hash also
 * occurs at an earlier position (the first occurrence of each hash gets 0); follow with gki_compact_flat. */
int gki_flag_repeated_kmers(const void *d_kmers, int64_t n, void *d_flags);
/* Stable compaction of FlatKmers columns: keeps record i iff d_flags[i] (uint8) != 0.  Output columns sized by the
 * caller (out_capacity records; the number of set flags is gki_column_checksum's sum for flags of 0/1). */
int gki_compact_flat(const void *d_flags, int64_t n, const void *d_hashes, const void *d_nodes, const void *d_ref_offsets,
                     const void *d_af32, void *d_out_hashes, void *d_out_nodes, void *d_out_ref_offsets, void *d_out_af32,
                     int64_t out_capacity, int64_t *n_out);

/* ---------------------------------------------------------------- hashing (A1, A8, A10)
 * hash = sum_i base[i] * 4^i, first base least significant, a/n/m=0 c=1 g=2 t=3
 * (flat_kmers.py:134-145, kmer_hashing.py:4-9, snp_kmer_finder.py:19-26). */

/* Every k-window of a numeric sequence: replaces np.convolve(seq, power_array(k), 'valid')
 * (read_kmers.py:67-70, kmer_finder.py:350-352).  d_codes: uint8[n]; d_out: uint64[n-k+1]. */
int gki_hash_sequence(const void *d_codes, int64_t n, int k, void *d_out);

/* Reads laid out back to back (read r = bytes [read_start[r], read_start[r+1]) of ASCII
 * letters); hashes of read r go to d_out[out_start[r] ...), out_start[r] = sum of
 * max(0, len-k+1) of earlier reads (computed by the call, also returned in d_out_start).
 * strand 0: forward (read_kmers.py:21-22); strand 1: reverse complement of the read
 * (read_kmers.py:23-26, Bio.Seq.reverse_complement then the same hash).
 * d_reads uint8[], d_read_start int64[n_reads+1], d_out_start int64[n_reads+1], d_out uint64[].
 * d_out NULL: count only -- d_out_start and *n_out are filled and d_reads is not read.
 * A read's k-mer count is kept in 32 bits: a read of more than 2^32 - 1 k-mers (2^32 + k - 1 letters or more) makes the
 * call return GKI_ERR_BAD_ARG with *n_out = 0, in count-only mode too, as gki_reads_parse_* refuses such a line. */
int gki_hash_reads(const void *d_reads, const void *d_read_start, int64_t n_reads, int k, int strand,
                   void *d_out_start, void *d_out, int64_t out_capacity, int64_t *n_out);

/* kmer_hashing.py:24-28 kmer_hashes_to_reverse_complement_hash / :31-36 complement.
 * d_in, d_out: uint64[n] (may alias). */
int gki_reverse_complement(const void *d_in, int64_t n, int k, void *d_out);
int gki_complement(const void *d_in, int64_t n, int k, void *d_out);

/* K-mers of a linear reference as FlatKmers columns: replaces SnpKmerFinder.find_kmers_on_linear_reference
 * (snp_kmer_finder.py:298-312) for every chunk of `make -R` (command_line_interface.py:105-153) in one call.
 * d_letters uint8[n_letters]: ASCII, either case; c/g/t are 1/2/3 and every other byte is 0 (flat_kmers.py:134-145).
 * The output is described by n_segments segments (host arrays h_seg_first, h_seg_count, int64): record j of a segment is
 * the k-mer at position h_seg_first[s] + j * spacing.  Segments follow each other in the output in table order and may
 * overlap or repeat.  with_reverse_complement: the h_seg_count[s] records of a segment are followed by as many records
 * whose hash is the reverse complement of theirs (kmer_hashing.py:24-28), the other columns repeated.
 * Columns (device, out_capacity records each): hashes uint64, nodes uint32 (all 1), ref_offsets uint64 (the position),
 * allele_frequencies float32 (all 1.0).  d_hashes NULL: count only (*n_out is set, nothing is written); d_nodes NULL:
 * hashes only.  kernel_ms NULL or float[2]: HIP-event times of the 2-bit pack and of the emit kernel.
 * GKI_ERR_BAD_ARG: k outside 1..31, spacing < 1, a segment whose last k-mer ends past the sequence (nothing is clipped
 * here), or *n_out > out_capacity. */
int gki_linear_kmers(const void *d_letters, int64_t n_letters, int k, int64_t spacing, const int64_t *h_seg_first,
                     const int64_t *h_seg_count, int64_t n_segments, int with_reverse_complement, void *d_hashes,
                     void *d_nodes, void *d_ref_offsets, void *d_af32, int64_t out_capacity, int64_t *n_out,
                     float *kernel_ms);

/* ---------------------------------------------------------------- graph (the obgraph arrays in HBM)
 * Replaces the per-node obgraph accessor calls of kmer_finder.py:50,62,259,279,350,384,138,143,374.
 * Host arrays in (copied to HBM, 2-bit packed on device):
 *   node_size int32[n_nodes]; seq uint8[n_bases] numeric bases, nodes concatenated in id order;
 *   edge_start int64[n_nodes+1] / edges int32[n_edges]   successors (CSR, get_edges order);
 *   rev_start  int64[n_nodes+1] / rev_edges int32[n_edges] predecessors (CSR);
 *   is_ref uint8[n_nodes] (is_linear_ref_node_or_linear_ref_dummy_node); allele_freq double[n_nodes];
 *   position_base int64[n_nodes] or NULL: PositionId.get(node, 0) (kmer_finder.py:117); NULL = the
 *   exclusive prefix sum of node_size. */
typedef struct gki_graph gki_graph;
int gki_graph_create(gki_graph **out, int64_t n_nodes, const int32_t *h_node_size,
                     const uint8_t *h_seq, int64_t n_bases,
                     const int64_t *h_edge_start, const int32_t *h_edges,
                     const int64_t *h_rev_start, const int32_t *h_rev_edges, int64_t n_edges,
                     const uint8_t *h_is_ref, const double *h_allele_freq,
                     const int64_t *h_position_base);
/* Same, but seq already resident in HBM as uint8[n_bases] (synthetic generators, sharded loaders). */
int gki_graph_create_dseq(gki_graph **out, int64_t n_nodes, const int32_t *h_node_size,
                          const void *d_seq, int64_t n_bases,
                          const int64_t *h_edge_start, const int32_t *h_edges,
                          const int64_t *h_rev_start, const int32_t *h_rev_edges, int64_t n_edges,
                          const uint8_t *h_is_ref, const double *h_allele_freq,
                          const int64_t *h_position_base);
/* Re-run the device-side preparation (2-bit pack, node-start bitmap + rank) from the resident
 * uint8 sequence; gki_graph_create already did it once.  Exposed so a benchmark can time it. */
int gki_graph_prepare(gki_graph *g);
int gki_graph_destroy(gki_graph *g);
int64_t gki_graph_n_bases(const gki_graph *g);

/* critical_graph_paths.py:42-104 CriticalGraphPaths.from_graph (host-side walk over the
 * linear reference; O(#linear nodes)).  h_chrom_start: chromosome start nodes.
 * Outputs sized n_nodes by the caller.  GKI_ERR_BAD_ARG when the reference would raise
 * (not exactly one linear successor :96-100, or offset -1 :104). */
int gki_critical_paths(int64_t n_nodes, const int32_t *h_node_size,
                       const int64_t *h_edge_start, const int32_t *h_edges,
                       const int64_t *h_rev_start, const uint8_t *h_is_ref,
                       const int32_t *h_chrom_start, int n_chrom, int k,
                       uint32_t *h_out_nodes, uint16_t *h_out_offsets, int64_t *n_out);
/* The same walk on the device, over a resident graph: next-node table -> pointer-doubling jump tables -> the path of
 * every chromosome -> depth / bp_since_last_join as prefix sums over the path -> the test, compacted in walk order
 * (csrc/gki_critical.hip).  Same outputs (host arrays sized n_nodes by the caller) and same errors as
 * gki_critical_paths; at most 64 chromosomes. */
int gki_graph_critical_paths(gki_graph *g, const int32_t *h_chrom_start, int n_chrom, int k, uint32_t *h_out_nodes,
                             uint16_t *h_out_offsets, int64_t *n_out);

/* ---------------------------------------------------------------- DenseKmerFinder (A3-A5)
 * Replaces DenseKmerFinder.find() (kmer_finder.py:179-244: search_from :254-347,
 * _process_whole_node :349-381, _search_next_nodes :383-417, _add_kmer :128-168).
 * Output = the reference's record multiset, ordered by end node; inside a node first the windows
 * that reach into predecessors (walk order over the predecessor lists, offset ascending inside one
 * step, nodes of a window ascending), then the offsets whose window lies inside the node. */
/* Record order.  BY_NODE: by end node; inside a node first the windows that reach into predecessors, then the
 * offsets whose window lies inside the node (on a linear graph this is the reference's order).  SPLIT: all
 * inside-the-node records first (by position), then all others (by end node) -- the same multiset in two dense
 * streams, which is what the writes like best; meant for consumers that sort anyway (the index build). */
#define GKI_LAYOUT_BY_NODE 0
#define GKI_LAYOUT_SPLIT 1
/* Per-node flag word (uint16: GKI_NODE_* byte | history bound << 8) of gki_find_params.h_node_flags, computed by
 * gki_classify_nodes (host).  History bound: an upper bound (saturating at 255) on the distinct non-linear-ref nodes any
 * backward path holds in the k bases before the node -- when window + bound stay under the limit, any history will do.  The search of
 * kmer_finder.py:383-417 reaches a window iff SOME history satisfied the variant limit at every step into a node whose
 * entry is not free (free: linear-ref(-dummy) node, or a forced `only_follow_nodes` successor :386-388).  Walking
 * backwards, a history need not be enumerated past a node with GKI_NODE_T: a linear-ref node reachable through >= k
 * linear-ref bases (or from a chromosome start) -- that history adds no variant node to any later window and is always
 * allowed, so it dominates every other one. */
#define GKI_NODE_REF 1       /* is_linear_ref_node_or_linear_ref_dummy_node: not counted by the variant limit */
#define GKI_NODE_FORCED 2    /* member of only_follow_nodes */
#define GKI_NODE_T 4         /* see above */
#define GKI_NODE_SIMPLE 8    /* not T, but a predecessor is: the history through that predecessor dominates */
#define GKI_NODE_NESTED 16   /* not T, no T predecessor: histories are enumerated through its predecessors */
#define GKI_NODE_CHECK 32    /* has successors, none of them forced, and not exactly one linear-ref successor (:402) */
#define GKI_NODE_HFS 64      /* has a forced successor: its edges to other successors do not exist for the search */
#define GKI_NODE_DEAD 128    /* exact: the search never enters the node (no alive edge from an entered node, or no history
                                within the limit): no records, never stepped on */
/* Host, one pass in topological order, O(nodes + edges) plus a backward enumeration for every non-free NESTED node.
 * h_follow: uint8[n_nodes] membership of only_follow_nodes or NULL; h_roots: the nodes a search starts from with no
 * history -- chromosome starts and every critical node (kmer_finder.py:190-232: each critical point starts its own search).
 * h_out_flags uint16[n_nodes].  *general = 1 if any node is NESTED / CHECK / HFS / FORCED or cut off, i.e.
 * gki_finder_count needs the flags; 0 = the graph is in the class where "at most max_variant_nodes variant nodes in
 * the window" is the whole rule and h_node_flags may stay NULL.  GKI_ERR_BAD_ARG if the graph has a cycle. */
int gki_classify_nodes(int64_t n_nodes, const int32_t *h_node_size, const int64_t *h_edge_start, const int32_t *h_edges,
                       const int64_t *h_rev_start, const int32_t *h_rev_edges, const uint8_t *h_is_ref,
                       const uint8_t *h_follow, const int32_t *h_roots, int n_roots, int k, int max_variant_nodes,
                       uint16_t *h_out_flags, int32_t *general);

typedef struct {
    uint32_t struct_size;         /* sizeof(gki_find_params): a binding built against another layout is refused */
    int32_t k;                    /* 1..31 */
    int32_t max_variant_nodes;    /* kmer_finder.py:42 */
    int32_t one_node_per_kmer;    /* only_save_one_node_per_kmer :145-146 */
    int32_t layout;               /* GKI_LAYOUT_BY_NODE or GKI_LAYOUT_SPLIT: order of the records in the output */
    /* end positions processed: (node_begin, off_begin) inclusive .. (node_end, off_end) exclusive,
     * in (node id, offset) order -- the chunking of command_line_interface.py:588-601.  Whole
     * graph: node_begin = 0, off_begin = 0, node_end = n_nodes, off_end = 0. */
    int64_t node_begin, off_begin, node_end, off_end;
    /* per-node critical offset for lossy restarts (0 < c < k-1, SURVEY.md 8a' E1), uint16[n_nodes],
     * 0xFFFF = none; NULL when the graph has none. */
    const uint16_t *h_lossy_crit;
    /* host int32[n_nodes] or NULL.  NULL: node ids increase along every edge and the run is the id range
     * [node_begin, node_end].  Otherwise a topological rank of every node (gki_topological_rank): the run is the nodes
     * whose rank lies between the ranks of node_begin and node_end (node_end == n_nodes: to the end); costs a pass
     * over all nodes instead of over the run's. */
    const int32_t *h_node_rank;
    /* host uint16[n_nodes] from gki_classify_nodes, or NULL when it reported general == 0. */
    const uint16_t *h_node_flags;
    /* host uint8[n_nodes] membership of only_store_nodes (kmer_finder.py:153) or NULL: a record is written only for a
     * node in the set -- except the records of the bulk path (offsets k+2 .. size-2 of a node longer than 2k+3), which
     * the reference writes regardless (:370-374).  Needs h_node_flags (the general kernels apply it). */
    const uint8_t *h_store_nodes;
    /* The same four tables already RESIDENT on the finder's device (same dtypes and lengths); a non-NULL d_ pointer is
     * used as it is and its h_ twin is ignored: nothing is uploaded by gki_finder_count.  For chunked runs (one count per
     * chunk of critical-path numbers, every `index -t N` rank) and for flags that gki_graph_classify_nodes left on the
     * device.  The tables must stay valid until the emit that follows the count has completed.  With d_node_rank the
     * ranks of node_begin and node_end come in rank_begin / rank_end (node_end == n_nodes: INT32_MAX). */
    const uint16_t *d_lossy_crit;
    const int32_t *d_node_rank;
    const uint16_t *d_node_flags;
    const uint8_t *d_store_nodes;
    int32_t rank_begin, rank_end;
} gki_find_params;
/* sizeof(gki_find_params) of this build, for bindings to check at load time. */
int64_t gki_find_params_size(void);

/* gki_classify_nodes on the device, over a resident graph (csrc/gki_classify.hip): the classes are a least fixed point
 * ("entered" spreads from the search roots, the linear-ref run before a node and the variant bound only grow), reached
 * by relaxation sweeps instead of one pass in topological order; whether a nested non-free node has an admissible history
 * is enumerated on the device as well, in rounds with the relaxation (a node without one is dead, which takes histories
 * away from the nodes after it).  *needs_host = 1 when the call cannot finish the job -- a history deeper than 64 nodes
 * or longer than 2^20 steps, more than 48 rounds, or a dependency chain that outlasts the sweep budget -- then nothing
 * is written and the caller runs gki_classify_nodes.
 * h_out_flags (host uint16[n_nodes] or NULL) is filled when the graph is general, or always with always_copy_flags. */
int gki_graph_classify_nodes(gki_graph *g, const uint8_t *h_follow, const int32_t *h_roots, int n_roots, int k,
                             int max_variant_nodes, uint16_t *h_out_flags, int always_copy_flags, int32_t *general,
                             int32_t *needs_host);

/* Host: a topological rank of every node (Kahn; ties by node id), for gki_find_params.h_node_rank.  GKI_ERR_BAD_ARG if
 * the graph has a cycle. */
int gki_topological_rank(int64_t n_nodes, const int64_t *edge_start, const int32_t *edges, int32_t *out_rank);

typedef struct gki_finder gki_finder;
int gki_finder_create(gki_graph *g, gki_finder **out);
int gki_finder_destroy(gki_finder *f);
/* pass 1: counts records (device count pass + prefix sums); returns the total. */
int gki_finder_count(gki_finder *f, const gki_find_params *p, int64_t *n_records);
/* pass 2, FlatKmers layout after FlatKmers.from_multiple_flat_kmers (flat_kmers.py:71-90):
 * hashes uint64, nodes uint32, ref_offsets uint64 (= position id of the END position,
 * kmer_finder.py:116-117), allele_frequencies float32.  Any pointer may be NULL (column skipped). */
int gki_finder_emit_flat(gki_finder *f, void *d_hashes, void *d_nodes, void *d_ref_offsets, void *d_af32);
/* pass 2, get_flat_kmers(v="2") layout (kmer_finder.py:124-126): hashes int64, start_nodes int32,
 * start_offsets int16, nodes int32, allele_frequencies float64. */
int gki_finder_emit_v2(gki_finder *f, void *d_hashes, void *d_start_nodes, void *d_start_offsets,
                       void *d_nodes, void *d_af64);
/* Waits for the emit kernels; GKI_ERR_WINDOW_TOO_DEEP if an emit kernel had to leave records unwritten (all-nodes mode:
 * 64 consecutive nodes hold more than 2^32 records between them -- run such a graph in chunks of nodes). */
int gki_finder_synchronize(gki_finder *f);
/* HIP-event time of the most recent launch of one kernel of this finder (after synchronize).
 * which: 0 count-boundary, 1 emit-interior, 2 emit-boundary, 3 scans (sum), 4 graph prepare. */
int gki_finder_kernel_ms(gki_finder *f, int which, float *ms);
/* Records written by the interior kernel in the last emit (for roofline accounting). */
int64_t gki_finder_interior_records(const gki_finder *f);

/* Forward windows from given start positions: replaces DenseKmerFinder.find_only_kmers_starting_at_position
 * (kmer_finder.py:170-177): for every start position (d_nodes[i], d_offsets[i]) every forward path of exactly k
 * bases gives one window; records carry the END position like all finder records.  count -> emit; records of
 * start position i are [rec_start[i], rec_start[i+1]) in depth-first successor order (the reference's order).
 * d_nodes int32[n_pos], d_offsets int32[n_pos], d_rec_start int64[n_pos+1]; output = the v2 columns.
 * d_follow: uint8[n_nodes] membership of only_follow_nodes (:386-388) or NULL.
 * The first search on a graph (and the first after gki_graph_prepare) builds the search's per-node records: 32 bytes per
 * node, owned by the graph and freed with it.
 * gki_forward_count may leave the finished k-mers in a buffer owned by the graph (193 bytes per start position, both
 * modes); the next gki_forward_emit with the SAME arguments expands them instead of walking again and releases the buffer.
 * Any other sequence of calls (count(A), count(B), emit(A); a second emit) is answered by walking, and the emit pass
 * settles by itself whether it needs the slow path's deeper stacks: the results are the same.  The slow path's arena
 * (up to 5.6 GB) goes back to the library's pool when the emit call returns.  Calls on one graph handle must not overlap
 * in time (two host threads sharing a graph serialise their searches). */
int gki_forward_count(gki_graph *g, int k, int max_variant_nodes, int one_node, const void *d_follow,
                      const void *d_nodes, const void *d_offsets, int64_t n_pos, void *d_rec_start,
                      int64_t *n_records);
int gki_forward_emit(gki_graph *g, int k, int max_variant_nodes, int one_node, const void *d_follow,
                     const void *d_nodes, const void *d_offsets, int64_t n_pos, const void *d_rec_start, void *d_hashes,
                     void *d_start_nodes, void *d_start_offsets, void *d_nodes_out, void *d_af64);

/* ---------------------------------------------------------------- CollisionFreeKmerIndex (A9)
 * Build: replaces CollisionFreeKmerIndex.from_flat_kmers (collision_free_kmer_index.py:423-467)
 * and set_frequencies (:267-293).  Inputs are device columns of n records; outputs are device
 * arrays sized by the caller: hashes_to_index int32[modulo], n_kmers uint32[modulo], and the
 * permuted payload kmers uint64[n], nodes uint32[n], ref_offsets uint64[n], af float32[n],
 * frequencies uint16[n], and optionally the permutation uint32[n] (`sorting` of :435; NULL to skip)
 * so a caller can permute columns of other dtypes itself.  The sort is stable: inside a bucket
 * records keep their input order (np.argsort leaves it unspecified).
 * GKI_ERR_OVERFLOW if n >= 2^31 (the reference's directory is int32, :453). */
int gki_index_build(const void *d_kmers, const void *d_nodes, const void *d_ref_offsets, const void *d_af32,
                    int64_t n, uint64_t modulo, int skip_frequencies,
                    void *d_hashes_to_index, void *d_n_kmers,
                    void *d_out_kmers, void *d_out_nodes, void *d_out_ref_offsets, void *d_out_af32,
                    void *d_out_frequencies, void *d_out_permutation);

/* Bucket-range partitioned build.  Part p of n_parts owns the buckets
 * [modulo*p/n_parts, modulo*(p+1)/n_parts) (integer division): every GPU sorts and owns 1/n_parts of the directory,
 * which removes the redundant full sort of the all-gather build and the 2^31-records-per-index limit.
 * gki_partition_by_bucket_range: stable partition of n records (any number: more than 2^31 - 1 are taken in several
 *   passes whose runs of a part are laid out behind each other) by part; h_part_start[n_parts+1] (host) receives the
 *   slice boundaries in the output columns.  n_parts <= 256.  The output columns must not overlap the input.
 * gki_partition_by_bucket_range_chunked: the same with at most max_rows_per_pass records per pass (0: the default);
 *   bounds the pass's temporaries (a histogram entry per part and 4096 records).
 * gki_index_build_range: gki_index_build for the records of one slice: directory arrays int32 / uint32 [n_buckets],
 *   indexed by bucket - bucket_begin; a record whose bucket lies outside the range is GKI_ERR_BAD_ARG. */
int gki_partition_by_bucket_range(const void *d_kmers, const void *d_nodes, const void *d_ref_offsets, const void *d_af32,
                                  int64_t n, uint64_t modulo, int n_parts, void *d_out_kmers, void *d_out_nodes,
                                  void *d_out_ref_offsets, void *d_out_af32, int64_t *h_part_start);
int gki_partition_by_bucket_range_chunked(const void *d_kmers, const void *d_nodes, const void *d_ref_offsets,
                                          const void *d_af32, int64_t n, uint64_t modulo, int n_parts,
                                          int64_t max_rows_per_pass, void *d_out_kmers, void *d_out_nodes,
                                          void *d_out_ref_offsets, void *d_out_af32, int64_t *h_part_start);
int gki_index_build_range(const void *d_kmers, const void *d_nodes, const void *d_ref_offsets, const void *d_af32,
                          int64_t n, uint64_t modulo, uint64_t bucket_begin, uint64_t n_buckets, int skip_frequencies,
                          void *d_hashes_to_index, void *d_n_kmers,
                          void *d_out_kmers, void *d_out_nodes, void *d_out_ref_offsets, void *d_out_af32,
                          void *d_out_frequencies, void *d_out_permutation);
/* Grouped partition and build: one sort pass less per slice on ONE GPU (the slices of a whole-genome index: 26 key bits at
 * 7 records per bucket = 7 bits grouped + one pass of 10 + 9 in LDS, against two passes without the grouping; the whole index
 * of the 3 Gbp graph in 187 ms against 195).
 * gki_partition_by_bucket_range_grouped: as _chunked, and the records of part p additionally leave grouped (stably) by
 *   the top group_bits bits of their key in that part (key = bucket - part begin; "top bits" = key >> (bits of the part's
 *   largest key - group_bits), 0 when the key has fewer bits): h_start[(n_parts << group_bits) + 1], entry
 *   p << group_bits | g = first row of group g of part p.  n_parts << group_bits <= 1024.  group_bits = 0: _chunked.
 * gki_index_build_range_grouped: gki_index_build_range for records that arrive so grouped: h_group_start[2^group_bits + 1]
 *   = the part's slice of that table, relative to the part's first row.  Same outputs, element by element. */
int gki_partition_by_bucket_range_grouped(const void *d_kmers, const void *d_nodes, const void *d_ref_offsets,
                                          const void *d_af32, int64_t n, uint64_t modulo, int n_parts, int group_bits,
                                          int64_t max_rows_per_pass, void *d_out_kmers, void *d_out_nodes,
                                          void *d_out_ref_offsets, void *d_out_af32, int64_t *h_start);
int gki_index_build_range_grouped(const void *d_kmers, const void *d_nodes, const void *d_ref_offsets, const void *d_af32,
                                  int64_t n, uint64_t modulo, uint64_t bucket_begin, uint64_t n_buckets,
                                  int skip_frequencies, int group_bits, const int64_t *h_group_start,
                                  void *d_hashes_to_index, void *d_n_kmers,
                                  void *d_out_kmers, void *d_out_nodes, void *d_out_ref_offsets, void *d_out_af32,
                                  void *d_out_frequencies, void *d_out_permutation);
/* The same pair with the partitioned records kept as ROWS between the two calls -- what the whole-genome index on one GPU
 * uses (collision_free_kmer_index.PartitionedDeviceIndex): with hundreds of digits a run of a few records is one
 * contiguous piece as rows and four short ones as columns.
 * gki_partition_rows_by_bucket_range: d_rows uint64[3 * n] (per record: k-mer, ref offset, node | allele frequency bits
 *   << 32), d_keys uint32[n] (the bucket's offset in its part), both device buffers of the caller; h_start as above.
 * gki_index_build_range_from_rows: the slice build from one part's rows and keys (pointers into those buffers at the
 *   part's first record, n = its records, h_group_start relative to it).  No permutation output.  A key outside
 *   [0, n_buckets) is GKI_ERR_BAD_ARG; GKI_ERR_OUT_OF_DOMAIN when the records need the pair-sorting form. */
int gki_partition_rows_by_bucket_range(const void *d_kmers, const void *d_nodes, const void *d_ref_offsets,
                                       const void *d_af32, int64_t n, uint64_t modulo, int n_parts, int group_bits,
                                       int64_t max_rows_per_pass, void *d_rows, void *d_keys, int64_t *h_start);
int gki_index_build_range_from_rows(const void *d_rows, const void *d_keys, int64_t n, uint64_t modulo,
                                    uint64_t bucket_begin, uint64_t n_buckets, int skip_frequencies, int group_bits,
                                    const int64_t *h_group_start, void *d_hashes_to_index, void *d_n_kmers,
                                    void *d_out_kmers, void *d_out_nodes, void *d_out_ref_offsets, void *d_out_af32,
                                    void *d_out_frequencies);
/* The build has two forms with identical results.  gki_index_build(_range) runs the row-carrying form (the 24-byte
 * payload travels with its key through stable partition passes, the last bits are sorted inside LDS; no random access)
 * and hands over to the pair-sorting form (stable LSD sort of (bucket, index) pairs, then one gather of the payload)
 * when a group of 2^L neighbouring buckets holds more than 2^22 records (an index that is a handful of buckets).
 * gki_index_build_pairs runs the pair-sorting form directly: same arguments, same outputs. */
int gki_index_build_pairs(const void *d_kmers, const void *d_nodes, const void *d_ref_offsets, const void *d_af32,
                          int64_t n, uint64_t modulo, uint64_t bucket_begin, uint64_t n_buckets, int skip_frequencies,
                          void *d_hashes_to_index, void *d_n_kmers,
                          void *d_out_kmers, void *d_out_nodes, void *d_out_ref_offsets, void *d_out_af32,
                          void *d_out_frequencies, void *d_out_permutation);

/* ---------------------------------------------------------------- ReverseKmerIndex
 * Replaces ReverseKmerIndex.from_flat_kmers (reverse_kmer_index.py:47-60): records stably sorted by
 * node.  Inputs: device columns nodes uint32[n], kmers uint64[n], ref_offsets uint64[n]; n_nodes =
 * max node id + 1.  Outputs (device, sized by the caller): index_positions uint32[n_nodes] (first
 * record of the node, 0 if none), n_hashes uint16[n_nodes] (records of the node, modulo 2^16 as the
 * NumPy assignment at :56 stores it), and the permuted kmers / ref_offsets uint64[n].
 * Built by the row-carrying form of the index build with the node id as the key; the pair-sorting form it replaced
 * answers what that form declines, and every call when the environment holds GKI_REVERSE_FORM=pairs (read per call;
 * for the parity tests of that path).  A node id >= n_nodes is GKI_ERR_BAD_ARG. */
int gki_reverse_index_build(const void *d_nodes, const void *d_kmers, const void *d_ref_offsets, int64_t n,
                            int64_t n_nodes, void *d_index_positions, void *d_n_hashes, void *d_out_kmers,
                            void *d_out_ref_offsets);

/* Probe: replaces a loop of CollisionFreeKmerIndex.get (:303-315) over q queries
 * (get_nodes_and_ref_offsets_from_multiple_kmers :354-376).  count -> emit.
 * d_hit_start int64[q+1]: hits of query i are [hit_start[i], hit_start[i+1]) in bucket order;
 * a query with no hit, or whose first hit has frequency > max_hits, contributes none.
 * Emit columns (any may be NULL): nodes uint32, ref_offsets uint64, query index int64
 * (`read_offsets` of :365), frequencies uint16, af float32, and the hit's position int64 in the
 * payload arrays (lets a caller gather from its own columns of any dtype). */
typedef struct {
    const void *d_hashes_to_index, *d_n_kmers, *d_kmers, *d_nodes, *d_ref_offsets, *d_frequencies, *d_af32;
    uint64_t modulo;
    int64_t n;
    /* bucket-range slice (gki_index_build_range): the directory arrays hold buckets [bucket_begin, bucket_begin +
     * n_buckets) only and a k-mer whose bucket lies outside is a miss; n_buckets == 0 means the whole [0, modulo). */
    uint64_t bucket_begin, n_buckets;
} gki_index_view;
int gki_index_lookup_count(const gki_index_view *ix, const void *d_queries, int64_t q, int64_t max_hits,
                           void *d_hit_start, int64_t *n_hits);
/* Node counting fused with the probe: d_counts[node] += 1 (uint32[n_counts], caller-zeroed or accumulated across
 * batches) for every hit of every query -- what kmer_mapper's map_kmers_to_graph_index gives KAGE
 * (collision_free_kmer_index.py:210-212) and CounterKmerIndex.get_node_counts (:39-40). */
int gki_index_count_nodes(const gki_index_view *ix, const void *d_queries, int64_t q, int64_t max_hits,
                          void *d_counts, int64_t n_counts);
int gki_index_lookup_emit(const gki_index_view *ix, const void *d_queries, int64_t q, int64_t max_hits,
                          const void *d_hit_start, void *d_hit_nodes, void *d_hit_ref_offsets,
                          void *d_hit_query, void *d_hit_frequencies, void *d_hit_af32, void *d_hit_position);

/* CollisionFreeKmerIndex.get (:303-315) for a few k-mers from HOST memory (q <= 64): one launch, one wave per query,
 * queries and results travel through pinned host memory the kernel addresses directly.  h_n_hits[i] = number of hits of
 * query i (0 for a miss or when the first hit's frequency exceeds max_hits); its first min(h_n_hits[i], 1024,
 * capacity_per_query) payload positions, in bucket order, are h_positions[i * capacity_per_query ...].  A caller that
 * sees more hits than it got positions for uses the batched gki_index_lookup_* pair. */
int gki_index_get_small(const gki_index_view *ix, const uint64_t *h_queries, int q, int64_t max_hits,
                        int64_t *h_n_hits, int64_t *h_positions, int64_t capacity_per_query);

/* ---------------------------------------------------------------- UniqueVariantKmersFinder (dense path)
 * unique_variant_kmers.py:114-270: per variant, the k-mers that stand for its ref and alt node, chosen among its
 * P = len(range(2, k-2)[::4]) start positions.  Steps (graph_kmer_index_amd/unique_variant_kmers.py drives them):
 * gki_uvk_starts -> gki_forward_count / gki_forward_emit over all starts (no store filter, both nodes per window) ->
 * gki_uvk_summarize -> gki_uvk_select -> gki_uvk_emit.  Start i of variant v is v * P + i, farthest from POS first.
 *
 * gki_uvk_starts: d_lin_start int64[n_lin] ascending linear-ref offsets of the first base of the linear-ref nodes of
 *   nonzero size d_lin_node int32[n_lin]; d_var_ref_offset int64[n_var] = graph ref offset of POS (chromosome's start
 *   offset + POS).  Writes (node, offset) int32 of every start and its variant int32.  *first_bad_variant = the lowest
 *   variant with a start before 0 or past the linear path (-1: none); such starts get (0, 0).
 * gki_uvk_summarize: one gki_uvk_summary per start from the forward search's v2 columns (records of start i are
 *   [rec_start[i], rec_start[i+1])) and the frequency index: n_ref / n_alt records of the ref / alt node (n_alt stays 0
 *   when alt == ref), f_ref / f_alt their maximum CollisionFreeKmerIndex.get_frequency (first hit of h plus first hit of
 *   its 31-mer reverse complement), flags bit 0: a hash lies on a ref window and on an alt window among the first 500
 *   windows (for alt == ref: a ref window among them), bit 1: alt == ref.
 * gki_uvk_select: rules 5-6 per variant for store set d_store_mask uint8[n_var] (bit 0 ref stored, bit 1 alt stored;
 *   NULL = both): d_choice int32[n_var] the chosen start (0..P-1), d_out_start int64[n_var+1] the exclusive scan of
 *   the chosen records, *n_records the total.
 * gki_uvk_emit: the chosen records of the stored nodes in emission order, as FlatKmers columns (uint64, uint32,
 *   uint64 = position id of the record's end position, float32). */
typedef struct {
    uint32_t n_ref, n_alt, f_ref, f_alt, flags;
} gki_uvk_summary;
int gki_uvk_starts(gki_graph *g, const void *d_lin_start, const void *d_lin_node, int64_t n_lin,
                   const void *d_var_ref_offset, int64_t n_var, int n_starts_per_variant, void *d_nodes, void *d_offsets,
                   void *d_variant, int64_t *first_bad_variant);
int gki_uvk_summarize(gki_graph *g, const gki_index_view *ix, const void *d_rec_start, int64_t n_var,
                      int n_starts_per_variant, const void *d_hashes, const void *d_start_nodes, const void *d_start_offsets,
                      const void *d_nodes, const void *d_ref_nodes, const void *d_alt_nodes, void *d_summary);
/* gki_uvk_summarize with a gki_counter (below) as frequency source: f_ref / f_alt are maxima of KmerCounter.get_frequency,
 * the count of the hash alone with no reverse complement added, stored as 2^32 - 1 when above it. */
typedef struct gki_counter gki_counter;
int gki_uvk_summarize_counter(gki_graph *g, const gki_counter *counter, const void *d_rec_start, int64_t n_var,
                              int n_starts_per_variant, const void *d_hashes, const void *d_start_nodes,
                              const void *d_start_offsets, const void *d_nodes, const void *d_ref_nodes,
                              const void *d_alt_nodes, void *d_summary);
int gki_uvk_select(const void *d_summary, int64_t n_var, int n_starts_per_variant, int choose_lowest,
                   const void *d_store_mask, void *d_choice, void *d_out_start, int64_t *n_records);
int gki_uvk_emit(gki_graph *g, const void *d_rec_start, int64_t n_var, int n_starts_per_variant, const void *d_choice,
                 const void *d_store_mask, const void *d_ref_nodes, const void *d_alt_nodes, const void *d_out_start,
                 const void *d_hashes, const void *d_start_nodes, const void *d_start_offsets, const void *d_nodes,
                 const void *d_af64, void *d_out_hashes, void *d_out_nodes, void *d_out_ref_offsets, void *d_out_af32);

/* ---------------------------------------------------------------- variant k-mers by simple selection
 * unique_variant_kmers.py:66-111, 241-269 (use_simple=True, make_unique_variant_kmers -S True): for every variant one
 * early-stop search for its ref node, then one for its alt node, each with only_store_nodes = only_follow_nodes = {node}.
 * No frequency index, no choice among start positions.  Steps (graph_kmer_index_amd/unique_variant_kmers.py drives them):
 * gki_uvk_simple_starts -> gki_forward_node_count -> gki_forward_node_emit.  Search 2 v is variant v's ref node, 2 v + 1
 * its alt node.
 *
 * gki_uvk_simple_starts: d_lin_start / d_lin_node / d_var_ref_offset as for gki_uvk_starts; d_is_snp uint8[n_var] (REF and
 *   ALT one base long); d_ref_nodes / d_alt_nodes int32[n_var].  Writes int32[2 n_var] each: the start (node, offset) and
 *   the search's target node.  A SNP's node with bases starts at (node, 0); an indel's node, and a SNP's empty node, at
 *   the linear-ref position 8 bases before P (0-based chromosome offset P = POS for an indel, POS - 1 for a SNP).
 *   *first_bad_variant = the lowest variant with such a start before 0 or past the linear path, or with a node outside
 *   the graph (-1: none); its starts get (0, 0).
 * gki_forward_node_count / _emit: the early-stop search of gki_forward_* in which start position i follows and stores
 *   d_targets[i] alone: where a node on the path has the target among its successors only the target is taken and the
 *   variant limit is waived for that step; a finished k-mer gives one record, of the target, when the target is on its
 *   path.  Records of start i are [rec_start[i], rec_start[i+1]) in depth-first successor order.  Output = FlatKmers
 *   columns written by the walk: d_hashes uint64, d_nodes_out uint32, d_position_ids uint64 = position base of the END
 *   node + END offset (at full width, not through an int16 column), d_af32 float32 = the path's minimum allele frequency.
 *   Errors, the slow path for deep windows and its arena are those of gki_forward_count / gki_forward_emit
 *   (GKI_ERR_NOT_ONE_REF_SUCC where the reference asserts, GKI_ERR_WINDOW_TOO_DEEP for the refusals).  The count pass
 *   leaves no script for the emit pass: the emit pass always walks, so any sequence of calls is answered alike. */
int gki_uvk_simple_starts(gki_graph *g, const void *d_lin_start, const void *d_lin_node, int64_t n_lin,
                          const void *d_var_ref_offset, const void *d_is_snp, const void *d_ref_nodes,
                          const void *d_alt_nodes, int64_t n_var, void *d_nodes, void *d_offsets, void *d_targets,
                          int64_t *first_bad_variant);
int gki_forward_node_count(gki_graph *g, int k, int max_variant_nodes, const void *d_targets, const void *d_nodes,
                           const void *d_offsets, int64_t n_pos, void *d_rec_start, int64_t *n_records);
int gki_forward_node_emit(gki_graph *g, int k, int max_variant_nodes, const void *d_targets, const void *d_nodes,
                          const void *d_offsets, int64_t n_pos, const void *d_rec_start, void *d_hashes,
                          void *d_nodes_out, void *d_position_ids, void *d_af32);

/* ---------------------------------------------------------------- sample_kmers_from_structural_variants
 * structural_variants.py:6-43: extra signature k-mers of big variant nodes.  d_cand_nodes int32[n_cand] are the nodes in
 * visiting order (every (ref, var) pair flattened, ref first; duplicates stay and give their records again).  A candidate
 * is looked at when its size exceeds k + 5; its windows j = 0 .. size - k are hashed from the packed sequence, window j is
 * valid when CollisionFreeKmerIndex.get_frequency (first hit of h plus first hit of its 31-mer reverse complement, as in
 * gki_uvk_summarize) is below max_frequency, and valid windows are chosen in ascending order iff they lie k or more after
 * the previous chosen one.
 * gki_sv_sample_count: probes every window once into a bitmap the plan keeps, counts the chosen windows per candidate;
 *   d_rec_start (nullable) int64[n_cand + 1] = their exclusive scan, *n_records the total, *plan what the emit call
 *   needs (release it with gki_sv_sample_destroy; the graph must outlive it).  kernel_ms (nullable) float[2]: probe pass,
 *   greedy count pass with its scan.  GKI_ERR_BAD_ARG: k outside 1..31, max_frequency < 0, no index, a candidate that is
 *   not a node of the graph (nothing is read through it).
 * gki_sv_sample_emit: the records of candidate i at [rec_start[i], rec_start[i+1]) in window order: hashes uint64, nodes
 *   uint32, and when given ref_offsets uint64 (all 0) and allele frequencies float32 (all 1), each sized n_records.
 *   kernel_ms (nullable) float[1]: greedy emit pass and record pass. */
typedef struct gki_sv_plan gki_sv_plan;
int gki_sv_sample_count(gki_graph *g, const gki_index_view *ix, const void *d_cand_nodes, int64_t n_cand, int k,
                        int64_t max_frequency, void *d_rec_start, int64_t *n_records, gki_sv_plan **plan,
                        float *kernel_ms);
int gki_sv_sample_emit(gki_sv_plan *plan, void *d_hashes, void *d_nodes, void *d_ref_offsets, void *d_af32,
                       float *kernel_ms);
int gki_sv_sample_destroy(gki_sv_plan *plan);
/* gki_sv_sample_count with a gki_counter as frequency source (window j is valid when the count of its hash alone is below
 * max_frequency); the plan is emitted and destroyed like any other. */
int gki_sv_sample_count_counter(gki_graph *g, const gki_counter *counter, const void *d_cand_nodes, int64_t n_cand, int k,
                                int64_t max_frequency, void *d_rec_start, int64_t *n_records, gki_sv_plan **plan,
                                float *kernel_ms);

/* ---------------------------------------------------------------- k-mer counting (KmerCounter, KmerFrequencyIndex)
 * np.unique(kmers[::stride], return_counts=True) of the reference (kmer_counter.py:24-43, kmer_frequency_index.py:18-25) on
 * the device: a key-only stable radix sort, least significant 8-bit digit first, then run lengths.
 * gki_unique_counts_count: d_kmers uint64[n], every stride-th of them taken (stride >= 1), read in place and never
 *   written; key_bits in 1..64 (2k for k-mer hashes): digits above it are not sorted on, a key that does not fit is
 *   GKI_ERR_BAD_ARG.  n in 0..2^33.  *n_unique = number of distinct keys, *plan what the emit call needs (release it with
 *   gki_unique_counts_destroy).  kernel_ms (nullable) float[2]: the sort, the run-head count with its scan.  A failed
 *   allocation is GKI_ERR_HIP with HIP's out-of-memory message, and nothing stays allocated.
 * gki_unique_counts_emit: d_unique uint64[n_unique] ascending, d_counts int64[n_unique] exact.  kernel_ms (nullable)
 *   float[1]. */
typedef struct gki_unique_plan gki_unique_plan;
int gki_unique_counts_count(const void *d_kmers, int64_t n, int64_t stride, int key_bits, int64_t *n_unique,
                            gki_unique_plan **plan, float *kernel_ms);
int gki_unique_counts_emit(gki_unique_plan *plan, void *d_unique, void *d_counts, float *kernel_ms);
int gki_unique_counts_destroy(gki_unique_plan *plan);
/* A counter over ascending distinct keys (uint64[n_unique], all below 2^key_bits) and their counts (int64[n_unique]), both
 * of which must outlive it: a prefix directory over the keys' top bits (2^P + 1 int64 entries, 2^P in (n / 4, n / 2], at
 * most 2^28) narrows a lookup to a bucket of a few keys.  gki_counter_lookup: d_out int64[q], the count of every query
 * (uint64[q]) or 0 when it is absent -- KmerCounter.get_frequency (kmer_counter.py:72-74), no reverse complement. */
int gki_counter_create(const void *d_unique, const void *d_counts, int64_t n_unique, int key_bits, gki_counter **out);
int gki_counter_lookup(gki_counter *c, const void *d_queries, int64_t q, void *d_out);
int gki_counter_destroy(gki_counter *c);

/* ---------------------------------------------------------------- probe table (read-side hot loop)
 * A device-only re-layout of an index for counting: dir uint2[modulo] = {first record, count (16 bit, saturating)
 * | 16-bit fingerprint set << 16}, rows uint4[n] = {kmer, node, frequency}: one random 64-byte sector per query,
 * one more per candidate bucket (the reference layout touches five arrays per hit).  Costs modulo*8 + n*16 bytes
 * of HBM.  The view's d_n_kmers must outlive the probe (read for buckets of >= 65535 records).
 * gki_probe_count_nodes       = gki_index_count_nodes on the table; *n_hits (nullable) = hits counted.
 * gki_probe_reads_count_nodes = ReadKmers hashing (read_kmers.py:21-26,70) fused with the probe: reads are ASCII
 *   letters uint8[] with int64 read_start[n_reads+1]; strands bit 0 = forward k-mers, bit 1 = k-mers of the
 *   reverse-complemented read; no k-mer array is materialised.  *n_kmers (nullable) = k-mers probed. */
typedef struct gki_probe gki_probe;
int gki_probe_create(const gki_index_view *ix, gki_probe **out);
int gki_probe_destroy(gki_probe *p);
int gki_probe_count_nodes(gki_probe *p, const void *d_queries, int64_t q, int64_t max_hits, void *d_counts,
                          int64_t n_counts, int64_t *n_hits);
/* gki_index_lookup_count / _emit on the table: d_hit_start int64[q+1] as above; the emit pass writes the query index and
 * the hit's position in the payload arrays (int64 each), from which a caller gathers any column. */
int gki_probe_lookup_count(gki_probe *p, const void *d_queries, int64_t q, int64_t max_hits, void *d_hit_start,
                           int64_t *n_hits);
int gki_probe_lookup_emit(gki_probe *p, const void *d_queries, int64_t q, int64_t max_hits, const void *d_hit_start,
                          void *d_hit_query, void *d_hit_position);
/* `kmer in index` (collision_free_kmer_index.py:295-296) for q k-mers: d_flags uint8[q] = 1 / 0.  The whitelist test of
 * DenseKmerFinder (kmer_finder.py:130-132, 362-365); follow with gki_compact_flat. */
int gki_probe_contains(gki_probe *p, const void *d_queries, int64_t q, void *d_flags);
int gki_probe_reads_count_nodes(gki_probe *p, const void *d_reads, const void *d_read_start, int64_t n_reads, int k,
                                int strands, int64_t max_hits, void *d_counts, int64_t n_counts, int64_t *n_kmers,
                                int64_t *n_hits);

/* ---------------------------------------------------------------- reads files (FASTA / FASTQ text -> the layout above)
 * The raw ASCII bytes of a reads file in HBM, or of a piece of one that ends at a line end, become what gki_hash_reads and
 * gki_probe_reads_count_nodes take: the letters of all reads back to back and read_start.  Count, allocate, emit, in the
 * manner of gki_hash_reads(.., NULL, ..); both calls parse the buffer themselves and nothing is kept between them.
 *   line    ends at '\n'; the last one may lack it: n_lines = number of '\n' + (n_bytes > 0 and the last byte is not '\n').
 *   strip   str.strip() of ASCII text, at both ends: 0x09-0x0D, 0x1C-0x1F, 0x20 (so CRLF files work; a lone '\r' inside
 *           a line is unsupported input).
 *   FASTA   read_kmers.py:18-25: a line whose first raw byte is '>' is a header, every other line, stripped, is one read
 *           (a multi-line record is several reads; " >x" is a read).
 *   FASTQ   by position only (quality lines may begin with '>' or '@'): with g = (line_phase + the line's number in the
 *           buffer) % 4, line g == 1 is a read; *n_bad_lines counts the lines g == 0 that do not begin with '@' and the
 *           lines g == 2 that do not begin with '+'.  line_phase = lines before this buffer, mod 4 (0..3; ignored for
 *           FASTA), so that a file may be cut after any '\n'.
 *   reads   read r is the r-th such line; one that is empty after the strip is a read of length 0.  Letters are copied
 *           unchanged: case, N and the rest are the hash kernels' business.
 * d_bytes uint8[n_bytes] (any alignment; 16-byte aligned buffers take the fast loads), d_letters uint8[letters_capacity],
 * d_read_start int64[read_start_capacity]; the emit call writes *n_letters letters and *n_reads + 1 offsets and returns
 * GKI_ERR_BAD_ARG, writing nothing, when either capacity is too small.  GKI_ERR_BAD_ARG also for another format or phase
 * and for a single read of 2^32 letters or more; every total is 64-bit and a line may be of any length below that. */
#define GKI_READS_FASTA 0
#define GKI_READS_FASTQ 1
int gki_reads_parse_count(const void *d_bytes, int64_t n_bytes, int format, int line_phase, int64_t *n_lines,
                          int64_t *n_reads, int64_t *n_letters, int64_t *n_bad_lines);
int gki_reads_parse_emit(const void *d_bytes, int64_t n_bytes, int format, int line_phase, void *d_letters,
                         int64_t letters_capacity, void *d_read_start, int64_t read_start_capacity);

/* ---------------------------------------------------------------- VCF files (VCF text -> POS, is_snp, chromosome runs)
 * The raw bytes of a VCF file in HBM, or of a piece of one that ends at a line end, become what VariantArrays holds
 * (unique_variant_kmers.py): POS and is_snp of every data line, and its chromosome as the number of a run of equal names.
 * Count, allocate, emit, as above; both calls parse the buffer themselves and nothing is kept between them.  The rules
 * give VariantArrays.from_vcf's result on every input where that function returns:
 *   line       ends at '\n'; the last one may lack it.  Every '\r' at its end is then dropped (rstrip("\r\n"), so CRLF files
 *              work; a lone '\r' inside a line is unsupported input).
 *   skipped    a line whose first raw byte is '#', and a line that str.strip() empties (the ASCII strip set of the reads
 *              files: 0x09-0x0D, 0x1C-0x1F, 0x20), so a line of blanks and tabs too.
 *   data line  every other line; data lines are numbered from 0 in the buffer, in file order.
 *   fields     separated by '\t'.  CHROM is the bytes before the first tab; it may be empty and is copied unchanged.  POS is
 *              field 1, ending at the second tab or the line's end.
 *   POS        1 to 18 ASCII digits, leading zeros allowed; anything else (a sign, a blank, an underscore, a 19th digit) is
 *              bad kind 2.  A data line without any tab is bad kind 1 (fewer than two columns).
 *   is_snp     -1 when the line has fewer than five fields; otherwise 1 exactly when field 3 (REF) and field 4 (ALT, ending
 *              at the fifth tab or the line's end) are one byte long each, else 0 (an empty ALT, "C,G" and "<DEL>" give 0).
 *              Nothing behind the fifth tab is read.
 *   runs       a data line begins a chromosome run when it is the buffer's first data line or its CHROM differs from the
 *              previous data line's in length or bytes; an unsorted file simply has more runs.
 * gki_vcf_parse_count: the totals; *first_bad_variant is the number of the lowest bad data line and *first_bad_kind its
 * kind, -1 and 0 when there is none.  A bad line is reported, not refused: the call still returns 0.
 * gki_vcf_parse_emit: d_positions int64, d_is_snp int8, d_chrom_run int32 (the run variant v belongs to), each
 * [variant_capacity]; d_run_name_start int64[run_capacity + 1] and d_run_names uint8[name_capacity]: run r's name is
 * d_run_names[run_name_start[r], run_name_start[r + 1]).  It writes *n_variants entries, *n_chrom_runs + 1 offsets and
 * *n_chrom_bytes name bytes, and returns GKI_ERR_BAD_ARG, writing nothing, when a capacity is too small or the buffer has a
 * bad line.  n_bytes == 0 and a buffer of headers only give zero variants and zero runs (run_name_start = [0]).
 * d_bytes uint8[n_bytes], any alignment.  Every total is 64-bit and a line may be of any length; a CHROM of 2^32 bytes or
 * more and more than 2^31 - 1 runs in one buffer are GKI_ERR_BAD_ARG. */
int gki_vcf_parse_count(const void *d_bytes, int64_t n_bytes, int64_t *n_lines, int64_t *n_variants, int64_t *n_chrom_runs,
                        int64_t *n_chrom_bytes, int64_t *first_bad_variant, int *first_bad_kind);
int gki_vcf_parse_emit(const void *d_bytes, int64_t n_bytes, void *d_positions, void *d_is_snp, void *d_chrom_run,
                       int64_t variant_capacity, void *d_run_name_start, int64_t run_capacity, void *d_run_names,
                       int64_t name_capacity);

/* ---------------------------------------------------------------- FASTA files (reference FASTA text -> record names and letters)
 * The raw bytes of a reference FASTA in HBM, or of a piece of one that ends at a line end (only the stream's last piece may
 * be unterminated), become the names of its records and the letters of the records the caller wants.  Every call parses
 * the buffer itself and nothing is kept between them.  The rules are those of snp_kmer_finder.read_fasta_records:
 *   header   a '>' at byte 0 of the buffer or right behind a '\n'; any other '>' is a letter.  Its line ends at the next
 *            '\n' or at the buffer's end, so a header line never spans two buffers.
 *   name     the first word of the header line behind the '>', words separated as by bytes.split(): blank, '\t', '\n',
 *            '\v', '\f', '\r'; empty when the line has no word.  The bytes are copied unchanged.
 *   body     every byte from behind the header line's '\n' up to the next header or the buffer's end, the bytes 10 and 13
 *            removed and nothing else: a blank stays, a lone '\r' goes.
 *   lead     the bytes before the buffer's first header continue the record the buffer before ended in (the carried
 *            record); in the stream's first buffer they belong to no record.
 * gki_fasta_parse_count: the number of headers, the bytes of their names together, and the letters of the lead.
 * gki_fasta_parse_names: d_name_start int64[header_capacity + 1] and d_names uint8[name_capacity]: header h's name is
 * d_names[name_start[h], name_start[h + 1]); d_body_letters int64[header_capacity]: the letters of header h's body in this
 * buffer.  No header gives name_start = [0].  GKI_ERR_BAD_ARG, writing nothing, when a capacity is too small.
 * gki_fasta_parse_emit: d_wanted uint8[n_wanted], one flag per header of the buffer (n_wanted must be their number), and
 * carry_wanted the flag of the carried record; the letters of the wanted records go to d_letters back to back in file
 * order, *n_letters of them: the sum of the wanted d_body_letters, plus the lead when carry_wanted.  GKI_ERR_BAD_ARG,
 * writing nothing, when letters_capacity is smaller.
 * d_bytes uint8[n_bytes], any alignment (16-byte aligned buffers take the fast loads).  Every offset and total is 64-bit
 * and a line may be of any length; a name of 2^32 bytes or more is GKI_ERR_BAD_ARG.  kernel_ms (may be NULL): the device
 * time of the call, from its first kernel to its last. */
int gki_fasta_parse_count(const void *d_bytes, int64_t n_bytes, int64_t *n_headers, int64_t *n_name_bytes,
                          int64_t *n_lead_letters, float *kernel_ms);
int gki_fasta_parse_names(const void *d_bytes, int64_t n_bytes, void *d_name_start, void *d_body_letters,
                          int64_t header_capacity, void *d_names, int64_t name_capacity, float *kernel_ms);
int gki_fasta_parse_emit(const void *d_bytes, int64_t n_bytes, int carry_wanted, const void *d_wanted, int64_t n_wanted,
                         void *d_letters, int64_t letters_capacity, int64_t *n_letters, float *kernel_ms);

/* ---------------------------------------------------------------- graph build (reference letters + VCF text -> graph arrays)
 * The flat arrays of graph.py and a variant-to-nodes table from the letters of the chosen chromosomes, concatenated in
 * graph order in HBM, and the VCF text that gki_vcf_parse_* has already split into chromosome runs.
 * Coordinates are global and 0-based: chromosome c occupies [C0_c, C1_c) of the concatenated letters.
 *   lines      data lines, skipped lines and fields are those of "VCF files".  A data line with fewer than five fields
 *              is at fault (kind 1).  The CHROM runs must name chosen chromosomes, each in at most one run, the runs in
 *              graph order (the host checks the few run names), POS must be 1 .. length (kind 2) and must not decrease
 *              inside a run (first_unordered_line).
 *   plain      an allele is plain when it is non-empty and every byte is one of ACGTNacgtn.  A line whose REF or ALT is
 *              not plain ("C,G", "<DEL>", "*", ".", IUPAC letters) gets status 1.
 *   site       when REF and ALT differ in length and their first bytes are equal ignoring case, that byte is stripped
 *              from both and lo = C0 + POS; otherwise the alleles are taken whole and lo = C0 + POS - 1.  Either allele
 *              may be empty after the strip.  hi = lo + length of the ref allele.
 *   REF check  a plain REF, padding base included, must equal the reference letters ignoring case (kind 3) and end
 *              inside its chromosome (kind 4), whatever the ALT is.
 *   before     a plain line with lo == C0 gets status 2: there is no base before the site.
 *   overlap    with reach_i the largest hi of the lines j < i whose status is neither 1 nor 2 (0 when there are none),
 *              such a line is kept, status 0, exactly when lo_i >= reach_i, and gets status 3 otherwise.  Dropped lines
 *              still count in reach: one prefix maximum, narrower than a greedy choice.  Two insertions at one point and
 *              an insertion followed by a SNP at its lo are all kept; of two SNPs at one POS the first is.
 *   nodes      id 0 is unused (exists 0, size 0).  Then per chromosome in order and per kept site in order: the gap
 *              [previous hi or C0, lo) as one node when it is non-empty, the ref allele, the alt allele; behind the last
 *              site the gap to C1 when it is non-empty.  A gap is never split, so it must be shorter than 2^31.  is_ref is
 *              1 for gaps and ref alleles (an empty ref allele is a linear-ref dummy), 0 for alt alleles.
 *              node_to_ref_offset[n_nodes + 1]: a gap its start, a ref allele its lo, every other entry 0.  seq holds
 *              codes (c 1, g 2, t 3 in either case, anything else 0) in node order: gaps and ref alleles from the
 *              reference, alt alleles from ALT.  Allele frequencies: the line's (ref_af, alt_af) on its two allele
 *              nodes when given, 1.0 everywhere else.
 *   edges      every node of an element (a gap: itself; a site: both alleles) has the entry nodes of its chromosome's
 *              next element as successors: [gap], or [ref, alt] in that order.  The last element has none and nothing
 *              connects chromosomes.  rev_edges ascend by source id.  chromosome_start_nodes[c] is chromosome c's first
 *              node, always a gap; a chromosome without kept sites is a single node.
 *   variant-to-nodes   ref_nodes[v], var_nodes[v]: the two allele nodes of kept line v, 0 and 0 for every other line.
 * gki_graph_sites_count / _emit work on one piece of text, d_text[n_bytes] of whole lines with n_variants data lines:
 * d_chrom_run int32[n_variants] is gki_vcf_parse_emit's for the same bytes, d_run_c0 / d_run_c1 int64[n_runs] each run's
 * C0 / C1, d_reference the concatenated letters.  Both calls do the whole pass; nothing is kept between them.  count:
 * *n_alt_bytes letters the emit call puts into the alt pool (the alt alleles of the lines with status 0 here, back to
 * back in line order), *first_bad_variant / *first_bad_kind the lowest data line at fault and why (-1 and 0: none); a line
 * at fault is reported, not refused.  emit: d_gpos int64 (C0 + POS - 1), d_lo int64, d_ref_len int32, d_alt_len int32,
 * d_status uint8 (0, 1 or 2; lengths are 0 where the status is 1), each [n_variants], and d_alt_pool uint8[alt_capacity];
 * GKI_ERR_BAD_ARG when a line is at fault or the pool is too small (the five site arrays may have been written by then).  An allele of 2^31 letters or more is GKI_ERR_BAD_ARG.
 * gki_graph_build_count takes those arrays of all pieces appended ([n_lines], d_status is updated in place to the final
 * 0 .. 3) and h_chromosome_bounds int64[n_chromosomes + 1] (C0 of every chromosome and the total; no chromosome is
 * empty, and a gap or a chromosome without a kept site is one node and must be shorter than 2^31), applies the order
 * check and the overlap rule and sizes the graph.  When POS decreases,
 * *first_unordered_line is the first line whose gpos is below its predecessor's, *plan is NULL and the call returns 0.
 * Otherwise -1 and *plan holds what the emit call needs; the per-line arrays must stay as they are until then.
 * *n_alt_bytes: the letters the appended alt pools must hold.
 * gki_graph_build_emit writes d_node_size int32[n_nodes], d_edge_start / d_rev_start / d_node_to_ref_offset
 * int64[n_nodes + 1] (seq_start is the prefix sum of node_size and is left to the caller), d_seq uint8[n_bases] (16-byte aligned), d_edges / d_rev_edges int32[n_edges],
 * d_is_ref / d_exists uint8[n_nodes], d_allele_freq float64[n_nodes], d_chromosome_start_nodes int64[n_chromosomes],
 * d_ref_nodes / d_var_nodes uint32[n_lines].  d_ref_af / d_alt_af float64[n_lines] or both NULL.  *sequence_ms (may be
 * NULL): the device time of the kernel that writes d_seq.  gki_graph_build_destroy frees the plan (NULL is allowed). */
typedef struct gki_graph_build gki_graph_build;
int gki_graph_sites_count(const void *d_text, int64_t n_bytes, const void *d_chrom_run, int64_t n_variants,
                          const void *d_run_c0, const void *d_run_c1, int64_t n_runs, const void *d_reference,
                          int64_t *n_alt_bytes, int64_t *first_bad_variant, int *first_bad_kind);
int gki_graph_sites_emit(const void *d_text, int64_t n_bytes, const void *d_chrom_run, int64_t n_variants,
                         const void *d_run_c0, const void *d_run_c1, int64_t n_runs, const void *d_reference,
                         void *d_gpos, void *d_lo, void *d_ref_len, void *d_alt_len, void *d_status, void *d_alt_pool,
                         int64_t alt_capacity);
int gki_graph_build_count(const void *d_gpos, const void *d_lo, const void *d_ref_len, const void *d_alt_len, void *d_status,
                          int64_t n_lines, const int64_t *h_chromosome_bounds, int64_t n_chromosomes, int64_t *n_nodes,
                          int64_t *n_edges, int64_t *n_bases, int64_t *n_alt_bytes, int64_t *first_unordered_line,
                          gki_graph_build **plan);
int gki_graph_build_emit(gki_graph_build *plan, const void *d_reference, const void *d_alt_pool, const void *d_ref_af,
                         const void *d_alt_af, void *d_node_size, void *d_seq, void *d_edge_start,
                         void *d_edges, void *d_rev_start, void *d_rev_edges, void *d_is_ref, void *d_allele_freq,
                         void *d_exists, void *d_node_to_ref_offset, void *d_chromosome_start_nodes, void *d_ref_nodes,
                         void *d_var_nodes, float *sequence_ms);
int gki_graph_build_destroy(gki_graph_build *plan);

/* ---------------------------------------------------------------- VCF allele frequencies (VCF text -> ref_af, alt_af per data line)
 * The allele frequencies gki_graph_build_emit puts on a kept line's two allele nodes, read from the VCF text itself
 * (DESIGN.md 4.17).  Lines, '\r' at line ends, data lines and their numbers are those of "VCF files"; field f is closed by
 * tab f + 1 or by the line's end.  Per data line the result is ref_af, alt_af (float64) and a route (uint8): 0 parsed on
 * the device, 1 absent (ref_af = alt_af = 1.0, what every node has without a source), 2 the value text is outside the
 * device's grammar and the host parses it (ref_af = alt_af = 1.0 until then).
 *   source GKI_AF_SOURCE_INFO        INFO is field 7; a line with fewer than 8 fields is absent.  INFO's entries are separated
 *              by ';'.  The first entry whose bytes begin with "AF=" gives the value text: the bytes behind '=' up to the next
 *              ';', the next ',' or the field's end ("XAF=", "MAF=" and "AF_EUR=" do not match; of "AF=0.1,0.2" the first
 *              value counts).  No such entry, an empty value text and "." are absent.
 *              Device grammar: D* [ . D* ] [ (e|E) [+|-] D+ ] with at least one mantissa digit.  m = the mantissa's digits
 *              without the dot as an integer, q = the exponent minus the number of fraction digits.  The device parses the
 *              text when the mantissa has at most 15 digits in all, the exponent at most 3 and |q| <= 22; the value is then
 *              m / 10^-q or m * 10^q, one IEEE double operation on exact operands (a table of the 23 powers, no pow, no
 *              fast-math), hence correctly rounded and bit-equal to strtod.  Everything else -- more digits, a larger
 *              exponent, nan, inf, a sign, stray bytes -- is route 2: d_span_begin[v] / d_span_len[v] give the value text's
 *              place in d_text and the host applies its own conversion to those bytes alone.
 *              alt_af = value, ref_af = 1.0 - value.  A device value above 1 is at fault, kind 1 (the grammar has no sign
 *              and |q| <= 22 keeps it finite).
 *   source GKI_AF_SOURCE_GENOTYPES   FORMAT is field 8, the samples are fields 9 and up; a line with fewer than 10 fields is
 *              absent.  FORMAT must begin with "GT" followed by ':' or its end, else the line is at fault, kind 2.  A
 *              sample's GT is its bytes up to the first ':' or the field's end: one or more alleles separated by '/' or '|',
 *              an allele '.' (missing, not counted) or 1 to 9 digits taken as a decimal number ("10" is allele ten, "01"
 *              allele one).  An empty GT, an empty allele and any other byte are at fault, kind 3.  n_called = the numeric
 *              alleles of all samples, n_ref those equal to 0, n_alt those equal to 1; n_called == 0 is absent, otherwise
 *              ref_af = n_ref / n_called and alt_af = n_alt / n_called, double divisions of exact integers.  Ploidy is free.
 * gki_vcf_allele_frequencies works on one piece of text, d_text[n_bytes] of whole lines (any alignment; no byte behind
 * n_bytes is read) with n_variants data lines: *n_data_lines is what the pass itself counted, and GKI_ERR_BAD_ARG when the
 * two differ.  d_ref_af / d_alt_af float64, d_route uint8, d_span_begin int64, d_span_len int32, each [n_variants]; the two
 * span arrays are written by source INFO only (0 where the route is not 2) and may be NULL for genotypes.
 * *first_bad_variant / *first_bad_kind: the lowest data line at fault and why (-1 and 0: none); a line at fault is reported,
 * not refused, and holds the absent values.  *kernel_ms (may be NULL): the device time of the source's kernel. */
#define GKI_AF_SOURCE_INFO 0
#define GKI_AF_SOURCE_GENOTYPES 1
int gki_vcf_allele_frequencies(const void *d_text, int64_t n_bytes, int source, int64_t n_variants, void *d_ref_af,
                               void *d_alt_af, void *d_route, void *d_span_begin, void *d_span_len, int64_t *n_data_lines,
                               int64_t *first_bad_variant, int *first_bad_kind, float *kernel_ms);

/* ---------------------------------------------------------------- VCF haplotype matrix (VCF text -> one code per sample haplotype and data line)
 * Which allele every sample haplotype carries at every data line, read from the GT columns.  Lines, '\r'
 * at line ends, data lines and their numbers are those of "VCF files"; fields, FORMAT and the GT grammar are those of
 * "VCF allele frequencies", source genotypes, unchanged: FORMAT is field 8 and must begin with "GT" followed by ':' or its
 * end; sample s is field 9 + s and its GT its bytes up to the first ':'; alleles are separated by '/' or '|'; an allele is
 * '.' or 1 to 9 digits.
 *   parameters   ploidy P, 1 <= P <= 8; n_samples S >= 0; H = S * P slots per line.
 *   slot codes   (uint8) 0: allele number 0; 1: allele number 1; 2: any other number; 3: no allele -- the allele '.', and a
 *                slot the GT does not fill (a GT of fewer than P alleles).  A GT's alleles fill its sample's slots in text
 *                order, whatever the separators.
 *   output       per data line v: codes[v][s * P + j], row-major, H bytes a row; phased[v] (uint8) 1 when no GT of the line
 *                holds a '/', else 0.
 *   faults       a line of 10 fields or more is at fault when FORMAT does not begin with GT (kind 2), when one of its sample
 *                fields holds a GT outside the grammar (kind 3), when it does not have exactly S sample fields (kind 4) or
 *                when a GT has more than P alleles (kind 5); of several the lowest kind is reported.  A line of fewer than
 *                10 fields has no sample field and its FORMAT is not looked at: kind 4 when S > 0, and with S = 0 it is fine
 *                and its row is empty.  A line at fault is reported, not refused: its row is all 3 and its phased is 0.
 * gki_vcf_haplotype_matrix works on one piece of text, d_text[n_bytes] of whole lines (any alignment; no byte behind n_bytes
 * is read) with n_variants data lines: *n_data_lines is what the pass itself counted, and GKI_ERR_BAD_ARG when the two
 * differ.  d_codes uint8[n_variants * H] (offsets are formed in 64 bits; may be NULL when H is 0), d_phased
 * uint8[n_variants]; the kernel writes every byte of both, whatever they held.  *first_bad_variant / *first_bad_kind: the
 * lowest data line at fault and why (-1 and 0: none).  *kernel_ms (may be NULL): the device time of the matrix kernel.
 * GKI_ERR_BAD_ARG for a negative size, a ploidy outside 1..8 and a NULL buffer where its size is positive; zero sizes do
 * nothing and succeed.
 * gki_haplotype_planes turns d_codes uint8[n_variants][n_slots] into two bit planes, the form whole-genome data is kept
 * in: d_ref_bits and d_alt_bits uint64[n_slots][W], W = ceil(n_variants / 64).  Bit v mod 64 (least significant first) of
 * word [h][v / 64] is set in ref_bits when codes[v][h] == 0 and in alt_bits when it is 1; any other byte value sets neither;
 * bits at and beyond n_variants in the last word are 0.  The kernel writes every word of both planes.  It runs once, over
 * the rows of all pieces: a piece's first line is no multiple of 64.  *kernel_ms (may be NULL): its device time. */
int gki_vcf_haplotype_matrix(const void *d_text, int64_t n_bytes, int64_t n_variants, int64_t n_samples, int ploidy,
                             void *d_codes, void *d_phased, int64_t *n_data_lines, int64_t *first_bad_variant,
                             int *first_bad_kind, float *kernel_ms);
int gki_haplotype_planes(const void *d_codes, int64_t n_variants, int64_t n_slots, void *d_ref_bits, void *d_alt_bits,
                         float *kernel_ms);

/* ---------------------------------------------------------------- haplotype paths (graph + variant-to-nodes + alt plane -> sequences, alt nodes)
 * What a sample haplotype of "VCF haplotype matrix" is in the graph of "graph build": its sequence and the variant nodes it
 * carries.
 *   inputs        the graph's flat arrays; variant-to-nodes with one entry per VCF data line, V of them -- a line is kept
 *                 exactly when var_nodes[v] != 0; the codes of V lines x H slots, on the device as the alt plane
 *                 alt_bits uint64[H][W], W = ceil(V / 64), of gki_haplotype_planes.  A matrix of another number of lines
 *                 than variant-to-nodes is refused.
 *   bubble chain  the kept lines' ref_nodes ascend strictly and var_nodes[v] == ref_nodes[v] + 1; every existing node that is
 *                 not an allele node of a kept line has is_ref 1.  Any other graph is refused, naming the first line or node
 *                 at fault (the host checks this once per graph; edges are not inspected).  In such a graph node ids ascend
 *                 along every path.
 *   choice        slot h takes the alt allele of kept line v exactly when codes[v][h] == 1.  Codes 0, 2 (another allele) and
 *                 3 (none) take the ref allele.  Lines that are not kept are ignored.
 *   sequence      per chromosome c the node sequences joined in id order from chromosome_start_nodes[c] up to the next
 *                 chromosome's start node (the graph's end for the last), leaving out the allele not taken at every kept
 *                 line.  Letters are upper-case "ACGT"[code]: an N of the reference is code 0 in the graph and comes out A.
 *   alt nodes     slot h's alt nodes are var_nodes[v] of the kept lines v with codes[v][h] == 1, in line order.
 * gki_haplotype_paths_create uploads one graph's plan from host arrays: h_seq uint8[n_bases]; h_var_nodes uint32[n_lines];
 * h_kept_bits uint64[ceil(n_lines / 64)], bit v mod 64 of word v / 64 set for a kept line, the tail zero; per kept line
 * j = 0 .. n_kept - 1 in line order its line number h_kept_line and its two allele nodes' seq_start and node_size
 * (h_ref_start, h_ref_size, h_alt_start, h_alt_size); h_chrom_seq_start / h_chrom_first_kept int64[n_chromosomes + 1]:
 * seq_start of chromosome c's start node and the first j of chromosome c, then n_bases and n_kept.  GKI_ERR_BAD_ARG unless
 * the kept lines ascend, every one has its bit and no other bit is set, alt_start == ref_start + ref_size and the next kept
 * line begins behind it: what keeps every read of the gather inside seq.
 * gki_haplotype_spell_count / _emit spell one slot of d_alt_bits uint64[n_slots][W]: count returns *n_out letters and
 * h_bounds int64[n_chromosomes + 1], where each chromosome begins in them and n_out; emit writes d_letters uint8[n_out]
 * (16-byte aligned) and must follow its count call (GKI_ERR_STATE otherwise).  Offsets are 64 bits wide throughout.
 * *count_ms / *spell_ms (may be NULL): the device time of the count pass' kernels and of the spelling kernel.
 * gki_haplotype_alt_nodes_count / _emit list the alt nodes of all slots: count writes d_start int64[n_slots + 1] (slot h's
 * nodes are [start[h], start[h + 1])) and returns *n_nodes = start[n_slots]; emit, given the same plane, writes d_nodes
 * uint32[n_nodes].  Bits of the plane at and beyond n_lines are not relied on: every word is ANDed with kept_bits.
 * gki_haplotype_paths_destroy frees the plan (NULL is allowed). */
typedef struct gki_haplotype_paths gki_haplotype_paths;
int gki_haplotype_paths_create(const uint8_t *h_seq, int64_t n_bases, int64_t n_lines, const uint32_t *h_var_nodes,
                               const uint64_t *h_kept_bits, int64_t n_kept, const int64_t *h_kept_line,
                               const int64_t *h_ref_start, const int32_t *h_ref_size, const int64_t *h_alt_start,
                               const int32_t *h_alt_size, int64_t n_chromosomes, const int64_t *h_chrom_seq_start,
                               const int64_t *h_chrom_first_kept, gki_haplotype_paths **plan);
int gki_haplotype_spell_count(gki_haplotype_paths *plan, const void *d_alt_bits, int64_t n_slots, int64_t slot,
                              int64_t *n_out, int64_t *h_bounds, float *count_ms);
int gki_haplotype_spell_emit(gki_haplotype_paths *plan, void *d_letters, float *spell_ms);
int gki_haplotype_alt_nodes_count(gki_haplotype_paths *plan, const void *d_alt_bits, int64_t n_slots, void *d_start,
                                  int64_t *n_nodes, float *kernel_ms);
int gki_haplotype_alt_nodes_emit(gki_haplotype_paths *plan, const void *d_alt_bits, int64_t n_slots, void *d_nodes,
                                 float *kernel_ms);
int gki_haplotype_paths_destroy(gki_haplotype_paths *plan);

/* ---------------------------------------------------------------- haplotype segments (node counts by difference from the all-ref path)
 * A slot's node counts without probing what it shares with the linear reference.  Everything is said per
 * sequence, in that sequence's own coordinates.  A sequence is either the all-ref path (a slot whose plane is all zero) or
 * slot h.  Each has chromosome bounds bounds[c], as gki_haplotype_spell_count returns them.
 *   taken lines    the taken lines t of slot h are the kept lines with alt_bits[h] & kept_bits set, in line order.  Codes 0,
 *                  2 and 3 are not taken, as in "haplotype paths".
 *   interval       a taken line has a half-open interval [a, b) in each sequence: in the all-ref path the position of the
 *                  line's ref allele, in the slot's sequence the position of its alt allele.  Either may be empty, with
 *                  a == b at the junction: an insertion's ref allele or a deletion's alt allele.
 *   dirty windows  window start s (letters s .. s + k - 1) is dirty with respect to [a, b) exactly when s < b and
 *                  a < s + k.  With a == b this means the window holds both a - 1 and a.
 *   segments       each dirty window goes to the first taken line it is dirty for.  That makes the dirty windows of line t
 *                  in chromosome c the run lo = max(a_t - k + 1, b_prev, bounds[c]) .. hi = min(b_t - 1, bounds[c + 1] - k),
 *                  b_prev the interval end of the previous taken line, or 0 for the first.  The run is empty when hi < lo; a
 *                  chromosome shorter than k has no runs.  A segment is (start = lo, windows = hi - lo + 1); its letters are
 *                  [lo, hi + k).
 *   identity       over the k-mers of both strands as asked for: counts(slot) = counts(all-ref path) - counts(segments of
 *                  the all-ref path) + counts(segments of the slot's sequence), exact node by node.  max_hits is a rule per
 *                  k-mer and passes through unchanged.
 * gki_haplotype_segments_count / _emit list both sequences' segments of one slot.  The count call must follow the
 * gki_haplotype_spell_count call of the same slot and plane (GKI_ERR_STATE otherwise; the spell emit call may lie between):
 * it reads the before / cut / bounds that call left in the plan.  It returns the taken lines, and per sequence the segments
 * and the windows in them; no per-line array leaves the device.  The emit call writes d_ref_seg_start / d_ref_seg_windows
 * int64[n_ref_segs] and d_slot_seg_start / d_slot_seg_windows int64[n_slot_segs], in line order (a list of no segments may be
 * NULL), and must follow its count call with no other slot or plane spelled between (GKI_ERR_STATE).  k is 1..31.  *kernel_ms (may be
 * NULL): the device time of the call's kernels. */
int gki_haplotype_segments_count(gki_haplotype_paths *plan, const void *d_alt_bits, int64_t n_slots, int64_t slot, int k,
                                 int64_t *n_taken, int64_t *n_ref_segs, int64_t *n_ref_windows, int64_t *n_slot_segs,
                                 int64_t *n_slot_windows, float *kernel_ms);
int gki_haplotype_segments_emit(gki_haplotype_paths *plan, void *d_ref_seg_start, void *d_ref_seg_windows,
                                void *d_slot_seg_start, void *d_slot_seg_windows, float *kernel_ms);
/* gki_probe_reads_count_nodes over segments of a sequence that stays where it is: segment i is the d_seg_windows[i] windows
 * (int64) that start at d_seg_start[i] (int64) .. in d_letters uint8[n_letters], so it reads the letters [seg_start[i],
 * seg_start[i] + seg_windows[i] + k - 1).  Segments may overlap one another; nothing is copied and no hash is stored.  Every
 * hit adds sign (+1 or -1) to d_counts uint32[n_counts] modulo 2^32: an intermediate wrap is harmless where the final value
 * is not negative.  strands and max_hits as in gki_probe_reads_count_nodes; *n_kmers / *n_hits (nullable) the k-mers probed
 * and the hits.  The kernel reads nothing outside d_letters[0, n_letters) whatever the segment arrays hold: a segment that
 * reaches outside is cut to what lies inside, the others are counted as they are, and the call returns GKI_ERR_BAD_ARG. */
int gki_probe_segments_count_nodes(gki_probe *p, const void *d_letters, int64_t n_letters, const void *d_seg_start,
                                   const void *d_seg_windows, int64_t n_segs, int k, int strands, int64_t max_hits, int sign,
                                   void *d_counts, int64_t n_counts, int64_t *n_kmers, int64_t *n_hits);
/* ---------------------------------------------------------------- node count model
 * What a genotyper fits on the node counts of sampled individuals: per kept line, allele (0 ref node, 1 var node) and number
 * of copies of that allele the individual carries (0 .. ploidy), a histogram of the node's count over the individuals and
 * the counts' sum.  d_histogram uint32[V][2][ploidy + 1][n_bins], d_count_sum uint64[V][2][ploidy + 1]; lines that are not
 * kept are never touched.
 * gki_node_count_model_accumulate adds one individual: d_row uint32[n_nodes] its node counts (a node at or beyond n_nodes
 * counts 0) and the slots first_slot .. first_slot + ploidy - 1 of d_alt_bits uint64[n_slots][W] its haplotypes.  With
 * c_alt = the number of those slots that take the line's alt allele, entry (line, 0, ploidy - c_alt) is updated with
 * row[ref node] and entry (line, 1, c_alt) with row[var node]; an update does histogram[..][min(count, n_bins - 1)] += 1
 * and count_sum[..] += count.  One lane per kept line, no atomics.  GKI_ERR_BAD_ARG for a ploidy outside 1..8, n_bins
 * outside 2..65536 and slots outside the plane.
 * gki_node_count_model_row_start writes d_row[i] = ploidy * d_base[i] (uint32[n_nodes] both, modulo 2^32): where an
 * individual's row starts when d_base holds the all-ref path's counts and each of its slots' two segment passes follows. */
int gki_node_count_model_row_start(const void *d_base, int64_t n_nodes, int ploidy, void *d_row);
int gki_node_count_model_accumulate(gki_haplotype_paths *plan, const void *d_alt_bits, int64_t n_slots, int64_t first_slot,
                                    int ploidy, const void *d_row, int64_t n_nodes, int n_bins, void *d_histogram,
                                    void *d_count_sum, float *kernel_ms);
/* ---------------------------------------------------------------- genotyping
 * The node count model and one sample's node counts -> a genotype per data line.  P = the model's ploidy (1..8), V = data
 * lines, N = the individuals the model holds; allele a is 0 for the ref node and 1 for the var node, c a copy number 0..P,
 * g a genotype = the number of alt copies, 0..P.  Line v is kept when var_nodes[v] != 0; its nodes are ref_nodes[v] and
 * var_nodes[v] as variant-to-nodes has them (no bubble chain is assumed); a node at or beyond n_nodes counts 0.
 *   n[v][a][c] = the sum of histogram[v][a][c][.] over the bins, s[v][a][c] = count_sum[v][a][c].
 * fit, once per model (gki_genotype_fit):
 *   mean      n > 0: mu[v][a][c] = double(s) / double(n), one division.  n == 0: with c' the populated copy number (n > 0)
 *             nearest to c, the lower at a tie, mu[v][a][c] = max(0, mu[v][a][c'] + (c - c')).  A line that is not kept: 0.
 *   n_alt     n_alt[v][g] = n[v][1][g], the prior's counts.
 *   total     T = the sum of s[v][a][c] over the kept lines, all a and c: exact, modulo 2^64.
 *   faults    the lowest line at fault and its kind: 1 = an allele of a kept line has no populated entry, 2 = an allele's
 *             n[v][a][.] do not sum to N.  (*first_bad_line = -1, *first_bad_kind = 0: none.)
 *   No log, no sum of doubles, nothing a compiler may contract: every mean is bit-equal to NumPy's.  d_mean is
 *   double[2 (P + 1)][V] with entry a (P + 1) + c as its row, d_n_alt uint32[P + 1][V]: entry-major, so that a wave of the
 *   call kernel reads whole lines.  n_bins is 2..65536.
 * scale, once per row x = uint32[n_nodes] of a batch (gki_genotype_scale): h_sums[r] = S = the sum over the kept lines of
 *   x[ref node] + x[var node], exact.  The caller's estimate is lambda = (double(S) * double(N)) / double(T): a baseline
 *   that takes the sample's genotypes to be spread as the population's are.
 * call, per row and kept line (gki_genotype_call), with error e > 0, pseudo_count alpha > 0 and the row's coverage
 *   lambda > 0, all finite:
 *     m[a][c] = lambda * (mu[v][a][c] + e)       pi[g] = (n_alt[v][g] + alpha) / (N + (P + 1) * alpha)
 *     x0 = x[ref node], x1 = x[var node]
 *     L[g] = x0 * log(m[0][P - g]) - m[0][P - g] + x1 * log(m[1][g]) - m[1][g] + log(pi[g])       left to right
 *   (the Poisson term -lgamma(x + 1) is the same for every g and is left out).
 *     loglik[v][g] = L[g] - max L         call[v] = the lowest g at the maximum (int8)
 *     q = 4.342944819032518 * (L[call] - the greatest L[g] of g != call);  gq[v] = 99 when q >= 99, else floor(q) (uint8)
 *   A line that is not kept gets call -1, gq 0 and loglik all 0.  d_counts uint32[n_samples][n_nodes] (at most 65535 rows),
 *   h_coverage double[n_samples] on the host, d_call int8[n_samples][V], d_gq uint8[n_samples][V], d_loglik
 *   double[n_samples][V][P + 1] or NULL.  Double precision throughout; no atomics.
 * GKI_ERR_BAD_ARG for sizes, ploidy, n_bins, e, alpha or a coverage out of range.  *kernel_ms (may be NULL): the device time
 * of the call's kernel. */
int gki_genotype_fit(const void *d_histogram, const void *d_count_sum, const void *d_var_nodes, int64_t n_lines, int ploidy,
                     int n_bins, int64_t n_individuals, void *d_mean, void *d_n_alt, uint64_t *model_total,
                     int64_t *first_bad_line, int *first_bad_kind, float *kernel_ms);
int gki_genotype_scale(const void *d_ref_nodes, const void *d_var_nodes, int64_t n_lines, const void *d_counts,
                       int64_t n_samples, int64_t n_nodes, uint64_t *h_sums, float *kernel_ms);
int gki_genotype_call(const void *d_mean, const void *d_n_alt, const void *d_ref_nodes, const void *d_var_nodes,
                      int64_t n_lines, int ploidy, int64_t n_individuals, const void *d_counts, int64_t n_samples,
                      int64_t n_nodes, const double *h_coverage, double error, double pseudo_count, void *d_call, void *d_gq,
                      void *d_loglik, float *kernel_ms);
/* ---------------------------------------------------------------- genotyped VCF text
 * One piece of whole lines of VCF text in HBM -> the data lines of a VCF with one sample column.  Lines, '\r' and data
 * lines are those of "VCF haplotype matrix" (vcf_line; the data lines numbered in text order).  d_call int8 and d_gq uint8
 * hold n_calls entries and sit at the piece's first data line; a piece with more data lines than n_calls is refused
 * (GKI_ERR_BAD_ARG, *n_data_lines set).
 *   per data line   the bytes of its first eight fields -- from the line's begin to its eighth tab, or to its end --
 *                   followed by "\tGT:GQ\t" GT ":" GQ "\n".  GT: P alleles joined by '/', first P - call times '0', then
 *                   call times '1'; P times '.' for call -1.  GQ: the decimal number without leading zeros; '.' for call -1.
 *   not written     header lines, blank lines, and whatever follows field 8 (FORMAT and sample columns of the input).
 *   faults          the lowest data line at fault (numbered from the piece's first) and its kind: 1 = fewer than eight
 *                   fields, 2 = a call outside -1 .. P.
 * gki_vcf_genotypes_count gives the piece's data lines, the bytes of its output and the fault.  gki_vcf_genotypes_emit
 * writes d_out[0, *n_out_bytes) (16-byte aligned); it keeps no state and makes the count pass again.  It refuses a piece at
 * fault and an out_capacity below the output's bytes with GKI_ERR_BAD_ARG and then writes nothing.  Offsets are 64 bits
 * wide; a line may be of any length; a piece is at most 2^32 - 65 bytes.  ploidy is 1..8.  *kernel_ms (may be NULL): the
 * device time of the lengths kernel and its scan, in the emit call with that of the emit kernels added. */
int gki_vcf_genotypes_count(const void *d_text, int64_t n_bytes, const void *d_call, const void *d_gq, int64_t n_calls,
                            int ploidy, int64_t *n_data_lines, int64_t *n_out_bytes, int64_t *first_bad_line,
                            int *first_bad_kind, float *kernel_ms);
int gki_vcf_genotypes_emit(const void *d_text, int64_t n_bytes, const void *d_call, const void *d_gq, int64_t n_calls,
                           int ploidy, void *d_out, int64_t out_capacity, int64_t *n_out_bytes, float *kernel_ms);
/* ---------------------------------------------------------------- genotyped cohort VCF text
 * One piece of whole lines of VCF text in HBM -> the data lines of a VCF with S = n_samples sample columns.  Lines, data
 * lines, what is not written and P = ploidy (1..8) are those of "genotyped VCF text".
 *   per data line   the bytes of its first eight fields, then "\tGT:GQ", then for every sample s = 0 .. S - 1 in order
 *                   "\t" GT ":" GQ, then "\n".  GT and GQ as in "genotyped VCF text"; a gq above 99 is written as 99.  With
 *                   S = 1 and gq <= 99 the output is byte for byte that of gki_vcf_genotypes_emit.
 *   column width    a column has 2P + 2 + w bytes, w = 1 when call >= 0 and gq >= 10 (a wide column), w = 0 otherwise: so
 *                   column s of a line begins (2P + 2) s + (the number of wide columns below s) bytes behind "\tGT:GQ".
 *                   The emit kernel finds a byte's column from this identity, with a bit mask of the line's wide columns
 *                   and a running count per 64 columns, and walks no columns.
 *   faults          the lowest data line at fault (numbered from the piece's first) and its kind: 1 = fewer than eight
 *                   fields, 2 = a call outside -1 .. P in any sample's column (the line is named, not the sample).
 * d_call int8 and d_gq uint8 are the call kernel's own [S][row_stride] (gki_genotype_call with V = row_stride); the piece's
 * first data line is entry `first` of every row and n_calls entries are left there (first + n_calls <= row_stride): nothing
 * is transposed or copied by the caller.  A piece with more data lines than n_calls is refused (GKI_ERR_BAD_ARG,
 * *n_data_lines set).  n_samples is 1 .. 2^20; 0 is GKI_ERR_BAD_ARG.
 * gki_vcf_cohort_count gives the piece's data lines, the bytes of its output and the fault; d_line_start (may be NULL):
 * int64[line_start_capacity >= data lines + 1] in HBM, where each data line's output begins, from 0, and the total.
 * gki_vcf_cohort_emit writes the data lines [line_from, line_to) of the piece to d_out[0, *n_out_bytes) (16-byte aligned),
 * so that a caller bounds one call's output by the line starts; it keeps no state and makes the count pass again.  It
 * refuses a piece at fault (wherever the line), a range beyond the piece's data lines and an out_capacity below the range's
 * bytes with GKI_ERR_BAD_ARG and then writes nothing.  Offsets are 64 bits wide; a line's columns may be longer than any
 * tile; the piece's bytes + 7 + (2P + 3) S stay below 2^32 - 64.  *kernel_ms (may be NULL): the device time of the pack
 * pass, the lengths kernel and the scan, in the emit call with that of the emit kernels added.
 * gki_vcf_cohort_kernel_ms: those times of the calling thread's last call apart -- the pack pass, the lengths kernel with
 * the scan, the tile search with the emit kernel (0 for what that call did not launch), for tools/bench_genotype_cohort.py. */
int gki_vcf_cohort_count(const void *d_text, int64_t n_bytes, const void *d_call, const void *d_gq, int64_t row_stride,
                         int64_t first, int64_t n_samples, int64_t n_calls, int ploidy, int64_t *n_data_lines,
                         int64_t *n_out_bytes, int64_t *first_bad_line, int *first_bad_kind, void *d_line_start,
                         int64_t line_start_capacity, float *kernel_ms);
int gki_vcf_cohort_emit(const void *d_text, int64_t n_bytes, const void *d_call, const void *d_gq, int64_t row_stride,
                        int64_t first, int64_t n_samples, int64_t n_calls, int ploidy, int64_t line_from, int64_t line_to,
                        void *d_out, int64_t out_capacity, int64_t *n_out_bytes, float *kernel_ms);
int gki_vcf_cohort_kernel_ms(float *pack_ms, float *lengths_ms, float *emit_ms);

/* ---------------------------------------------------------------- BGZF (blocked gzip: the .gz reads files of bgzip / htslib)
 * A BGZF file is a chain of gzip members of at most 64 KiB, each with its compressed size in a 'BC' extra subfield, so
 * every member's raw DEFLATE payload, CRC-32 and ISIZE are found without inflating anything (graph_kmer_index_amd/bgzf.py
 * does that on the host).  gki_bgzf_inflate inflates n_blocks payloads of one device buffer side by side: block b reads
 * d_in[payload_start[b], payload_start[b] + payload_len[b]) and writes d_out[out_start[b], out_start[b + 1]), whose length
 * is the member's ISIZE, then compares the CRC-32 of what it wrote with crc32[b].  No dictionary: a distance reaches no
 * further back than the block's own output.
 *   d_payload_start int64[n_blocks], d_payload_len int32[n_blocks], d_crc32 uint32[n_blocks], d_out_start int64[n_blocks + 1],
 *   all in HBM.  GKI_ERR_BAD_ARG, before anything is inflated, unless every payload lies inside n_in, out_start is
 *   non-decreasing from >= 0 to <= out_capacity and no block's output exceeds 65 536 bytes.  n_blocks == 0 does nothing.
 *   GKI_ERR_INFLATE when a block fails: *first_bad_block is the lowest such block and *first_bad_status why (-1 and 0
 *   otherwise); every other block's output is written all the same.  The status values (csrc/gki_inflate_core.h):
 *     1 the input ends inside the stream      2 block type 3                     3 stored LEN / NLEN mismatch
 *     4 invalid code lengths (over-subscribed, incomplete, too many, a repeat past the end, no end-of-block code)
 *     5 repeat code 16 first                  6 literal/length symbol 286, 287   7 distance symbol 30, 31
 *     8 distance before the block's start     9 more output than ISIZE           10 less output than ISIZE
 *     11 input bytes behind the final block   12 CRC-32 mismatch                 13 bits that are no code of the set
 * gki_bgzf_inflate_kernel_ms: the device time of the inflate kernel alone in the calling thread's last gki_bgzf_inflate
 * (events around the one launch; 0 when that call launched nothing), for tools/bench_read_files.py.
 * gki_last_byte_position: *position = the greatest p with d_bytes[p] == value (0..255), -1 when there is none -- where
 * the streaming route cuts a piece of inflated text behind its last line end, without copying the text to the host. */
int gki_bgzf_inflate(const void *d_in, int64_t n_in, const void *d_payload_start, const void *d_payload_len,
                     const void *d_crc32, const void *d_out_start, int64_t n_blocks, void *d_out, int64_t out_capacity,
                     int64_t *first_bad_block, int *first_bad_status);
int gki_bgzf_inflate_kernel_ms(float *ms);
int gki_last_byte_position(const void *d_bytes, int64_t n_bytes, int value, int64_t *position);

/* ---------------------------------------------------------------- BGZF deflate (the way out: text in HBM to a .gz file's bytes)
 * gki_bgzf_deflate compresses the n_in bytes of d_in into complete BGZF members, packed back to back in d_out: one member
 * per block_size (1..0xff00) input bytes, the last one shorter, each with the 18-byte header of bgzip (MTIME 0, XFL 0,
 * OS 255, 'BC' with BSIZE), a raw DEFLATE payload, CRC-32 and ISIZE.  No end-of-file member is written: that is the
 * writer's.  A payload is one final block: LZ77 matches with dynamic Huffman codes from the member's own counts, or a stored
 * block when that is not smaller, so a member is at most its input + 31 bytes.  The bytes are a function of the input and
 * block_size alone (csrc/gki_deflate_core.h; a host program built from that header writes the same bytes).
 *   *n_out: the bytes written; *n_members: ceil(n_in / block_size); d_member_end (may be NULL): int64[n_members] in HBM,
 *   where each member ends in d_out.  n_in == 0 writes nothing and gives 0 and 0.
 *   GKI_ERR_BAD_ARG, with nothing written, for a block_size outside 1..0xff00, a negative size, a NULL buffer with a
 *   positive size, or an out_capacity below gki_bgzf_deflate_bound's *bytes = n_in + 31 * n_members.
 * gki_bgzf_deflate_kernel_ms: the device time of the calling thread's last gki_bgzf_deflate, by events around its launches
 * (the deflate kernel, the scan of the members' sizes, the pack); 0 when that call launched nothing. */
int gki_bgzf_deflate_bound(int64_t n_in, int block_size, int64_t *bytes);
int gki_bgzf_deflate(const void *d_in, int64_t n_in, int block_size, void *d_out, int64_t out_capacity, int64_t *n_out,
                     int64_t *n_members, void *d_member_end);
int gki_bgzf_deflate_kernel_ms(float *ms);

/* Measurement aid: independent random 8-byte loads per second the device sustains from a table of table_bytes (every
 * load that misses L2 is one 64-byte request -- the unit the probe kernels are bound by, not bytes).  Runs n_loads loads
 * twice and reports the second launch.  bench.py reports the read-side rate as a fraction of this. */
int gki_measure_random_loads(int64_t table_bytes, int64_t n_loads, double *loads_per_s);
/* The store ceiling of THIS device for the FlatKmers column pattern: writes n records of the four columns (8 + 4 + 8 + 4
 * bytes; the caller's buffers, e.g. the output columns before a run) with nothing else in the kernel, three launches,
 * best of the last two; bytes_per_s = 24 n / time.  bench.py prints it beside the 8 TB/s spec peak. */
int gki_measure_store_bw(void *d_hashes, void *d_nodes, void *d_ref_offsets, void *d_af32, int64_t n, double *bytes_per_s);
/* The yardstick a streaming kernel's device time is set beside: *ms = the device time, by HIP events, of one
 * device-to-device copy of `bytes` bytes (the buffers must not overlap). */
int gki_measure_copy_ms(void *d_dst, const void *d_src, int64_t bytes, float *ms);
/* Device self-test of the kernels' wave prefix sum (DPP row shifts and broadcasts, csrc/gki_common.h) against the shuffle
 * form on random and extreme inputs: *n_bad = lanes that disagree (0 on a correct build).  No reference counterpart. */
int gki_selftest_wave_scan(int64_t *n_bad);
/* Read simulator on the device (benchmark input for BASELINE configs[4]): n_reads reads of read_len
 * letters (ASCII ACGT) sampled from a haplotype (uint8 codes 0..3 in HBM): uniform start, either strand, every base
 * substituted with p_substitution, a read replaced by uniform random letters with p_random_read.  Counter-based: read
 * first_read + q is a pure function of (seed, its index), so batches of one run and a NumPy restatement agree. */
int gki_simulate_reads(const void *d_haplotype, int64_t hap_len, int64_t n_reads, int read_len, uint64_t seed,
                       double p_substitution, double p_random_read, int64_t first_read, void *d_letters);

/* ---------------------------------------------------------------- multi-GPU exchange (RCCL over xGMI)
 * One process per GPU.  The reference gathers its per-process FlatKmers by pickling them through a
 * process pool and concatenating (command_line_interface.py:607-614, flat_kmers.py:71-90); here every
 * rank's finished columns are exchanged once, shard r landing at offset sum(counts[:r]), so that every
 * GPU holds the concatenation in rank order.  The 128-byte id comes from rank 0 and travels over the
 * caller's control plane (parallel.SocketControlPlane: plain TCP to rank 0); h_counts[world] likewise. */
/* Ordering: every exchange entry point first waits for all work already submitted to the device (the columns come
 * from finder / partition streams), runs on the communicator's own stream and returns when the exchange has completed;
 * a caller needs no synchronisation of its own on either side. */
#define GKI_COMM_ID_BYTES 128
typedef struct gki_comm gki_comm;
int gki_comm_get_unique_id(void *h_id);
int gki_comm_create(gki_comm **out, int world_size, int rank, const void *h_id);
int gki_comm_destroy(gki_comm *c);
/* What RCCL itself says about the communicator (ncclCommCount / ncclCommUserRank). */
int gki_comm_info(gki_comm *c, int *rccl_world, int *rccl_rank);
/* Ranks that share ONE device.  RCCL refuses a communicator with two ranks on the same device (ncclInvalidUsage), so
 * a multi-rank run on a single GPU exchanges through HIP IPC instead: gki_device_bus_id tells the ranks apart
 * (PCI bus id of the current device), gki_ipc_export gives the 64-byte handle of the allocation that holds d_ptr and
 * d_ptr's offset inside it, gki_ipc_open maps a peer's allocation (returns its base), gki_ipc_close unmaps it.  The
 * handles travel over the caller's control plane (parallel.SharedDeviceComm). */
#define GKI_IPC_HANDLE_BYTES 64
int gki_device_bus_id(char *buf, int len);
int gki_ipc_export(const void *d_ptr, void *h_handle, int64_t *offset);
int gki_ipc_open(const void *h_handle, void **d_base);
int gki_ipc_close(void *d_base);
/* All-to-all(v) of FlatKmers columns for the bucket-range partitioned build: the send columns hold this rank's records
 * partitioned by destination, slice r = [h_send_start[r], h_send_start[r+1]); what rank r sends to this rank lands at
 * [h_recv_start[r], h_recv_start[r+1]) of the receive columns (both tables host int64[world+1]; the counts travel
 * over the caller's control plane first). */
int gki_comm_alltoall_flat(gki_comm *c, const int64_t *h_send_start, const void *d_hashes, const void *d_nodes,
                           const void *d_ref_offsets, const void *d_af32, const int64_t *h_recv_start, void *d_out_hashes,
                           void *d_out_nodes, void *d_out_ref_offsets, void *d_out_af32);
/* In-place sum over ranks of a uint32 device array (node counts of a bucket-partitioned lookup). */
int gki_comm_allreduce_u32(gki_comm *c, void *d_buf, int64_t n);
int gki_comm_allgather_flat(gki_comm *c, const int64_t *h_counts, const void *d_hashes, const void *d_nodes,
                            const void *d_ref_offsets, const void *d_af32, void *d_out_hashes, void *d_out_nodes,
                            void *d_out_ref_offsets, void *d_out_af32);

#ifdef __cplusplus
}
#endif
#endif
