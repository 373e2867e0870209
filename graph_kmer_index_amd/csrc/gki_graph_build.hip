// Graph build in HBM: reference letters and VCF text become the flat arrays of graph.py and a variant-to-nodes table.
// The rules are those of include/gki.h ("graph build") and DESIGN.md 4.15.
//
// 1. per piece of text (gki_graph_sites_count / _emit), beside the unchanged gki_vcf_parse_*:
//   (data lines)             gki_vcf_data_lines (gki_text_lines.hip): line ends, header / blank / data by vcf_line -- the
//                            rule k_vcf_classify applies, so both number the data lines alike --, line -> data lines before
//                            it; vcf_fields and vcf_pos_value are shared too
//   k_gb_sites               one lane per data line: fields, POS against its chromosome, plain or not, the strip rule, REF
//                            against the reference; writes the line's site and how many alt letters it has for the pool
//   (exclusive scan)         data line -> alt letters before it
//   k_gb_copy_alt            the alt alleles' letters into the pool
// 2. over all lines (gki_graph_build_count / _emit):
//   k_gb_tile_max, k_gb_scan_tiles, k_gb_keep    the prefix maximum of hi: kept or dropped for overlap; the order check
//   (two scans) k_gb_compact                     the kept sites, dense, with their chromosome
//   k_gb_site_counts (four scans)                nodes, successors, predecessors and alt letters of every kept site
//   k_gb_emit_nodes / k_gb_emit_whole            every per-node array, the edges and variant-to-nodes
// 3. k_gb_tile_sites, k_gb_sequence   output-dense: a workgroup owns 4096 consecutive codes of `seq`, reads which kept
//                            sites fall into them (one binary search per tile boundary, done by k_gb_tile_sites for all
//                            tiles at once), and every lane encodes and stores 16 bytes.  The output is the
//                            reference with every kept alt allele put in behind its site's ref allele, so a lane's 16
//                            codes come from 16 consecutive letters of the reference or of the alt pool unless a site's
//                            boundary falls among them (then byte by byte).
#include "gki_seq_gather.h"
#include "gki_text_lines.h"

namespace {

constexpr int GB_ITEMS = 8;                                // lines per lane in the prefix-maximum kernels
constexpr int GB_TILE = PARSE_BLOCK * GB_ITEMS;            // 2048 lines per workgroup
constexpr int SEQ_TILE = PARSE_BLOCK * 16;                 // 4096 codes per workgroup

// beside the lowest data line at fault, flags: bit 0 an allele of 2^31 letters or more, bit 1 the text and chrom_run disagree
struct SiteTotals : LineFault { unsigned int flags = 0, pad = 0; };

__device__ __forceinline__ bool plain_letter(uint8_t c) {  // ACGTN in either case: none of them has bit 5 set
    const uint8_t u = c & 0xDF;
    return u == (uint8_t)'A' || u == (uint8_t)'C' || u == (uint8_t)'G' || u == (uint8_t)'T' || u == (uint8_t)'N';
}

// Data line v of the piece: gpos = C0 + POS - 1, the site (lo, ref_len, alt_len), status 0 / 1 / 2, where its alt allele
// lies in the text and how many letters of it go to the pool (those of a well-formed line).
__global__ __launch_bounds__(PARSE_BLOCK) void k_gb_sites(const uint8_t *__restrict__ bytes,
                                                          const int64_t *__restrict__ line_end, int64_t n_lines,
                                                          const uint32_t *__restrict__ is_data,
                                                          const int64_t *__restrict__ variant_index,
                                                          const int32_t *__restrict__ chrom_run, int64_t n_variants,
                                                          const int64_t *__restrict__ run_c0,
                                                          const int64_t *__restrict__ run_c1, int64_t n_runs,
                                                          const uint8_t *__restrict__ reference,
                                                          int64_t *__restrict__ gpos, int64_t *__restrict__ lo,
                                                          int32_t *__restrict__ ref_len, int32_t *__restrict__ alt_len,
                                                          uint8_t *__restrict__ status, int64_t *__restrict__ alt_begin,
                                                          uint32_t *__restrict__ pool_len,
                                                          SiteTotals *__restrict__ totals) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_lines; i += stride) {
        if (!is_data[i]) continue;
        const int64_t v = variant_index[i];
        if (v >= n_variants) { atomicOr(&totals->flags, 2u); continue; }
        const VcfLine l = vcf_line(bytes, line_end, i);
        const VcfFields f = vcf_fields(bytes, l.b, l.e);
        int kind = 0, st = 0;
        int64_t g = 0, site_lo = 0, rl = 0, al = 0, ab = 0;
        const int32_t r = chrom_run[v];
        if (r < 0 || r >= n_runs) { atomicOr(&totals->flags, 2u); kind = 7; }
        else if (f.n < VCF_FIELDS) kind = 1;
        else {
            const int64_t c0 = run_c0[r], c1 = run_c1[r];
            int64_t value;
            if (!vcf_pos_value(bytes, f.begin(1), f.end[1], &value) || value < 1 || value > c1 - c0) kind = 2;
            else {
                const int64_t ref_b = f.begin(3), ref_e = f.end[3], alt_b = f.begin(4), alt_e = f.end[4];
                g = c0 + value - 1;
                rl = ref_e - ref_b;
                al = alt_e - alt_b;
                bool ref_plain = rl > 0, alt_plain = al > 0;
                for (int64_t p = ref_b; ref_plain && p < ref_e; p++) ref_plain = plain_letter(bytes[p]);
                for (int64_t p = alt_b; alt_plain && p < alt_e; p++) alt_plain = plain_letter(bytes[p]);
                if (ref_plain) {
                    if (g + rl > c1) kind = 4;
                    else
                        for (int64_t j = 0; j < rl; j++)
                            if ((bytes[ref_b + j] & 0xDF) != (reference[g + j] & 0xDF)) { kind = 3; break; }
                }
                if (rl > 0x7FFFFFFFll || al > 0x7FFFFFFFll) { atomicOr(&totals->flags, 1u); kind = kind ? kind : 7; }
                ab = alt_b;
                if (!ref_plain || !alt_plain) { st = 1; rl = 0; al = 0; }
                else {
                    if (rl != al && (bytes[ref_b] & 0xDF) == (bytes[alt_b] & 0xDF)) { site_lo = g + 1; rl--; al--; ab++; }
                    else site_lo = g;
                    if (site_lo == c0) st = 2;
                }
            }
        }
        if (kind && kind != 7) line_fault(&totals->first_bad, v, kind);
        if (kind) { g = site_lo = rl = al = 0; st = 1; }
        gpos[v] = g;
        lo[v] = site_lo;
        ref_len[v] = (int32_t)rl;
        alt_len[v] = (int32_t)al;
        status[v] = (uint8_t)st;
        alt_begin[v] = ab;
        pool_len[v] = st == 0 ? (uint32_t)al : 0u;
    }
}

__global__ __launch_bounds__(PARSE_BLOCK) void k_gb_copy_alt(const uint8_t *__restrict__ bytes,
                                                             const int64_t *__restrict__ alt_begin,
                                                             const uint32_t *__restrict__ pool_len,
                                                             const int64_t *__restrict__ pool_off, int64_t n_variants,
                                                             int64_t pool_capacity, uint8_t *__restrict__ pool) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_variants; v += stride) {
        const int64_t n = pool_len[v], src = alt_begin[v], dst = pool_off[v];
        if (dst + n > pool_capacity) continue;
        for (int64_t j = 0; j < n; j++) pool[dst + j] = bytes[src + j];
    }
}

// What the site pass of one piece leaves on the device.  Both entry points build it; neither keeps it.
struct SitePlan {
    DevBuf alt_begin, pool_len, pool_off;
    int64_t n_alt_bytes = 0, first_bad = -1;
    int first_bad_kind = 0;
};

int site_pass(const uint8_t *bytes, int64_t n, const int32_t *chrom_run, int64_t nv, const int64_t *run_c0,
              const int64_t *run_c1, int64_t n_runs, const uint8_t *reference, int64_t *gpos, int64_t *lo,
              int32_t *ref_len, int32_t *alt_len, uint8_t *status, SitePlan &p) {
    if (n < 0 || nv < 0 || n_runs < 0) return gki_set_error(GKI_ERR_BAD_ARG, "graph_sites: a negative size");
    if (nv == 0) return GKI_OK;
    if (n == 0 || bytes == nullptr || chrom_run == nullptr || run_c0 == nullptr || run_c1 == nullptr || reference == nullptr)
        return gki_set_error(GKI_ERR_BAD_ARG, "graph_sites: %lld data lines need the text, their runs and the reference",
                             (long long)nv);
    VcfDataLines d;                                        // of the pass alone: both waits below come before it is freed
    GKI_TRY(gki_vcf_data_lines(bytes, n, "graph_sites", d));
    GKI_TRY(gki_vcf_expect_data_lines("graph_sites", d.n_data, nv, "chrom_run"));
    DevBuf tmp, d_totals;
    const int64_t tmp_bytes = gki_scan_tmp_bytes(nv);
    HIP_TRY(tmp.alloc((size_t)tmp_bytes));
    HIP_TRY(p.alt_begin.alloc((size_t)nv * 8));
    HIP_TRY(p.pool_len.alloc((size_t)nv * 4));
    HIP_TRY(p.pool_off.alloc((size_t)(nv + 1) * 8));
    GKI_TRY(line_fault_init<SiteTotals>(d_totals));
    HIP_TRY(hipMemset(p.pool_len.get(), 0, (size_t)nv * 4));      // a data line the text does not have stays without letters
    hipLaunchKernelGGL(k_gb_sites, dim3(stream_grid(d.n_lines, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0, bytes,
                       d.line_end.get<const int64_t>(), d.n_lines, d.is_data.get<const uint32_t>(),
                       d.variant_index.get<const int64_t>(), chrom_run, nv, run_c0, run_c1, n_runs, reference,
                       gpos, lo, ref_len, alt_len, status, p.alt_begin.get<int64_t>(), p.pool_len.get<uint32_t>(),
                       d_totals.get<SiteTotals>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(gki_scan_u32_to_i64(p.pool_len.get<const uint32_t>(), nv, p.pool_off.get<int64_t>(), tmp.get(), tmp_bytes, 0));
    SiteTotals totals;
    GKI_TRY(gki_scan_total(p.pool_off, nv, &p.n_alt_bytes));
    GKI_TRY(line_fault_read(d_totals, &totals));
    if (totals.flags & 2u) return gki_set_error(GKI_ERR_BAD_ARG, "graph_sites: chrom_run does not belong to this text");
    if (totals.flags & 1u) return gki_set_error(GKI_ERR_BAD_ARG, "graph_sites: an allele of 2^31 letters or more");
    p.first_bad = totals.line();
    p.first_bad_kind = totals.kind();
    return GKI_OK;
}

// ------------------------------------------------------------------------------------------------ over all lines

// inclusive maximum over the workgroup's lanes, in lane order; lds[t] holds lane t's result afterwards (values >= 0)
__device__ __forceinline__ int64_t block_incl_max(int64_t v, int64_t *lds) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < PARSE_BLOCK; d <<= 1) {
        const int64_t o = t >= d ? lds[t - d] : 0;
        __syncthreads();
        v = v > o ? v : o;
        lds[t] = v;
        __syncthreads();
    }
    return v;
}

// tile_max[b] = the largest hi of the well-formed lines of tile b; the order check: gpos never decreases
__global__ __launch_bounds__(PARSE_BLOCK) void k_gb_tile_max(const uint8_t *__restrict__ status,
                                                             const int64_t *__restrict__ lo,
                                                             const int32_t *__restrict__ ref_len,
                                                             const int64_t *__restrict__ gpos, int64_t n,
                                                             int64_t *__restrict__ tile_max,
                                                             unsigned long long *__restrict__ first_unordered) {
    __shared__ int64_t lds[PARSE_BLOCK];
    const int64_t base = (int64_t)blockIdx.x * GB_TILE + (int64_t)threadIdx.x * GB_ITEMS;
    int64_t m = 0;
#pragma unroll
    for (int j = 0; j < GB_ITEMS; j++) {
        const int64_t i = base + j;
        if (i >= n) break;
        if (status[i] == 0) { const int64_t hi = lo[i] + ref_len[i]; m = hi > m ? hi : m; }
        if (i > 0 && gpos[i] < gpos[i - 1]) atomicMin(first_unordered, (unsigned long long)i);
    }
    block_incl_max(m, lds);
    if (threadIdx.x == 0) tile_max[blockIdx.x] = lds[PARSE_BLOCK - 1];
}

// one workgroup: tile_max[b] becomes the maximum over the tiles before b
__global__ __launch_bounds__(PARSE_BLOCK) void k_gb_scan_tiles(int64_t *__restrict__ tile_max, int64_t n_tiles) {
    __shared__ int64_t lds[PARSE_BLOCK];
    const int64_t per = (n_tiles + PARSE_BLOCK - 1) / PARSE_BLOCK;
    const int64_t begin = (int64_t)threadIdx.x * per, end = begin + per < n_tiles ? begin + per : n_tiles;
    int64_t m = 0;
    for (int64_t j = begin; j < end; j++) m = tile_max[j] > m ? tile_max[j] : m;
    block_incl_max(m, lds);
    int64_t carry = threadIdx.x ? lds[threadIdx.x - 1] : 0;
    for (int64_t j = begin; j < end; j++) {
        const int64_t own = tile_max[j];
        tile_max[j] = carry;
        carry = own > carry ? own : carry;
    }
}

// reach_i = the largest hi of the well-formed lines before i; a well-formed line is kept when lo_i >= reach_i, else status 3.
// pool_len[i]: the letters line i has in the alt pool, as k_gb_sites counted them.
__global__ __launch_bounds__(PARSE_BLOCK) void k_gb_keep(uint8_t *__restrict__ status, const int64_t *__restrict__ lo,
                                                         const int32_t *__restrict__ ref_len, int64_t n,
                                                         const int32_t *__restrict__ alt_len,
                                                         const int64_t *__restrict__ tile_reach,
                                                         uint32_t *__restrict__ kept, uint32_t *__restrict__ pool_len) {
    __shared__ int64_t lds[PARSE_BLOCK];
    const int64_t base = (int64_t)blockIdx.x * GB_TILE + (int64_t)threadIdx.x * GB_ITEMS;
    int64_t m = 0;
#pragma unroll
    for (int j = 0; j < GB_ITEMS; j++) {
        const int64_t i = base + j;
        if (i < n && status[i] == 0) { const int64_t hi = lo[i] + ref_len[i]; m = hi > m ? hi : m; }
    }
    block_incl_max(m, lds);
    int64_t reach = tile_reach[blockIdx.x];
    if (threadIdx.x) reach = lds[threadIdx.x - 1] > reach ? lds[threadIdx.x - 1] : reach;
#pragma unroll
    for (int j = 0; j < GB_ITEMS; j++) {
        const int64_t i = base + j;
        if (i >= n) break;
        bool keep = false;
        const bool well_formed = status[i] == 0;
        if (well_formed) {
            const int64_t l = lo[i], hi = l + ref_len[i];
            keep = l >= reach;
            if (!keep) status[i] = 3;
            reach = hi > reach ? hi : reach;
        }
        kept[i] = keep ? 1u : 0u;
        pool_len[i] = well_formed ? (uint32_t)alt_len[i] : 0u;  // the pool holds the well-formed lines' alt letters
    }
}

// kept site k: its line, lo, hi, alt length, chromosome (by gpos, which lies inside it) and where its alt letters lie
__global__ __launch_bounds__(PARSE_BLOCK) void k_gb_compact(const uint32_t *__restrict__ kept,
                                                            const int64_t *__restrict__ kept_before, int64_t n, int64_t K,
                                                            const int64_t *__restrict__ gpos, const int64_t *__restrict__ lo,
                                                            const int32_t *__restrict__ ref_len,
                                                            const int32_t *__restrict__ alt_len,
                                                            const int64_t *__restrict__ pool_off,
                                                            const int64_t *__restrict__ bounds, int n_chrom,
                                                            int64_t *__restrict__ kline, int64_t *__restrict__ klo,
                                                            int64_t *__restrict__ khi, uint32_t *__restrict__ kal,
                                                            int32_t *__restrict__ kchrom, int64_t *__restrict__ kpool) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (!kept[i]) continue;
        const int64_t k = kept_before[i];
        if (k >= K) continue;
        const int64_t g = gpos[i];
        int a = 0, b = n_chrom;                            // the last chromosome whose C0 <= g
        while (b - a > 1) { const int mid = (a + b) >> 1; if (bounds[mid] <= g) a = mid; else b = mid; }
        kline[k] = i;
        klo[k] = lo[i];
        khi[k] = lo[i] + ref_len[i];
        kal[k] = (uint32_t)alt_len[i];
        kchrom[k] = a;
        kpool[k] = pool_off[i];
    }
}

// The nodes a kept site accounts for, in id order: the chromosomes without a kept site before the first site (one node
// each), its gap, its two alleles, the gap to its chromosome's end and the chromosomes without a kept site behind it.
struct SiteShape {
    int64_t c0, c1, prev_hi;
    int chrom, lead, after;
    bool first, last, gap, tail, next_gap;
    int succ;                                              // successors of each allele
};
__device__ __forceinline__ SiteShape site_shape(int64_t k, int64_t K, const int64_t *__restrict__ klo,
                                                const int64_t *__restrict__ khi, const int32_t *__restrict__ kchrom,
                                                const int64_t *__restrict__ bounds, int n_chrom) {
    SiteShape s;
    s.chrom = kchrom[k];
    s.first = k == 0 || kchrom[k - 1] != s.chrom;
    s.last = k == K - 1 || kchrom[k + 1] != s.chrom;
    s.c0 = bounds[s.chrom];
    s.c1 = bounds[s.chrom + 1];
    s.prev_hi = s.first ? s.c0 : khi[k - 1];
    s.gap = klo[k] > s.prev_hi;
    s.lead = k == 0 ? s.chrom : 0;
    s.tail = s.last && khi[k] < s.c1;
    s.after = s.last ? (k == K - 1 ? n_chrom : kchrom[k + 1]) - s.chrom - 1 : 0;
    s.next_gap = !s.last && klo[k + 1] > khi[k];
    s.succ = s.tail ? 1 : s.last ? 0 : s.next_gap ? 1 : 2;
    return s;
}
__device__ __forceinline__ int allele_preds(const SiteShape &s) { return s.gap ? 1 : s.first ? 0 : 2; }

__global__ __launch_bounds__(PARSE_BLOCK) void k_gb_site_counts(int64_t K, const int64_t *__restrict__ klo,
                                                                const int64_t *__restrict__ khi,
                                                                const int32_t *__restrict__ kchrom,
                                                                const int64_t *__restrict__ bounds, int n_chrom,
                                                                uint32_t *__restrict__ n_nodes, uint32_t *__restrict__ n_succ,
                                                                uint32_t *__restrict__ n_pred, unsigned int *__restrict__ too_long) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += stride) {
        const SiteShape s = site_shape(k, K, klo, khi, kchrom, bounds, n_chrom);
        n_nodes[k] = (uint32_t)(s.lead + (s.gap ? 1 : 0) + 2 + (s.tail ? 1 : 0) + s.after);
        n_succ[k] = (uint32_t)((s.gap ? 2 : 0) + 2 * s.succ);
        n_pred[k] = (uint32_t)((s.gap && !s.first ? 2 : 0) + 2 * allele_preds(s) + (s.tail ? 2 : 0));
        bool long_node = klo[k] - s.prev_hi > 0x7FFFFFFFll || (s.tail && s.c1 - khi[k] > 0x7FFFFFFFll);
        for (int j = 0; j < s.lead; j++) long_node |= bounds[j + 1] - bounds[j] > 0x7FFFFFFFll;
        for (int j = s.chrom + 1; j <= s.chrom + s.after; j++) long_node |= bounds[j + 1] - bounds[j] > 0x7FFFFFFFll;
        if (long_node) atomicOr(too_long, 1u);              // a gap or a whole chromosome that does not fit node_size
    }
}

struct GraphOut {
    int32_t *node_size; int64_t *edge_start; int32_t *edges; int64_t *rev_start; int32_t *rev_edges;
    uint8_t *is_ref; double *allele_freq; uint8_t *exists; int64_t *node_to_ref_offset, *chromosome_start_nodes;
    uint32_t *ref_nodes, *var_nodes;
};

__device__ __forceinline__ void put_node(const GraphOut &o, int64_t id, int64_t size, int64_t edge_at,
                                         int64_t rev_at, bool linear, double af, int64_t ref_offset) {
    o.node_size[id] = (int32_t)size;
    o.edge_start[id] = edge_at;
    o.rev_start[id] = rev_at;
    o.is_ref[id] = linear ? 1 : 0;
    o.allele_freq[id] = af;
    o.exists[id] = 1;
    o.node_to_ref_offset[id] = ref_offset;
}
// a chromosome without a kept site: one node, no edges
__device__ __forceinline__ void put_whole(const GraphOut &o, int64_t id, int chrom, const int64_t *__restrict__ bounds,
                                          int64_t edge_at, int64_t rev_at) {
    put_node(o, id, bounds[chrom + 1] - bounds[chrom], edge_at, rev_at, true, 1.0, bounds[chrom]);
    o.chromosome_start_nodes[chrom] = id;
}
// id 0 and the arrays' closing entries
__device__ __forceinline__ void put_ends(const GraphOut &o, int64_t n_nodes, int64_t n_edges) {
    o.node_size[0] = 0;
    o.edge_start[0] = o.rev_start[0] = o.node_to_ref_offset[0] = 0;
    o.is_ref[0] = o.exists[0] = 0;
    o.allele_freq[0] = 1.0;
    o.edge_start[n_nodes] = o.rev_start[n_nodes] = n_edges;
    o.node_to_ref_offset[n_nodes] = 0;
}

__global__ __launch_bounds__(PARSE_BLOCK) void k_gb_emit_whole(GraphOut o, const int64_t *__restrict__ bounds, int n_chrom) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0) put_ends(o, 1 + n_chrom, 0);
    if (c < n_chrom) put_whole(o, 1 + c, c, bounds, 0, 0);
}

// node_before / succ_before / pred_before / alt_before: the exclusive scans of the site counts and of kal (K + 1 entries).
// alt_end[k] = khi[k] + alt_before[k + 1]: where site k's alt allele ends in `seq` (k_gb_sequence searches it).
__global__ __launch_bounds__(PARSE_BLOCK) void k_gb_emit_nodes(int64_t K, const int64_t *__restrict__ kline,
                                                               const int64_t *__restrict__ klo,
                                                               const int64_t *__restrict__ khi,
                                                               const uint32_t *__restrict__ kal,
                                                               const int32_t *__restrict__ kchrom,
                                                               const int64_t *__restrict__ bounds, int n_chrom,
                                                               const int64_t *__restrict__ node_before,
                                                               const int64_t *__restrict__ succ_before,
                                                               const int64_t *__restrict__ pred_before,
                                                               const int64_t *__restrict__ alt_before,
                                                               const double *__restrict__ ref_af,
                                                               const double *__restrict__ alt_af, GraphOut o,
                                                               int64_t *__restrict__ alt_end) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        put_ends(o, 1 + node_before[K], succ_before[K]);
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += stride) {
        const SiteShape s = site_shape(k, K, klo, khi, kchrom, bounds, n_chrom);
        const int64_t line = kline[k], lo = klo[k], hi = khi[k], al = kal[k], A = alt_before[k];
        int64_t id = 1 + node_before[k], e = succ_before[k], r = pred_before[k];
        const int64_t first_id = id;
        alt_end[k] = hi + A + al;
        for (int j = 0; j < s.lead; j++) put_whole(o, id++, j, bounds, e, r);
        if (s.gap) {
            put_node(o, id, lo - s.prev_hi, e, r, true, 1.0, s.prev_hi);
            if (s.first) o.chromosome_start_nodes[s.chrom] = id;
            else { o.rev_edges[r] = (int32_t)(first_id - 2); o.rev_edges[r + 1] = (int32_t)(first_id - 1); r += 2; }
            o.edges[e] = (int32_t)(id + 1);
            o.edges[e + 1] = (int32_t)(id + 2);
            e += 2;
            id++;
        }
        const int64_t ref_id = id, alt_id = id + 1;
        // the entry nodes of the next element: the tail gap, or the next site's first node (and the one behind it)
        const int64_t next = s.tail ? alt_id + 1 : 1 + node_before[k + 1];
        const int preds = allele_preds(s);
        for (int allele = 0; allele < 2; allele++) {
            if (allele == 0) put_node(o, ref_id, hi - lo, e, r, true, ref_af ? ref_af[line] : 1.0, lo);
            else put_node(o, alt_id, al, e, r, false, alt_af ? alt_af[line] : 1.0, 0);
            if (s.succ >= 1) o.edges[e] = (int32_t)next;
            if (s.succ == 2) o.edges[e + 1] = (int32_t)(next + 1);
            e += s.succ;
            if (preds == 1) o.rev_edges[r] = (int32_t)(ref_id - 1);
            else if (preds == 2) { o.rev_edges[r] = (int32_t)(first_id - 2); o.rev_edges[r + 1] = (int32_t)(first_id - 1); }
            r += preds;
        }
        o.ref_nodes[line] = (uint32_t)ref_id;
        o.var_nodes[line] = (uint32_t)alt_id;
        id += 2;
        if (s.tail) {
            put_node(o, id, s.c1 - hi, e, r, true, 1.0, hi);
            o.rev_edges[r] = (int32_t)ref_id;
            o.rev_edges[r + 1] = (int32_t)alt_id;
            r += 2;
            id++;
        }
        for (int j = 0; j < s.after; j++) put_whole(o, id++, s.chrom + 1 + j, bounds, e, r);
    }
}

// ------------------------------------------------------------------------------------------------ the sequence

// four letters -> four codes (c 1, g 2, t 3 in either case, anything else 0), a byte each
__device__ __forceinline__ uint32_t encode4(uint32_t w) {
    const uint32_t u = w & 0xDFDFDFDFu;
    auto is = [u](uint32_t letter) {                       // 0x80 in every byte of u that equals `letter`, exactly
        const uint32_t x = u ^ (letter * 0x01010101u);
        return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
    };
    const uint32_t c = is('C'), g = is('G'), t = is('T');
    return (c >> 7) | (g >> 6) | (t >> 7) | (t >> 6);
}
__device__ __forceinline__ uint32_t encode1(uint8_t c) {
    const uint8_t u = c & 0xDF;
    return u == (uint8_t)'C' ? 1u : u == (uint8_t)'G' ? 2u : u == (uint8_t)'T' ? 3u : 0u;
}

// Letters16 and first_site_after (the first k in [a, b) with alt_end[k] > p) are gki_seq_gather.h's

// tile_site[t] = the first kept site whose alt allele ends behind output byte t * SEQ_TILE (K when there is none), for
// t = 0 .. n_tiles: one lane per tile boundary does the search over all K sites, so that k_gb_sequence starts every
// tile from one load instead of a chain of dependent ones
__global__ __launch_bounds__(PARSE_BLOCK) void k_gb_tile_sites(const int64_t *__restrict__ alt_end, int64_t K,
                                                               int64_t n_tiles, int64_t *__restrict__ tile_site) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t <= n_tiles; t += stride)
        tile_site[t] = first_site_after(alt_end, 0, K, t * SEQ_TILE);
}

// seq[p] for p in [0, n_bases): with k the first kept site whose alt allele ends behind p, p lies in that allele when
// p >= alt_end[k] - kal[k] (letter kpool[k] + p - that of the pool), else in the reference at p - alt_before[k].
__global__ __launch_bounds__(PARSE_BLOCK) void k_gb_sequence(const uint8_t *__restrict__ reference,
                                                             const uint8_t *__restrict__ pool, int64_t K,
                                                             const int64_t *__restrict__ alt_end,
                                                             const int64_t *__restrict__ alt_before,
                                                             const int64_t *__restrict__ kpool,
                                                             const int64_t *__restrict__ tile_site, int64_t n_bases,
                                                             uint8_t *__restrict__ seq) {
    const int64_t n_tiles = (n_bases + SEQ_TILE - 1) / SEQ_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t tile_begin = tile * SEQ_TILE;
        const int64_t k_lo = tile_site[tile], k_hi = tile_site[tile + 1];         // the same for every lane
        const int64_t p0 = tile_begin + (int64_t)threadIdx.x * 16;
        if (p0 >= n_bases) continue;
        int64_t k = first_site_after(alt_end, k_lo, k_hi, p0);
        const int64_t alt_begin = k < K ? alt_end[k] - (alt_before[k + 1] - alt_before[k]) : n_bases;
        const uint8_t *src = nullptr;
        if (p0 + 16 <= n_bases) {
            if (p0 + 16 <= alt_begin) src = reference + (p0 - alt_before[k]);
            else if (p0 >= alt_begin && p0 + 16 <= alt_end[k]) src = pool + (kpool[k] + (p0 - alt_begin));
        }
        if (src != nullptr) {                              // 16 letters in a row, at any alignment; the store is aligned
            Letters16 in;
            __builtin_memcpy(&in, src, 16);
            uint4 out;
            out.x = encode4(in.w[0]);
            out.y = encode4(in.w[1]);
            out.z = encode4(in.w[2]);
            out.w = encode4(in.w[3]);
            *reinterpret_cast<uint4 *>(seq + p0) = out;
            continue;
        }
        // a site's boundary among the 16, or the end of seq: piece by piece -- the rest of the reference before site k's
        // alt allele, then that allele -- so that a piece's byte loads do not wait for one another
        uint64_t low = 0, high = 0;
        const int count = n_bases - p0 < 16 ? (int)(n_bases - p0) : 16;
        const int64_t p_end = p0 + count;
        int64_t p = p0;
        while (p < p_end) {
            while (k < K && alt_end[k] <= p) k++;
            int64_t before = alt_before[k], begin = n_bases, end = n_bases, from = 0;
            if (k < K) {
                end = alt_end[k];
                begin = end - (alt_before[k + 1] - before);
                from = kpool[k];
            }
            const int64_t ref_end = begin < p_end ? begin : p_end, alt_stop = end < p_end ? end : p_end;
            const int64_t alt_from = p > begin ? p : begin;
            // all 16 loads are issued whatever the piece covers (a byte outside it reads reference[0]), so that they
            // are in flight together
            uint32_t letter[16];                           // indexed by unrolled loops only: registers
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int64_t q = p0 + j;
                const bool in_ref = q >= p && q < ref_end, in_alt = q >= alt_from && q < alt_stop;
                const int64_t ref_at = in_ref ? q - before : 0, pool_at = in_alt ? from + (q - begin) : 0;
                const uint8_t *at = in_alt ? pool + pool_at : reference + ref_at;
                letter[j] = *at;
            }
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int64_t q = p0 + j;
                const bool mine = q >= p && q < (alt_stop > ref_end ? alt_stop : ref_end);
                const uint64_t code = mine ? encode1((uint8_t)letter[j]) : 0u;
                if (j < 8) low |= code << (8 * j); else high |= code << (8 * (j - 8));
            }
            p = alt_stop > ref_end ? alt_stop : ref_end;
        }
        if (count == 16) {
            uint4 out;
            out.x = (uint32_t)low; out.y = (uint32_t)(low >> 32); out.z = (uint32_t)high; out.w = (uint32_t)(high >> 32);
            *reinterpret_cast<uint4 *>(seq + p0) = out;
        } else
            for (int j = 0; j < count; j++) seq[p0 + j] = (uint8_t)((j < 8 ? low >> (8 * j) : high >> (8 * (j - 8))) & 0xFF);
    }
}

}  // namespace

// What gki_graph_build_count leaves for gki_graph_build_emit.  The per-line arrays are the caller's and must outlive it.
struct gki_graph_build {
    const int64_t *gpos = nullptr, *lo = nullptr;
    const int32_t *ref_len = nullptr, *alt_len = nullptr;
    int64_t n_lines = 0, K = 0, n_nodes = 0, n_edges = 0, n_bases = 0, n_pool = 0;
    int n_chrom = 0, device = 0;
    DevBuf bounds, kline, klo, khi, kal, kchrom, kpool, node_before, succ_before, pred_before, alt_before, alt_end;
};

extern "C" {

int gki_graph_sites_count(const void *d_text, int64_t n_bytes, const void *d_chrom_run, int64_t n_variants,
                          const void *d_run_c0, const void *d_run_c1, int64_t n_runs, const void *d_reference,
                          int64_t *n_alt_bytes, int64_t *first_bad_variant, int *first_bad_kind) {
    if (n_alt_bytes) *n_alt_bytes = 0;
    if (first_bad_variant) *first_bad_variant = -1;
    if (first_bad_kind) *first_bad_kind = 0;
    SitePlan p;
    DevBuf gpos, lo, ref_len, alt_len, status;             // the count call has no use for the sites themselves
    const size_t nv = n_variants > 0 ? (size_t)n_variants : 0;
    HIP_TRY(gpos.alloc(nv * 8 + 8));
    HIP_TRY(lo.alloc(nv * 8 + 8));
    HIP_TRY(ref_len.alloc(nv * 4 + 4));
    HIP_TRY(alt_len.alloc(nv * 4 + 4));
    HIP_TRY(status.alloc(nv + 1));
    GKI_TRY(site_pass((const uint8_t *)d_text, n_bytes, (const int32_t *)d_chrom_run, n_variants, (const int64_t *)d_run_c0,
                      (const int64_t *)d_run_c1, n_runs, (const uint8_t *)d_reference, gpos.get<int64_t>(), lo.get<int64_t>(),
                      ref_len.get<int32_t>(), alt_len.get<int32_t>(), status.get<uint8_t>(), p));
    if (n_alt_bytes) *n_alt_bytes = p.n_alt_bytes;
    if (first_bad_variant) *first_bad_variant = p.first_bad;
    if (first_bad_kind) *first_bad_kind = p.first_bad_kind;
    return GKI_OK;
}

int gki_graph_sites_emit(const void *d_text, int64_t n_bytes, const void *d_chrom_run, int64_t n_variants,
                         const void *d_run_c0, const void *d_run_c1, int64_t n_runs, const void *d_reference,
                         void *d_gpos, void *d_lo, void *d_ref_len, void *d_alt_len, void *d_status, void *d_alt_pool,
                         int64_t alt_capacity) {
    if (n_variants > 0 && (d_gpos == nullptr || d_lo == nullptr || d_ref_len == nullptr || d_alt_len == nullptr || d_status == nullptr))
        return gki_set_error(GKI_ERR_BAD_ARG, "graph_sites_emit: an output buffer is NULL");
    SitePlan p;                                            // the sites go straight into the caller's arrays
    GKI_TRY(site_pass((const uint8_t *)d_text, n_bytes, (const int32_t *)d_chrom_run, n_variants, (const int64_t *)d_run_c0,
                      (const int64_t *)d_run_c1, n_runs, (const uint8_t *)d_reference, (int64_t *)d_gpos, (int64_t *)d_lo,
                      (int32_t *)d_ref_len, (int32_t *)d_alt_len, (uint8_t *)d_status, p));
    if (n_variants == 0) return GKI_OK;
    if (p.first_bad >= 0)
        return gki_set_error(GKI_ERR_BAD_ARG, "graph_sites_emit: data line %lld is at fault (kind %d)", (long long)p.first_bad,
                             p.first_bad_kind);
    if (p.n_alt_bytes > alt_capacity || (p.n_alt_bytes > 0 && d_alt_pool == nullptr))
        return gki_set_error(GKI_ERR_BAD_ARG, "graph_sites_emit: %lld alt letters, capacity %lld", (long long)p.n_alt_bytes,
                             (long long)alt_capacity);
    if (p.n_alt_bytes > 0) {
        hipLaunchKernelGGL(k_gb_copy_alt, dim3(stream_grid(n_variants, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0,
                           (const uint8_t *)d_text, p.alt_begin.get<const int64_t>(), p.pool_len.get<const uint32_t>(),
                           p.pool_off.get<const int64_t>(), n_variants, p.n_alt_bytes, (uint8_t *)d_alt_pool);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

int gki_graph_build_destroy(gki_graph_build *plan) {
    delete plan;
    return GKI_OK;
}

int gki_graph_build_count(const void *d_gpos, const void *d_lo, const void *d_ref_len, const void *d_alt_len, void *d_status,
                          int64_t n_lines, const int64_t *h_chromosome_bounds, int64_t n_chromosomes, int64_t *n_nodes,
                          int64_t *n_edges, int64_t *n_bases, int64_t *n_alt_bytes, int64_t *first_unordered_line,
                          gki_graph_build **plan_out) {
    if (plan_out == nullptr || n_nodes == nullptr || n_edges == nullptr || n_bases == nullptr || first_unordered_line == nullptr)
        return gki_set_error(GKI_ERR_BAD_ARG, "graph_build_count: an output pointer is NULL");
    *plan_out = nullptr;
    *n_nodes = *n_edges = *n_bases = 0;
    *first_unordered_line = -1;
    if (n_alt_bytes) *n_alt_bytes = 0;
    if (n_lines < 0 || n_chromosomes < 1 || n_chromosomes > 0x7FFFFFFFll / 2 || h_chromosome_bounds == nullptr)
        return gki_set_error(GKI_ERR_BAD_ARG, "graph_build_count: needs n_lines >= 0 and at least one chromosome");
    for (int64_t c = 0; c < n_chromosomes; c++) {
        const int64_t len = h_chromosome_bounds[c + 1] - h_chromosome_bounds[c];
        if (h_chromosome_bounds[0] != 0 || len < 1)
            return gki_set_error(GKI_ERR_BAD_ARG, "graph_build_count: chromosome %lld has %lld letters", (long long)c,
                                 (long long)len);
    }
    if (n_lines > 0 && (d_gpos == nullptr || d_lo == nullptr || d_ref_len == nullptr || d_alt_len == nullptr || d_status == nullptr))
        return gki_set_error(GKI_ERR_BAD_ARG, "graph_build_count: a per-line array is NULL");
    gki_graph_build *raw = new gki_graph_build;
    struct Guard { gki_graph_build *p; ~Guard() { delete p; } } guard{raw};
    gki_graph_build &g = *raw;
    g.gpos = (const int64_t *)d_gpos;
    g.lo = (const int64_t *)d_lo;
    g.ref_len = (const int32_t *)d_ref_len;
    g.alt_len = (const int32_t *)d_alt_len;
    g.n_lines = n_lines;
    g.n_chrom = (int)n_chromosomes;
    HIP_TRY(hipGetDevice(&g.device));
    HIP_TRY(g.bounds.alloc((size_t)(n_chromosomes + 1) * 8));
    HIP_TRY(hipMemcpy(g.bounds.get(), h_chromosome_bounds, (size_t)(n_chromosomes + 1) * 8, hipMemcpyHostToDevice));
    const int64_t total_ref = h_chromosome_bounds[n_chromosomes];
    uint8_t *status = (uint8_t *)d_status;
    DevBuf pool_off;                                       // int64[n_lines + 1]: alt letters of the well-formed lines before
    if (n_lines > 0) {
        const int64_t n_tiles = ceil_div(n_lines, GB_TILE), tmp_bytes = gki_scan_tmp_bytes(n_lines);
        DevBuf tile_max, flags, kept, kept_before, pool_len, tmp;
        HIP_TRY(tile_max.alloc((size_t)n_tiles * 8));
        HIP_TRY(flags.alloc(8));
        HIP_TRY(kept.alloc((size_t)n_lines * 4));
        HIP_TRY(kept_before.alloc((size_t)(n_lines + 1) * 8));
        HIP_TRY(pool_off.alloc((size_t)(n_lines + 1) * 8));
        HIP_TRY(tmp.alloc((size_t)tmp_bytes));
        HIP_TRY(hipMemset(flags.get(), 0xFF, 8));
        hipLaunchKernelGGL(k_gb_tile_max, dim3((unsigned)n_tiles), dim3(PARSE_BLOCK), 0, 0, status, g.lo, g.ref_len, g.gpos,
                           n_lines, tile_max.get<int64_t>(), flags.get<unsigned long long>());
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_gb_scan_tiles, dim3(1), dim3(PARSE_BLOCK), 0, 0, tile_max.get<int64_t>(), n_tiles);
        HIP_TRY(hipGetLastError());
        unsigned long long unordered = ~0ull;
        HIP_TRY(hipMemcpy(&unordered, flags.get(), 8, hipMemcpyDeviceToHost));
        if (unordered != ~0ull) {
            *first_unordered_line = (int64_t)unordered;
            return GKI_OK;
        }
        HIP_TRY(pool_len.alloc((size_t)n_lines * 4));
        hipLaunchKernelGGL(k_gb_keep, dim3((unsigned)n_tiles), dim3(PARSE_BLOCK), 0, 0, status, g.lo, g.ref_len, n_lines,
                           g.alt_len, tile_max.get<const int64_t>(), kept.get<uint32_t>(), pool_len.get<uint32_t>());
        HIP_TRY(hipGetLastError());
        GKI_TRY(gki_scan_u32_to_i64(kept.get<const uint32_t>(), n_lines, kept_before.get<int64_t>(), tmp.get(), tmp_bytes, 0));
        GKI_TRY(gki_scan_u32_to_i64(pool_len.get<const uint32_t>(), n_lines, pool_off.get<int64_t>(), tmp.get(), tmp_bytes, 0));
        HIP_TRY(hipMemcpy(&g.K, kept_before.get<const int64_t>() + n_lines, 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&g.n_pool, pool_off.get<const int64_t>() + n_lines, 8, hipMemcpyDeviceToHost));
        if (g.K > 0) {
            const int64_t K = g.K, k_tmp_bytes = gki_scan_tmp_bytes(K);
            DevBuf n_of, succ_of, pred_of, too_long;
            HIP_TRY(g.kline.alloc((size_t)K * 8));
            HIP_TRY(g.klo.alloc((size_t)K * 8));
            HIP_TRY(g.khi.alloc((size_t)K * 8));
            HIP_TRY(g.kal.alloc((size_t)K * 4));
            HIP_TRY(g.kchrom.alloc((size_t)K * 4));
            HIP_TRY(g.kpool.alloc((size_t)K * 8));
            HIP_TRY(g.node_before.alloc((size_t)(K + 1) * 8));
            HIP_TRY(g.succ_before.alloc((size_t)(K + 1) * 8));
            HIP_TRY(g.pred_before.alloc((size_t)(K + 1) * 8));
            HIP_TRY(g.alt_before.alloc((size_t)(K + 1) * 8));
            HIP_TRY(g.alt_end.alloc((size_t)K * 8));
            HIP_TRY(n_of.alloc((size_t)K * 4));
            HIP_TRY(succ_of.alloc((size_t)K * 4));
            HIP_TRY(pred_of.alloc((size_t)K * 4));
            HIP_TRY(too_long.alloc(4));
            HIP_TRY(hipMemset(too_long.get(), 0, 4));
            HIP_TRY(tmp.alloc((size_t)k_tmp_bytes));
            hipLaunchKernelGGL(k_gb_compact, dim3(stream_grid(n_lines, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0,
                               kept.get<const uint32_t>(), kept_before.get<const int64_t>(), n_lines, K, g.gpos, g.lo,
                               g.ref_len, g.alt_len, pool_off.get<const int64_t>(), g.bounds.get<const int64_t>(), g.n_chrom,
                               g.kline.get<int64_t>(), g.klo.get<int64_t>(), g.khi.get<int64_t>(), g.kal.get<uint32_t>(),
                               g.kchrom.get<int32_t>(), g.kpool.get<int64_t>());
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_gb_site_counts, dim3(stream_grid(K, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0, K,
                               g.klo.get<const int64_t>(), g.khi.get<const int64_t>(), g.kchrom.get<const int32_t>(),
                               g.bounds.get<const int64_t>(), g.n_chrom, n_of.get<uint32_t>(), succ_of.get<uint32_t>(),
                               pred_of.get<uint32_t>(), too_long.get<unsigned int>());
            HIP_TRY(hipGetLastError());
            GKI_TRY(gki_scan_u32_to_i64(n_of.get<const uint32_t>(), K, g.node_before.get<int64_t>(), tmp.get(), k_tmp_bytes, 0));
            GKI_TRY(gki_scan_u32_to_i64(succ_of.get<const uint32_t>(), K, g.succ_before.get<int64_t>(), tmp.get(), k_tmp_bytes, 0));
            GKI_TRY(gki_scan_u32_to_i64(pred_of.get<const uint32_t>(), K, g.pred_before.get<int64_t>(), tmp.get(), k_tmp_bytes, 0));
            GKI_TRY(gki_scan_u32_to_i64(g.kal.get<const uint32_t>(), K, g.alt_before.get<int64_t>(), tmp.get(), k_tmp_bytes, 0));
            int64_t nodes = 0, succ = 0, pred = 0, alt = 0;
            unsigned int long_gap = 0;
            HIP_TRY(hipMemcpy(&nodes, g.node_before.get<const int64_t>() + K, 8, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(&succ, g.succ_before.get<const int64_t>() + K, 8, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(&pred, g.pred_before.get<const int64_t>() + K, 8, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(&alt, g.alt_before.get<const int64_t>() + K, 8, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(&long_gap, too_long.get(), 4, hipMemcpyDeviceToHost));
            if (long_gap) return gki_set_error(GKI_ERR_BAD_ARG, "graph_build_count: a gap, or a chromosome without a kept site, of 2^31 letters or more does not fit a node");
            if (succ != pred) return gki_set_error(GKI_ERR_BAD_ARG, "graph_build_count: %lld successors and %lld predecessors (internal)", (long long)succ, (long long)pred);
            g.n_nodes = 1 + nodes;
            g.n_edges = succ;
            g.n_bases = total_ref + alt;
        }
    }
    if (g.K == 0) {                                        // alt_before = [0]: the sequence is the reference
        HIP_TRY(g.alt_before.alloc(8));
        HIP_TRY(hipMemset(g.alt_before.get(), 0, 8));
        for (int64_t c = 0; c < n_chromosomes; c++)
            if (h_chromosome_bounds[c + 1] - h_chromosome_bounds[c] > 0x7FFFFFFFll)
                return gki_set_error(GKI_ERR_BAD_ARG, "graph_build_count: chromosome %lld without a kept site has 2^31 letters or "
                                     "more and does not fit a node", (long long)c);
        g.n_nodes = 1 + n_chromosomes;
        g.n_edges = 0;
        g.n_bases = total_ref;
    }
    if (g.n_nodes > 0x7FFFFFFFll)
        return gki_set_error(GKI_ERR_BAD_ARG, "graph_build_count: %lld nodes do not fit int32 edges", (long long)g.n_nodes);
    *n_nodes = g.n_nodes;
    *n_edges = g.n_edges;
    *n_bases = g.n_bases;
    if (n_alt_bytes) *n_alt_bytes = g.n_pool;
    *plan_out = raw;
    guard.p = nullptr;
    return GKI_OK;
}

int gki_graph_build_emit(gki_graph_build *plan, const void *d_reference, const void *d_alt_pool, const void *d_ref_af,
                         const void *d_alt_af, void *d_node_size, void *d_seq, void *d_edge_start,
                         void *d_edges, void *d_rev_start, void *d_rev_edges, void *d_is_ref, void *d_allele_freq,
                         void *d_exists, void *d_node_to_ref_offset, void *d_chromosome_start_nodes, void *d_ref_nodes,
                         void *d_var_nodes, float *sequence_ms) {
    if (sequence_ms) *sequence_ms = 0.0f;
    if (plan == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "graph_build_emit: plan is NULL");
    const gki_graph_build &g = *plan;
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    if (device != g.device) return gki_set_error(GKI_ERR_BAD_ARG, "graph_build_emit: the plan was made on device %d", g.device);
    if (d_reference == nullptr || d_node_size == nullptr || d_seq == nullptr || d_edge_start == nullptr ||
        d_rev_start == nullptr || d_is_ref == nullptr || d_allele_freq == nullptr || d_exists == nullptr ||
        d_node_to_ref_offset == nullptr || d_chromosome_start_nodes == nullptr ||
        (g.n_edges > 0 && (d_edges == nullptr || d_rev_edges == nullptr)) ||
        (g.n_lines > 0 && (d_ref_nodes == nullptr || d_var_nodes == nullptr)) || (g.n_pool > 0 && d_alt_pool == nullptr))
        return gki_set_error(GKI_ERR_BAD_ARG, "graph_build_emit: an input or output buffer is NULL");
    GraphOut o;
    o.node_size = (int32_t *)d_node_size; o.edge_start = (int64_t *)d_edge_start;
    o.edges = (int32_t *)d_edges; o.rev_start = (int64_t *)d_rev_start; o.rev_edges = (int32_t *)d_rev_edges;
    o.is_ref = (uint8_t *)d_is_ref; o.allele_freq = (double *)d_allele_freq; o.exists = (uint8_t *)d_exists;
    o.node_to_ref_offset = (int64_t *)d_node_to_ref_offset; o.chromosome_start_nodes = (int64_t *)d_chromosome_start_nodes;
    o.ref_nodes = (uint32_t *)d_ref_nodes; o.var_nodes = (uint32_t *)d_var_nodes;
    if (g.n_lines > 0) {
        HIP_TRY(hipMemsetAsync(d_ref_nodes, 0, (size_t)g.n_lines * 4, 0));
        HIP_TRY(hipMemsetAsync(d_var_nodes, 0, (size_t)g.n_lines * 4, 0));
    }
    if (g.K == 0)
        hipLaunchKernelGGL(k_gb_emit_whole, dim3((unsigned)ceil_div(g.n_chrom, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0, o,
                           g.bounds.get<const int64_t>(), g.n_chrom);
    else
        hipLaunchKernelGGL(k_gb_emit_nodes, dim3(stream_grid(g.K, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0, g.K,
                           g.kline.get<const int64_t>(), g.klo.get<const int64_t>(), g.khi.get<const int64_t>(),
                           g.kal.get<const uint32_t>(), g.kchrom.get<const int32_t>(), g.bounds.get<const int64_t>(), g.n_chrom,
                           g.node_before.get<const int64_t>(), g.succ_before.get<const int64_t>(),
                           g.pred_before.get<const int64_t>(), g.alt_before.get<const int64_t>(), (const double *)d_ref_af,
                           (const double *)d_alt_af, o, g.alt_end.get<int64_t>());
    HIP_TRY(hipGetLastError());
    TimerEvents ev;
    DevBuf tile_site;                                      // int64[n_tiles + 1], freed behind the synchronise below
    HIP_TRY(tile_site.alloc((size_t)(ceil_div(g.n_bases, SEQ_TILE) + 1) * 8));
    GKI_TRY(ev.start(0));
    const int64_t n_tiles = ceil_div(g.n_bases, SEQ_TILE);
    hipLaunchKernelGGL(k_gb_tile_sites, dim3(stream_grid(n_tiles + 1, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0,
                       g.alt_end.get<const int64_t>(), g.K, n_tiles, tile_site.get<int64_t>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_gb_sequence, dim3((unsigned)(n_tiles < 256 * 8 ? n_tiles : 256 * 8)), dim3(PARSE_BLOCK), 0, 0,
                       (const uint8_t *)d_reference, (const uint8_t *)d_alt_pool, g.K, g.alt_end.get<const int64_t>(),
                       g.alt_before.get<const int64_t>(), g.kpool.get<const int64_t>(), tile_site.get<const int64_t>(),
                       g.n_bases, (uint8_t *)d_seq);
    HIP_TRY(hipGetLastError());
    return ev.stop(0, sequence_ms);
}

}  // extern "C"
