// VCF text parsed in HBM: the raw bytes of a VCF file (or of a piece of one that ends at a line end) become what
// VariantArrays holds -- POS, is_snp and the chromosome of every data line, the chromosomes as runs of equal names.  The
// rules are those of include/gki.h ("VCF files"), chosen so that the result equals VariantArrays.from_vcf
// (unique_variant_kmers.py) wherever that function returns.
//
//   (line ends)              gki_text_line_ends: the coalesced 16-byte pass of gki_text_lines.hip, the only whole-line work
//   k_vcf_classify           one lane per line: header / blank / data; a data line is walked to its fifth tab at the most
//                            (never into the genotype columns) for POS, is_snp, where CHROM lies and whether the line is bad
//                            (the line, field and POS rules are gki_text_lines.h's, shared with the graph build's site pass)
//   (exclusive scan)         line -> number of data lines (variants) before it
//   k_vcf_compact            line_of_variant[v]
//   k_vcf_run_flags          one lane per variant: its CHROM against the previous variant's, in length and bytes
//   (two exclusive scans)    variant -> runs begun before it, variant -> name bytes of the runs begun before it
//   k_vcf_emit               one lane per variant: POS, is_snp, its run; the lane of a run's first variant copies the name
//
// A line may be of any length.  A CHROM of 2^32 bytes or more is refused (GKI_ERR_BAD_ARG): a name's length passes through
// the 32-bit input of the scan.
#include "gki_text_lines.h"

namespace {

// beside the lowest bad line (a line of the text, not a data line; kinds 1 and 2), too_long: a CHROM of 2^32 bytes or more
struct VcfTotals : LineFault { unsigned int too_long = 0, pad = 0; };

// One lane per line, by the rules of gki_text_lines.h (vcf_line, vcf_fields, vcf_pos_value).  is_data[i];
// for a data line pos[i], snp[i], and CHROM as bytes [chrom_begin[i], chrom_begin[i] + chrom_len[i]).
__global__ __launch_bounds__(PARSE_BLOCK) void k_vcf_classify(const uint8_t *__restrict__ bytes,
                                                              const int64_t *__restrict__ line_end, int64_t n_lines,
                                                              uint32_t *__restrict__ is_data, int64_t *__restrict__ pos,
                                                              int8_t *__restrict__ snp, int64_t *__restrict__ chrom_begin,
                                                              uint32_t *__restrict__ chrom_len,
                                                              VcfTotals *__restrict__ totals) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_lines; i += stride) {
        const VcfLine l = vcf_line(bytes, line_end, i);
        is_data[i] = l.data ? 1u : 0u;
        if (!l.data) continue;
        const VcfFields f = vcf_fields(bytes, l.b, l.e);
        int64_t value = 0, len0 = f.len(0);
        const int kind = f.n < 2 ? 1 : !vcf_pos_value(bytes, f.begin(1), f.end[1], &value) ? 2 : 0;
        if (kind) line_fault(&totals->first_bad, i, kind);
        if (len0 > 0xFFFFFFFFll) { atomicOr(&totals->too_long, 1u); len0 = 0; }
        pos[i] = value;
        snp[i] = f.n < VCF_FIELDS ? (int8_t)-1 : (int8_t)(f.len(3) == 1 && f.len(4) == 1);
        chrom_begin[i] = l.b;
        chrom_len[i] = (uint32_t)len0;
    }
}

__global__ __launch_bounds__(PARSE_BLOCK) void k_vcf_compact(const uint32_t *__restrict__ is_data,
                                                             const int64_t *__restrict__ variant_index, int64_t n_lines,
                                                             int64_t n_variants, int64_t *__restrict__ line_of_variant) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_lines; i += stride) {
        const int64_t v = variant_index[i];
        if (is_data[i] && v < n_variants) line_of_variant[v] = i;
    }
}

// run_flag[v] = 1 where variant v begins a run of equal CHROM; name_len[v] = the length of the name there, else 0
__global__ __launch_bounds__(PARSE_BLOCK) void k_vcf_run_flags(const uint8_t *__restrict__ bytes,
                                                               const int64_t *__restrict__ line_of_variant,
                                                               const int64_t *__restrict__ chrom_begin,
                                                               const uint32_t *__restrict__ chrom_len, int64_t n_variants,
                                                               uint32_t *__restrict__ run_flag,
                                                               uint32_t *__restrict__ name_len) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_variants; v += stride) {
        const int64_t line = line_of_variant[v];
        const uint32_t len = chrom_len[line];
        bool starts = v == 0;
        if (!starts) {
            const int64_t before = line_of_variant[v - 1];
            starts = chrom_len[before] != len;
            const int64_t a = chrom_begin[line], c = chrom_begin[before];
            for (uint32_t j = 0; !starts && j < len; j++) starts = bytes[a + j] != bytes[c + j];
        }
        run_flag[v] = starts ? 1u : 0u;
        name_len[v] = starts ? len : 0u;
    }
}

// runs_before / name_bytes_before: the exclusive scans of run_flag / name_len.  Thread 0 of the grid closes run_name_start.
__global__ __launch_bounds__(PARSE_BLOCK) void k_vcf_emit(const uint8_t *__restrict__ bytes,
                                                          const int64_t *__restrict__ line_of_variant,
                                                          const int64_t *__restrict__ pos, const int8_t *__restrict__ snp,
                                                          const int64_t *__restrict__ chrom_begin,
                                                          const uint32_t *__restrict__ name_len,
                                                          const uint32_t *__restrict__ run_flag,
                                                          const int64_t *__restrict__ runs_before,
                                                          const int64_t *__restrict__ name_bytes_before, int64_t n_variants,
                                                          int64_t n_runs, int64_t n_name_bytes,
                                                          int64_t *__restrict__ positions, int8_t *__restrict__ is_snp,
                                                          int32_t *__restrict__ chrom_run,
                                                          int64_t *__restrict__ run_name_start,
                                                          uint8_t *__restrict__ run_names) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) run_name_start[n_runs] = n_name_bytes;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_variants; v += stride) {
        const int64_t line = line_of_variant[v];
        const bool starts = run_flag[v] != 0u;
        const int64_t r = runs_before[v] + (starts ? 1 : 0) - 1;   // the run this variant is in
        positions[v] = pos[line];
        is_snp[v] = snp[line];
        chrom_run[v] = (int32_t)r;
        if (starts) {
            const int64_t off = name_bytes_before[v], src = chrom_begin[line];
            const int64_t len = name_len[v];
            if (r >= n_runs || off + len > n_name_bytes) continue;
            run_name_start[r] = off;
            for (int64_t j = 0; j < len; j++) run_names[off + j] = bytes[src + j];
        }
    }
}

// What one parse of a buffer leaves on the device, and its totals.  Both entry points build it; neither keeps it.
struct VcfPlan {
    DevBuf line_end, is_data, pos, snp, chrom_begin, chrom_len, variant_index, line_of_variant, run_flag, name_len,
        runs_before, name_bytes_before, tmp, totals;
    int64_t n_lines = 0, n_variants = 0, n_runs = 0, n_name_bytes = 0, first_bad_variant = -1;
    int first_bad_kind = 0;
};

int vcf_parse(const uint8_t *bytes, int64_t n, VcfPlan &p) {
    if (n < 0) return gki_set_error(GKI_ERR_BAD_ARG, "vcf_parse: n_bytes must be >= 0");
    if (n == 0) return GKI_OK;
    if (bytes == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "vcf_parse: d_bytes is NULL");
    int64_t n_lines = 0;
    GKI_TRY(gki_text_line_ends(bytes, n, "vcf_parse", p.line_end, &n_lines));

    // lines -> variants
    HIP_TRY(p.is_data.alloc((size_t)n_lines * 4));
    HIP_TRY(p.pos.alloc((size_t)n_lines * 8));
    HIP_TRY(p.snp.alloc((size_t)n_lines));
    HIP_TRY(p.chrom_begin.alloc((size_t)n_lines * 8));
    HIP_TRY(p.chrom_len.alloc((size_t)n_lines * 4));
    HIP_TRY(p.variant_index.alloc((size_t)(n_lines + 1) * 8));
    HIP_TRY(p.tmp.alloc((size_t)gki_scan_tmp_bytes(n_lines)));
    GKI_TRY(line_fault_init<VcfTotals>(p.totals));
    hipLaunchKernelGGL(k_vcf_classify, dim3(stream_grid(n_lines, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0, bytes,
                       p.line_end.get<const int64_t>(), n_lines, p.is_data.get<uint32_t>(), p.pos.get<int64_t>(),
                       p.snp.get<int8_t>(), p.chrom_begin.get<int64_t>(), p.chrom_len.get<uint32_t>(),
                       p.totals.get<VcfTotals>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(gki_scan_u32_to_i64(p.is_data.get<const uint32_t>(), n_lines, p.variant_index.get<int64_t>(), p.tmp.get(),
                                gki_scan_tmp_bytes(n_lines), 0));
    VcfTotals totals;
    GKI_TRY(gki_scan_total(p.variant_index, n_lines, &p.n_variants));
    GKI_TRY(line_fault_read(p.totals, &totals));
    p.line_end.reset();
    if (totals.too_long) return gki_set_error(GKI_ERR_BAD_ARG, "vcf_parse: a CHROM of 2^32 bytes or more");
    p.n_lines = n_lines;
    if (totals.line() >= 0) {                              // the data lines before the bad line: its number among them
        GKI_TRY(gki_scan_total(p.variant_index, totals.line(), &p.first_bad_variant));
        p.first_bad_kind = totals.kind();
    }
    if (p.n_variants == 0) return GKI_OK;

    // variants -> runs of equal CHROM
    const int64_t nv = p.n_variants, run_tmp_bytes = gki_scan_tmp_bytes(nv);
    HIP_TRY(p.line_of_variant.alloc((size_t)nv * 8));
    HIP_TRY(p.run_flag.alloc((size_t)nv * 4));
    HIP_TRY(p.name_len.alloc((size_t)nv * 4));
    HIP_TRY(p.runs_before.alloc((size_t)(nv + 1) * 8));
    HIP_TRY(p.name_bytes_before.alloc((size_t)(nv + 1) * 8));
    HIP_TRY(p.tmp.alloc((size_t)run_tmp_bytes));
    hipLaunchKernelGGL(k_vcf_compact, dim3(stream_grid(n_lines, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0,
                       p.is_data.get<const uint32_t>(), p.variant_index.get<const int64_t>(), n_lines, nv,
                       p.line_of_variant.get<int64_t>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_vcf_run_flags, dim3(stream_grid(nv, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0, bytes,
                       p.line_of_variant.get<const int64_t>(), p.chrom_begin.get<const int64_t>(),
                       p.chrom_len.get<const uint32_t>(), nv, p.run_flag.get<uint32_t>(), p.name_len.get<uint32_t>());
    HIP_TRY(hipGetLastError());
    GKI_TRY(gki_scan_u32_to_i64(p.run_flag.get<const uint32_t>(), nv, p.runs_before.get<int64_t>(), p.tmp.get(),
                                run_tmp_bytes, 0));
    GKI_TRY(gki_scan_u32_to_i64(p.name_len.get<const uint32_t>(), nv, p.name_bytes_before.get<int64_t>(), p.tmp.get(),
                                run_tmp_bytes, 0));
    GKI_TRY(gki_scan_total(p.runs_before, nv, &p.n_runs));
    GKI_TRY(gki_scan_total(p.name_bytes_before, nv, &p.n_name_bytes));
    if (p.n_runs > 0x7FFFFFFFll) return gki_set_error(GKI_ERR_BAD_ARG, "vcf_parse: %lld chromosome runs do not fit int32", (long long)p.n_runs);
    return GKI_OK;
}

}  // namespace

extern "C" {

int gki_vcf_parse_count(const void *d_bytes, int64_t n_bytes, int64_t *n_lines, int64_t *n_variants, int64_t *n_chrom_runs,
                        int64_t *n_chrom_bytes, int64_t *first_bad_variant, int *first_bad_kind) {
    if (n_lines) *n_lines = 0;
    if (n_variants) *n_variants = 0;
    if (n_chrom_runs) *n_chrom_runs = 0;
    if (n_chrom_bytes) *n_chrom_bytes = 0;
    if (first_bad_variant) *first_bad_variant = -1;
    if (first_bad_kind) *first_bad_kind = 0;
    VcfPlan p;
    GKI_TRY(vcf_parse((const uint8_t *)d_bytes, n_bytes, p));
    if (n_lines) *n_lines = p.n_lines;
    if (n_variants) *n_variants = p.n_variants;
    if (n_chrom_runs) *n_chrom_runs = p.n_runs;
    if (n_chrom_bytes) *n_chrom_bytes = p.n_name_bytes;
    if (first_bad_variant) *first_bad_variant = p.first_bad_variant;
    if (first_bad_kind) *first_bad_kind = p.first_bad_kind;
    return GKI_OK;
}

int gki_vcf_parse_emit(const void *d_bytes, int64_t n_bytes, void *d_positions, void *d_is_snp, void *d_chrom_run,
                       int64_t variant_capacity, void *d_run_name_start, int64_t run_capacity, void *d_run_names,
                       int64_t name_capacity) {
    if (d_run_name_start == nullptr || run_capacity < 0)
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_parse_emit: d_run_name_start needs at least one entry");
    VcfPlan p;
    GKI_TRY(vcf_parse((const uint8_t *)d_bytes, n_bytes, p));
    if (p.first_bad_variant >= 0)
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_parse_emit: data line %lld is malformed (kind %d)",
                             (long long)p.first_bad_variant, p.first_bad_kind);
    if (p.n_variants > variant_capacity || p.n_runs > run_capacity || p.n_name_bytes > name_capacity)
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_parse_emit: %lld variants, %lld runs and %lld name bytes, capacity %lld, "
                             "%lld and %lld", (long long)p.n_variants, (long long)p.n_runs, (long long)p.n_name_bytes,
                             (long long)variant_capacity, (long long)run_capacity, (long long)name_capacity);
    if (p.n_variants == 0) {                               // no data line: run_name_start = [0]
        HIP_TRY(hipMemset(d_run_name_start, 0, 8));
        return GKI_OK;
    }
    if (d_positions == nullptr || d_is_snp == nullptr || d_chrom_run == nullptr || (p.n_name_bytes > 0 && d_run_names == nullptr))
        return gki_set_error(GKI_ERR_BAD_ARG, "vcf_parse_emit: an output buffer is NULL");
    hipLaunchKernelGGL(k_vcf_emit, dim3(stream_grid(p.n_variants, PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, 0,
                       (const uint8_t *)d_bytes, p.line_of_variant.get<const int64_t>(), p.pos.get<const int64_t>(),
                       p.snp.get<const int8_t>(), p.chrom_begin.get<const int64_t>(), p.name_len.get<const uint32_t>(),
                       p.run_flag.get<const uint32_t>(), p.runs_before.get<const int64_t>(),
                       p.name_bytes_before.get<const int64_t>(), p.n_variants, p.n_runs, p.n_name_bytes,
                       (int64_t *)d_positions, (int8_t *)d_is_snp, (int32_t *)d_chrom_run, (int64_t *)d_run_name_start,
                       (uint8_t *)d_run_names);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return GKI_OK;
}

}  // extern "C"
