// One graph's haplotype plan (include/gki.h, "haplotype paths"), shared by the spelling passes (gki_haplotype_paths.hip)
// and the segment and count-model passes (gki_haplotype_counts.hip): what create uploads, what a spell count call leaves
// for the calls behind it, and what a segments count call leaves for its emit call.
#pragma once
#include "gki_common.h"

struct gki_haplotype_paths {
    int64_t n_bases = 0, n_lines = 0, K = 0, W = 0;
    int n_chrom = 0, device = 0;
    DevBuf seq, kline, ref_start, ref_size, alt_start, alt_size, kept_bits, var_nodes, chrom_seq_start, chrom_first_kept;
    DevBuf drop_len, drop_start, before, cut, bounds, tile_site, scan_tmp;      // the spell passes' own, sized once
    int64_t scan_tmp_bytes = 0;
    int64_t n_out = -1;                                    // of the last spell count call; -1: none since the last emit
    // whose before / cut / bounds the plan holds: the slot and plane of the last spell count call that succeeded (-1: none)
    int64_t spelled_slot = -1;
    const void *spelled_plane = nullptr;
    DevBuf alt_tile_before;                                // int64[n_slots * T + 1] of the last alt-nodes count call
    int64_t alt_slots = -1, alt_total = 0;
    const void *alt_plane = nullptr;
    // segments.  The all-ref path's before and bounds, made on first use; and, between a segments count call
    // and its emit call, the taken kept lines and where each one's run goes in the two segment lists
    DevBuf ref_before, ref_bounds;
    bool has_ref_path = false;
    DevBuf seg_taken, seg_ref_at, seg_slot_at;             // int64[n_taken], int64[n_taken + 1] twice
    int64_t seg_n_taken = -1, seg_n_ref = 0, seg_n_slot = 0, seg_slot = -1;
    const void *seg_plane = nullptr;                       // with seg_slot: whose spelling the counted runs belong to
    int seg_k = 0;
};

// the plan is there and was made on the device that is current now
static inline int gki_check_haplotype_plan(const gki_haplotype_paths *p, const char *who) {
    if (p == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "%s: plan is NULL", who);
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    if (device != p->device) return gki_set_error(GKI_ERR_BAD_ARG, "%s: the plan was made on device %d", who, p->device);
    return GKI_OK;
}
