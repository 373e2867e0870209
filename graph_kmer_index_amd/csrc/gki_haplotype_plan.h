// One graph's haplotype plan (include/gki.h, "haplotype paths"), shared by the spelling passes (gki_haplotype_paths.hip)
// and the segment and count-model passes (gki_haplotype_counts.hip): the chain create uploads, the paths built through it,
// and what each count call leaves for its emit call.
#pragma once
#include "gki_common.h"

// A slot of an alt plane on the device: whose path a record holds, whose counts a pending record holds.
struct HapKey {
    int64_t slot = -1;                                     // -1: none
    const void *plane = nullptr;
    bool operator==(const HapKey &o) const { return slot == o.slot && plane == o.plane; }
    bool operator!=(const HapKey &o) const { return !(*this == o); }
    static HapKey all_ref() { return {-2, nullptr}; }      // the path that takes no alt allele, of no plane
};

// A path through the chain: before[j] = letters dropped in front of kept line j (K + 1 entries), cut[j] =
// where line j's dropped allele is skipped in the path's own letters (K + 1 allocated), bounds[c] = where chromosome c
// begins in them (n_chrom + 1).  Filled by gki_haplotype_build_path only; `of` is none while the arrays hold nothing whole.
struct HapPath {
    HapKey of;
    DevBuf before, cut, bounds;
    hipError_t alloc(int64_t K, int n_chrom) {
        hipError_t e = before.alloc((size_t)(K + 1) * 8);
        if (e == hipSuccess) e = cut.alloc((size_t)(K + 1) * 8);
        return e == hipSuccess ? bounds.alloc((size_t)(n_chrom + 1) * 8) : e;
    }
};

struct gki_haplotype_paths {
    // the chain: uploaded by create, never written again
    int64_t n_bases = 0, n_lines = 0, K = 0, W = 0;
    int n_chrom = 0, device = 0;
    DevBuf seq, kline, ref_start, ref_size, alt_start, alt_size, kept_bits, var_nodes, chrom_seq_start, chrom_first_kept;
    // the path builder's scratch, sized once.  The two paths share it: every build overwrites it and nothing reads it
    // behind the build, and a build writes no path but the one it was given.
    DevBuf drop_len, drop_start, scan_tmp;
    int64_t scan_tmp_bytes = 0;
    HapPath slot_path;                                     // of the last spell count call that succeeded
    HapPath ref_path;                                      // the all-ref path, built at the first segments count call
    // a spell count call's for its emit call, of slot_path
    DevBuf tile_site;
    int64_t n_out = -1;                                    // -1: none since the last emit
    // an alt-nodes count call's for its emit call: of.slot is the call's n_slots, tile_before int64[n_slots * T + 1]
    struct { HapKey of; DevBuf tile_before; int64_t total = 0; } alt;
    // a segments count call's for its emit call: the taken kept lines of `of`, whose path slot_path held,
    // and where each one's run goes in the two segment lists: int64[n_taken], int64[n_taken + 1] twice
    struct { HapKey of; DevBuf taken, ref_at, slot_at; int64_t n_taken = 0, n_ref = 0, n_slot = 0; int k = 0; } seg;
};

// the plan is there and was made on the device that is current now
static inline int gki_check_haplotype_plan(const gki_haplotype_paths *p, const char *who) {
    if (p == nullptr) return gki_set_error(GKI_ERR_BAD_ARG, "%s: plan is NULL", who);
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    if (device != p->device) return gki_set_error(GKI_ERR_BAD_ARG, "%s: the plan was made on device %d", who, p->device);
    return GKI_OK;
}

// path = the path of the slot whose bit row is slot_bits (uint64[W] on the device; NULL: it takes no alt allele), on the
// null stream and without a host wait: k_hap_drops, the scan, k_hap_cuts.  path.of is none when it returns; the caller
// names the path once its own call has succeeded.  gki_haplotype_paths.hip
int gki_haplotype_build_path(gki_haplotype_paths &g, const uint64_t *slot_bits, HapPath &path);

// the alt bit of data line `line` in a slot's bit row
__device__ __forceinline__ bool hap_alt_bit(const uint64_t *__restrict__ slot_bits, int64_t line) {
    return (slot_bits[line >> 6] >> (line & 63)) & 1ull;
}
