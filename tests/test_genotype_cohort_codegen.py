"""The kernels of the genotyped cohort VCF's text (csrc/gki_vcf_cohort.hip) compiled for gfx950: every kernel present, no
scratch, no FLAT memory instruction, 16-byte loads and stores in the emit kernel, and the register and LDS footprints at
what the build gives, as upper bounds.  CPU only: hipcc cross-compiles."""
import re

from codegen_asm import _bodies, _metadata, _of, asm_of, needs_hipcc

pytestmark = needs_hipcc
# kernel -> (VGPRs, LDS bytes): exactly what the build this was written against gives, upper bounds from then on.
# k_vcf_gt_tile_lines is gki_vcf_text.h's, compiled into this file as into gki_vcf_write.hip.
COHORT_FOOTPRINT = {"k_vcf_cohort_pack": (68, 8448), "k_vcf_cohort_lengths": (17, 0), "k_vcf_gt_tile_lines": (14, 0),
                    "k_vcf_cohort_emit": (72, 0)}
asm = asm_of("gki_vcf_cohort")


def test_every_kernel_is_present(asm):
    for k in COHORT_FOOTPRINT:
        assert sum(("%d%s" % (len(k), k)) in n for n in _bodies(asm)) == 1, k
    assert len(_metadata(asm)) == len(COHORT_FOOTPRINT)


def test_no_flat_memory_instructions_and_no_scratch(asm):
    for name, body in _bodies(asm).items():
        assert not re.search(r"^\s*flat_", body, re.M), name
        assert not re.search(r"^\s*scratch_", body, re.M), name
    for name, md in _metadata(asm).items():
        assert md["private_segment_fixed_size"] == 0, name


def test_footprints(asm):
    md = _metadata(asm)
    for k, (vgprs, lds) in COHORT_FOOTPRINT.items():
        m = _of(md, k)
        assert m["vgpr_count"] <= vgprs and m["group_segment_fixed_size"] <= lds, (k, m)


def test_the_dense_emit_moves_sixteen_bytes_a_lane_and_has_no_atomics(asm):
    body = next(b for n, b in _bodies(asm).items() if "k_vcf_cohort_emit" in n)
    assert "global_load_dwordx4" in body and "global_store_dwordx4" in body
    assert "atomic" not in body
    # the pack pass keeps one atomic-min, issued once per wave, for the lowest line at fault
    pack = next(b for n, b in _bodies(asm).items() if "k_vcf_cohort_pack" in n)
    assert len(re.findall(r"^\s*global_atomic_", pack, re.M)) == 1
