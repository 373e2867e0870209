"""The kernels of the genotyper and of the genotyped VCF's text (csrc/gki_genotype.hip, csrc/gki_vcf_write.hip) compiled for
gfx950: every kernel present, no scratch, no FLAT memory instruction, no atomic in the call kernel, the double log from the
device library, and the register and LDS footprints at what the build gives, as upper bounds.  CPU only: hipcc
cross-compiles."""
import re

from codegen_asm import _bodies, _metadata, _of, asm_of, needs_hipcc

pytestmark = needs_hipcc
# kernel -> (VGPRs, LDS bytes): exactly what the build this was written against gives, upper bounds from then on
GENOTYPE_FOOTPRINT = {"k_genotype_fit": (44, 0), "k_genotype_scale": (16, 0), "k_genotype_call": (80, 0)}
WRITE_FOOTPRINT = {"k_vcf_gt_lengths": (17, 0), "k_vcf_gt_tile_lines": (14, 0), "k_vcf_gt_emit": (66, 0)}
asm = asm_of("gki_genotype")
write_asm = asm_of("gki_vcf_write")


def test_every_kernel_is_present(asm, write_asm):
    for txt, table in ((asm, GENOTYPE_FOOTPRINT), (write_asm, WRITE_FOOTPRINT)):
        for k in table:
            assert sum(("%d%s" % (len(k), k)) in n for n in _bodies(txt)) == 1, k
        assert len(_metadata(txt)) == len(table)


def test_no_flat_memory_instructions_and_no_scratch(asm, write_asm):
    for txt in (asm, write_asm):
        for name, body in _bodies(txt).items():
            assert not re.search(r"^\s*flat_", body, re.M), name
            assert not re.search(r"^\s*scratch_", body, re.M), name
        for name, md in _metadata(txt).items():
            assert md["private_segment_fixed_size"] == 0, name


def test_footprints(asm, write_asm):
    for txt, table in ((asm, GENOTYPE_FOOTPRINT), (write_asm, WRITE_FOOTPRINT)):
        md = _metadata(txt)
        for k, (vgprs, lds) in table.items():
            m = _of(md, k)
            assert m["vgpr_count"] <= vgprs and m["group_segment_fixed_size"] <= lds, (k, m)


def test_the_call_kernel_uses_no_atomics_and_double_precision(asm):
    body = next(b for n, b in _bodies(asm).items() if "k_genotype_call" in n)
    assert "atomic" not in body
    assert "v_log_f32" not in body and "v_exp_f32" not in body            # no single-precision shortcut for the log
    assert re.search(r"v_(fma|mul|add)_f64", body)
    # one atomic per wave in the other two: the add of the totals (and the fit's lowest line at fault)
    for k, most in (("k_genotype_fit", 3), ("k_genotype_scale", 1)):
        other = next(b for n, b in _bodies(asm).items() if k in n)
        assert 1 <= len(re.findall(r"^\s*global_atomic_", other, re.M)) <= most, k


def test_the_dense_emit_moves_sixteen_bytes_a_lane(write_asm):
    body = next(b for n, b in _bodies(write_asm).items() if "k_vcf_gt_emit" in n)
    assert "global_load_dwordx4" in body and "global_store_dwordx4" in body
