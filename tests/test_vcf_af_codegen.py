"""The allele-frequency kernels (csrc/gki_vcf_af.hip) compiled for gfx950: every kernel present, no scratch, no FLAT
memory instruction, the register and LDS footprints at what the build gives, as upper bounds, and the genotype kernel's
16-byte load.  CPU only: hipcc cross-compiles."""
import re

from codegen_asm import _bodies, _metadata, _of, asm_of, needs_hipcc

pytestmark = needs_hipcc
# kernel -> (VGPRs, LDS bytes) of the build this was written against: none of them uses LDS
FOOTPRINT = {"k_af_info": (36, 0), "k_af_genotypes": (58, 0)}
asm = asm_of("gki_vcf_af")


def test_every_kernel_is_present(asm):
    names = list(_bodies(asm))
    for k in FOOTPRINT:
        assert sum(("%d%s" % (len(k), k)) in n for n in names) == 1, k
    assert len(_metadata(asm)) == len(FOOTPRINT)


def test_no_flat_memory_instructions(asm):
    for name, body in _bodies(asm).items():
        assert not re.search(r"^\s*flat_", body, re.M), name


def test_no_scratch(asm):
    for name, md in _metadata(asm).items():
        assert md["private_segment_fixed_size"] == 0, name


def test_footprints(asm):
    md = _metadata(asm)
    for k, (vgprs, lds) in FOOTPRINT.items():
        m = _of(md, k)
        assert m["vgpr_count"] <= vgprs and m["group_segment_fixed_size"] <= lds, (k, m)


def test_genotype_kernel_loads_16_bytes_per_lane(asm):
    assert re.search(r"^\s*global_load_dwordx4\s", _of(_bodies(asm), "k_af_genotypes"), re.M)
