"""The haplotype-path kernels (csrc/gki_haplotype_paths.hip) compiled for gfx950: every kernel present, no scratch, no FLAT
memory instruction, and the register and LDS footprints at what the build gives, as upper bounds.  CPU only: hipcc
cross-compiles."""
import re

from codegen_asm import _bodies, _metadata, _of, asm_of, needs_hipcc

pytestmark = needs_hipcc
# kernel -> (VGPRs, LDS bytes) of the build this was written against; the two alt-node kernels hold one int per wave in LDS
FOOTPRINT = {"k_hap_drops": (22, 0), "k_hap_cuts": (18, 0), "k_hap_tile_sites": (14, 0), "k_hap_spell": (79, 0),
             "k_hap_alt_count": (22, 16), "k_hap_alt_starts": (8, 0), "k_hap_alt_emit": (34, 16)}
asm = asm_of("gki_haplotype_paths")


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


def test_the_spelling_kernel_moves_16_bytes_per_lane(asm):
    body = _of(_bodies(asm), "k_hap_spell")
    assert re.search(r"^\s*global_load_dwordx4", body, re.M) and re.search(r"^\s*global_store_dwordx4", body, re.M)
