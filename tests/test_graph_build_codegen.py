"""The graph-build kernels (csrc/gki_graph_build.hip) compiled for gfx950: every kernel present, no scratch, no FLAT
memory instruction, and the register and LDS footprints at what the build gives, as upper bounds.  CPU only: hipcc
cross-compiles."""
import re

from codegen_asm import _bodies, _metadata, _of, asm_of, needs_hipcc

pytestmark = needs_hipcc
# kernel -> (VGPRs, LDS bytes) of the build this was written against; the three prefix-maximum kernels hold one int64 per
# lane in LDS
FOOTPRINT = {"k_gb_sites": (40, 0), "k_gb_copy_alt": (18, 0), "k_gb_tile_max": (16, 2048),
             "k_gb_scan_tiles": (16, 2048), "k_gb_keep": (16, 2048), "k_gb_compact": (24, 0), "k_gb_site_counts": (23, 0),
             "k_gb_emit_whole": (26, 0), "k_gb_emit_nodes": (56, 0), "k_gb_tile_sites": (14, 0), "k_gb_sequence": (102, 0)}
asm = asm_of("gki_graph_build")


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


def test_the_sequence_kernel_moves_16_bytes_per_lane(asm):
    body = _of(_bodies(asm), "k_gb_sequence")
    assert re.search(r"^\s*global_load_dwordx4", body, re.M) and re.search(r"^\s*global_store_dwordx4", body, re.M)
