"""The FASTA parse kernels (csrc/gki_fasta_parse.hip) compiled for gfx950: every kernel present, no scratch, no FLAT
memory instruction, the register and LDS footprints at what the build gives, as upper bounds, and one 16-byte load per
lane in the dense passes.  CPU only: hipcc cross-compiles."""
import re

from codegen_asm import _bodies, _metadata, _of, asm_of, needs_hipcc

pytestmark = needs_hipcc
# kernel -> (VGPRs, LDS bytes) of the build this was written against.  LDS: the four waves' sums (16 bytes a set), and in
# the emit kernel the stage of one tile plus one 16-byte chunk for the shift
FOOTPRINT = {"k_fasta_count_tiles": (22, 16), "k_fasta_header_positions": (22, 16), "k_fasta_header_lines": (25, 0),
             "k_fasta_names": (15, 0), "k_fasta_keep_tiles": (30, 32), "k_fasta_emit": (38, 4144)}
DENSE = ("k_fasta_count_tiles", "k_fasta_header_positions", "k_fasta_keep_tiles", "k_fasta_emit")
asm = asm_of("gki_fasta_parse")


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


def test_dense_passes_load_16_bytes_per_lane(asm):
    bodies = _bodies(asm)
    for k in DENSE:
        assert re.search(r"^\s*global_load_dwordx4\b", _of(bodies, k), re.M), k
