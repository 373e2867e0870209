"""The kernels of the node counts by difference and of the count model (csrc/gki_haplotype_counts.hip, and k_probe_segments
beside k_probe_reads in csrc/gki_probe.hip) compiled for gfx950: every kernel present, no scratch, no FLAT memory
instruction, and the register and LDS footprints at what the build gives, as upper bounds.  CPU only: hipcc cross-compiles."""
import re

from codegen_asm import _bodies, _metadata, _of, asm_of, needs_hipcc

pytestmark = needs_hipcc
# kernel -> (VGPRs, LDS bytes): exactly what the build this was written against gives, upper bounds from then on
FOOTPRINT = {"k_seg_taken_flags": (10, 0), "k_seg_taken_emit": (8, 0), "k_seg_runsILb0EE": (33, 0),
             "k_seg_runsILb1EE": (25, 0), "k_model_row_start": (16, 0), "k_model_accumulate": (23, 0)}
# the two span walks share one body: a candidate queue of 4 waves x 320 entries of 16 bytes
PROBE_FOOTPRINT = {"k_probe_reads": (53, 20480), "k_probe_segments": (55, 20480)}
asm = asm_of("gki_haplotype_counts")
probe_asm = asm_of("gki_probe")


def test_every_kernel_is_present(asm, probe_asm):
    names = list(_bodies(asm))
    for k in FOOTPRINT:
        assert sum(("%d%s" % (len(k.split("IL")[0]), k)) in n for n in names) == 1, k
    assert len(_metadata(asm)) == len(FOOTPRINT)
    for k in PROBE_FOOTPRINT:
        assert sum(("%d%s" % (len(k), k)) in n for n in _bodies(probe_asm)) == 1, k


def test_no_flat_memory_instructions(asm, probe_asm):
    for txt in (asm, probe_asm):
        for name, body in _bodies(txt).items():
            assert not re.search(r"^\s*flat_", body, re.M), name


def test_no_scratch(asm, probe_asm):
    for txt in (asm, probe_asm):
        for name, md in _metadata(txt).items():
            assert md["private_segment_fixed_size"] == 0, name


def test_footprints(asm, probe_asm):
    md = _metadata(asm)
    for k, (vgprs, lds) in FOOTPRINT.items():
        m = md[next(n for n in md if ("%d%s" % (len(k.split("IL")[0]), k)) in n)]
        assert m["vgpr_count"] <= vgprs and m["group_segment_fixed_size"] <= lds, (k, m)
    md = _metadata(probe_asm)
    for k, (vgprs, lds) in PROBE_FOOTPRINT.items():
        m = _of(md, k)
        assert m["vgpr_count"] <= vgprs and m["group_segment_fixed_size"] <= lds, (k, m)


def test_the_model_kernel_uses_no_atomics(asm):
    body = next(b for n, b in _bodies(asm).items() if "k_model_accumulate" in n)
    assert "atomic" not in body
