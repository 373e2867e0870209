"""The BGZF deflate kernels (csrc/gki_bgzf_deflate.hip) compiled for gfx950: both kernels present, no FLAT memory
instruction (the member's state is LDS, its input, match words and output global, the two small count arrays of the code
construction private), and the private segment and LDS sizes at what the build gives.  The LDS of k_bgzf_deflate is one
gki_def_state, static, below the 64 KiB a static allocation may take.  CPU only: hipcc cross-compiles."""
import re

from codegen_asm import _bodies, _metadata, _of, asm_of, needs_hipcc

pytestmark = needs_hipcc
asm = asm_of("gki_bgzf_deflate")

# kernel -> (private segment bytes, LDS bytes) of the build this was written against
FOOTPRINT = {"k_bgzf_deflate": (80, 40424), "k_bgzf_pack": (0, 0)}


def test_every_kernel_is_present(asm):
    names = list(_bodies(asm))
    for k in FOOTPRINT:
        assert sum(("%d%s" % (len(k), k)) in n for n in names) == 1, k
    assert len(_metadata(asm)) == len(FOOTPRINT)


def test_no_flat_memory_instructions(asm):
    for name, body in _bodies(asm).items():
        assert not re.search(r"^\s*flat_", body, re.M), name


def test_footprints(asm):
    md = _metadata(asm)
    for k, (private, lds) in FOOTPRINT.items():
        m = _of(md, k)
        assert (m["private_segment_fixed_size"], m["group_segment_fixed_size"]) == (private, lds), (k, m)
    assert _of(md, "k_bgzf_deflate")["group_segment_fixed_size"] < 65536


def test_the_shared_words_are_atomics_and_the_pack_moves_16_bytes(asm):
    bodies = _bodies(asm)
    deflate = next(b for n, b in bodies.items() if "14k_bgzf_deflate" in n)
    assert re.search(r"^\s*global_atomic_or\b", deflate, re.M)           # a word two emitters share
    assert re.search(r"^\s*ds_max_u32\b", deflate, re.M)                 # the round's insert
    pack = next(b for n, b in bodies.items() if "11k_bgzf_pack" in n)
    assert re.search(r"^\s*global_load_dwordx4\b", pack, re.M) and re.search(r"^\s*global_store_dwordx4\b", pack, re.M)
