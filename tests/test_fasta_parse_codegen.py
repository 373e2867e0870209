"""The FASTA parse kernels (csrc/gki_fasta_parse.hip) compiled for gfx950: every kernel present, no scratch, no FLAT
memory instruction, the register and LDS footprints at what the build gives, as upper bounds, and one 16-byte load per
lane in the dense passes.  CPU only: hipcc cross-compiles."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "graph_kmer_index_amd", "csrc", "gki_fasta_parse.hip")
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
# kernel -> (VGPRs, LDS bytes) of the build this was written against.  LDS: the four waves' sums (16 bytes a set), and in
# the emit kernel the stage of one tile plus one 16-byte chunk for the shift
FOOTPRINT = {"k_fasta_count_tiles": (22, 16), "k_fasta_header_positions": (22, 16), "k_fasta_header_lines": (25, 0),
             "k_fasta_names": (15, 0), "k_fasta_keep_tiles": (30, 32), "k_fasta_emit": (38, 4144)}
DENSE = ("k_fasta_count_tiles", "k_fasta_header_positions", "k_fasta_keep_tiles", "k_fasta_emit")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("codegen_fasta_parse") / "gki_fasta_parse.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "--cuda-device-only", "-S",
                    SRC, "-o", out], check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def _bodies(txt):
    return {m.group(1): m.group(2) for m in re.finditer(r"\n(_Z\w+):[^\n]*\n(.*?)\n\.Lfunc_end\d+:", txt, re.S)}


def _metadata(txt):
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", txt)[1:]:
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        out[name] = {key: int(re.search(r"\.%s:\s*(\d+)" % key, blk).group(1))
                     for key in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count")}
    return out


def _of(table, kernel):
    return table[next(n for n in table if ("%d%s" % (len(kernel), kernel)) in n)]


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
