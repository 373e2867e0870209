"""The BGZF inflate kernels (csrc/gki_inflate.hip) compiled for gfx950: every kernel present, no FLAT memory instruction
(the Huffman tables of a lane are private memory reached through scratch instructions, the CRC table LDS, the streams
global), and the private segment and LDS sizes at what the build gives.  CPU only: hipcc cross-compiles."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "graph_kmer_index_amd", "csrc", "gki_inflate.hip")
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
# kernel -> (private segment bytes, LDS bytes) of the build this was written against: k_bgzf_inflate keeps one
# gki_inf_tables per lane (1 024 bytes and a spill slot) and the 256-entry CRC table in LDS; k_last_byte one uint64 in LDS
FOOTPRINT = {"k_bgzf_validate": (0, 0), "k_bgzf_inflate": (1028, 1024), "k_bgzf_first_bad": (0, 0), "k_last_byte": (0, 8)}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("codegen_inflate") / "gki_inflate.s")
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
        m = md[next(n for n in md if ("%d%s" % (len(k), k)) in n)]
        assert (m["private_segment_fixed_size"], m["group_segment_fixed_size"]) == (private, lds), (k, m)
