"""The graph-build kernels (csrc/gki_graph_build.hip) compiled for gfx950: every kernel present, no scratch, no FLAT
memory instruction, and the register and LDS footprints at what the build gives, as upper bounds.  CPU only: hipcc
cross-compiles."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "graph_kmer_index_amd", "csrc", "gki_graph_build.hip")
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
# kernel -> (VGPRs, LDS bytes) of the build this was written against; the three prefix-maximum kernels hold one int64 per
# lane in LDS
FOOTPRINT = {"k_gb_is_data": (9, 0), "k_gb_sites": (40, 0), "k_gb_copy_alt": (18, 0), "k_gb_tile_max": (16, 2048),
             "k_gb_scan_tiles": (16, 2048), "k_gb_keep": (16, 2048), "k_gb_compact": (24, 0), "k_gb_site_counts": (23, 0),
             "k_gb_emit_whole": (26, 0), "k_gb_emit_nodes": (56, 0), "k_gb_tile_sites": (14, 0), "k_gb_sequence": (102, 0)}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("codegen_graph_build") / "gki_graph_build.s")
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


def test_no_scratch(asm):
    for name, md in _metadata(asm).items():
        assert md["private_segment_fixed_size"] == 0, name


def test_footprints(asm):
    md = _metadata(asm)
    for k, (vgprs, lds) in FOOTPRINT.items():
        m = md[next(n for n in md if ("%d%s" % (len(k), k)) in n)]
        assert m["vgpr_count"] <= vgprs and m["group_segment_fixed_size"] <= lds, (k, m)


def test_the_sequence_kernel_moves_16_bytes_per_lane(asm):
    body = next(b for n, b in _bodies(asm).items() if "13k_gb_sequence" in n)
    assert re.search(r"^\s*global_load_dwordx4", body, re.M) and re.search(r"^\s*global_store_dwordx4", body, re.M)
