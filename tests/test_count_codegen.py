"""The k-mer counting kernels (csrc/gki_count.hip) compiled for gfx950: every kernel present, no FLAT memory instruction,
no scratch, and the scatter kernel's LDS and register footprint at what the build gives (35 864 bytes of
LDS and at most 112 VGPRs are four workgroups per CU either way, 4 waves per SIMD).  CPU only: hipcc cross-compiles."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "graph_kmer_index_amd", "csrc", "gki_count.hip")
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
KERNELS = ("k_count_hist", "k_count_scatter", "k_run_count", "k_run_emit", "k_run_lengths", "k_counter_directory",
           "k_counter_lookup", "k_sv_probe_counter", "k_uvk_summarize_counter")
SCATTER_LDS = 35864          # s_items 32 768 + s_wcnt 2 048 (16-bit counts) + s_dstart 1 024 + s_scan 20, rounded up to 8
SCATTER_VGPRS = 112          # of the build this was written against (an upper bound from then on)


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("codegen_count") / "gki_count.s")
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
                     for key in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count", "sgpr_count")}
    return out


def test_every_kernel_is_present(asm):
    names = list(_bodies(asm))
    for k in KERNELS:
        assert sum(("%d%s" % (len(k), k)) in n for n in names) == 1, k
    assert len(_metadata(asm)) == len(KERNELS)


def test_no_flat_memory_instructions(asm):
    for name, body in _bodies(asm).items():
        assert not re.search(r"^\s*flat_", body, re.M), name


def test_no_scratch(asm):
    for name, md in _metadata(asm).items():
        assert md["private_segment_fixed_size"] == 0, name


def test_scatter_footprint(asm):
    md = _metadata(asm)
    scatter = md[next(n for n in md if "k_count_scatter" in n)]
    assert scatter["group_segment_fixed_size"] == SCATTER_LDS, scatter
    assert scatter["vgpr_count"] <= SCATTER_VGPRS, scatter
    # four workgroups of 256 threads per CU by LDS (160 KB) and by registers (512 per SIMD lane): 4 waves per SIMD
    assert 4 * scatter["group_segment_fixed_size"] <= 160 * 1024 < 5 * scatter["group_segment_fixed_size"]
    assert 4 * SCATTER_VGPRS <= 512
    for k in KERNELS:
        if k != "k_count_scatter":
            m = md[next(n for n in md if ("%d%s" % (len(k), k)) in n)]
            assert m["vgpr_count"] <= 64 and m["group_segment_fixed_size"] <= 1024, (k, m)
