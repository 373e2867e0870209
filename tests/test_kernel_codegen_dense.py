"""Properties of the compiled split-layout interior kernel (k_emit_interior_dense) that its speed rests on (CPU only:
hipcc cross-compiles).  The block loop issues the next block's loads ahead of the 256 stores of the current block; that
only pays if nothing in the loop waits for the wave's stores to drain, i.e. no s_waitcnt vmcnt(0) after the loop header."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graph_kmer_index_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("codegen_dense") / "gki_finder.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "--cuda-device-only", "-S",
                    os.path.join(CSRC, "gki_finder.hip"), "-o", out], check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def _body(txt, name):
    m = re.search(r"\n(_Z\w*%d%s\w*):[^\n]*\n(.*?)\n\.Lfunc_end\d+:" % (len(name), name), txt, re.S)
    assert m, name
    return m.group(2)


def _resources(txt, name):
    for blk in re.split(r"\n  - \.agpr_count:", txt)[1:]:
        blk = ".agpr_count:" + blk
        get = lambda key: re.search(r"\.%s:\s*(\S+)" % key, blk).group(1)
        if "%d%sE" % (len(name), name) in get("name"):
            return dict(vgpr=int(get("vgpr_count")) + int(get("agpr_count")), lds=int(get("group_segment_fixed_size")),
                        scratch=int(get("private_segment_fixed_size")))
    raise AssertionError(name)


def test_dense_interior_kernel_memory_instructions(asm):
    body = _body(asm, "k_emit_interior_dense")
    assert not re.findall(r"\n\s*(flat|scratch)_(load|store|atomic)", body)
    # 64 groups x 4 columns, one straight line of stores per block
    assert len(re.findall(r"\n\s*global_store_", body)) == 256
    # the block table comes in through scalar loads (the LDS/scalar counter), never queued behind the stores on vmcnt
    assert re.findall(r"\n\s*s_load_dwordx4", body)
    loop = body[body.rfind("Loop Header: Depth=1"):]
    waits = re.findall(r"s_waitcnt[^\n]*vmcnt\((\d+)\)", loop)
    assert waits and all(int(w) >= 32 for w in waits), waits      # counted waits only: stores stay in flight


def test_dense_interior_kernel_footprint(asm):
    r = _resources(asm, "k_emit_interior_dense")
    assert r["scratch"] == 0, r
    assert r["lds"] == 20480, r                  # 5 KB per wave: 8 workgroups of 4 waves per CU
    assert r["vgpr"] <= 64, r                    # registers never the limit at 8 waves per SIMD
    rest = _resources(asm, "k_emit_interior_dense_rest")
    assert rest["scratch"] == 0 and not re.findall(r"\n\s*flat_(load|store)", _body(asm, "k_emit_interior_dense_rest"))
