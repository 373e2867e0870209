"""Properties of the compiled linear-reference emit kernel (k_linear_emit_dense) that its speed rests on (CPU only: hipcc
cross-compiles).  A wave loads its next block's words ahead of the current block's 256 stores; that only pays if
nothing inside the block loop waits for the wave's stores to drain."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graph_kmer_index_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("codegen_linear") / "gki_linear.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "--cuda-device-only", "-S",
                    os.path.join(CSRC, "gki_linear.hip"), "-o", out], check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def _bodies(txt, name):
    found = re.findall(r"\n(_Z\w*%d%s\w*):[^\n]*\n(.*?)\n\.Lfunc_end\d+:" % (len(name), name), txt, re.S)
    assert found, name
    return dict(found)


def _resources(txt, symbol):
    for blk in re.split(r"\n  - \.agpr_count:", txt)[1:]:
        blk = ".agpr_count:" + blk
        get = lambda key: re.search(r"\.%s:\s*(\S+)" % key, blk).group(1)
        if get("name") == symbol:
            return dict(vgpr=int(get("vgpr_count")) + int(get("agpr_count")), lds=int(get("group_segment_fixed_size")),
                        scratch=int(get("private_segment_fixed_size")))
    raise AssertionError(symbol)


def test_dense_linear_kernel(asm):
    bodies = _bodies(asm, "k_linear_emit_dense")
    assert len(bodies) == 2                                  # four columns, hashes only
    for symbol, body in bodies.items():
        columns = "ILb1E" in symbol
        assert not re.findall(r"\n\s*(flat|scratch)_(load|store|atomic)", body)
        assert not re.findall(r"\n\s*ds_", body)
        # 64 groups of a block in one straight line: a record per lane and store, 8-byte and 4-byte columns
        assert len(re.findall(r"\n\s*global_store_dwordx2 ", body)) == (128 if columns else 64)
        assert len(re.findall(r"\n\s*global_store_dword ", body)) == (128 if columns else 0)
        # a block's words: three loads per lane for the first block, three for the next one, nothing else from memory
        assert len(re.findall(r"\n\s*global_load_", body)) == 6
        # the span table comes in through scalar loads, never queued behind the stores on vmcnt
        assert re.findall(r"\n\s*s_load_dwordx2", body)
        loop = body[body.rfind("s_waitcnt vmcnt(0)"):]       # the first block's words are waited for before the loop ...
        assert "ASMSTART" in loop[:200]
        waits = re.findall(r"s_waitcnt[^\n]*vmcnt\((\d+)\)", loop)[1:]
        assert waits and all(int(w) >= 32 for w in waits), waits      # ... inside it counted waits only: stores stay in flight
        r = _resources(asm, symbol)
        assert r["scratch"] == 0 and r["lds"] == 0, r
        assert r["vgpr"] <= 72, r                            # seven waves per SIMD or more


def test_rest_and_pack_kernels_footprint(asm):
    for name in ("k_linear_emit_rest", "k_pack_letters"):
        for symbol, body in _bodies(asm, name).items():
            r = _resources(asm, symbol)
            assert r["scratch"] == 0 and r["lds"] == 0 and r["vgpr"] <= 64, (symbol, r)
            assert not re.findall(r"\n\s*(flat|scratch)_(load|store|atomic)", body)
    assert re.findall(r"\n\s*global_load_dwordx4", _bodies(asm, "k_pack_letters").popitem()[1])      # 16 letters per lane
