"""The per-node early-stop search (k_forward_node, csrc/gki_forward.hip) and its start kernel (k_uvk_simple_starts,
csrc/gki_variant_kmers.hip) compiled for gfx950: the properties tests/test_kernel_codegen.py pins for k_forward -- the
product kernels at 8 waves per SIMD, no FLAT memory instruction, the first levels of the walk in registers -- and the slow
path's stacks out of scratch.  CPU only: hipcc cross-compiles."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graph_kmer_index_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
PRODUCT = ("k_forward_node<false, false>", "k_forward_node<true, false>")
DEEP = ("k_forward_node<false, true>", "k_forward_node<true, true>")


def _asm(tmp_path_factory, source):
    out = str(tmp_path_factory.mktemp("codegen_node") / (source + ".s"))
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "--cuda-device-only", "-S",
                    os.path.join(CSRC, source + ".hip"), "-o", out], check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.fixture(scope="module")
def forward_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "gki_forward")


@pytest.fixture(scope="module")
def starts_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "gki_variant_kmers")


def _demangled(names):
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    return [re.sub(r"\(anonymous namespace\)::|void ", "", d).split("(")[0] for d in dem]


def _functions(txt):
    found = {m.group(1): m.group(2) for m in re.finditer(r"\n(_Z\w+):[^\n]*\n(.*?)\n\.Lfunc_end\d+:", txt, re.S)}
    return dict(zip(_demangled(list(found)), found.values()))


def _resources(txt):
    res = {}
    for blk in re.split(r"\n  - \.agpr_count:", txt)[1:]:
        blk = ".agpr_count:" + blk
        get = lambda key: re.search(r"\.%s:\s*(\S+)" % key, blk).group(1)
        res[get("name")] = dict(vgpr=int(get("vgpr_count")) + int(get("agpr_count")), lds=int(get("group_segment_fixed_size")),
                                scratch=int(get("private_segment_fixed_size")))
    return dict(zip(_demangled(list(res)), res.values()))


def test_both_passes_exist_as_product_and_deep_kernels(forward_asm):
    names = set(_resources(forward_asm))
    for v in PRODUCT + DEEP:
        assert v in names, (v, sorted(names))


def test_product_kernels_run_at_full_occupancy(forward_asm):
    r = _resources(forward_asm)
    for v in PRODUCT:
        assert r[v]["vgpr"] <= 64 and r[v]["lds"] == 0, (v, r[v])
        # (no `last` stack and no script: never more scratch than the walk with a follow mask)
        assert r[v]["scratch"] <= r["k_forward<false, false, false>"]["scratch"], (v, r[v])


def test_no_flat_memory_instructions_and_register_levels(forward_asm):
    f = _functions(forward_asm)
    for v in PRODUCT:
        body = f[v]
        assert not re.findall(r"\n\s*flat_(load|store|atomic)", body), v
        assert len(re.findall(r"\n\s*scratch_store", body)) <= 12, (v, len(re.findall(r"\n\s*scratch_store", body)))
        assert len(re.findall(r"\n\s*scratch_store_\w+ off,", body)) <= 2, v


def test_deep_kernels_keep_their_stacks_out_of_scratch(forward_asm):
    r = _resources(forward_asm)
    for v in DEEP:
        assert r[v]["scratch"] <= 256, (v, r[v])


def test_start_kernel_has_no_flat_instruction_and_no_scratch(starts_asm):
    r, f = _resources(starts_asm), _functions(starts_asm)
    assert r["k_uvk_simple_starts"]["scratch"] == 0 and r["k_uvk_simple_starts"]["lds"] == 0
    assert not re.search(r"^\s*flat_", f["k_uvk_simple_starts"], re.M)
