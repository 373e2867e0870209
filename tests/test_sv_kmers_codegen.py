"""The sample_kmers_from_structural_variants kernels (csrc/gki_sv_kmers.hip) compiled for gfx950: no FLAT memory
instruction, no scratch, no LDS, and the register footprint the build obtained: every kernel
fits 8 waves per SIMD with room to spare.  CPU only: hipcc cross-compiles."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "graph_kmer_index_amd", "csrc", "gki_sv_kmers.hip")
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
# kernel -> VGPRs of the build this was written against (an upper bound from then on)
VGPRS = {"k_sv_words": 8, "k_sv_probe": 18, "k_sv_greedyILb0": 18, "k_sv_greedyILb1": 18, "k_sv_records": 20}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("codegen_sv") / "gki_sv_kmers.s")
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
    for k in VGPRS:
        assert sum(k in n for n in names) == 1, k
    assert len(_metadata(asm)) == len(VGPRS)


def test_no_flat_memory_instructions(asm):
    for name, body in _bodies(asm).items():
        assert not re.search(r"^\s*flat_", body, re.M), name


def test_no_scratch_and_no_lds(asm):
    for name, md in _metadata(asm).items():
        assert md["private_segment_fixed_size"] == 0, name
        assert md["group_segment_fixed_size"] == 0, name


def test_register_footprint(asm):
    md = _metadata(asm)
    for k, vgprs in VGPRS.items():
        name = next(n for n in md if k in n)
        assert md[name]["vgpr_count"] <= vgprs, (name, md[name])
        assert md[name]["sgpr_count"] <= 96, (name, md[name])

