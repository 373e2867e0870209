"""The UniqueVariantKmersFinder kernels (csrc/gki_variant_kmers.hip) compiled for gfx950: no FLAT memory instruction
and no scratch.  CPU only: hipcc cross-compiles."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "graph_kmer_index_amd", "csrc", "gki_variant_kmers.hip")
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
KERNELS = ("k_uvk_starts", "k_uvk_summarize", "k_uvk_select", "k_uvk_emit")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("codegen_uvk") / "gki_variant_kmers.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "--cuda-device-only", "-S",
                    SRC, "-o", out], check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def _bodies(txt):
    return {m.group(1): m.group(2) for m in re.finditer(r"\n(_Z\w+):[^\n]*\n(.*?)\n\.Lfunc_end\d+:", txt, re.S)}


def test_every_kernel_is_present(asm):
    names = list(_bodies(asm))
    for k in KERNELS:
        assert any(k in n for n in names), k


def test_no_flat_memory_instructions(asm):
    for name, body in _bodies(asm).items():
        assert not re.search(r"^\s*flat_", body, re.M), name


def test_no_scratch(asm):
    blocks = re.split(r"\n  - \.agpr_count:", asm)[1:]
    assert len(blocks) >= len(KERNELS)
    for blk in blocks:
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1)) == 0, name
