"""What the codegen tests of the text parsers share (test_reads_parse_codegen, test_text_lines_codegen,
test_vcf_parse_codegen, test_graph_build_codegen, test_fasta_parse_codegen): one file of csrc compiled to gfx950 assembly,
and the kernels' bodies and metadata read out of it.  CPU only: hipcc cross-compiles."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


def asm_of(stem):
    """A module-scoped fixture: the device assembly of graph_kmer_index_amd/csrc/<stem>.hip, as text."""
    @pytest.fixture(scope="module")
    def asm(tmp_path_factory):
        src = os.path.join(ROOT, "graph_kmer_index_amd", "csrc", stem + ".hip")
        out = str(tmp_path_factory.mktemp("codegen_" + stem) / (stem + ".s"))
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "--cuda-device-only",
                        "-S", src, "-o", out], check=True, stderr=subprocess.DEVNULL)
        return open(out).read()
    return asm


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
