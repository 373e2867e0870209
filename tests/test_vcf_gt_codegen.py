"""The haplotype-matrix kernels (csrc/gki_vcf_gt.hip) compiled for gfx950: every kernel present, no scratch, no FLAT memory
instruction; the matrix kernel without LDS and within the 64 VGPRs that keep it at eight waves per SIMD, with its 16-byte
load; the plane kernel with an LDS size of exactly the declared tile.  CPU only: hipcc cross-compiles."""
import ctypes as C
import os
import re

from codegen_asm import ROOT, _bodies, _metadata, _of, asm_of, needs_hipcc

pytestmark = needs_hipcc
KERNELS = ("k_gt_matrix", "k_haplotype_planes")
MATRIX_MAX_VGPRS = 64
PLANES_LINES = 64                                          # a tile's lines; its slots are vcf_files.PLANES_TILE_SLOTS
asm = asm_of("gki_vcf_gt")


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


def test_matrix_kernel_footprint(asm):
    m = _of(_metadata(asm), "k_gt_matrix")
    assert m["group_segment_fixed_size"] == 0 and m["vgpr_count"] <= MATRIX_MAX_VGPRS, m
    assert re.search(r"^\s*global_load_dwordx4\s", _of(_bodies(asm), "k_gt_matrix"), re.M)


def test_planes_kernel_lds_is_the_declared_tile(asm):
    from graph_kmer_index_amd.vcf_files import PLANES_TILE_SLOTS
    m = _of(_metadata(asm), "k_haplotype_planes")
    assert m["group_segment_fixed_size"] == PLANES_LINES * (PLANES_TILE_SLOTS + 4), m    # rows padded by one dword
    source = os.path.join(ROOT, "graph_kmer_index_amd", "csrc", "gki_vcf_gt.hip")
    assert ("PLANES_T = %d;" % PLANES_TILE_SLOTS) in open(source).read()      # the tile the Python layer and the tests name
    assert re.search(r"^\s*global_load_dwordx4\s", _of(_bodies(asm), "k_haplotype_planes"), re.M)


def test_new_symbols_are_exported():
    from graph_kmer_index_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("gki_vcf_haplotype_matrix", "gki_haplotype_planes"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert len(_lib.SYMBOLS["gki_vcf_haplotype_matrix"][1]) == 11 and len(_lib.SYMBOLS["gki_haplotype_planes"][1]) == 6
