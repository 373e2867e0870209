"""The read side compiled for gfx950 (csrc/gki_hash.hip and csrc/gki_probe.hip over the walk of csrc/gki_read_windows.h):
the kernels that moved onto the shared walk and the shared candidate queue are present, use no scratch and no FLAT memory
instruction, and their register and LDS footprints are at most what the same kernels had BEFORE they shared that code.
k_probe_reads and k_probe_segments are pinned by test_haplotype_count_model_codegen.py.  CPU only: hipcc cross-compiles.

Where the bounds come from: the two files as they stood in the commit before the walk was shared ("Genotype a sample on
the GPU: fit the count model, call, write the VCF"), compiled with the command of codegen_asm.asm_of, gave
    k_hash_reads<0>   26 VGPRs    k_hash_reads<1>   30 VGPRs    (no LDS, each with its own loop over the letters)
    k_probe_kmers     40 VGPRs, 20 480 bytes of LDS             (4 waves x 320 queue entries of 16 bytes)
    k_probe_contains  22 VGPRs, 30 720 bytes of LDS             (the same queue and an int64 tag beside every entry)"""
import re

from codegen_asm import _bodies, _metadata, _of, asm_of, needs_hipcc

pytestmark = needs_hipcc
HASH_READS_VGPRS = {0: 26, 1: 30}                    # strand -> VGPRs
QUEUE_FOOTPRINT = {"k_probe_kmers": (40, 20480), "k_probe_contains": (22, 30720)}     # kernel -> (VGPRs, LDS bytes)
hash_asm = asm_of("gki_hash")
probe_asm = asm_of("gki_probe")
measure_asm = asm_of("gki_measure")


def hash_reads_name(names, strand):
    (name,) = [n for n in names if "12k_hash_readsILi%dEE" % strand in n]
    return name


def test_hash_reads_footprints(hash_asm):
    md, bodies = _metadata(hash_asm), _bodies(hash_asm)
    for strand, vgprs in HASH_READS_VGPRS.items():
        m = md[hash_reads_name(md, strand)]
        assert m["private_segment_fixed_size"] == 0, strand
        assert m["group_segment_fixed_size"] == 0, strand
        assert m["vgpr_count"] <= vgprs, (strand, m)
        assert not re.search(r"^\s*flat_", bodies[hash_reads_name(bodies, strand)], re.M), strand


def test_queue_kernels_footprints(probe_asm):
    md, bodies = _metadata(probe_asm), _bodies(probe_asm)
    for k, (vgprs, lds) in QUEUE_FOOTPRINT.items():
        m = _of(md, k)
        assert m["private_segment_fixed_size"] == 0, k
        assert m["vgpr_count"] <= vgprs and m["group_segment_fixed_size"] <= lds, (k, m)
        assert not re.search(r"^\s*flat_", _of(bodies, k), re.M), k


def test_random_loads_kernel_lives_with_the_measurements(probe_asm, measure_asm):
    assert sum("14k_random_loads" in n for n in _bodies(measure_asm)) == 1
    assert not any("k_random_loads" in n for n in _bodies(probe_asm))
