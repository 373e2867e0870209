"""What the BGZF writer's Python layer and its command-line names check before they touch a device: argument errors of
bgzf.deflate_on_device, BgzfWriter and write_bgzf_on_device and of genotyper.write_genotyped_vcf(compress=...), the parsing
of `genotype --compress` and of the `bgzf` sub-command, and the binding of the three new symbols.  No device is needed:
every check here comes before `_lib.require_device()`."""
import os

import pytest

from graph_kmer_index_amd import _lib, bgzf
from graph_kmer_index_amd.command_line_interface import bgzf_command, build_parser, genotype, output_compression
from graph_kmer_index_amd.genotyper import write_genotyped_vcf


@pytest.mark.parametrize("block_size", [0, -1, 0xff01, 1 << 20])
def test_a_block_size_outside_1_to_0xff00_is_refused_and_no_file_is_made(tmp_path, block_size):
    path = str(tmp_path / "out.gz")
    with pytest.raises(ValueError, match="block_size"):
        bgzf.deflate_on_device(b"text", block_size)
    with pytest.raises(ValueError, match="block_size"):
        bgzf.BgzfWriter(path, block_size)
    with pytest.raises(ValueError, match="block_size"):
        bgzf.write_bgzf_on_device(path, b"text", block_size)
    assert not os.path.exists(path)


def test_other_arguments(tmp_path):
    path = str(tmp_path / "out.gz")
    with pytest.raises(ValueError, match="n must be"):
        bgzf.deflate_on_device(b"text", n=-1)
    with pytest.raises(ValueError, match="chunk_bytes"):
        bgzf.write_bgzf_on_device(path, b"text", chunk_bytes=0)
    with pytest.raises(FileNotFoundError):
        bgzf.write_bgzf_on_device(path, str(tmp_path / "missing.fa"))
    assert not os.path.exists(path)


def test_write_genotyped_vcf_refuses_an_unknown_compression_first(tmp_path):
    out = str(tmp_path / "out.vcf")
    with pytest.raises(ValueError, match="compress"):
        write_genotyped_vcf(str(tmp_path / "missing.vcf"), out, [0], [0], 2, compress="gzip")
    assert not os.path.exists(out)


def test_the_symbols_are_bound():
    for name in ("gki_bgzf_deflate_bound", "gki_bgzf_deflate", "gki_bgzf_deflate_kernel_ms"):
        assert name in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["gki_bgzf_deflate"][1]) == 8


def test_the_genotype_command_takes_compress_and_defaults_to_none():
    common = ["genotype", "-V", "v", "-M", "m", "-c", "c", "-v", "in.vcf", "-o", "out.vcf.gz"]
    parser = build_parser()
    args = parser.parse_args(common)
    assert args.compress == "none" and args.func is genotype
    for choice in ("none", "bgzf", "auto"):
        assert parser.parse_args(common + ["--compress", choice]).compress == choice
    with pytest.raises(SystemExit):
        parser.parse_args(common + ["--compress", "gzip"])
    assert output_compression("auto", "out.vcf.gz") == "bgzf" and output_compression("auto", "out.vcf") == "none"
    assert output_compression("none", "out.vcf.gz") == "none" and output_compression("bgzf", "out.vcf") == "bgzf"


def test_the_bgzf_command_parses():
    parser = build_parser()
    args = parser.parse_args(["bgzf", "-i", "reads.fq", "-o", "reads.fq.gz"])
    assert (args.in_file_name, args.out_file_name, args.block_size, args.chunk_bytes) == ("reads.fq", "reads.fq.gz", 0xff00, 64 << 20)
    assert args.func is bgzf_command
    args = parser.parse_args(["bgzf", "-i", "a", "-o", "b", "--block-size", "100", "--chunk-bytes", "4096"])
    assert (args.block_size, args.chunk_bytes) == (100, 4096)
    with pytest.raises(SystemExit):
        parser.parse_args(["bgzf", "-i", "a"])
