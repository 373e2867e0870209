"""The data-line numbering the VCF passes share (gki_vcf_data_lines, csrc/gki_text_lines.hip) against the line rule of
tests/spec_vcf_parse.py: the parser, the graph build's site pass, the allele frequencies of both sources and the haplotype
matrix count the same data lines in a text of every kind of skipped line, whole and with any number of its last bytes cut
off; each counting pass refuses a caller's count that is one off, under its own name; and the one-lane-per-line kernel
numbers a text of more lines than its largest grid has lanes."""
import ctypes as C

import numpy as np
import pytest

import spec_vcf_parse as spec

pytestmark = pytest.mark.gpu

GKI_OK, GKI_ERR_BAD_ARG = 0, 2                             # include/gki.h
DATA = b"1\t%d\t.\tA\tC"                                   # a data line the site pass finds well-formed: REF is the reference's
REFERENCE_LETTERS = 100                                    # one chromosome of that many 'A'
STRIP_ONLY = (b" ", b"\t", b"\x0b\x0c", b"\x1c\x1d\x1e\x1f", b" \t\x0b\x0c\x0d\x1c\x1d\x1e\x1f \t")
# headers before and between the data lines, lines of strip bytes only, an empty line, \r\n and \r\r\n ends, a '#' line in
# the middle, a data line that begins with a blank, and an unterminated last data line
MIXED = b"".join([
    b"##fileformat=VCFv4.2\n", b"#CHROM\tPOS\tID\tREF\tALT\n", DATA % 5 + b"\n", b"\n", STRIP_ONLY[0] + b"\n",
    DATA % 6 + b"\r\n", b"#a header in the middle\n", DATA % 7 + b"\r\r\n", b"\r\n", STRIP_ONLY[1] + b"\n",
    STRIP_ONLY[2] + b"\r\n", DATA % 8 + b"\n", b"##another header\r\n", b" " + DATA % 9 + b"\n", STRIP_ONLY[3] + b"\n",
    b"#\n", STRIP_ONLY[4] + b"\n", b"\r\r\n", DATA % 10 + b"\n", b"#\r\n", DATA % 11])
SWEEP_GRID_LANES = 2048 * 256                              # stream_grid's largest grid x PARSE_BLOCK (csrc/gki_common.h)


class Passes:
    """The entry points that number data lines, on one device text and the site pass's inputs for up to `max_lines` data
    lines: every line is of chromosome run 0, the whole reference."""

    def __init__(self, scope, text, max_lines):
        from graph_kmer_index_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        self.text = scope.on_device(np.frombuffer(text, dtype=np.uint8), np.uint8)
        n = max_lines + 1
        self.chrom_run = scope.on_device(np.zeros(n, dtype=np.int32), np.int32)
        self.run_c0 = scope.on_device(np.zeros(1, dtype=np.int64), np.int64)
        self.run_c1 = scope.on_device(np.full(1, REFERENCE_LETTERS, dtype=np.int64), np.int64)
        self.reference = scope.on_device(np.frombuffer(b"A" * REFERENCE_LETTERS, dtype=np.uint8), np.uint8)
        self.f64 = [scope.array(n, np.float64) for _ in range(2)]
        self.u8 = [scope.array(n, np.uint8) for _ in range(2)]
        self.span_begin, self.span_len = scope.array(n, np.int64), scope.array(n, np.int32)

    def message(self):
        return self.lib.gki_last_error().decode("utf-8", "replace")

    def parse_count(self, n_bytes):
        from graph_kmer_index_amd.vcf_files import vcf_count
        return vcf_count(self.text, n_bytes)[1]

    def sites(self, n_bytes, nv):
        """(return code, first bad data line)"""
        n_alt, bad, kind = C.c_int64(0), C.c_int64(-1), C.c_int(0)
        rc = self.lib.gki_graph_sites_count(self.text.ptr, n_bytes, self.chrom_run.ptr, nv, self.run_c0.ptr, self.run_c1.ptr,
                                            1, self.reference.ptr, C.byref(n_alt), C.byref(bad), C.byref(kind))
        return rc, bad.value

    def allele_frequencies(self, n_bytes, nv, source):
        """(return code, the data lines the pass found)"""
        found, bad, kind, ms = C.c_int64(-1), C.c_int64(-1), C.c_int(0), C.c_float(0)
        rc = self.lib.gki_vcf_allele_frequencies(self.text.ptr, n_bytes, source, nv, self.f64[0].ptr, self.f64[1].ptr,
                                                 self.u8[0].ptr, self.span_begin.ptr, self.span_len.ptr, C.byref(found),
                                                 C.byref(bad), C.byref(kind), C.byref(ms))
        return rc, found.value

    def haplotype_matrix(self, n_bytes, nv):
        """(return code, the data lines the pass found); no sample columns, so a line of five fields is not at fault"""
        found, bad, kind, ms = C.c_int64(-1), C.c_int64(-1), C.c_int(0), C.c_float(0)
        rc = self.lib.gki_vcf_haplotype_matrix(self.text.ptr, n_bytes, nv, 0, 2, self.u8[0].ptr, self.u8[1].ptr,
                                               C.byref(found), C.byref(bad), C.byref(kind), C.byref(ms))
        return rc, found.value

    def assert_all_count(self, n_bytes, want):
        assert self.parse_count(n_bytes) == want
        assert self.sites(n_bytes, want)[0] == GKI_OK, self.message()      # the site pass reports a count by accepting it
        for source in (0, 1):
            assert self.allele_frequencies(n_bytes, want, source) == (GKI_OK, want), (source, self.message())
        assert self.haplotype_matrix(n_bytes, want) == (GKI_OK, want), self.message()


def spec_count(text):
    return len(spec.parse(text)["positions"])


def test_every_pass_counts_the_spec_s_data_lines_whole_and_cut_anywhere_at_the_end():
    from graph_kmer_index_amd import _lib
    assert spec_count(MIXED) == 7 and not MIXED.endswith(b"\n") and MIXED.count(b"\n") == 20
    with _lib.DeviceScope() as s:
        passes = Passes(s, MIXED, spec_count(MIXED))
        for n_bytes in range(len(MIXED), -1, -1):           # the device text is one; its first n_bytes are the cut text
            passes.assert_all_count(n_bytes, spec_count(MIXED[:n_bytes]))


def test_a_count_one_off_is_refused_under_the_pass_s_name():
    from graph_kmer_index_amd import _lib
    want = spec_count(MIXED)
    with _lib.DeviceScope() as s:
        passes = Passes(s, MIXED, want + 1)
        calls = {"graph_sites": lambda nv: passes.sites(len(MIXED), nv)[0],
                 "vcf_allele_frequencies": lambda nv: passes.allele_frequencies(len(MIXED), nv, 0)[0],
                 "vcf_allele_frequencies ": lambda nv: passes.allele_frequencies(len(MIXED), nv, 1)[0],
                 "vcf_haplotype_matrix": lambda nv: passes.haplotype_matrix(len(MIXED), nv)[0]}
        for name, call in calls.items():
            for nv in (want + 1, want - 1):
                assert call(nv) == GKI_ERR_BAD_ARG, (name, nv)
                message = passes.message()
                assert message.startswith(name.strip() + ": "), message
                assert (" %d " % want) in message and message.endswith(" %d" % nv), message
            assert call(want) == GKI_OK, (name, passes.message())


def test_more_lines_than_the_largest_grid_has_lanes():
    from graph_kmer_index_amd import _lib
    from graph_kmer_index_amd.vcf_files import VariantPieces, parse_vcf_on_device
    n_lines = SWEEP_GRID_LANES + 3
    lines = [b"#"] * n_lines
    for i in list(range(0, n_lines, 1000)) + [n_lines - 3, n_lines - 2, n_lines - 1]:
        lines[i] = DATA % 5
    text = b"\n".join(lines) + b"\n"
    want = spec.parse(text)
    n_data = len(want["positions"])
    assert want["n_lines"] == n_lines and n_data == len(range(0, n_lines, 1000)) + 3
    joined = VariantPieces()
    joined.add(*parse_vcf_on_device(text))
    got = joined.variant_arrays()
    assert joined.n_lines == n_lines and np.array_equal(got.positions, want["positions"])
    assert np.array_equal(got.line_numbers, np.arange(n_data))
    with _lib.DeviceScope() as s:
        passes = Passes(s, text, n_data)
        passes.assert_all_count(len(text), n_data)
        assert passes.sites(len(text), n_data) == (GKI_OK, -1)   # every data line found its own entry of chrom_run
