"""CPU checks of tests/primitive_cases.py: the constants still stand where the sources have them, the cases are the ones
the seams of the kernels ask for, and the NumPy references agree with plain Python on small inputs.  No device."""
import os
import re

import numpy as np
import pytest

import primitive_cases as cases
from graph_kmer_index_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("path,line,pattern", cases.SOURCE_LINES)
def test_constants_stand_where_the_sources_have_them(path, line, pattern):
    with open(os.path.join(ROOT, path)) as fh:
        text = fh.read().split("\n")[line - 1]
    assert re.search(pattern, text), "%s:%d reads %r" % (path, line, text)


def test_derived_constants():
    assert cases.STILE == cases.SB * cases.SI == 2048
    assert cases.GRID_THREADS == 524288
    assert cases.HASH_SEQUENCE_BASE == 8388608
    assert cases.SEARCH_NS[-1] == 5 * (1 << 20) + 3


def test_the_binding_and_the_header_declare_the_scan_entry():
    assert cases.SCAN_KINDS.keys() == {0, 1, 2}
    assert "gki_exclusive_scan" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "gki.h")) as fh:
        assert re.search(r"int gki_exclusive_scan\(const void \*d_in, int64_t n, int kind, void \*d_out\);", fh.read())


# ------------------------------------------------------------------ scans
def test_scan_sizes_cross_both_seams():
    want = {0: 1, 1: 1, 7: 1, 8: 1, 9: 1, 2047: 1, 2048: 1, 2049: 2, 4095: 2, 4096: 2, 4097: 2,
            2048 ** 2 - 1: 2, 2048 ** 2: 2, 2048 ** 2 + 1: 3, 2048 ** 2 + 2049: 3}
    assert tuple(want) == cases.SCAN_NS
    for n, levels in want.items():
        assert cases.scan_levels(n) == levels, n
    # the temporaries: sums[nb] and scanned[nb + 1] of 8 bytes per level above the first, and 64 bytes
    assert cases.scan_tmp_bytes(2048) == 64
    assert cases.scan_tmp_bytes(2049) == 64 + 8 * 5
    assert cases.scan_tmp_bytes(2048 ** 2) == 64 + 8 * (2 * 2048 + 1)
    assert cases.scan_tmp_bytes(2048 ** 2 + 1) == 64 + 8 * (2 * 2049 + 1) + 8 * 5
    # the third level's last tile: one item, and one item after a full one
    assert (-(-(2048 ** 2 + 1) // 2048)) == 2049 and (-(-(2048 ** 2 + 2049) // 2048)) == 2050
    assert (2048 ** 2 + 1) % 2048 == 1 and (2048 ** 2 + 2049) % 2048 == 1
    assert set(cases.SCAN_ALIGN_NS) >= {4097, 2048 ** 2 + 1}
    assert cases.SCAN_IN_OFFSETS == (0, 1, 2, 3) and cases.SCAN_OUT_OFFSETS == (0, 1)


def test_scan_cases_hold_what_they_claim():
    listed = cases.scan_cases()
    for kind in (0, 1, 2):
        assert {n for k, n, _ in listed if k == kind} == set(cases.SCAN_NS)
    assert [(k, n) for k, n, name in listed if name == "all_ones"] == [(0, 4097)]
    for kind, n, name in listed:
        if n > 4097 and n != 2048 ** 2 + 1:                # the large ones are all built the same way
            continue
        v = cases.scan_values(kind, n, name)
        assert v.dtype == cases.SCAN_KINDS[kind][0] and len(v) == n
        total = sum(int(x) for x in v[:5000]) if n <= 5000 else int(v.sum(dtype=np.int64))
        if (kind, name) == (0, "random") and n >= 9:
            assert total > 2 ** 32
        if name == "zeros":
            assert total == 0
        if name == "last_only" and n:
            assert total == int(v[-1]) == 0x89ABCDEF and not v[:-1].any()
        if (kind, name) == (1, "random") and n >= 4:
            assert v.min() == -2 ** 31 and v.max() == 2 ** 31 - 1 and (v < 0).any() and (v > 0).any()
        if name == "walk":
            assert set(np.unique(v).tolist()) <= {-1, 1}
        if name == "below_wrap":
            assert total <= 2 ** 32 - 1
        if name == "exactly_u32_max":
            assert total == 2 ** 32 - 1
    assert int(cases.scan_values(0, 4097, "all_ones").sum(dtype=np.int64)) == 4097 * 0xFFFFFFFF


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_scan_ref_is_the_running_sum(kind):
    for name, _ in cases.SCAN_VALUES[kind]:
        v = cases.scan_values(kind, 9 if name != "all_ones" else 4097, name)[:9]
        want, run = [0], 0
        for x in v.tolist():
            run += x
            want.append(run)
        got = cases.scan_ref(kind, v)
        assert got.dtype == cases.SCAN_KINDS[kind][1] and len(got) == 10
        assert got.tolist() == [w % 2 ** 32 if kind == 2 else w for w in want]
    assert cases.scan_ref(kind, np.zeros(0, cases.SCAN_KINDS[kind][0])).tolist() == [0]


def test_guarded_input_and_sentinels():
    buf = cases.in_guarded(np.arange(5, dtype=np.uint32), 3, 0xFFFFFFFF)
    assert buf.tolist() == [0xFFFFFFFF] * 3 + [0, 1, 2, 3, 4] + [0xFFFFFFFF] * cases.GUARD
    assert cases.scan_sentinel(0).dtype == np.int64 and cases.scan_sentinel(2).dtype == np.uint32


def test_huge_reads_are_on_both_sides_of_the_limit():
    k = cases.K_READS
    for name, (start, accepted) in cases.HUGE_READS.items():
        counts = [max(b - a - k + 1, 0) for a, b in zip(start, start[1:])]
        assert (max(counts) <= 2 ** 32 - 1) == accepted, name
        assert cases.read_counts_ref(start, k).tolist() == counts
    assert sum(cases.read_counts_ref(cases.HUGE_READS["three_of_2^31"][0], k).tolist()) > 2 ** 32
    assert cases.read_counts_ref(cases.HUGE_READS["largest_accepted"][0], k).tolist() == [2 ** 32 - 1]
    # the two reads that were counted modulo 2^32
    assert cases.HUGE_READS["refused_2^32_k-mers"][0] == [0, 2 ** 32 + 30]
    assert cases.HUGE_READS["refused_2^32+5_k-mers"][0] == [0, 2 ** 32 + 35]
    start = cases.many_short_reads(5000)
    lengths = np.diff(start)
    assert lengths.min() == 0 and lengths.max() == 40 and (lengths < k).any() and (lengths >= k).any()


# ------------------------------------------------------------------ compaction
def test_compaction_cases():
    assert cases.COMPACT_NS == (1, 2047, 2048, 2049, 524287, 524288, 524289, 2048 ** 2 + 1)
    n = 2049
    cols = cases.flat_columns(n)
    assert [c.dtype for c in cols] == [np.uint64, np.uint32, np.uint64, np.float32]
    for c in cols:
        assert len(np.unique(c)) == n
    assert np.isfinite(cols[3]).all()
    big = cases.flat_columns(2048 ** 2 + 1)
    assert len(np.unique(big[1])) == len(big[1]) and len(np.unique(big[3].view(np.uint32))) == len(big[3])
    assert not np.array_equal(cols[0], cols[2]) and not np.array_equal(cols[1], cols[3].view(np.uint32))
    kept = {name: int((cases.compact_flags(n, name) != 0).sum()) for name in cases.COMPACT_FLAGS}
    assert (kept["none"], kept["all"], kept["first"], kept["last"], kept["every_other"]) == (0, n, 1, 1, 1025)
    assert 0 < kept["random_1pct"] < n // 20 and n - n // 20 < kept["random_99pct"] < n
    assert set(np.unique(cases.compact_flags(n, "all")).tolist()) == {1, 2, 255}
    assert cases.compact_flags(n, "last").nonzero()[0].tolist() == [n - 1]
    flags = cases.compact_flags(n, "every_other")
    got = cases.compact_ref(flags, cols)
    for g, c in zip(got, cols):
        assert g.tolist() == [x for x, f in zip(c.tolist(), flags.tolist()) if f]
    assert len(set(type(x) for x in cases.COLUMN_SENTINELS)) == 3 and len(cases.COLUMN_SENTINELS) == 4


# ------------------------------------------------------------------ checksum
def test_checksum_reference():
    assert cases.CHECKSUM_NS == (0, 1, 63, 64, 65, 255, 256, 257, 524287, 524288, 524289, 1048577)
    for elem_bytes, dtype in cases.CHECKSUM_DTYPES.items():
        assert np.dtype(dtype).itemsize == elem_bytes
        v = cases.checksum_values(elem_bytes, 257)
        assert v.dtype == dtype and len(v) == 257 + 3 + cases.GUARD
        assert int(v[3]) == 2 ** (8 * elem_bytes) - 1 and int(v[4]) == 2 ** (8 * elem_bytes - 1)
        for off in cases.CHECKSUM_OFFSETS:
            part = v[off:off + 257]
            s = x = 0
            for e in part.tolist():
                s, x = (s + e) % 2 ** 64, x ^ e
            assert cases.checksum_ref(part) == (s, x)
            assert cases.checksum_ref(part) != cases.checksum_ref(v[off:off + 258])     # what lies behind would show
        assert cases.checksum_ref(v[:0]) == (0, 0)
    wide = cases.checksum_values(8, 1048577)[:1048577]
    assert sum(wide.tolist()) >= 2 ** 64                                                 # the 64-bit sum wraps
    assert cases.checksum_ref(wide)[0] == sum(wide.tolist()) % 2 ** 64


# ------------------------------------------------------------------ last byte
def test_search_cases():
    mib = 1 << 20
    assert cases.SEARCH_NS == (0, 1, mib - 1, mib, mib + 1, 5 * mib + 3)
    assert [len(cases.search_windows(n)) for n in cases.SEARCH_NS] == [0, 1, 1, 1, 2, 3]
    assert cases.search_windows(5 * mib + 3) == [(4 * mib + 3, 5 * mib + 3), (3, 4 * mib + 3), (0, 3)]
    background = cases.search_background(4096)
    assert not np.isin(background, cases.SEARCH_VALUES).any() and len(np.unique(background)) == 253
    for n in cases.SEARCH_NS:
        placements = cases.search_placements(n)
        assert placements["absent"] == ()
        for name, positions in placements.items():
            assert all(0 <= p < n for p in positions), (n, name)
        if n > mib:
            first = cases.search_windows(n)[0][0]
            assert placements["seam"] == (first,) and placements["seam-1"] == (first - 1,)
            assert all(p < first for p in placements["several_in_second_window"])
        if n:
            assert placements["at_both_ends"] == (0, n - 1)
    third = cases.search_placements(5 * mib + 3)
    assert len(third["several_in_second_window"]) == 3 and max(third["several_in_third_window"]) < 3
    buf = np.array([7, 10, 7, 10, 7], np.uint8)
    assert cases.search_ref(buf, 10) == 3 and cases.search_ref(buf, 0) == -1 and cases.search_ref(buf[:0], 10) == -1


def test_long_last_line_file():
    text = cases.long_last_line_fasta()
    lines = text.split(b"\n")
    assert lines[-1] == b"" and len(lines[-2]) == 1_200_000 and lines[-3] == b">long"
    assert max(len(line) for line in lines[:-2]) < 200 and len(lines) == 2 * 300 + 3
    assert len(lines[-2]) > cases.FIRST_WINDOW                                           # the carried tail outgrows the window


# ------------------------------------------------------------------ hash helpers
def test_hash_helper_sizes():
    assert cases.COMPLEMENT_NS == (524289, 1048577) and cases.COMPLEMENT_KS == (1, 31)
    assert cases.HASH_SEQUENCE_NS == (8388608, 8388609, 8388623, 8388625, 31)
    assert cases.HASH_VIEW_N == 100003 and cases.HASH_VIEW_BYTE_OFFSETS == (1, 3, 8)
    assert cases.random_codes(1000).max() == 3 and cases.random_hashes(1000).max() > 2 ** 63
