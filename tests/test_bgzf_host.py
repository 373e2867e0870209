"""Host side of the BGZF route (graph_kmer_index_amd/bgzf.py, read_files.py), no device: detection, the member scan with
its refusals, the writer read back by Python's gzip, the route of a file, the piece cutter's two limits, and the `map`
parser's --inflate option."""
import gzip
import io
import os
import struct
import zlib

import pytest

import bgzf_cases as cases
from graph_kmer_index_amd import bgzf, read_files
from graph_kmer_index_amd.command_line_interface import build_parser


def test_is_bgzf():
    for name, members in cases.GOOD.items():
        assert bgzf.is_bgzf(cases.file_bytes(members)), name
    assert bgzf.is_bgzf(cases.EOF_MEMBER) and bgzf.EOF_MEMBER == cases.EOF_MEMBER
    assert bgzf.is_bgzf(cases.file_bytes(cases.GOOD["extra_first"])[:25])          # 12 + XLEN bytes are enough
    assert not bgzf.is_bgzf(cases.file_bytes(cases.GOOD["extra_first"])[:24])
    assert not bgzf.is_bgzf(gzip.compress(b">a\nACGT\n"))                           # FLG 0
    assert not bgzf.is_bgzf(b"") and not bgzf.is_bgzf(b">a\nACGT\nACGTACGTACGT\n")
    good = bytearray(cases.EOF_MEMBER)
    for at, value in ((0, 30), (1, 138), (2, 7), (3, 12), (12, 67), (14, 3)):      # ID1, ID2, CM, FLG (FEXTRA | FNAME), SI1, SLEN
        bad = bytearray(good)
        bad[at] = value
        assert not bgzf.is_bgzf(bytes(bad)), at
    other = struct.pack("<BBBBIBBH", 31, 139, 8, 4, 0, 0, 255, 7) + struct.pack("<BBH", 88, 89, 3) + b"xyz"   # no BC at all
    assert not bgzf.is_bgzf(other + b"\x03\x00" + bytes(8))


@pytest.mark.parametrize("name", sorted(cases.GOOD))
def test_scan_members_finds_every_member(name):
    members = cases.GOOD[name]
    data = cases.file_bytes(members)
    got, left = bgzf.scan_all(data)
    assert left == 0 and len(got) == len(members)
    at = 0
    for (start, length, crc, isize, nxt), m in zip(got, members):
        assert data[start:start + length] == m[0] and (crc, isize) == (m[1], m[2])
        assert zlib.decompress(data[start:start + length], -15) == m[3]
        assert start == at + 18 + len(m[4]) and nxt == start + length + 8
        at = nxt
    assert gzip.decompress(data) == b"".join(m[3] for m in members)              # Python's gzip reads the same file
    # from an offset, and over other bytes-like objects
    if len(got) > 1:
        assert bgzf.scan_all(bytearray(data), got[0][4])[0] == got[1:]
    assert bgzf.scan_all(memoryview(data))[0] == got


def test_scan_members_stops_at_a_member_that_is_cut_off():
    data = cases.file_bytes(cases.GOOD["odd_starts"])
    whole, _ = bgzf.scan_all(data)
    for cut in (0, 5, 12, 17, 18, whole[0][4] - 1, whole[0][4], whole[0][4] + 11, whole[2][4] + 30, len(data) - 1):
        got, left = bgzf.scan_all(data[:cut])
        n = sum(1 for m in whole if m[4] <= cut)
        assert got == whole[:n] and left == cut - (whole[n - 1][4] if n else 0), cut


def test_scan_members_refuses_what_is_not_bgzf():
    first = cases.member_bytes(cases.GOOD["fixed"][0])
    base = 1000                                                                  # where the buffer lies in its file

    def refused(second, word):
        with pytest.raises(ValueError) as e:
            bgzf.scan_all(first + second, 0, base)
        assert "offset %d" % (base + len(first)) in str(e.value) and word in str(e.value), str(e.value)

    refused(gzip.compress(b"ACGT") + bytes(20), "FLG")                           # a plain gzip member
    refused(b"ACGTACGTACGTACGT", "not a gzip member")
    named = bytearray(cases.EOF_MEMBER); named[3] = 12
    refused(bytes(named), "FLG")
    no_bc = struct.pack("<BBBBIBBH", 31, 139, 8, 4, 0, 0, 255, 7) + struct.pack("<BBH", 88, 89, 3) + b"xyz" + b"\x03\x00" + bytes(8)
    refused(no_bc, "'BC'")
    small = bytearray(cases.EOF_MEMBER); small[16:18] = struct.pack("<H", 24)     # BSIZE + 1 = 25 < 18 + 8
    refused(bytes(small), "BSIZE")
    big = bytearray(cases.member_bytes(cases.GOOD["one_byte"][0])); big[-4:] = struct.pack("<I", 65537)
    refused(bytes(big), "ISIZE")
    ok = bytearray(cases.member_bytes(cases.GOOD["one_byte"][0])); ok[-4:] = struct.pack("<I", 65536)
    assert len(bgzf.scan_all(first + bytes(ok))[0]) == 2                         # 65 536 itself is allowed


@pytest.mark.parametrize("block_size", [1, 100, 0xff00])
def test_write_bgzf_is_read_back_by_gzip(tmp_path, block_size):
    data = cases.fasta_text(300 if block_size == 1 else 70000, 31)
    path = str(tmp_path / "reads.fa.gz")
    bgzf.write_bgzf(path, data, block_size)
    raw = open(path, "rb").read()
    assert gzip.decompress(raw) == data and raw.endswith(cases.EOF_MEMBER) and bgzf.is_bgzf(raw)
    members, left = bgzf.scan_all(raw)
    assert left == 0 and len(members) == -(-len(data) // block_size) + 1
    assert [m[3] for m in members[:-2]] == [block_size] * (len(members) - 2) and members[-1][3] == 0
    other = str(tmp_path / "threads.fa.gz")
    bgzf.write_bgzf(other, data, block_size, threads=3)                          # members compressed side by side: same file
    assert open(other, "rb").read() == raw
    with pytest.raises(ValueError):
        bgzf.write_bgzf(path, data, 0xff01)
    bgzf.write_bgzf(path, b"")
    assert open(path, "rb").read() == cases.EOF_MEMBER


def test_reads_file_route(tmp_path):
    data = cases.fasta_text(2000, 32)
    plain, packed, blocked = (str(tmp_path / n) for n in ("reads.fa", "reads.fa.gz", "blocked.fa.gz"))
    open(plain, "wb").write(data)
    with gzip.open(packed, "wb") as f:
        f.write(data)
    bgzf.write_bgzf(blocked, data, 512)
    assert read_files.reads_file_route(plain) == "raw"
    assert read_files.reads_file_route(packed) == "gzip-host"
    assert read_files.reads_file_route(blocked) == "bgzf-device"
    renamed = str(tmp_path / "blocked.fa")                                       # by the name first: not .gz is raw
    os.rename(blocked, renamed)
    assert read_files.reads_file_route(renamed) == "raw"
    empty = str(tmp_path / "empty.fa.gz")
    open(empty, "wb").close()
    assert read_files.reads_file_route(empty) == "gzip-host"


def _pieces(raw, chunk_bytes):
    return list(read_files.iter_bgzf_pieces(io.BytesIO(raw), chunk_bytes, "reads.gz"))


def test_piece_cutter_keeps_both_limits(tmp_path):
    data = cases.fasta_text(40000, 33)
    path = str(tmp_path / "reads.fa.gz")
    bgzf.write_bgzf(path, data, 1000)
    raw = open(path, "rb").read()
    members, _ = bgzf.scan_all(raw)
    one = members[0][4]                                                          # the first member's size in the file
    for chunk_bytes in (1, 64, one, 1000, 3000, read_files.DEFAULT_CHUNK_BYTES):
        pieces = _pieces(raw, chunk_bytes)
        assert b"".join(p[0] for p in pieces) == raw
        at, text = 0, b""
        for i, (comp, ms, base) in enumerate(pieces):
            assert base == at and len(ms) >= 1 and ms[-1][4] == len(comp)
            n_out = sum(m[3] for m in ms)
            if len(ms) > 1:
                assert len(comp) <= chunk_bytes and n_out <= chunk_bytes
            if i + 1 < len(pieces):                                              # and no member more would have fitted
                nxt = pieces[i + 1][1][0]
                assert len(comp) + nxt[4] > chunk_bytes or n_out + nxt[3] > chunk_bytes
            text += b"".join(zlib.decompress(comp[m[0]:m[0] + m[1]], -15) for m in ms)
            at += len(comp)
        assert text == data
        if chunk_bytes < one:
            assert len(pieces) == len(members)                                   # one member per piece
        if chunk_bytes == 1000:
            assert [len(p[1]) for p in pieces] == [1] * 39 + [2]                 # ISIZE binds; the empty last member fits
        if chunk_bytes == read_files.DEFAULT_CHUNK_BYTES:
            assert len(pieces) == 1
    with pytest.raises(ValueError):
        _pieces(raw, 0)


def test_piece_cutter_with_members_near_64_kib():
    members = cases.GOOD["max_in"] + cases.GOOD["far"] + cases.GOOD["run"] + cases.GOOD["max_in"] + [cases.EMPTY]
    raw = cases.file_bytes(members)
    for chunk_bytes in (1, 65536, 70000, 140000):
        pieces = _pieces(raw, chunk_bytes)
        assert b"".join(p[0] for p in pieces) == raw and sum(len(p[1]) for p in pieces) == len(members)
        for comp, ms, _ in pieces:
            assert len(ms) == 1 or (len(comp) <= chunk_bytes and sum(m[3] for m in ms) <= chunk_bytes)


def test_the_error_code_and_statuses_are_the_headers():
    """bgzf.GKI_ERR_INFLATE and the status numbers of tests/bgzf_cases.py against include/gki.h and gki_inflate_core.h."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "gki.h")).read()
    assert int(re.search(r"#define GKI_ERR_INFLATE (\d+)", header).group(1)) == bgzf.GKI_ERR_INFLATE
    core = open(os.path.join(root, "graph_kmer_index_amd", "csrc", "gki_inflate_core.h")).read()
    enum = {name: int(value) for name, value in re.findall(r"GKI_INF_([A-Z_]+) = (\d+)", core)}
    for name in ("OK", "INPUT_END", "STORED_LEN", "CODE_LENGTHS", "REPEAT_FIRST", "LITLEN_SYMBOL", "DIST_SYMBOL", "DISTANCE",
                 "OUTPUT_OVERFLOW", "OUTPUT_SHORT", "TRAILING_INPUT", "CRC", "INVALID_CODE"):
        assert enum[name] == getattr(cases, name), name
    assert enum["BLOCK_TYPE"] == cases.BLOCK_TYPE and set(enum.values()) == set(range(14))
    assert set(bgzf.STATUS_TEXT) == set(range(1, 14))


def test_piece_cutter_refuses_a_cut_off_or_foreign_member():
    raw = cases.file_bytes(cases.GOOD["odd_starts"])
    second = bgzf.scan_all(raw)[0][0][4]
    for chunk_bytes in (1, 1 << 20):
        with pytest.raises(ValueError) as e:
            _pieces(raw[:-3], chunk_bytes)
        assert "reads.gz" in str(e.value) and "ends inside" in str(e.value)
        with pytest.raises(ValueError) as e:
            _pieces(raw[:second] + gzip.compress(b"ACGT"), chunk_bytes)
        assert "reads.gz" in str(e.value) and "offset %d" % second in str(e.value)
    assert _pieces(b"", 64) == []


def test_map_parser_has_the_inflate_option():
    parser = build_parser()
    base = ["map", "-i", "index", "-f", "reads.fq.gz", "-o", "out"]
    assert parser.parse_args(base).inflate == "auto"
    for choice in ("auto", "host", "device"):
        assert parser.parse_args(base + ["--inflate", choice]).inflate == choice
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--inflate", "fpga"])
    assert read_files.INFLATE_CHOICES == ("auto", "host", "device")
