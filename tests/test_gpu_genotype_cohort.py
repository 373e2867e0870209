"""The genotyped cohort VCF on the device (csrc/gki_vcf_cohort.hip, genotyper.write_cohort_vcf, `genotype` with a batch of
rows) against tests/spec_genotype_cohort.py: the text at the mask's word edges, with columns longer than a tile and a
16-byte word at every offset across every seam; pieces that begin inside the batch; line ranges; refusals; files; and the
closed loop through haplotype_matrix_from_file."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import bgzf_cases
import spec_genotype as single
import spec_genotype_cohort as spec
from graph_kmer_index_amd import _lib
from graph_kmer_index_amd.genotyper import (cohort_header_text, cohort_lines_on_device, genotyped_lines_on_device,
                                            write_cohort_vcf)

pytestmark = pytest.mark.gpu
TILE = 4096
QUALITIES = np.array([0, 9, 10, 99], dtype=np.uint8)


def site(i, info=b".", more=b""):
    return b"1\t%d\trs%d\tA\tC\t.\tPASS\t%s%s" % (100 + i, i, info, more)


def calls_for(n_samples, n, ploidy, seed):
    rng = np.random.default_rng([n_samples, n, ploidy, seed])
    return rng.integers(-1, ploidy + 1, size=(n_samples, n)).astype(np.int8), rng.choice(QUALITIES, size=(n_samples, n))


def ranges_on_device(text, call, gq, ploidy, first=0, pad=0, max_out_bytes=1 << 30):
    """The piece `text` against the batch call[S][V], gq[S][V] laid out with `pad` more entries behind every row; the
    piece's first data line is entry `first`.  Returns the ranges' bytes and the data lines they hold."""
    call, gq = np.asarray(call, dtype=np.int8), np.asarray(gq, dtype=np.uint8)
    n_samples, n = call.shape
    rows_c, rows_q = np.full((n_samples, n + pad), 77, np.int8), np.full((n_samples, n + pad), 200, np.uint8)
    rows_c[:, :n], rows_q[:, :n] = call, gq
    if pad:                                                # a piece never reads what lies behind its lines
        rows_c[:, n:], rows_q[:, n:] = 0, 0
    with _lib.DeviceScope() as s:
        d_text = s.on_device(np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, np.uint8), np.uint8)
        d_call = s.on_device(rows_c.reshape(-1) if rows_c.size else np.zeros(1, np.int8), np.int8)
        d_gq = s.on_device(rows_q.reshape(-1) if rows_q.size else np.zeros(1, np.uint8), np.uint8)
        parts, lines = [], []
        for out, n_out, n_lines in cohort_lines_on_device(d_text, len(text), d_call, d_gq, n_samples, n + pad, first, ploidy,
                                                          max_out_bytes):
            parts.append(out.to_host(n_out).tobytes())
            lines.append(n_lines)
        return parts, lines


def lines_on_device(text, call, gq, ploidy, **kw):
    parts, lines = ranges_on_device(text, call, gq, ploidy, **kw)
    return b"".join(parts), sum(lines)


@pytest.mark.parametrize("ploidy", [1, 2, 3, 8])
def test_the_lines_equal_the_spec_at_the_masks_word_edges(ploidy):
    text = b"##x\n" + b"\n".join(site(i) if i % 3 else site(i, b"AF=0.25", b"\tGT\t0|1") for i in range(70)) + b"\r\n\n"
    for n_samples in (1, 2, 63, 64, 65, 129):
        call, gq = calls_for(n_samples, 70, ploidy, 1)
        got, n = lines_on_device(text, call, gq, ploidy)
        assert n == 70 and got == spec.data_lines_text(text, call, gq, ploidy), n_samples
    # every call and every quality by hand, then all-wide, all-narrow and alternating lines
    n_samples = 66
    text = b"\n".join(site(i) for i in range(5)) + b"\n"
    call = np.array([[(s + v) % (ploidy + 2) - 1 for v in range(5)] for s in range(n_samples)], dtype=np.int8)
    gq = np.array([[QUALITIES[(s // (ploidy + 2) + v) % 4] for v in range(5)] for s in range(n_samples)], dtype=np.uint8)
    call[:, 1], gq[:, 1] = ploidy, 99                      # all wide
    call[:, 2], gq[:, 2] = 0, 9                            # all narrow
    call[:, 3], gq[:, 3] = 1, np.where(np.arange(n_samples) % 2, 10, 0)          # alternating
    call[:, 4], gq[:, 4] = -1, 99                          # no calls: narrow whatever the quality
    got, _ = lines_on_device(text, call, gq, ploidy)
    assert got == spec.data_lines_text(text, call, gq, ploidy)
    assert got.split(b"\n")[4].endswith(b"\t" + b"/".join([b"."] * ploidy) + b":.")


def test_one_sample_equals_the_single_sample_call():
    header = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\n"
    text = header + b"\n".join(site(i, b"L=" + b"ACGT" * (i % 7)) for i in range(400)) + b"\n"
    for ploidy in (1, 2, 3):
        call, gq = calls_for(1, 400, ploidy, 2)
        with _lib.DeviceScope() as s:
            d_text = s.on_device(np.frombuffer(text, dtype=np.uint8), np.uint8)
            d_call, d_gq = s.on_device(call[0], np.int8), s.on_device(gq[0], np.uint8)
            out, n_out, _ = genotyped_lines_on_device(s, d_text, len(text), d_call, d_gq, 0, 400, ploidy)
            want = out.to_host(n_out).tobytes()
        assert lines_on_device(text, call, gq, ploidy)[0] == want == single.data_lines_text(text, call[0], gq[0], ploidy)


def test_columns_longer_than_a_tile_and_fields_longer_than_a_tile():
    n_samples = 700                                        # about 4 900 bytes of columns a line at ploidy 2
    text = b"\n".join([site(0), site(1, b"L=" + b"ACGT" * 2500), site(2), site(3, b"", b"\t" + b"x" * 9000), site(4)]) + b"\n"
    call, gq = calls_for(n_samples, 5, 2, 3)
    call[:, 2], gq[:, 2] = 2, 99                           # a line of wide columns only: 4 900 bytes with no narrow one
    got, n = lines_on_device(text, call, gq, 2)
    want = spec.data_lines_text(text, call, gq, 2)
    assert n == 5 and len(want) > 8 * TILE and got == want
    one, _ = lines_on_device(site(7) + b"\n", call[:, :1], gq[:, :1], 2)         # V = 1, with and without a line end
    assert one == spec.data_lines_text(site(7), call[:, :1], gq[:, :1], 2) == lines_on_device(site(7), call[:, :1], gq[:, :1], 2)[0]


def seam_case(seam):
    """(text of three lines with a filler INFO field of `fill` bytes in the first, calls, the offset in the output that is
    to meet the tile boundary) for one seam.  Three samples at ploidy 2: columns 0 and 1 of the first line are the pair."""
    call = np.array([[1, 0, 2], [2, 1, -1], [0, 2, 1]], dtype=np.int8)
    gq = np.array([[5, 10, 99], [40, 3, 7], [9, 99, 0]], dtype=np.uint8)
    if seam == "wide -> narrow":
        gq[0][0], gq[1][0] = 40, 5

    def text(fill):
        return b"\n".join([site(0, b"N" * fill), site(1), site(2)]) + b"\n"

    first = spec.data_lines_text(site(0, b""), call[:, :1], gq[:, :1], 2)
    where = {"fields -> GT:GQ": first.index(b"\tGT:GQ"),
             "narrow -> wide": first.index(b"\tGT:GQ") + 6 + spec.column_offsets(call[:, 0], gq[:, 0], 2)[1],
             "wide -> narrow": first.index(b"\tGT:GQ") + 6 + spec.column_offsets(call[:, 0], gq[:, 0], 2)[1],
             "last column -> the next line's fields": len(first)}[seam]
    return text, call, gq, where


@pytest.mark.parametrize("seam", ["fields -> GT:GQ", "narrow -> wide", "wide -> narrow", "last column -> the next line's fields"])
def test_a_word_starts_at_every_offset_across_every_seam(seam):
    """The seam lies 8 bytes in front of output byte 64, where a lane's 16-byte word begins, ..., 8 bytes behind it, so a
    word meets it at every offset; and the same 8 bytes either side of the first 4096-byte tile's end."""
    text, call, gq, where = seam_case(seam)
    for base in (64, TILE):
        for shift in range(-8, 9):
            t = text(base + shift - where)
            want = spec.data_lines_text(t, call, gq, 2)
            at = base + shift
            if seam == "fields -> GT:GQ":
                assert want[at:at + 6] == b"\tGT:GQ"
            elif seam == "last column -> the next line's fields":
                assert want[at - 1:at + 2] == b"\n1\t"
            else:
                assert want[at:at + 1] == b"\t" and want[at - 1:at].isdigit()
            assert lines_on_device(t, call, gq, 2)[0] == want, (base, shift)


def test_empty_and_header_only_text():
    call, gq = np.zeros((3, 0), np.int8), np.zeros((3, 0), np.uint8)
    assert lines_on_device(b"", call, gq, 2) == (b"", 0)
    assert lines_on_device(b"##a=b\n#CHROM\tPOS\n\n", call, gq, 2) == (b"", 0)


def test_a_piece_that_begins_inside_the_batch_with_a_longer_row_stride():
    n_samples, n = 67, 150
    lines = [site(i) for i in range(n)]
    call, gq = calls_for(n_samples, n, 2, 4)
    whole = spec.data_lines_text(b"\n".join(lines), call, gq, 2)
    for first, last in ((0, 40), (37, 101), (101, 150)):
        piece = b"\n".join(lines[first:last]) + b"\n"
        want = spec.data_lines_text(piece, call[:, first:last], gq[:, first:last], 2)
        assert want in whole
        got, n_lines = lines_on_device(piece, call, gq, 2, first=first, pad=13)
        assert n_lines == last - first and got == want, first
    with pytest.raises(ValueError, match="more than the"):
        lines_on_device(b"\n".join(lines[100:]) + b"\n", call, gq, 2, first=101)


def test_line_ranges_join_to_the_whole():
    n_samples, n = 65, 40
    text = b"\n".join(site(i, b"N" * (i % 5)) for i in range(n)) + b"\n"
    call, gq = calls_for(n_samples, n, 2, 5)
    want = spec.data_lines_text(text, call, gq, 2)
    per_line = [len(l) + 1 for l in want.split(b"\n")[:-1]]
    for max_out_bytes in (1, min(per_line) - 1, per_line[0], 3 * max(per_line), len(want) - 1, len(want)):
        parts, lines = ranges_on_device(text, call, gq, 2, max_out_bytes=max_out_bytes)
        assert b"".join(parts) == want and sum(lines) == n, max_out_bytes
        assert all(len(p) <= max_out_bytes or k == 1 for p, k in zip(parts, lines))
        if max_out_bytes <= per_line[0]:
            assert lines[0] == 1 and len(parts) > 1
        if max_out_bytes == len(want):
            assert len(parts) == 1


def test_both_fault_kinds_are_named_by_the_lowest_line(tmp_path):
    lines = [site(i) for i in range(200)]
    lines[150] = b"1\t250\t.\tA\tC\t.\tPASS"               # seven fields
    lines[70] = b"1\t170"
    text = b"\n".join(lines) + b"\n"
    call, gq = np.zeros((70, 200), np.int8), np.zeros((70, 200), np.uint8)
    with pytest.raises(ValueError, match="data line 70: fewer than eight fields"):
        lines_on_device(text, call, gq, 2)
    call[69][60], call[0][90], call[3][199] = 3, -2, 9     # in any sample's column
    with pytest.raises(ValueError, match="data line 60: a call outside"):
        lines_on_device(text, call, gq, 2)
    call[69][60], call[5][70] = 2, 7                       # both kinds on line 70: kind 1
    with pytest.raises(ValueError, match="data line 70: fewer than eight fields"):
        lines_on_device(text, call, gq, 2)
    name, out = str(tmp_path / "in.vcf"), str(tmp_path / "out.vcf")
    open(name, "wb").write(text)
    with pytest.raises(ValueError, match="data line 70: fewer than eight fields"):      # numbered in the file, not the piece
        write_cohort_vcf(name, out, call, gq, 2, ["s%d" % i for i in range(70)], chunk_bytes=500)
    assert not os.path.exists(out)


def test_the_emit_call_refuses_a_fault_a_small_capacity_and_no_samples_and_writes_nothing():
    lib = _lib.load()
    n_samples, n = 5, 100
    text = b"\n".join(site(i) for i in range(n)) + b"\n"
    call, gq = calls_for(n_samples, n, 2, 6)
    want = spec.data_lines_text(text, call, gq, 2)
    bad = call.copy()
    bad[3][40] = 5
    with _lib.DeviceScope() as s:
        d_text = s.on_device(np.frombuffer(text, dtype=np.uint8), np.uint8)
        d_call, d_gq, d_bad = s.on_device(call.reshape(-1), np.int8), s.on_device(gq.reshape(-1), np.uint8), s.on_device(bad.reshape(-1), np.int8)
        out = s.on_device(np.full(len(want) + 64, 0xAA, dtype=np.uint8), np.uint8)
        n_out = C.c_int64(-1)

        def emit(calls=d_call, samples=n_samples, n_calls=n, ploidy=2, lines=(0, n), at=out.ptr, capacity=out.n):
            return lib.gki_vcf_cohort_emit(d_text.ptr, len(text), calls.ptr, d_gq.ptr, n, 0, samples, n_calls, ploidy, lines[0],
                                           lines[1], at, capacity, C.byref(n_out), None)
        assert emit(capacity=len(want) - 1) == 2
        assert b"needs %d bytes" % len(want) in lib.gki_last_error() and n_out.value == 0
        assert emit(calls=d_bad) == 2
        assert b"data line 40" in lib.gki_last_error() and n_out.value == 0
        assert emit(calls=d_bad, lines=(50, 60)) == 2      # a piece at fault, wherever the line
        assert emit(samples=0) == 2 and emit(n_calls=n - 1) == 2 and emit(ploidy=0) == 2 and emit(ploidy=9) == 2
        assert emit(lines=(0, n + 1)) == 2 and emit(lines=(3, 2)) == 2 and emit(lines=(-1, 2)) == 2
        assert emit(at=C.c_void_p(out.ptr.value + 4), capacity=out.n - 4) == 2
        counted = [C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int(0)]
        assert lib.gki_vcf_cohort_count(d_text.ptr, len(text), d_call.ptr, d_gq.ptr, n, 0, 0, n, 2, *map(C.byref, counted), None,
                                        0, None) == 2
        assert not (out.to_host() != 0xAA).any()           # nothing was written by any of them
        assert emit(capacity=len(want)) == 0
        got = out.to_host()
        assert n_out.value == len(want) and got[:len(want)].tobytes() == want and not (got[len(want):] != 0xAA).any()
        # the count call: the lines, the bytes, and where each line begins
        d_start = s.array(n + 1, np.int64)
        assert lib.gki_vcf_cohort_count(d_text.ptr, len(text), d_call.ptr, d_gq.ptr, n, 0, n_samples, n, 2, *map(C.byref, counted),
                                        d_start.ptr, n, None) == 2             # one entry too few
        assert lib.gki_vcf_cohort_count(d_text.ptr, len(text), d_call.ptr, d_gq.ptr, n, 0, n_samples, n, 2, *map(C.byref, counted),
                                        d_start.ptr, n + 1, None) == 0
        assert [c.value for c in counted] == [n, len(want), -1, 0]
        ends = np.cumsum([len(l) + 1 for l in want.split(b"\n")[:-1]])
        assert d_start.to_host().tolist() == [0] + ends.tolist()


def vcf_text(n):
    head = (b"##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"x\">\n##contig=<ID=1>\n"
            b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\n")
    return head + b"".join(site(i, b"AF=0.5" if i % 4 else b".", b"\tGT\t0|1\t1|1") + b"\n" for i in range(n))


def inflated(file_name):
    return gzip.open(file_name, "rb").read()


def test_files_in_small_pieces_from_every_encoding_to_plain_and_bgzf(tmp_path):
    n_samples, n = 66, 333
    text = vcf_text(n)
    call, gq = calls_for(n_samples, n, 2, 7)
    names = ["NA%d" % i for i in range(n_samples)]
    want = spec.genotyped_vcf(text, call, gq, 2, names)
    paths = {k: str(tmp_path / k) for k in ("in.vcf", "bgzf.vcf.gz", "gzip.vcf.gz", "out.vcf", "out.vcf.gz")}
    open(paths["in.vcf"], "wb").write(text)
    cuts = list(range(0, len(text), 5000)) + [len(text)]
    open(paths["bgzf.vcf.gz"], "wb").write(bgzf_cases.file_bytes(
        [bgzf_cases.member(text[a:b]) for a, b in zip(cuts[:-1], cuts[1:])] + [bgzf_cases.member(b"")]))
    with gzip.open(paths["gzip.vcf.gz"], "wb") as f:
        f.write(text)
    assert cohort_header_text(paths["in.vcf"], names) == spec.header_text(text, names)
    timings = {}
    assert write_cohort_vcf(paths["in.vcf"], paths["out.vcf"], call, gq, 2, names, chunk_bytes=1000, timings=timings) == n
    assert open(paths["out.vcf"], "rb").read() == want and timings["lengths_ms"] > 0 and timings["emit_call_ms"] > 0
    assert write_cohort_vcf(paths["bgzf.vcf.gz"], paths["out.vcf"], call, gq, 2, names, chunk_bytes=6000, inflate="device",
                            max_out_bytes=20000) == n
    assert open(paths["out.vcf"], "rb").read() == want
    assert write_cohort_vcf(paths["gzip.vcf.gz"], paths["out.vcf"], call, gq, 2, names, inflate="host") == n
    assert open(paths["out.vcf"], "rb").read() == want
    for source, kw in (("in.vcf", dict(chunk_bytes=3000, max_out_bytes=7000)), ("bgzf.vcf.gz", {})):
        assert write_cohort_vcf(paths[source], paths["out.vcf.gz"], call, gq, 2, names, compress="bgzf", **kw) == n
        assert inflated(paths["out.vcf.gz"]) == want
    # the errors of write_genotyped_vcf, and names that do not match the rows; the output is removed
    for calls in (call[:, :-1], np.append(call, np.zeros((n_samples, 1), np.int8), axis=1)):
        with pytest.raises(ValueError, match="data lines"):
            write_cohort_vcf(paths["in.vcf"], paths["out.vcf"], calls, np.zeros(calls.shape, np.uint8), 2, names, chunk_bytes=1000)
        assert not os.path.exists(paths["out.vcf"])
    for bad in (names[:-1], names[:-1] + [names[0]], names[:-1] + ["a b"]):
        with pytest.raises(ValueError, match="name"):
            write_cohort_vcf(paths["in.vcf"], paths["out.vcf"], call, gq, 2, bad)
    with pytest.raises(ValueError):
        write_cohort_vcf(paths["in.vcf"], paths["out.vcf"], call, gq[:-1], 2, names)
    with pytest.raises(ValueError, match="ploidy"):
        write_cohort_vcf(paths["in.vcf"], paths["out.vcf"], call, gq, 9, names)
    assert not os.path.exists(paths["out.vcf"])
    # header-only and empty inputs
    for i, head in enumerate([b"", b"##a=b\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\ts\n"]):
        name = str(tmp_path / ("empty%d.vcf" % i))
        open(name, "wb").write(head)
        assert write_cohort_vcf(name, paths["out.vcf"], np.zeros((2, 0), np.int8), np.zeros((2, 0), np.uint8), 2, ["x", "y"]) == 0
        assert open(paths["out.vcf"], "rb").read() == spec.genotyped_vcf(head, [[], []], [[], []], 2, ["x", "y"])


@pytest.mark.parametrize("ploidy", [1, 2, 3])
def test_the_written_file_reads_back_as_its_haplotype_matrix(tmp_path, ploidy):
    from graph_kmer_index_amd.vcf_files import haplotype_matrix_from_file
    n_samples, n = 65, 90
    call, gq = calls_for(n_samples, n, ploidy, 8)
    names = ["who_%d" % i for i in range(n_samples)]
    name, out = str(tmp_path / "in.vcf"), str(tmp_path / "out.vcf.gz")
    open(name, "wb").write(vcf_text(n))
    assert write_cohort_vcf(name, out, call, gq, ploidy, names, chunk_bytes=2000, compress="bgzf") == n
    matrix = haplotype_matrix_from_file(out, ploidy=ploidy)
    assert (matrix.n_samples, matrix.ploidy, matrix.n_variants) == (n_samples, ploidy, n) and matrix.sample_names == names
    slot = np.arange(ploidy)
    want = np.where(call.T[:, :, None] < 0, 3, slot[None, None, :] >= ploidy - call.T[:, :, None]).astype(np.uint8)
    assert np.array_equal(matrix.codes, want.reshape(n, n_samples * ploidy))
    # the alleles are joined by '/': no line is phased.  (A haploid GT holds no '/' at all, and the matrix's rule -- phased
    # when no GT of the line holds one -- then calls every line phased.)
    assert not (matrix.phased != (1 if ploidy == 1 else 0)).any()


def test_the_genotype_command_with_a_cohort(tmp_path):
    from genotype_cases import case
    from graph_kmer_index_amd.command_line_interface import main
    from graph_kmer_index_amd.haplotype_paths import NodeCountModel
    from graph_kmer_index_amd.unique_variant_kmers import VariantToNodesArrays
    c = case("v257_p2_b5")
    rows = np.ascontiguousarray(c.sample_rows, dtype=np.uint32)
    n_rows = len(rows)
    assert n_rows == 3
    text = vcf_text(c.n_lines)
    f = {n: str(tmp_path / n) for n in ("v2n", "model", "rows.npy", "in.vcf", "a.vcf", "b.vcf", "c.vcf", "one.vcf", "ll", "ll1")}
    VariantToNodesArrays(c.ref_nodes, c.var_nodes).to_file(f["v2n"])
    NodeCountModel(c.histogram, c.count_sum, 31, c.ploidy, c.n_bins, c.samples).to_file(f["model"])
    np.save(f["rows.npy"], rows)
    singles = []
    for r in range(n_rows):
        singles.append(str(tmp_path / ("row%d.npy" % r)))
        np.save(singles[-1], rows[r])
    open(f["in.vcf"], "wb").write(text)
    common = ["genotype", "-V", f["v2n"] + ".npz", "-M", f["model"], "-v", f["in.vcf"]]
    assert main(common + ["-c", f["rows.npy"], "-o", f["a.vcf"], "-L", f["ll"]]) == 0
    assert main(common + ["-c", ",".join(singles), "-o", f["b.vcf"], "--batch-bytes", "1", "--chunk-bytes", "900"]) == 0
    a = open(f["a.vcf"], "rb").read()
    assert a == open(f["b.vcf"], "rb").read()              # a 2-D file or a list; one batch or a row a batch
    names = ["sample_%d" % (i + 1) for i in range(n_rows)]
    assert a.startswith(spec.header_text(text, names))
    loglik = np.load(f["ll"] + ".npy")
    assert loglik.shape == (n_rows, c.n_lines, 3)
    # column s is the single-sample command's column for row s, and its loglik that command's
    body = [l.split(b"\t") for l in a[len(spec.header_text(text, names)):].split(b"\n")[:-1]]
    for r in range(n_rows):
        assert main(common + ["-c", singles[r], "-o", f["one.vcf"], "-s", "who", "-L", f["ll1"]]) == 0
        one = open(f["one.vcf"], "rb").read()
        assert one.startswith(single.header_text(text, "who"))
        lines = [l.split(b"\t") for l in one[len(single.header_text(text, "who")):].split(b"\n")[:-1]]
        assert [l[:9] for l in lines] == [l[:9] for l in body] and [l[9] for l in lines] == [l[9 + r] for l in body]
        assert np.array_equal(np.load(f["ll1"] + ".npy"), loglik[r])
    # names and coverages per row; one coverage for all
    picked = ",".join("n%d" % i for i in range(n_rows))
    assert main(common + ["-c", f["rows.npy"], "-o", f["c.vcf"], "-s", picked, "--coverage", "0.5"]) == 0
    assert main(common + ["-c", f["rows.npy"], "-o", f["b.vcf"], "-s", picked, "--coverage", ",".join(["0.5"] * n_rows)]) == 0
    assert open(f["c.vcf"], "rb").read() == open(f["b.vcf"], "rb").read()
    assert b"\tFORMAT\t" + picked.replace(",", "\t").encode() + b"\n" in open(f["c.vcf"], "rb").read()
    for wrong in (["-s", "a,a,b"], ["-s", "a,b"], ["-s", "a,b,c d"], ["--coverage", "1,2"], ["--coverage", "1,2,0"]):
        with pytest.raises(ValueError):
            main(common + ["-c", f["rows.npy"], "-o", f["c.vcf"]] + wrong)
    np.save(f["rows.npy"], rows[0][:-1])
    with pytest.raises(ValueError, match="one length"):
        main(common + ["-c", singles[0] + "," + f["rows.npy"], "-o", f["c.vcf"]])
