"""-m gpu: reads files parsed on the device (csrc/gki_reads_parse.hip, graph_kmer_index_amd/read_files.py) against the
plain-Python semantics of tests/spec_read_files.py, and the file routes built on them -- map_reads_file, the .gz route,
CounterKmerIndex.count_reads_file, the `map` sub-command -- against the existing in-memory route, the NumPy read-side
reference and the hashes recorded from the reference.  Every comparison is exact.

The two constants below are copied from the kernel sources named beside them; the boundary files of
tests/read_file_cases.py are laid out from them."""
import gzip
import json
import os

import numpy as np
import pytest

import read_file_cases as cases
import spec_read_files as spec
from graph_kmer_index_amd import CollisionFreeKmerIndex, CounterKmerIndex, FlatKmers, _lib, read_files
from graph_kmer_index_amd.command_line_interface import main
from read_side_ref import build_index_ref, count_nodes_ref

pytestmark = pytest.mark.gpu

T = 4096            # csrc/gki_text_lines.h PARSE_TILE = 256 lanes * 16 bytes: the bytes one workgroup scans
S = 2048            # csrc/gki_runtime.hip:276 STILE = 256 * 8: the items one block of the exclusive scans covers
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX = 2 ** 62
N_NODES = 37
INDEX_KEYS = ("_hashes_to_index", "_n_kmers", "_kmers", "_nodes", "_ref_offsets", "_frequencies", "_allele_frequencies")


def device_parse(data, fmt, line_phase=0, buf=None):
    """(letters, read_start, n_reads, n_lines, n_bad) of the device, both calls checked against each other."""
    buf = np.frombuffer(data, dtype=np.uint8) if buf is None else buf
    n_lines, n_reads, n_letters, n_bad = read_files.count_reads_in_buffer(buf, fmt, line_phase)
    letters, read_start, n_reads2, n_lines2 = read_files.parse_reads_on_device(buf, fmt, line_phase)
    assert (n_reads2, n_lines2, letters.n, read_start.n) == (n_reads, n_lines, n_letters, n_reads + 1)
    out = letters.to_host(), read_start.to_host(), n_reads, n_lines, n_bad
    letters.free()
    read_start.free()
    return out


def assert_parse(data, fmt, line_phase=0, buf=None):
    reads, n_lines, n_bad = spec.parse(data, fmt, line_phase)
    want_letters, want_start = spec.layout(reads)
    letters, read_start, got_reads, got_lines, got_bad = device_parse(data, fmt, line_phase, buf)
    assert (got_reads, got_lines, got_bad) == (len(reads), n_lines, n_bad)
    assert np.array_equal(read_start, want_start)
    assert np.array_equal(letters, want_letters)


def _parse_files():
    out = dict(cases.PARSE_CASES)
    out.update({"golden_" + name: data for name, data in cases.GOLDEN_CASES.items()})
    out.update({"fastq_" + name: data for name, (data, _) in cases.FASTQ_CASES.items()})
    out["fastq_bad_third_line"] = cases.BAD_THIRD_LINE
    out.update(cases.boundary_cases(T, S))
    return out


PARSE_FILES = _parse_files()


# ------------------------------------------------------------------ parse parity
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
@pytest.mark.parametrize("name", sorted(PARSE_FILES))
def test_parse_equals_spec(name, fmt):
    """Every file under both formats: the FASTQ rules are positional, so any bytes have an answer (and a count of the
    lines that are not where a record has them)."""
    assert_parse(PARSE_FILES[name], fmt)


def test_the_listed_cases_are_there():
    """The files the parse has to get right, by what is in them."""
    f = PARSE_FILES
    assert f["empty"] == b"" and f["one_letter"] == b"A" and f["one_newline"] == b"\n"
    assert [len(r) for r in spec.parse(f["lengths_k_km1_1"], "fasta")[0]] == [5, 4, 1, 31, 30]
    for name, at in (("newline_at_T_minus_1", T - 1), ("newline_at_T", T), ("newline_at_T_plus_1", T + 1)):
        assert f[name].index(b"\n") == at
    assert max(len(x) for x in f["line_of_2T_plus_3"].split(b"\n")) == 2 * T + 3
    assert b"\n" not in f["tile_without_newline"][T:2 * T]
    assert f["T_plus_3_newlines"] == b"\n" * (T + 3)
    for n in (S - 1, S, S + 1, 2 * S + 1):
        assert f["%d_lines_of_A" % n] == b"A\n" * n
    quality = [rec[3][:1] for rec in cases.FASTQ_CASES["tricky_quality"][1]]
    assert {b">", b"@", b"+"} <= set(quality)
    assert spec.parse(f["fastq_cut_after_second_line"], "fastq")[1] % 4 == 2


def test_fastq_record_shape_is_counted_and_raised(tmp_path):
    data = cases.BAD_THIRD_LINE
    assert device_parse(data, "fastq")[4] == 1
    assert device_parse(cases.FASTQ_CASES["tricky_quality"][0], "fastq")[4] == 0
    path = str(tmp_path / "bad.fq")
    with open(path, "wb") as fh:
        fh.write(data)
    index, _ = small_index(5, 0)
    for chunk_bytes in (16, 1 << 20):
        with pytest.raises(ValueError) as e:
            index.map_reads_file(path, 5, N_NODES, chunk_bytes=chunk_bytes)
        assert "bad.fq" in str(e.value) and " 1 " in str(e.value)


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
@pytest.mark.parametrize("offset", [1, 3, 16])
def test_parse_of_an_unaligned_device_buffer(fmt, offset):
    """A device buffer that does not begin on a 16-byte boundary takes the byte loads; the answer is the same."""
    for name in ("golden_stream", "newline_at_T", "T_plus_3_newlines_then_read", "fastq_tricky_quality"):
        data = PARSE_FILES[name]
        whole = _lib.DeviceArray.from_host(np.frombuffer(b"\n" * offset + data + b"\nACGT\n", dtype=np.uint8))
        assert_parse(data, fmt, buf=whole.view(offset, len(data)))
        whole.free()


def test_arguments_are_checked():
    buf = np.frombuffer(b">a\nACGT\n", dtype=np.uint8)
    with pytest.raises(ValueError):
        read_files.parse_reads_on_device(buf, "sam")
    with pytest.raises(_lib.GkiError):
        read_files.parse_reads_on_device(buf, "fastq", line_phase=4)
    d = _lib.DeviceArray.from_host(buf)
    small = _lib.DeviceArray(1, np.uint8)
    start = _lib.DeviceArray(2, np.int64)
    start.zero()
    with pytest.raises(_lib.GkiError):          # four letters do not fit one byte: refused, nothing written
        _lib.check(_lib.load().gki_reads_parse_emit(d.ptr, d.n, 0, 0, small.ptr, 1, start.ptr, 2))
    assert start.to_host().tolist() == [0, 0]
    with pytest.raises(_lib.GkiError):
        _lib.check(_lib.load().gki_reads_parse_emit(d.ptr, d.n, 0, 0, small.ptr, 4, start.ptr, 1))
    for a in (d, small, start):
        a.free()


# ------------------------------------------------------------------ phase carry
def test_fastq_phase_is_carried_across_any_cut():
    data = cases.FORTY_LINES
    want_letters, want_start = spec.layout(spec.parse(data, "fastq")[0])
    cuts = [i + 1 for i, c in enumerate(data) if c == 0x0A]
    assert len(cuts) == 40
    for cut in cuts:
        a = device_parse(data[:cut], "fastq", 0)
        phase = a[3] % 4
        b = device_parse(data[cut:], "fastq", phase)
        assert a[4] == 0 and b[4] == 0
        assert a[3] + b[3] == 40
        assert np.array_equal(np.concatenate([a[0], b[0]]), want_letters)
        assert np.array_equal(np.concatenate([a[1][:-1], a[1][-1] + b[1]]), want_start)


# ------------------------------------------------------------------ streaming
with gzip.open(os.path.join(ROOT, "tests", "golden", "read_files_reference.json.gz"), "rt") as _fh:
    GOLDEN = json.load(_fh)


def golden_queries(name, k, reverse):
    """Every recorded hash of the case's reads: the forward pass, then the reverse-complement pass."""
    e = GOLDEN[name][str(k)]
    keys = ("forward", "reverse") if reverse else ("forward",)
    flat = [h for key in keys for hashes in e[key] if hashes is not None for h in hashes]
    return np.array(flat, dtype=np.uint64)


_INDEXES = {}


def small_index(k, seed):
    """(CollisionFreeKmerIndex on the device, the same index from NumPy): every third recorded forward k-mer of every
    golden case and half of the short-read case's k-mers of both strands, some twice, on nodes below N_NODES."""
    if (k, seed) not in _INDEXES:
        rng = np.random.default_rng(100 + seed)
        pool = np.unique(np.concatenate([golden_queries(name, k, False)[::3] for name in sorted(cases.GOLDEN_CASES)]
                                        + [golden_queries("short_reads", k, True)[::2]]))
        kmers = np.concatenate([pool, pool[::4]])
        nodes = rng.integers(0, N_NODES, size=len(kmers)).astype(np.uint32)
        refs = rng.integers(0, 3, size=len(kmers)).astype(np.uint64)
        af = np.ones(len(kmers), np.float32)
        idx = CollisionFreeKmerIndex.from_flat_kmers(FlatKmers(kmers, nodes, refs, af), modulo=10007)
        ref = build_index_ref(kmers, nodes, refs, af, 10007)
        for key in INDEX_KEYS:
            assert np.array_equal(getattr(idx, key), ref[key]), key
        _INDEXES[(k, seed)] = idx, ref
    return _INDEXES[(k, seed)]


def write(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(data)
    return path


@pytest.mark.parametrize("reverse", [True, False])
@pytest.mark.parametrize("k", cases.GOLDEN_KS)
@pytest.mark.parametrize("name", ["stream", "short_reads", "crlf_no_final_newline", "blank_padded"])
def test_map_reads_file_streams_to_the_same_counts(tmp_path, name, k, reverse):
    data = cases.GOLDEN_CASES[name]
    path = write(tmp_path, name + ".fa", data)
    index, ref = small_index(k, 0)
    want, want_hits = count_nodes_ref(ref, golden_queries(name, k, reverse), MAX, N_NODES)
    assert want_hits > 0
    reads = spec.parse(data, "fasta")[0]
    assert max(len(line) for line in data.split(b"\n")) > 7                        # 7 bytes hold no whole line: pieces grow
    in_memory = index.map_reads(spec.layout(reads), k, N_NODES, include_reverse_complement=reverse)
    assert np.array_equal(in_memory.astype(np.int64), want)
    for chunk_bytes in (7, 64, T, len(data), None):
        got = index.map_reads_file(path, k, N_NODES, include_reverse_complement=reverse, chunk_bytes=chunk_bytes)
        assert got.dtype == np.uint32 and np.array_equal(got, in_memory), chunk_bytes
    counts, n_reads, n_kmers, n_hits = read_files.count_nodes_from_file(index._device_index(), path, k, N_NODES,
                                                                       strands=3 if reverse else 1, chunk_bytes=64)
    counts.free()
    assert (n_reads, n_hits) == (len(reads), want_hits)
    assert n_kmers == sum(max(len(r) - k + 1, 0) for r in reads) * (2 if reverse else 1)


@pytest.mark.parametrize("k", cases.GOLDEN_KS)
def test_fastq_file_equals_its_fasta_rewriting(tmp_path, k):
    index, _ = small_index(k, 0)
    reads = spec.parse(cases.GOLDEN_CASES["stream"], "fasta")[0]
    records = [(b"@r%d" % i, r, b"+", bytes([62 + (i + j) % 3 for j in range(len(r))])) for i, r in enumerate(reads)]
    fq = write(tmp_path, "stream.fq", cases.fastq_of(records))
    want = index.map_reads(spec.layout(reads), k, N_NODES)
    assert want.sum() > 0
    for chunk_bytes in (7, 64, T, None):
        assert np.array_equal(index.map_reads_file(fq, k, N_NODES, chunk_bytes=chunk_bytes), want), chunk_bytes
    # the format is the file's first byte unless it is given; n_nodes defaults to the index's
    assert np.array_equal(index.map_reads_file(fq, k, fmt="fastq"), want[:int(index.max_node_id()) + 1])
    bare = cases.GOLDEN_CASES["no_headers"]                               # begins with a letter: only a given format reads it
    path = write(tmp_path, "no_headers.txt", bare)
    with pytest.raises(ValueError):
        index.map_reads_file(path, k, N_NODES)
    assert np.array_equal(index.map_reads_file(path, k, N_NODES, fmt="fasta"),
                          index.map_reads(spec.layout(spec.parse(bare, "fasta")[0]), k, N_NODES))
    empty = write(tmp_path, "empty.fa", b"")
    assert not index.map_reads_file(empty, k, N_NODES).any()
    with pytest.raises(ValueError):
        index.map_reads_file(write(tmp_path, "neither.txt", b"ACGT\n"), k, N_NODES)


# ------------------------------------------------------------------ other surfaces
@pytest.mark.parametrize("suffix,fmt", [(".fa.gz", "fasta"), (".fq.gz", "fastq")])
def test_gz_file_gives_the_same_counts(tmp_path, suffix, fmt):
    k = 31
    index, _ = small_index(k, 0)
    data = cases.GOLDEN_CASES["stream"]
    if fmt == "fastq":
        data = cases.fastq_of([(b"@r", r, b"+", b"I" * len(r)) for r in spec.parse(data, "fasta")[0]])
    plain = write(tmp_path, "reads" + suffix[:3], data)
    packed = write(tmp_path, "reads" + suffix, gzip.compress(data))
    want = index.map_reads_file(plain, k, N_NODES)
    assert want.sum() > 0
    for chunk_bytes in (64, None):
        assert np.array_equal(index.map_reads_file(packed, k, N_NODES, chunk_bytes=chunk_bytes), want)


def test_counter_index_counts_files_and_accumulates(tmp_path):
    k = 31
    index, _ = small_index(k, 0)
    first = write(tmp_path, "first.fa", cases.GOLDEN_CASES["stream"])
    second = write(tmp_path, "second.fa", cases.GOLDEN_CASES["short_reads"])
    h1, h2 = golden_queries("stream", k, True), golden_queries("short_reads", k, True)
    from_files, from_hashes = CounterKmerIndex.from_kmer_index(index), CounterKmerIndex.from_kmer_index(index)
    from_files.count_reads_file(first, k)
    from_hashes.count_kmers(h1)
    assert from_hashes.get_node_counts().sum() > 0
    assert np.array_equal(from_files.get_node_counts(), from_hashes.get_node_counts())
    from_files.count_reads_file(second, k)
    from_hashes.count_kmers(h2)
    assert np.array_equal(from_files.get_node_counts(), from_hashes.get_node_counts())
    from_files.count_reads_file(second, k, update_counter=False)          # starts again from zero
    from_hashes.count_kmers(h2, update_counter=False)
    assert np.array_equal(from_files.get_node_counts(), from_hashes.get_node_counts())
    # an index made from bare arrays builds its own table
    bare = CounterKmerIndex(np.asarray(index._kmers).astype(np.int64), index._nodes, modulo=10007)
    bare.count_reads_file(second, k)
    assert np.array_equal(bare.get_node_counts(), from_hashes.get_node_counts())


def test_map_command_writes_the_counts(tmp_path):
    k = 5
    index, _ = small_index(k, 0)
    index.to_file(str(tmp_path / "index"))
    reads = write(tmp_path, "reads.fa", cases.GOLDEN_CASES["stream"])
    out = str(tmp_path / "counts")
    assert main(["map", "-i", str(tmp_path / "index"), "-f", reads, "-k", str(k), "-o", out, "-c", "64", "-t", "4"]) == 0
    got = np.load(out + ".npy")
    want = CollisionFreeKmerIndex.from_file(str(tmp_path / "index")).map_reads_file(reads, k)
    assert got.dtype == np.uint32 and got.sum() > 0 and np.array_equal(got, want)
    assert main(["map", "-i", str(tmp_path / "index"), "-f", reads, "-k", str(k), "-o", out + "_fwd.npy", "-r", "False",
                 "-n", str(N_NODES), "-F", "fasta"]) == 0
    assert np.array_equal(np.load(out + "_fwd.npy"), index.map_reads_file(reads, k, N_NODES, include_reverse_complement=False))
