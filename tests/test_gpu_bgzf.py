"""-m gpu: BGZF members inflated on the device (csrc/gki_inflate.hip, graph_kmer_index_amd/bgzf.py) against the data zlib
compressed, byte for byte, and the .gz route of the reads-file surfaces -- map_reads_file, CounterKmerIndex.count_reads_file,
the `map` sub-command -- against the plain-file route and the in-memory route.  Every comparison is exact.

Malformed input is the business of tests/test_inflate_core_cpu.py; five of its vectors come here, each in one file that
is inflated directly and mapped once, to see the error reach both callers with the right block while the other blocks
are still written.  No loop over corrupt input and no fuzz runs on the device."""
import gzip

import numpy as np
import pytest

import bgzf_cases as cases
import read_file_cases as text_cases
import spec_read_files as spec
from graph_kmer_index_amd import CollisionFreeKmerIndex, CounterKmerIndex, _lib, bgzf, read_files
from graph_kmer_index_amd.command_line_interface import main
from test_gpu_read_files import N_NODES, small_index, write

pytestmark = pytest.mark.gpu

K = 31


def inflate(members, prefix=0):
    raw = cases.file_bytes(members)
    scanned, left = bgzf.scan_all(raw)
    assert left == 0 and len(scanned) == len(members)
    out = bgzf.inflate_on_device(raw, scanned, prefix)
    got = out.to_host()
    out.free()
    return got.tobytes()


# ------------------------------------------------------------------ inflate parity
@pytest.mark.parametrize("name", sorted(cases.GOOD))
def test_good_vectors_inflate_to_what_zlib_compressed(name):
    members = cases.GOOD[name]
    assert inflate(members) == b"".join(m[3] for m in members)


_MIXED = {}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1025])
def test_files_of_many_members(n):
    members = _MIXED.setdefault(n, cases.mixed_members(n, 40 + n))
    want = b"".join(m[3] for m in members)
    assert {0, 0xff00} <= {m[2] for m in members} or n < 6
    assert inflate(members) == want
    got = inflate(members, prefix=37)                    # the output begins at an odd address; the prefix is the caller's
    assert len(got) == 37 + len(want) and got[37:] == want


def test_a_device_buffer_and_no_members():
    members = cases.GOOD["odd_starts"]
    raw = cases.file_bytes(members)
    d = _lib.DeviceArray.from_host(np.frombuffer(raw, dtype=np.uint8))
    out = bgzf.inflate_on_device(d, bgzf.scan_all(raw)[0])
    assert out.to_host().tobytes() == b"".join(m[3] for m in members)
    import ctypes as C
    ms = C.c_float(-1)
    assert _lib.load().gki_bgzf_inflate_kernel_ms(C.byref(ms)) == 0 and 0 < ms.value < 1000    # the kernel of that call
    out.free()
    d.free()
    none = bgzf.inflate_on_device(b"", [], prefix=5)
    assert none.n == 5
    none.free()


def test_entry_validates_before_it_inflates():
    raw = cases.file_bytes(cases.GOOD["fixed"])
    (start, length, crc, isize, _), = bgzf.scan_all(raw)[0]
    with pytest.raises(_lib.GkiError) as e:
        bgzf.inflate_on_device(raw, [(start, len(raw), crc, isize)])            # a payload that runs past the input
    assert e.value.code == 2
    with pytest.raises(ValueError):
        bgzf.inflate_on_device(raw, [(start, length, crc, 65537)])
    d = _lib.DeviceArray.from_host(np.frombuffer(raw, dtype=np.uint8))
    cols = [_lib.DeviceArray.from_host(np.array(a, dtype=t)) for a, t in (([start], np.int64), ([length], np.int32),
                                                                         ([crc], np.uint32), ([0, isize], np.int64))]
    out = _lib.DeviceArray(isize, np.uint8)
    import ctypes as C
    bad, status = C.c_int64(0), C.c_int(0)
    args = (d.ptr, len(raw), cols[0].ptr, cols[1].ptr, cols[2].ptr, cols[3].ptr, 1, out.ptr)
    assert _lib.load().gki_bgzf_inflate(*args, isize - 1, C.byref(bad), C.byref(status)) == 2   # capacity too small
    assert _lib.load().gki_bgzf_inflate(*args, isize, C.byref(bad), C.byref(status)) == 0
    assert (bad.value, status.value) == (-1, 0) and out.to_host().tobytes() == cases.GOOD["fixed"][0][3]
    for a in cols + [d, out]:
        a.free()


@pytest.mark.parametrize("name", cases.GPU_MALFORMED)
def test_a_malformed_member_is_named_and_the_others_are_written(name, tmp_path):
    bad, status = cases.MALFORMED[name]
    before, after = cases.GOOD["fastq"][0], cases.GOOD["fixed"][0]
    members = [before, bad, after, cases.EMPTY]
    raw = cases.file_bytes(members)
    with pytest.raises(bgzf.BgzfInflateError) as e:
        bgzf.inflate_on_device(raw, bgzf.scan_all(raw)[0])
    err = e.value
    got = err.output.to_host().tobytes()
    err.output.free()
    assert err.block == 1 and err.status == status
    assert got[:before[2]] == before[3] and got[before[2] + bad[2]:] == after[3]
    path = write(tmp_path, "bad.fq.gz", raw)
    index, _ = small_index(K, 0)
    with pytest.raises(ValueError) as e:
        index.map_reads_file(path, K, N_NODES)
    assert "bad.fq.gz: BGZF block at offset %d: " % len(cases.member_bytes(before)) in str(e.value)


# ------------------------------------------------------------------ the file routes
def fastq_of_stream():
    reads = spec.parse(text_cases.GOLDEN_CASES["stream"], "fasta")[0]
    return text_cases.fastq_of([(b"@r%d" % i, r, b"+", bytes([62 + (i + j) % 3 for j in range(len(r))]))
                                for i, r in enumerate(reads)])


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
@pytest.mark.parametrize("block_size", [100, 0xff00])
def test_map_reads_file_of_a_bgzf_file(tmp_path, fmt, block_size):
    index, _ = small_index(K, 0)
    data = text_cases.GOLDEN_CASES["stream"] if fmt == "fasta" else fastq_of_stream()
    assert max(len(line) for line in data.split(b"\n")) < block_size or block_size == 100
    plain = write(tmp_path, "reads.f" + fmt[-1], data)
    packed = str(tmp_path / ("reads.%s.gz" % fmt))
    bgzf.write_bgzf(packed, data, block_size)
    assert read_files.reads_file_route(packed) == "bgzf-device"
    want = index.map_reads_file(plain, K, N_NODES)
    assert want.sum() > 0
    assert np.array_equal(index.map_reads(spec.layout(spec.parse(data, fmt)[0]), K, N_NODES), want)
    for chunk_bytes in (1, 64, 4096, None):
        got = index.map_reads_file(packed, K, N_NODES, chunk_bytes=chunk_bytes)
        assert got.dtype == np.uint32 and np.array_equal(got, want), chunk_bytes
    assert np.array_equal(index.map_reads_file(packed, K, N_NODES, inflate="host"), want)
    counts, n_reads, n_kmers, n_hits = read_files.count_nodes_from_file(index._device_index(), packed, K, N_NODES, chunk_bytes=64)
    counts.free()
    reads = spec.parse(data, fmt)[0]
    assert (n_reads, n_hits) == (len(reads), int(want.sum())) and n_kmers == 2 * sum(max(len(r) - K + 1, 0) for r in reads)


def test_line_ends_members_and_the_end_of_the_file(tmp_path):
    index, _ = small_index(K, 0)
    stream = text_cases.GOLDEN_CASES["stream"]
    long_line = b">long\n" + stream.replace(b"\n", b"").replace(b">", b"A")[:1500] + b"\n" + stream[:600]
    files = {"crlf_no_final_newline": text_cases.GOLDEN_CASES["crlf_no_final_newline"],
             "no_final_newline": stream.rstrip(b"\n"), "long_line": long_line, "empty": b""}
    for name, data in files.items():
        plain = write(tmp_path, name + ".fa", data)
        want = index.map_reads_file(plain, K, N_NODES)
        packed = str(tmp_path / (name + ".fa.gz"))
        bgzf.write_bgzf(packed, data, 100)
        for chunk_bytes in (1, 300, None):
            assert np.array_equal(index.map_reads_file(packed, K, N_NODES, chunk_bytes=chunk_bytes), want), (name, chunk_bytes)
    assert index.map_reads_file(str(tmp_path / "long_line.fa"), K, N_NODES).sum() > 0
    # an empty member in the middle of a line, and the file's end without the empty member
    a, b = stream[:1003], stream[1003:]
    raw = cases.file_bytes([cases.member(a), cases.EMPTY, cases.EMPTY, cases.member(b, level=9)])
    path = write(tmp_path, "hole.fa.gz", raw)
    want = index.map_reads_file(write(tmp_path, "hole.fa", stream), K, N_NODES)
    for chunk_bytes in (1, None):
        assert np.array_equal(index.map_reads_file(path, K, N_NODES, chunk_bytes=chunk_bytes), want)


def test_fastq_phase_is_carried_across_every_piece_cut(tmp_path):
    index, _ = small_index(K, 0)
    lines = fastq_of_stream().split(b"\n")[:40]
    data = b"\n".join(lines) + b"\n"
    want = index.map_reads_file(write(tmp_path, "forty.fq", data), K, N_NODES)
    assert want.sum() > 0
    cuts = [i + 1 for i, c in enumerate(data) if c == 0x0A]
    assert len(cuts) == 40
    for cut in cuts:
        raw = cases.file_bytes([cases.member(data[:cut]), cases.member(data[cut:]), cases.EMPTY])
        path = write(tmp_path, "forty.fq.gz", raw)
        assert np.array_equal(index.map_reads_file(path, K, N_NODES, chunk_bytes=1), want), cut     # one member per piece


def test_counter_index_counts_a_bgzf_file(tmp_path):
    index, _ = small_index(K, 0)
    data = text_cases.GOLDEN_CASES["stream"]
    plain = write(tmp_path, "reads.fa", data)
    packed = str(tmp_path / "reads.fa.gz")
    bgzf.write_bgzf(packed, data, 700)
    a, b = CounterKmerIndex.from_kmer_index(index), CounterKmerIndex.from_kmer_index(index)
    a.count_reads_file(plain, K)
    b.count_reads_file(packed, K)
    assert a.get_node_counts().sum() > 0 and np.array_equal(a.get_node_counts(), b.get_node_counts())


def test_map_command_inflate_option(tmp_path):
    index, _ = small_index(K, 0)
    index.to_file(str(tmp_path / "index"))
    data = fastq_of_stream()
    want = index.map_reads_file(write(tmp_path, "reads.fq", data), K)
    blocked, single = str(tmp_path / "blocked.fq.gz"), write(tmp_path, "single.fq.gz", gzip.compress(data))
    bgzf.write_bgzf(blocked, data, 900)
    base = ["map", "-i", str(tmp_path / "index"), "-k", str(K), "-c", "2000"]
    for i, (path, choice) in enumerate(((blocked, "auto"), (blocked, "host"), (blocked, "device"), (single, "auto"),
                                        (single, "host"))):
        out = str(tmp_path / ("counts%d.npy" % i))
        assert main(base + ["-f", path, "-o", out, "--inflate", choice]) == 0
        assert np.array_equal(np.load(out), want), (path, choice)
    with pytest.raises(ValueError) as e:
        main(base + ["-f", single, "-o", str(tmp_path / "no.npy"), "--inflate", "device"])
    assert "not a BGZF file" in str(e.value)
    assert read_files.reads_file_route(single) == "gzip-host"


def test_a_misplaced_fastq_record_still_raises(tmp_path):
    index, _ = small_index(5, 0)
    packed = str(tmp_path / "bad.fq.gz")
    bgzf.write_bgzf(packed, text_cases.BAD_THIRD_LINE, 100)
    for chunk_bytes in (1, 1 << 20):
        with pytest.raises(ValueError) as e:
            index.map_reads_file(packed, 5, N_NODES, chunk_bytes=chunk_bytes)
        assert "bad.fq.gz" in str(e.value) and "four-line FASTQ" in str(e.value)
