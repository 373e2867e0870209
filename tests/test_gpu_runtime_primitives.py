"""-m gpu: the device primitives every feature shares, each called alone through the C ABI and compared exactly with a
NumPy reference from tests/primitive_cases.py (np.cumsum in int64, boolean indexing, np.add.reduce / np.bitwise_xor.reduce,
np.flatnonzero) or, for the hashes, with the oracle:

  the exclusive scans        gki_exclusive_scan (a checking aid over gki_scan_*), and gki_hash_reads in count-only mode
  the stable compaction      gki_compact_flat and DeviceFlatKmers.compacted
  the column checksum        gki_column_checksum, the instrument bench.py and the full-size tests compare outputs with
  the last-byte search       gki_last_byte_position, and the file route that cuts its pieces with it
  hashes past one grid       gki_reverse_complement, gki_complement, gki_hash_sequence

The shapes stand at the seams of the kernels: the scan's levels (2048 and 2048^2 items), its 16-byte loads and stores
(pointer alignment), the 524 288 threads of one grid, the search's windows (1 MiB, then four times as much).  Inputs
carry garbage behind their end and outputs a sentinel, so a read or a store past the end shows.  Every pointer handed
to the library lies inside an allocation of the test; refusals are checked by return code.

Not tested: gki_compact_flat cuts its input into chunks of 2^27 records (csrc/gki_runtime.hip:216); a case across that
seam needs 3 GB of host arrays and stays out."""
import ctypes as C

import numpy as np
import pytest

import primitive_cases as cases
from graph_kmer_index_amd import DeviceFlatKmers, _lib, bgzf
from graph_kmer_index_amd._lib import DeviceArray
from oracle import oracle

pytestmark = pytest.mark.gpu

OK, BAD_ARG = 0, 2           # include/gki.h GKI_OK, GKI_ERR_BAD_ARG


def lib():
    return _lib.load()


# ------------------------------------------------------------------ scans
def run_scan(kind, values, in_offset=0, out_offset=0):
    """gki_exclusive_scan of `values` laid at element `in_offset` of a buffer of 0xFFFFFFFF, into element `out_offset` of
    a buffer of sentinels: the n + 1 results, after checking that nothing else of the output was written."""
    n = len(values)
    out_dtype = cases.SCAN_KINDS[kind][1]
    sentinel = cases.scan_sentinel(kind)
    with _lib.DeviceScope() as s:
        d_in = s.keep(DeviceArray.from_host(cases.in_guarded(values, in_offset, values.dtype.type(-1) if kind == 1
                                                             else cases.U32_MAX)))
        d_out = s.keep(DeviceArray.from_host(np.full(out_offset + n + 1 + cases.GUARD, sentinel, out_dtype)))
        rc = lib().gki_exclusive_scan(d_in.view(in_offset, n).ptr, n, kind, d_out.view(out_offset, n + 1).ptr)
        assert rc == OK, lib().gki_last_error()
        out = d_out.to_host()
    assert (out[:out_offset] == sentinel).all(), "stores before the output"
    assert (out[out_offset + n + 1:] == sentinel).all(), "stores behind out[n]"
    return out[out_offset:out_offset + n + 1]


def assert_scan(kind, values, in_offset=0, out_offset=0):
    got = run_scan(kind, values, in_offset, out_offset)
    want = cases.scan_ref(kind, values)
    assert got[-1] == want[-1], "total"
    assert np.array_equal(got, want)


@pytest.mark.parametrize("kind,n,name", cases.scan_cases())
def test_scan_equals_cumsum(kind, n, name):
    assert_scan(kind, cases.scan_values(kind, n, name))


@pytest.mark.parametrize("n", cases.SCAN_ALIGN_NS)
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_scan_at_every_pointer_alignment(kind, n):
    """load_items takes its 16-byte loads, and k_block_scan its 16-byte stores, only on an aligned address: input at
    0, 4, 8, 12 bytes past an aligned one, output at 0 and at one element past."""
    values = cases.scan_values(kind, n, cases.SCAN_VALUES[kind][0][0], seed=1)
    for in_offset in cases.SCAN_IN_OFFSETS:
        for out_offset in cases.SCAN_OUT_OFFSETS:
            assert_scan(kind, values, in_offset, out_offset)


def test_scan_refuses_what_it_cannot_do():
    with _lib.DeviceScope() as s:
        d_in = s.keep(DeviceArray.from_host(np.ones(4, np.uint32)))
        d_out = s.keep(DeviceArray.from_host(np.full(5, 77, np.int64)))
        for kind, n in ((3, 4), (-1, 4), (0, -1), (2, -5)):
            assert lib().gki_exclusive_scan(d_in.ptr, n, kind, d_out.ptr) == BAD_ARG
        assert d_out.to_host().tolist() == [77] * 5


def count_reads(read_start, k, n_guard=cases.GUARD):
    """gki_hash_reads in count-only mode (d_out NULL; d_reads one byte that is never read): (code, n_out, out_start)."""
    read_start = np.asarray(read_start, np.int64)
    n_reads = len(read_start) - 1
    n_out = C.c_int64(-1)
    with _lib.DeviceScope() as s:
        d_reads = s.array(1, np.uint8)
        d_start = s.keep(DeviceArray.from_host(read_start))
        d_out_start = s.keep(DeviceArray.from_host(np.full(n_reads + 1 + n_guard, -3, np.int64)))
        rc = lib().gki_hash_reads(d_reads.ptr, d_start.ptr, n_reads, k, 0, d_out_start.ptr, None, 0, C.byref(n_out))
        out = d_out_start.to_host()
    assert (out[n_reads + 1:] == -3).all()
    return rc, n_out.value, out[:n_reads + 1]


def test_read_counts_are_scanned_across_three_levels():
    k = cases.K_READS
    read_start = cases.many_short_reads(cases.STILE ** 2 + 1)
    want = cases.scan_ref(0, cases.read_counts_ref(read_start, k).astype(np.uint32))
    rc, n_out, out_start = count_reads(read_start, k)
    assert rc == OK and n_out == want[-1] > 0
    assert np.array_equal(out_start, want)


@pytest.mark.parametrize("name", sorted(cases.HUGE_READS))
def test_reads_of_2_to_the_31_letters_and_more(name):
    """A read's k-mer count is kept in 32 bits, the running total in 64: totals pass 2^32, the largest count that fits is
    exact, and a read with more k-mers is refused instead of counted modulo 2^32 (k = 31: 2^32 + 30 letters were 0
    k-mers, 2^32 + 35 were 5)."""
    read_start, accepted = cases.HUGE_READS[name]
    rc, n_out, out_start = count_reads(read_start, cases.K_READS)
    if accepted:
        want = cases.scan_ref(0, cases.read_counts_ref(read_start, cases.K_READS).astype(np.uint32))
        assert rc == OK and n_out == want[-1]
        assert np.array_equal(out_start, want)
    else:
        assert (rc, n_out) == (BAD_ARG, 0)


# ------------------------------------------------------------------ compaction
@pytest.fixture(scope="module")
def device_columns():
    """n -> the four columns of cases.flat_columns(n) on the device, uploaded once."""
    made = {}

    def get(n):
        if n not in made:
            made[n] = DeviceFlatKmers(n, *[DeviceArray.from_host(c) for c in cases.flat_columns(n)])
        return made[n]
    yield get
    for d in made.values():
        for a in (d.hashes, d.nodes, d.ref_offsets, d.allele_frequencies):
            a.free()


def compact(dev, d_flags, capacity, n_alloc, fetch=True):
    """gki_compact_flat into sentinel-filled columns of n_alloc records: (code, n_out, the four whole columns)."""
    n_out = C.c_int64(-1)
    with _lib.DeviceScope() as s:
        outs = [s.keep(DeviceArray.from_host(np.full(n_alloc, v, v.dtype))) for v in cases.COLUMN_SENTINELS]
        rc = lib().gki_compact_flat(d_flags.ptr, dev.n, dev.hashes.ptr, dev.nodes.ptr, dev.ref_offsets.ptr,
                                    dev.allele_frequencies.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr,
                                    capacity, C.byref(n_out))
        return rc, n_out.value, [o.to_host() for o in outs] if fetch else None


@pytest.mark.parametrize("name", cases.COMPACT_FLAGS)
@pytest.mark.parametrize("n", cases.COMPACT_NS)
def test_compaction_equals_boolean_indexing(device_columns, n, name):
    dev = device_columns(n)
    flags = cases.compact_flags(n, name)
    want = cases.compact_ref(flags, cases.flat_columns(n))
    kept = len(want[0])
    with _lib.DeviceScope() as s:
        d_flags = s.keep(DeviceArray.from_host(flags))
        # a capacity of exactly the kept count is enough, and nothing is written behind it
        rc, n_out, got = compact(dev, d_flags, kept, kept + cases.GUARD)
        assert (rc, n_out) == (OK, kept)
        for g, w, sentinel in zip(got, want, cases.COLUMN_SENTINELS):
            assert np.array_equal(g[:kept].view(np.uint8), w.view(np.uint8))
            assert (g[kept:].view(np.uint8) == np.full(cases.GUARD, sentinel).view(np.uint8)).all()
        if kept:                                                       # one less is refused
            rc, n_out, _ = compact(dev, d_flags, kept - 1, kept + cases.GUARD, fetch=False)
            assert (rc, n_out) == (BAD_ARG, 0)
        # the Python layer sizes its output by the 1-byte checksum of 0 / 1 flags
        d_01 = s.keep(DeviceArray.from_host((flags != 0).astype(np.uint8)))
        assert d_01.checksum()[0] == kept
        out = dev.compacted(d_01)
        s.keep(out.hashes), s.keep(out.nodes), s.keep(out.ref_offsets), s.keep(out.allele_frequencies)
        assert out.n == kept
        for g, w in zip((out.hashes, out.nodes, out.ref_offsets, out.allele_frequencies), want):
            assert np.array_equal(g.to_host(kept).view(np.uint8), w.view(np.uint8))


# ------------------------------------------------------------------ checksum
@pytest.mark.parametrize("n", cases.CHECKSUM_NS)
@pytest.mark.parametrize("elem_bytes", sorted(cases.CHECKSUM_DTYPES))
def test_checksum_equals_numpy(elem_bytes, n):
    """n elements at element offsets 0, 1 and 3 of a longer buffer: what lies behind them does not count."""
    values = cases.checksum_values(elem_bytes, n)
    d = DeviceArray.from_host(values)
    try:
        for offset in cases.CHECKSUM_OFFSETS:
            assert d.view(offset, n).checksum() == cases.checksum_ref(values[offset:offset + n]), offset
        assert d.checksum(n) == cases.checksum_ref(values[:n])
    finally:
        d.free()


def test_checksum_refuses_other_widths():
    d = DeviceArray.from_host(np.arange(12, dtype=np.uint8))
    s, x = C.c_uint64(5), C.c_uint64(5)
    try:
        for elem_bytes in (3, 0, 16, -1):
            assert lib().gki_column_checksum(d.ptr, 4, elem_bytes, C.byref(s), C.byref(x)) == BAD_ARG
        assert lib().gki_column_checksum(d.ptr, 12, 1, C.byref(s), C.byref(x)) == OK and (s.value, x.value) == (66, 0)
    finally:
        d.free()


# ------------------------------------------------------------------ last byte
def last_position(d_bytes, n, value):
    pos = C.c_int64(-7)
    rc = lib().gki_last_byte_position(d_bytes.ptr, n, value, C.byref(pos))
    return rc, pos.value


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("value", cases.SEARCH_VALUES)
@pytest.mark.parametrize("n", cases.SEARCH_NS)
def test_last_byte_position_in_every_window(n, value, offset):
    """The byte at the ends, at the seam of the first window, and only in the second or third window, in a buffer (or a
    view one byte into it) that holds the byte nowhere else -- except right before and behind the searched range."""
    host = np.concatenate([np.full(offset, value, np.uint8), cases.search_background(n),
                           np.full(cases.GUARD, value, np.uint8)])
    whole = DeviceArray.from_host(host)
    searched = whole.view(offset, n)
    one = np.array([value], np.uint8)
    try:
        for name, positions in cases.search_placements(n).items():
            for p in positions:                                        # poke the byte in, on both sides
                _lib.check(lib().gki_memcpy_h2d(searched.ptr.value + p, _lib.hptr(one), 1))
            saved = host[offset:offset + n][list(positions)].copy()
            host[offset:offset + n][list(positions)] = value
            want = cases.search_ref(host[offset:offset + n], value)
            assert want == (max(positions) if positions else -1)
            assert last_position(searched, n, value) == (OK, want), name
            host[offset:offset + n][list(positions)] = saved           # and take it out again
            for p, b in zip(positions, saved):
                _lib.check(lib().gki_memcpy_h2d(searched.ptr.value + p, _lib.hptr(np.array([b], np.uint8)), 1))
        assert last_position(searched, n, value) == (OK, -1)
    finally:
        whole.free()


def test_last_byte_position_refuses_bad_arguments():
    d = DeviceArray.from_host(np.full(8, 10, np.uint8))
    try:
        assert last_position(d, 8, 256) == (BAD_ARG, -1)
        assert last_position(d, 8, -1) == (BAD_ARG, -1)
        assert last_position(d, -1, 10) == (BAD_ARG, -1)
        assert last_position(d, 8, 10) == (OK, 7)
    finally:
        d.free()


def test_file_whose_last_line_outgrows_the_first_window(tmp_path):
    """Streamed in pieces of 64 KiB, the last read's single line of 1.2 M letters is carried on the device as an
    unfinished tail, and the cut of every later piece finds its line end beyond the first MiB from the end."""
    from test_gpu_read_files import N_NODES, small_index
    k = 5
    index, _ = small_index(k, 0)
    text = cases.long_last_line_fasta()
    plain, packed = str(tmp_path / "reads.fa"), str(tmp_path / "reads.fa.gz")
    with open(plain, "wb") as fh:
        fh.write(text)
    bgzf.write_bgzf(packed, text)
    want = index.map_reads_file(plain, k, N_NODES)
    assert want.sum() > 0
    assert np.array_equal(index.map_reads_file(plain, k, N_NODES, chunk_bytes=65536), want)
    assert np.array_equal(index.map_reads_file(packed, k, N_NODES, chunk_bytes=65536), want)
    assert np.array_equal(index.map_reads_file(packed, k, N_NODES, chunk_bytes=65536, inflate="device"), want)
    assert np.array_equal(index.map_reads_file(packed, k, N_NODES, chunk_bytes=65536, inflate="host"), want)


# ------------------------------------------------------------------ hash helpers past one grid
@pytest.mark.parametrize("k", cases.COMPLEMENT_KS)
@pytest.mark.parametrize("n", cases.COMPLEMENT_NS)
def test_complements_past_one_grid(n, k):
    hashes = cases.random_hashes(n, seed=k)
    with _lib.DeviceScope() as s:
        d_in = s.keep(DeviceArray.from_host(hashes))
        for fn, ref in ((lib().gki_reverse_complement, oracle.reverse_complement), (lib().gki_complement, oracle.complement)):
            d_out = s.keep(DeviceArray.from_host(np.full(n + cases.GUARD, 0x1234567812345678, np.uint64)))
            assert fn(d_in.ptr, n, k, d_out.ptr) == OK
            got = d_out.to_host()
            masked = hashes & np.uint64((1 << (2 * k)) - 1)          # the kernels mask to 2k bits; the reference takes k-mers
            assert np.array_equal(got[:n], ref(masked, k))
            assert (got[n:] == 0x1234567812345678).all()
            d_out.free()


def assert_hash_sequence(codes_buffer, byte_offset, n, k):
    """gki_hash_sequence of the n codes at `byte_offset` of the buffer against the oracle's."""
    n_out = max(n - k + 1, 0)
    with _lib.DeviceScope() as s:
        d_codes = s.keep(DeviceArray.from_host(codes_buffer))
        d_out = s.keep(DeviceArray.from_host(np.full(n_out + cases.GUARD, 0x1234567812345678, np.uint64)))
        assert lib().gki_hash_sequence(d_codes.view(byte_offset, n).ptr, n, k, d_out.ptr) == OK
        got = d_out.to_host()
    assert np.array_equal(got[:n_out], oracle.hash_sequence(codes_buffer[byte_offset:byte_offset + n], k))
    assert (got[n_out:] == 0x1234567812345678).all()


@pytest.mark.parametrize("n", cases.HASH_SEQUENCE_NS)
def test_hash_sequence_past_one_grid_of_packed_words(n):
    """k_pack_2bit packs 16 bases per lane: 8 388 608 bases fill one grid, the next ones take the second trip; a last
    word of 1, 15 and 16 + 1 bases takes the byte loads."""
    assert_hash_sequence(cases.random_codes(n + cases.GUARD), 0, n, cases.HASH_K)


@pytest.mark.parametrize("byte_offset", cases.HASH_VIEW_BYTE_OFFSETS)
def test_hash_sequence_of_an_unaligned_pointer(byte_offset):
    """k_pack_2bit takes its 16-byte loads only when the sequence begins on a 16-byte boundary."""
    n = cases.HASH_VIEW_N
    assert_hash_sequence(cases.random_codes(byte_offset + n + cases.GUARD, seed=byte_offset), byte_offset, n, cases.HASH_K)
