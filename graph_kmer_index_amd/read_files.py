"""Reads files on the device: FASTA / FASTQ text -> node counts, without a host pass over the lines.

The raw bytes of a file go to HBM in chunks that end at a line end; gki_reads_parse_count / _emit (csrc/gki_reads_parse.hip)
find the lines, pick the sequence lines, strip them and lay them out as (uint8 letters, int64 read_start), which
`DeviceIndex.count_nodes_from_reads` (gki_probe_reads_count_nodes) consumes unchanged.  The rules -- what a line, a header,
a read and a malformed FASTQ record are -- are stated in include/gki.h ("reads files") and DESIGN.md 4.12.

A name ending in .gz is read through Python's gzip module: that route is bound by the host's inflate, not by the device.
"""
import ctypes as C
import gzip
import numpy as np

from . import _lib

FORMATS = {"fasta": 0, "fastq": 1}            # GKI_READS_FASTA, GKI_READS_FASTQ
DEFAULT_CHUNK_BYTES = 256 << 20


def detect_format(first_bytes):
    """'fasta' or 'fastq' from the first byte of a file: '>' / '@'; an empty file is FASTA with no reads."""
    head = bytes(first_bytes[:1])
    if head == b"" or head == b">":
        return "fasta"
    if head == b"@":
        return "fastq"
    raise ValueError("cannot tell FASTA from FASTQ: the file begins with %r, not '>' or '@'" % head)


def open_reads_file(file_name):
    return gzip.open(file_name, "rb") if str(file_name).endswith(".gz") else open(file_name, "rb")


def _read_fully(f, n):
    """n bytes of f, fewer only at its end (a raw or compressed stream may answer a read in pieces)."""
    parts, got = [], 0
    while got < n:
        b = f.read(n - got)
        if not b:
            break
        parts.append(b)
        got += len(b)
    return parts[0] if len(parts) == 1 else b"".join(parts)


def iter_line_chunks(f, chunk_bytes):
    """The stream as pieces that end at a line end.  Every step reads `chunk_bytes` new bytes behind what the last piece
    left over, cuts after the last '\\n' and carries the rest; a piece without any '\\n' that is not the stream's end
    grows by doubling until it has one.  The end of the stream is a piece of its own, terminated or not."""
    chunk_bytes = int(chunk_bytes)
    if chunk_bytes < 1:
        raise ValueError("chunk_bytes must be at least 1")
    tail = b""
    while True:
        new = _read_fully(f, chunk_bytes)
        at_end = len(new) < chunk_bytes
        buf = tail + new if tail else new
        cut = buf.rfind(b"\n") + 1
        while cut == 0 and not at_end:
            new = _read_fully(f, len(buf))
            at_end = len(new) < len(buf)
            buf += new
            cut = buf.rfind(b"\n") + 1
        if at_end:
            if buf:
                yield buf
            return
        yield buf[:cut]
        tail = buf[cut:]


def _format_code(fmt):
    if fmt not in FORMATS:
        raise ValueError("fmt must be 'fasta' or 'fastq', not %r" % (fmt,))
    return FORMATS[fmt]


def _device_bytes(buf):
    """(DeviceArray of the bytes, number of bytes, whether this call owns it)."""
    if isinstance(buf, _lib.DeviceArray):
        if buf.dtype.itemsize != 1:
            raise ValueError("a device buffer of bytes is uint8")
        return buf, buf.n, False
    a = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview))
                             else np.asarray(buf, dtype=np.uint8))
    return _lib.DeviceArray.from_host(a if a.size else np.zeros(1, np.uint8)), a.size, True


def _count(d, n_bytes, code, line_phase):
    n_lines, n_reads, n_letters, n_bad = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.load().gki_reads_parse_count(d.ptr, n_bytes, code, int(line_phase), C.byref(n_lines), C.byref(n_reads),
                                                 C.byref(n_letters), C.byref(n_bad)))
    return n_lines.value, n_reads.value, n_letters.value, n_bad.value


def _parse(d, n_bytes, code, line_phase):
    """(letters, read_start, n_reads, n_lines, n_bad) of the device bytes d[:n_bytes]."""
    n_lines, n_reads, n_letters, n_bad = _count(d, n_bytes, code, line_phase)
    letters = _lib.DeviceArray(max(n_letters, 1), np.uint8)
    read_start = _lib.DeviceArray(n_reads + 1, np.int64)
    try:
        _lib.check(_lib.load().gki_reads_parse_emit(d.ptr, n_bytes, code, int(line_phase), letters.ptr, n_letters,
                                                    read_start.ptr, n_reads + 1))
    except Exception:
        letters.free(); read_start.free()
        raise
    letters.n = n_letters
    return letters, read_start, n_reads, n_lines, n_bad


def count_reads_in_buffer(buf, fmt, line_phase=0):
    """(n_lines, n_reads, n_letters, n_bad_lines) of a buffer of file bytes (gki_reads_parse_count): what
    `parse_reads_on_device` would lay out, and for FASTQ the lines that are not where a record has them."""
    _lib.require_device()
    code = _format_code(fmt)
    d, n_bytes, own = _device_bytes(buf)
    try:
        return _count(d, n_bytes, code, line_phase)
    finally:
        if own:
            d.free()


def parse_reads_on_device(buf, fmt, line_phase=0):
    """File bytes (NumPy uint8, bytes or a DeviceArray; whole lines, the last one terminated or not) -> (letters
    DeviceArray uint8, read_start DeviceArray int64[n_reads + 1], n_reads, n_lines).  fmt: 'fasta' or 'fastq';
    line_phase: lines of the file before this buffer, mod 4 (FASTQ only)."""
    _lib.require_device()
    code = _format_code(fmt)
    d, n_bytes, own = _device_bytes(buf)
    try:
        letters, read_start, n_reads, n_lines, _ = _parse(d, n_bytes, code, line_phase)
    finally:
        if own:
            d.free()
    return letters, read_start, n_reads, n_lines


def count_nodes_from_file(device_index, file_name, k, n_nodes, strands=3, max_hits=2 ** 62, counts=None, fmt=None,
                          chunk_bytes=DEFAULT_CHUNK_BYTES):
    """Node hit counts of every k-mer of every read of a FASTA / FASTQ file (`.gz`: through gzip on the host), streamed:
    the file is read in pieces of about `chunk_bytes` that end at a line end (`iter_line_chunks`), each piece is parsed
    on the device and probed with `device_index.count_nodes_from_reads`, all into one `counts`, and its buffers are
    freed before the next piece is read.  fmt None: by the file's first byte.  A FASTQ whose records do not have their
    '@' and '+' lines in place raises ValueError after the piece that shows it.
    Returns (counts DeviceArray uint32[n_nodes], reads, k-mers probed, hits)."""
    _lib.require_device()
    if counts is None:
        counts = _lib.DeviceArray(max(int(n_nodes), 1), np.uint32)
        counts.zero()
    code = None if fmt is None else _format_code(fmt)
    line_phase = n_reads = n_kmers = n_hits = n_bad = 0
    with open_reads_file(file_name) as f:
        for piece in iter_line_chunks(f, chunk_bytes):
            if code is None:
                code = _format_code(detect_format(piece))
            d = _lib.DeviceArray.from_host(np.frombuffer(piece, dtype=np.uint8))
            del piece
            letters = read_start = None
            try:
                letters, read_start, reads, lines, bad = _parse(d, d.n, code, line_phase)
                d.free()
                if reads:
                    _, kmers, hits = device_index.count_nodes_from_reads(letters, read_start, k, n_nodes, strands, max_hits,
                                                                         counts)
                    n_kmers += kmers
                    n_hits += hits
            finally:
                for a in (d, letters, read_start):
                    if a is not None:
                        a.free()
            n_reads += reads
            n_bad += bad
            line_phase = (line_phase + lines) % 4
            if n_bad:
                raise ValueError("%s is not a four-line FASTQ: %d record lines do not begin with '@' or '+' where they must"
                                 % (file_name, n_bad))
    return counts, n_reads, n_kmers, n_hits
