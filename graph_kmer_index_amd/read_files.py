"""Reads files on the device: FASTA / FASTQ text -> node counts, without a host pass over the lines.

The raw bytes of a file go to HBM in chunks that end at a line end; gki_reads_parse_count / _emit (csrc/gki_reads_parse.hip)
find the lines, pick the sequence lines, strip them and lay them out as (uint8 letters, int64 read_start), which
`DeviceIndex.count_nodes_from_reads` (gki_probe_reads_count_nodes) consumes unchanged.  The rules -- what a line, a header,
a read and a malformed FASTQ record are -- are stated in include/gki.h ("reads files") and DESIGN.md 4.12.

A name ending in .gz has two routes (`reads_file_route`).  A BGZF file -- the blocked gzip of bgzip / htslib, told by its
first member -- is uploaded compressed in pieces cut at member boundaries and inflated on the device (bgzf.py,
csrc/gki_inflate.hip), and the inflated text goes to the same parse and probe kernels without a host pass.  Any other
gzip file is one serial DEFLATE stream and is read through Python's gzip module: that route is bound by the host's
inflate, not by the device.
"""
import ctypes as C
import gzip
import numpy as np

from . import _lib, bgzf

FORMATS = {"fasta": 0, "fastq": 1}            # GKI_READS_FASTA, GKI_READS_FASTQ
DEFAULT_CHUNK_BYTES = 256 << 20
INFLATE_CHOICES = ("auto", "host", "device")


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


def reads_file_route(file_name):
    """How the file reaches the device: 'raw' (its bytes are the text), 'bgzf-device' (a name ending in .gz whose first
    member is BGZF: inflated on the device) or 'gzip-host' (any other name ending in .gz: Python's gzip on the host)."""
    if not str(file_name).endswith(".gz"):
        return "raw"
    with open(file_name, "rb") as f:
        head = f.read(12)
        if len(head) == 12:
            head += f.read(head[10] | head[11] << 8)
    return "bgzf-device" if bgzf.is_bgzf(head) else "gzip-host"


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


def iter_bgzf_pieces(f, chunk_bytes, file_name=""):
    """A BGZF stream as pieces of whole members: (compressed bytes, members, file offset of the piece).  `members` are
    `bgzf.scan_members`' tuples with positions in the piece's bytes.  A piece holds at least one member, and beyond the
    first one only as many as keep both the compressed bytes and the sum of ISIZE within `chunk_bytes`: the device memory
    a piece needs is bounded by `chunk_bytes` whatever the compression ratio.  ValueError for a member that is not BGZF
    and for a file that ends inside a member.
    The file is read `chunk_bytes` + 64 KiB at a time (a member is at most 64 KiB, so that much holds a full piece).  The
    pieces are windows (memoryview) of what was read: when ISIZE is the limit that binds, one read serves several pieces
    and none of them is copied; only what is left behind the last full piece moves in front of the next read."""
    chunk_bytes = int(chunk_bytes)
    if chunk_bytes < 1:
        raise ValueError("chunk_bytes must be at least 1")
    want = chunk_bytes + 65536
    pending, start, base, at_end = b"", 0, 0, False       # the piece to come begins at pending[start], `base` in the file
    while True:
        view = memoryview(pending)[start:]
        members, n_comp, n_out, full = [], 0, 0, False
        scan = bgzf.scan_members(view, 0, base)
        while True:
            try:
                m = next(scan)
            except StopIteration as stop:
                left = stop.value
                break
            except ValueError as e:
                raise ValueError("%s: %s" % (file_name, e)) from None
            if members and (m[4] > chunk_bytes or n_out + m[3] > chunk_bytes):
                full = True
                break
            members.append(m)
            n_comp, n_out = m[4], n_out + m[3]
        if not full and not at_end:                          # the data ran out first: read on, then look again
            need = max(want - len(view), 65536)              # at least one more member, whatever is left over
            new = _read_fully(f, need)
            at_end = len(new) < need
            pending, start = (bytes(view) + new if len(view) else new), 0
            continue
        if not members:
            if left:
                raise ValueError("%s: BGZF block at offset %d: the file ends inside the member" % (file_name, base))
            return
        yield view[:n_comp], members, base
        start, base = start + n_comp, base + n_comp


def _last_newline(d, n_bytes):
    pos = C.c_int64(-1)
    _lib.check(_lib.load().gki_last_byte_position(d.ptr, n_bytes, 10, C.byref(pos)))
    return pos.value


def _count_nodes_from_bgzf(device_index, file_name, k, n_nodes, strands, max_hits, counts, code, chunk_bytes):
    """`count_nodes_from_file` of a BGZF file.  Per piece: upload the compressed bytes, inflate them behind the tail the
    last piece left (an unfinished line), parse and probe the text up to and including its last line end, and keep what
    follows on the device as the next tail.  The end of the file flushes the tail as the last line."""
    lib = _lib.load()
    line_phase = n_reads = n_kmers = n_hits = n_bad = 0
    tail = None                                   # DeviceArray of the bytes behind the last line end so far

    def parse_and_probe(d, n_bytes):
        nonlocal line_phase, n_reads, n_kmers, n_hits, n_bad
        letters = read_start = None
        try:
            letters, read_start, reads, lines, bad = _parse(d, n_bytes, code, line_phase)
            if reads:
                _, kmers, hits = device_index.count_nodes_from_reads(letters, read_start, k, n_nodes, strands, max_hits, counts)
                n_kmers += kmers
                n_hits += hits
        finally:
            for a in (letters, read_start):
                if a is not None:
                    a.free()
        n_reads += reads
        n_bad += bad
        line_phase = (line_phase + lines) % 4
        if n_bad:
            raise ValueError("%s is not a four-line FASTQ: %d record lines do not begin with '@' or '+' where they must"
                             % (file_name, n_bad))

    try:
        with open(file_name, "rb") as f:
            for piece, members, base in iter_bgzf_pieces(f, chunk_bytes, file_name):
                prefix = tail.n if tail is not None else 0
                try:
                    text = bgzf.inflate_on_device(piece, members, prefix)
                except bgzf.BgzfInflateError as e:
                    e.output.free()
                    at = base + (members[e.block - 1][4] if e.block else 0)     # where the member begins in the file
                    reason = bgzf.STATUS_TEXT.get(e.status, "status %d" % e.status)
                    raise ValueError("%s: BGZF block at offset %d: %s" % (file_name, at, reason)) from None
                del piece
                try:
                    if prefix:
                        _lib.check(lib.gki_memcpy_d2d(text.ptr, tail.ptr, prefix))
                        tail.free()
                    tail = None
                    if text.n == 0:
                        continue
                    if code is None:
                        code = _format_code(detect_format(text.to_host(1)))
                    cut = _last_newline(text, text.n) + 1
                    if cut:
                        parse_and_probe(text, cut)
                    if cut < text.n:
                        tail = _lib.DeviceArray(text.n - cut, np.uint8)
                        _lib.check(lib.gki_memcpy_d2d(tail.ptr, text.ptr.value + cut, text.n - cut))
                finally:
                    text.free()
        if tail is not None:
            parse_and_probe(tail, tail.n)
    finally:
        if tail is not None:
            tail.free()
    return counts, n_reads, n_kmers, n_hits


def count_nodes_from_file(device_index, file_name, k, n_nodes, strands=3, max_hits=2 ** 62, counts=None, fmt=None,
                          chunk_bytes=DEFAULT_CHUNK_BYTES, inflate="auto"):
    """Node hit counts of every k-mer of every read of a FASTA / FASTQ file, streamed: the file is read in pieces of about
    `chunk_bytes` that end at a line end (`iter_line_chunks`), each piece is parsed on the device and probed with
    `device_index.count_nodes_from_reads`, all into one `counts`, and its buffers are freed before the next piece is
    read.  A `.gz` file goes by `reads_file_route`: BGZF is inflated on the device (pieces of whole members,
    `iter_bgzf_pieces`), any other gzip through Python's gzip on the host.  inflate: 'auto' that rule, 'host' gzip on the
    host for every `.gz`, 'device' ValueError unless the file is BGZF.  fmt None: by the first byte of the text.  A FASTQ
    whose records do not have their '@' and '+' lines in place raises ValueError after the piece that shows it.
    Returns (counts DeviceArray uint32[n_nodes], reads, k-mers probed, hits)."""
    _lib.require_device()
    if inflate not in INFLATE_CHOICES:
        raise ValueError("inflate must be one of %s, not %r" % (", ".join(INFLATE_CHOICES), inflate))
    route = reads_file_route(file_name)
    if inflate == "device" and route != "bgzf-device":
        raise ValueError("%s is not a BGZF file: only BGZF is inflated on the device" % file_name)
    if counts is None:
        counts = _lib.DeviceArray(max(int(n_nodes), 1), np.uint32)
        counts.zero()
    code = None if fmt is None else _format_code(fmt)
    if route == "bgzf-device" and inflate != "host":
        return _count_nodes_from_bgzf(device_index, file_name, k, n_nodes, strands, max_hits, counts, code, chunk_bytes)
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
