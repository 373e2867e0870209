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

Every route is the one loop of `count_nodes_from_file` over a source of pieces: `host_text_pieces` (raw and host gzip) or
`bgzf_text_pieces`, generators of (text on the device, bytes of it that are whole lines) built from the step functions
`upload_piece`, `inflate_piece` and `cut_at_line_end`; `count_piece` parses and probes one piece.  Device temporaries
belong to a `_lib.DeviceScope`, so that nothing stays behind on any way out.
"""
import contextlib
import ctypes as C
import gzip
import numpy as np

from . import _lib, bgzf
from .collision_free_kmer_index import zeroed_counts

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


def _device_bytes(scope, buf):
    """The bytes of `buf` on the device: a uint8 DeviceArray as it is, anything else uploaded into `scope`."""
    if isinstance(buf, _lib.DeviceArray):
        if buf.dtype.itemsize != 1:
            raise ValueError("a device buffer of bytes is uint8")
    elif isinstance(buf, (bytes, bytearray, memoryview)):
        buf = np.frombuffer(buf, dtype=np.uint8)
    return scope.on_device(buf, np.uint8)


def parse_count(text, n_bytes, code, line_phase):
    """(n_lines, n_reads, n_letters, n_bad_lines) of the device bytes text[:n_bytes] (gki_reads_parse_count)."""
    n_lines, n_reads, n_letters, n_bad = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.load().gki_reads_parse_count(text.ptr, n_bytes, code, int(line_phase), C.byref(n_lines),
                                                 C.byref(n_reads), C.byref(n_letters), C.byref(n_bad)))
    return n_lines.value, n_reads.value, n_letters.value, n_bad.value


def parse_emit(text, n_bytes, code, line_phase, n_reads, n_letters):
    """(letters, read_start) of the device bytes text[:n_bytes], sized by what `parse_count` said of them."""
    with _lib.DeviceScope() as s:
        letters, read_start = s.array(n_letters, np.uint8), s.array(n_reads + 1, np.int64)
        _lib.check(_lib.load().gki_reads_parse_emit(text.ptr, n_bytes, code, int(line_phase), letters.ptr, n_letters,
                                                    read_start.ptr, n_reads + 1))
        return s.release(letters), s.release(read_start)


def parse_piece(text, n_bytes, code, line_phase):
    """(letters, read_start, n_reads, n_lines, n_bad) of the device bytes text[:n_bytes]."""
    n_lines, n_reads, n_letters, n_bad = parse_count(text, n_bytes, code, line_phase)
    return parse_emit(text, n_bytes, code, line_phase, n_reads, n_letters) + (n_reads, n_lines, n_bad)


def count_reads_in_buffer(buf, fmt, line_phase=0):
    """(n_lines, n_reads, n_letters, n_bad_lines) of a buffer of file bytes (gki_reads_parse_count): what
    `parse_reads_on_device` would lay out, and for FASTQ the lines that are not where a record has them."""
    _lib.require_device()
    code = _format_code(fmt)
    with _lib.DeviceScope() as s:
        d = _device_bytes(s, buf)
        return parse_count(d, d.n, code, line_phase)


def parse_reads_on_device(buf, fmt, line_phase=0):
    """File bytes (NumPy uint8, bytes or a DeviceArray; whole lines, the last one terminated or not) -> (letters
    DeviceArray uint8, read_start DeviceArray int64[n_reads + 1], n_reads, n_lines).  fmt: 'fasta' or 'fastq';
    line_phase: lines of the file before this buffer, mod 4 (FASTQ only)."""
    _lib.require_device()
    code = _format_code(fmt)
    with _lib.DeviceScope() as s:
        d = _device_bytes(s, buf)
        return parse_piece(d, d.n, code, line_phase)[:4]


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


# ---- the steps of the streamed route; tools/bench_read_files.py puts a clock around each of them

def upload_piece(piece):
    """The bytes of a piece of the file as a uint8 DeviceArray."""
    return _lib.DeviceArray.from_host(np.frombuffer(piece, dtype=np.uint8))


def inflate_piece(piece, members, base, tail, file_name=""):
    """The text of one `iter_bgzf_pieces` piece (host bytes or a uint8 DeviceArray of them) behind `tail`, the unfinished
    line the piece before left on the device (or None): one DeviceArray.  The tail is freed right after its copy.  A
    member that does not inflate is a ValueError with the member's offset in the file."""
    prefix = tail.n if tail is not None else 0
    try:
        text = bgzf.inflate_on_device(piece, members, prefix)
    except bgzf.BgzfInflateError as e:
        e.output.free()
        at = base + (members[e.block - 1][4] if e.block else 0)     # where the member begins in the file
        reason = bgzf.STATUS_TEXT.get(e.status, "status %d" % e.status)
        raise ValueError("%s: BGZF block at offset %d: %s" % (file_name, at, reason)) from None
    with _lib.DeviceScope() as s:
        s.keep(text)
        if prefix:
            _lib.check(_lib.load().gki_memcpy_d2d(text.ptr, tail.ptr, prefix))
            tail.free()
        return s.release(text)


def cut_at_line_end(text):
    """(n_bytes, tail): text[:n_bytes] ends with the text's last line end (0: there is none), and what follows it is
    copied into `tail`, a DeviceArray of its own (None: nothing follows)."""
    pos = C.c_int64(-1)
    _lib.check(_lib.load().gki_last_byte_position(text.ptr, text.n, 10, C.byref(pos)))
    cut = pos.value + 1
    if cut == text.n:
        return cut, None
    with _lib.DeviceScope() as s:
        tail = s.array(text.n - cut, np.uint8)
        _lib.check(_lib.load().gki_memcpy_d2d(tail.ptr, text.ptr.value + cut, tail.n))
        return cut, s.release(tail)


def count_piece(device_index, text, n_bytes, code, line_phase, k, n_nodes, strands, max_hits, counts):
    """One piece into `counts`: text[:n_bytes] is parsed, the text freed, the reads probed and then freed too.
    Takes `text` over from the caller.  Returns (reads, lines, bad lines, k-mers probed, hits)."""
    kmers = hits = 0
    with _lib.DeviceScope() as s:
        s.keep(text)
        letters, read_start, reads, lines, bad = parse_piece(text, n_bytes, code, line_phase)
        s.keep(letters), s.keep(read_start)
        text.free()                               # early: the file bytes are not held through the probe
        if reads:
            _, kmers, hits = device_index.count_nodes_from_reads(letters, read_start, k, n_nodes, strands, max_hits, counts)
    return reads, lines, bad, kmers, hits


# ---- the two sources of pieces: generators of (text, n_bytes), text a uint8 DeviceArray that passes to the consumer and
# whose first n_bytes bytes are whole lines (only the stream's last piece may end unterminated)

def host_text_pieces(file_name, chunk_bytes):
    """The 'raw' and 'gzip-host' routes: the text read (and inflated) on the host in pieces that end at a line end
    (`iter_line_chunks`), each uploaded."""
    with open_reads_file(file_name) as f:
        for piece in iter_line_chunks(f, chunk_bytes):
            text = upload_piece(piece)
            del piece
            yield text, text.n


def bgzf_text_pieces(file_name, chunk_bytes):
    """The 'bgzf-device' route: the compressed pieces of `iter_bgzf_pieces`, each inflated on the device behind the tail
    of the piece before, cut at its last line end, and what follows kept on the device as the next tail; the end of the
    file gives the tail as the last piece.  The tail is this generator's own and goes back when it is closed, so a
    consumer that may stop early closes it (contextlib.closing)."""
    tail = None
    try:
        with open(file_name, "rb") as f:
            for piece, members, base in iter_bgzf_pieces(f, chunk_bytes, file_name):
                with _lib.DeviceScope() as s:
                    text = s.keep(inflate_piece(piece, members, base, tail, file_name))
                    del piece
                    cut, tail = cut_at_line_end(text)
                    if cut:
                        yield s.release(text), cut
        if tail is not None:
            text, tail = tail, None
            yield text, text.n
    finally:
        if tail is not None:
            tail.free()


def text_pieces(file_name, chunk_bytes=DEFAULT_CHUNK_BYTES, inflate="auto"):
    """The source of pieces of a text file by its route (`reads_file_route`).  inflate: 'auto' BGZF is inflated on the
    device and any other gzip on the host, 'host' gzip on the host for every `.gz`, 'device' ValueError unless the file is
    BGZF.  The consumer closes it (contextlib.closing)."""
    if inflate not in INFLATE_CHOICES:
        raise ValueError("inflate must be one of %s, not %r" % (", ".join(INFLATE_CHOICES), inflate))
    route = reads_file_route(file_name)
    if inflate == "device" and route != "bgzf-device":
        raise ValueError("%s is not a BGZF file: only BGZF is inflated on the device" % file_name)
    source = bgzf_text_pieces if route == "bgzf-device" and inflate != "host" else host_text_pieces
    return source(file_name, chunk_bytes)


def count_nodes_from_file(device_index, file_name, k, n_nodes, strands=3, max_hits=2 ** 62, counts=None, fmt=None,
                          chunk_bytes=DEFAULT_CHUNK_BYTES, inflate="auto"):
    """Node hit counts of every k-mer of every read of a FASTA / FASTQ file, streamed: one loop over the pieces of the
    text, about `chunk_bytes` each, that the file's route gives (`host_text_pieces`, `bgzf_text_pieces`); each piece is
    parsed on the device and probed with `device_index.count_nodes_from_reads` (`count_piece`), all into one `counts`,
    and everything of it is freed before the next piece is made.  A `.gz` file goes by `reads_file_route`: BGZF is inflated
    on the device, any other gzip through Python's gzip on the host.  inflate: 'auto' that rule, 'host' gzip on the host
    for every `.gz`, 'device' ValueError unless the file is BGZF.  fmt None: by the first byte of the text.  A FASTQ whose
    records do not have their '@' and '+' lines in place raises ValueError after the piece that shows it.
    Returns (counts DeviceArray uint32[n_nodes], reads, k-mers probed, hits)."""
    _lib.require_device()
    source = text_pieces(file_name, chunk_bytes, inflate)
    code = None if fmt is None else _format_code(fmt)
    line_phase = n_reads = n_kmers = n_hits = n_bad = 0
    with _lib.DeviceScope() as s, contextlib.closing(source) as pieces:
        counts = zeroed_counts(s, n_nodes) if counts is None else counts
        for text, n_bytes in pieces:
            if code is None:
                s.keep(text)                      # until count_piece has it
                code = _format_code(detect_format(text.to_host(1)))
                s.release(text)
            reads, lines, bad, kmers, hits = count_piece(device_index, text, n_bytes, code, line_phase, k, n_nodes, strands,
                                                         max_hits, counts)
            n_reads, n_kmers, n_hits, n_bad = n_reads + reads, n_kmers + kmers, n_hits + hits, n_bad + bad
            line_phase = (line_phase + lines) % 4
            if n_bad:
                raise ValueError("%s is not a four-line FASTQ: %d record lines do not begin with '@' or '+' where they must"
                                 % (file_name, n_bad))
        return s.release(counts), n_reads, n_kmers, n_hits
