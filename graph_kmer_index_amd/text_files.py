"""Text files on the device: the bytes of a file -> pieces of text in HBM that end at a line end.  The layer `read_files`,
`vcf_files`, `fasta_files` and `graph_files` share; what a piece means is theirs.

A name ending in .gz has two routes (`reads_file_route`).  A BGZF file -- the blocked gzip of bgzip / htslib, told by its
first member -- is uploaded compressed in pieces cut at member boundaries and inflated on the device (bgzf.py,
csrc/gki_inflate.hip), and the inflated text goes to the parse kernels without a host pass.  Any other gzip file is one
serial DEFLATE stream and is read through Python's gzip module: that route is bound by the host's inflate.

`text_pieces` gives a file's source of pieces: `host_text_pieces` (raw and host gzip) or `bgzf_text_pieces`, generators of
(text on the device, bytes of it that are whole lines) built from the step functions `upload_piece`, `inflate_piece` and
`cut_at_line_end`; `owned_pieces` is the same source for a consumer that is one loop and leaves the pieces' lifetime to it.
`device_bytes` takes a buffer that is in memory already; `names_from` decodes the parsers' name lists.
"""
import contextlib
import ctypes as C
import gzip
import numpy as np

from . import _lib, bgzf

DEFAULT_CHUNK_BYTES = 256 << 20
INFLATE_CHOICES = ("auto", "host", "device")


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


def device_bytes(scope, buf):
    """The bytes of `buf` on the device: a uint8 DeviceArray as it is, anything else uploaded into `scope`."""
    if isinstance(buf, _lib.DeviceArray):
        if buf.dtype.itemsize != 1:
            raise ValueError("a device buffer of bytes is uint8")
    elif isinstance(buf, (bytes, bytearray, memoryview)):
        buf = np.frombuffer(buf, dtype=np.uint8)
    return scope.on_device(buf, np.uint8)


def names_from(start, raw, encoding="utf-8", errors="strict"):
    """The names a parser brought back as `raw` bytes with their bounds `start` (n + 1 offsets), decoded: list[str]."""
    return [raw[a:b].decode(encoding, errors) for a, b in zip(start[:-1], start[1:])]


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


def text_pieces(file_name, chunk_bytes=None, inflate="auto"):
    """The source of pieces of a text file by its route (`reads_file_route`), about `chunk_bytes` each (None:
    DEFAULT_CHUNK_BYTES).  inflate: 'auto' BGZF is inflated on the device and any other gzip through Python's gzip on the
    host, 'host' gzip on the host for every `.gz`, 'device' ValueError unless the file is BGZF.  The consumer closes it
    (contextlib.closing)."""
    if inflate not in INFLATE_CHOICES:
        raise ValueError("inflate must be one of %s, not %r" % (", ".join(INFLATE_CHOICES), inflate))
    route = reads_file_route(file_name)
    if inflate == "device" and route != "bgzf-device":
        raise ValueError("%s is not a BGZF file: only BGZF is inflated on the device" % file_name)
    source = bgzf_text_pieces if route == "bgzf-device" and inflate != "host" else host_text_pieces
    return source(file_name, DEFAULT_CHUNK_BYTES if chunk_bytes is None else chunk_bytes)


def owned_pieces(file_name, chunk_bytes=None, inflate="auto"):
    """`text_pieces` for a consumer that is one loop: yields (text, n_bytes), holds each text in a DeviceScope of its own
    for the one iteration that uses it, and closes the source when the loop is left, at its end or by an exception (which
    closes this generator at its yield)."""
    with contextlib.closing(text_pieces(file_name, chunk_bytes, inflate)) as pieces:
        for text, n_bytes in pieces:
            with _lib.DeviceScope() as s:
                s.keep(text)
                yield text, n_bytes
