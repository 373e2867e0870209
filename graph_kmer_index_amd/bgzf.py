"""BGZF, the blocked gzip of bgzip / htslib: a chain of gzip members of at most 64 KiB, each carrying its own compressed
size in a 'BC' extra subfield.  The host walks the member headers (a few bytes per 64 KiB, nothing is inflated here) and
the device inflates all members of a piece side by side (gki_bgzf_inflate, csrc/gki_inflate.hip).

A plain gzip file -- one member, or several without the 'BC' subfield -- is one serial DEFLATE stream per member and is
not BGZF: `is_bgzf` says no and the reads-file route keeps it on the host (text_files.py).

`inflate_on_device` is one piece's inflate; text_files.bgzf_text_pieces streams a file through it."""
import ctypes as C
import struct
import zlib

import numpy as np

from . import _lib

MAX_ISIZE = 65536                 # a member inflates to at most 64 KiB
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")   # the 28 bytes bgzip ends a file with
GKI_ERR_INFLATE = 9               # include/gki.h
STATUS_TEXT = {
    1: "the compressed data ends inside the stream", 2: "block type 3", 3: "stored block length check failed",
    4: "invalid code lengths", 5: "repeat code with no length before it", 6: "invalid literal/length symbol",
    7: "invalid distance symbol", 8: "distance reaches before the block's start", 9: "more data than ISIZE states",
    10: "less data than ISIZE states", 11: "compressed bytes left over behind the final block", 12: "CRC-32 mismatch",
    13: "invalid code"}


class BgzfInflateError(ValueError):
    """A member that does not inflate: `block` is its number among the members given, `status` the reason
    (include/gki.h, "BGZF"), `output` the DeviceArray every other member was still inflated into (the caller frees it)."""

    def __init__(self, block, status, output):
        super().__init__("BGZF block %d: %s" % (block, STATUS_TEXT.get(status, "status %d" % status)))
        self.block, self.status, self.output = block, status, output


def _bc_bsize(extra):
    """BSIZE of the 'BC' subfield (SLEN 2) of an extra field, None when there is none.  Subfields are walked: 'BC' need
    not be the first; a subfield that runs past the field ends the walk."""
    p = 0
    while p + 4 <= len(extra):
        slen = extra[p + 2] | extra[p + 3] << 8
        if extra[p] == 66 and extra[p + 1] == 67 and slen == 2 and p + 6 <= len(extra):
            return extra[p + 4] | extra[p + 5] << 8
        p += 4 + slen
    return None


def is_bgzf(first_bytes):
    """Whether a file that begins with these bytes is BGZF: ID 31 / 139, CM 8, FLG exactly FEXTRA, and a 'BC' subfield
    of two bytes in the extra field.  Needs the first 12 + XLEN bytes; fewer is False."""
    b = bytes(first_bytes[:12])
    if len(b) < 12 or b[0] != 31 or b[1] != 139 or b[2] != 8 or b[3] != 4:
        return False
    xlen = b[10] | b[11] << 8
    extra = bytes(first_bytes[12:12 + xlen])
    return len(extra) == xlen and _bc_bsize(extra) is not None


def scan_members(buf, offset=0, file_offset=0):
    """Generator over the whole members of `buf` (bytes-like) from `offset` on: (payload_start, payload_len, crc32, isize,
    next_offset), positions in `buf`.  It stops at the end of the buffer or at a member that the buffer cuts off, and its
    return value (StopIteration.value; `scan_all` hands it out) is the number of bytes left behind the last whole member.
    ValueError, with the member's offset in the file (`file_offset` is where buf[0] lies in it), for a member that is not
    BGZF: no gzip magic or method, FLG other than FEXTRA, no 'BC' subfield, BSIZE too small for its own header and trailer,
    ISIZE above 65 536."""
    view = memoryview(buf)
    n = len(view)
    while True:
        if n - offset < 12:
            return n - offset
        head = bytes(view[offset:offset + 12])
        at = file_offset + offset
        if head[0] != 31 or head[1] != 139 or head[2] != 8:
            raise ValueError("BGZF member at offset %d: not a gzip member (bytes %s)" % (at, head[:3].hex()))
        if head[3] != 4:
            raise ValueError("BGZF member at offset %d: FLG is %d, not FEXTRA alone" % (at, head[3]))
        xlen = head[10] | head[11] << 8
        if n - offset < 12 + xlen:
            return n - offset
        bsize = _bc_bsize(bytes(view[offset + 12:offset + 12 + xlen]))
        if bsize is None:
            raise ValueError("BGZF member at offset %d: no 'BC' subfield (a plain gzip member)" % at)
        size = bsize + 1
        if size < 12 + xlen + 8:
            raise ValueError("BGZF member at offset %d: BSIZE %d is too small for its header and trailer" % (at, bsize))
        if n - offset < size:
            return n - offset
        crc, isize = struct.unpack_from("<II", view, offset + size - 8)
        if isize > MAX_ISIZE:
            raise ValueError("BGZF member at offset %d: ISIZE %d is above 65536" % (at, isize))
        yield offset + 12 + xlen, size - 12 - xlen - 8, crc, isize, offset + size
        offset += size


def scan_all(buf, offset=0, file_offset=0):
    """(list of the members `scan_members` yields, bytes left behind the last whole one)."""
    members, gen = [], scan_members(buf, offset, file_offset)
    while True:
        try:
            members.append(next(gen))
        except StopIteration as stop:
            return members, stop.value


def _member(payload, crc, isize):
    head = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(payload) + 25)
    return head + payload + struct.pack("<II", crc, isize)


def compress_member(data, level=6):
    """One BGZF member holding `data` (at most 65 536 bytes, and small enough that the member fits 64 KiB)."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    payload = co.compress(data) + co.flush()
    if len(data) > MAX_ISIZE or len(payload) + 26 > 65536:
        raise ValueError("%d bytes do not fit one BGZF member" % len(data))
    return _member(payload, zlib.crc32(data), len(data))


def write_bgzf(path, data, block_size=0xff00, level=6, threads=1):
    """Writes `data` (bytes-like) as a BGZF file: one member per `block_size` bytes (1..0xff00, bgzip's own size), raw
    deflate from zlib at `level`, and the 28-byte empty member at the end.  A host utility -- for converting a file once,
    and for the tests and the benchmark.  threads > 1 compresses that many members at a time (zlib releases the
    interpreter lock); the file is the same."""
    block_size = int(block_size)
    if not 1 <= block_size <= 0xff00:
        raise ValueError("block_size must be in 1..0xff00")
    view = memoryview(data).cast("B")
    one = lambda a: compress_member(bytes(view[a:a + block_size]), level)
    with open(path, "wb") as f:
        if threads > 1:
            from concurrent.futures import ThreadPoolExecutor
            batch = 64 * int(threads) * block_size
            with ThreadPoolExecutor(int(threads)) as pool:
                for b in range(0, len(view), batch):
                    f.writelines(pool.map(one, range(b, min(b + batch, len(view)), block_size)))
        else:
            for a in range(0, len(view), block_size):
                f.write(one(a))
        f.write(EOF_MEMBER)


def inflate_on_device(buf, members, prefix=0):
    """The members' data, inflated on the device: a DeviceArray of uint8 with `prefix` bytes left free (unwritten) at the
    front and the members' output back to back behind them.  `buf`: the compressed bytes, bytes-like or NumPy uint8 or a
    uint8 DeviceArray; `members`: (payload_start, payload_len, crc32, isize, ...) per member, positions in `buf`, as
    `scan_members` yields them.  BgzfInflateError (a ValueError) names the first member that does not inflate."""
    _lib.require_device()
    prefix = int(prefix)
    if prefix < 0:
        raise ValueError("prefix must be >= 0")
    n = len(members)
    cols = np.array([m[:4] for m in members], dtype=np.int64).reshape(n, 4)
    if n and (cols[:, 3].max() > MAX_ISIZE or cols.min() < 0 or cols[:, 1].max() > 0x7FFFFFFF):
        raise ValueError("a member's ISIZE is above 65536, or a field is out of range")
    out_start = np.empty(n + 1, dtype=np.int64)
    out_start[0] = prefix
    np.cumsum(cols[:, 3], out=out_start[1:])
    out_start[1:] += prefix
    total = int(out_start[n])
    if isinstance(buf, _lib.DeviceArray):
        if buf.dtype.itemsize != 1:
            raise ValueError("a device buffer of bytes is uint8")
    elif not isinstance(buf, np.ndarray):
        buf = np.frombuffer(buf, dtype=np.uint8)
    with _lib.DeviceScope() as s:
        out = s.array(total, np.uint8)
        if n:
            d_in = s.on_device(buf, np.uint8)
            d_cols = [s.on_device(col, dtype) for col, dtype in ((cols[:, 0], np.int64), (cols[:, 1], np.int32),
                                                                 (cols[:, 2], np.uint32), (out_start, np.int64))]
            bad, status = C.c_int64(-1), C.c_int(0)
            rc = _lib.load().gki_bgzf_inflate(d_in.ptr, d_in.n, *[d.ptr for d in d_cols], n, out.ptr, total, C.byref(bad),
                                              C.byref(status))
            if rc == GKI_ERR_INFLATE:
                raise BgzfInflateError(bad.value, status.value, s.release(out))     # the output travels with the error
            _lib.check(rc)
        return s.release(out)
