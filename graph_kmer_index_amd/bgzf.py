"""BGZF, the blocked gzip of bgzip / htslib: a chain of gzip members of at most 64 KiB, each carrying its own compressed
size in a 'BC' extra subfield.  The host walks the member headers (a few bytes per 64 KiB, nothing is inflated here) and
the device inflates all members of a piece side by side (gki_bgzf_inflate, csrc/gki_inflate.hip).

A plain gzip file -- one member, or several without the 'BC' subfield -- is one serial DEFLATE stream per member and is
not BGZF: `is_bgzf` says no and the reads-file route keeps it on the host (text_files.py).

`inflate_on_device` is one piece's inflate; text_files.bgzf_text_pieces streams a file through it.

The way out is the same split: `deflate_on_device` turns text that is in HBM into members there (gki_bgzf_deflate,
csrc/gki_bgzf_deflate.hip), `BgzfWriter` cuts a stream of writes into members and writes the file, and
`write_bgzf_on_device` converts a buffer or a plain file.  `write_bgzf` is zlib on host threads: the route of the tests
and one of the oracles."""
import ctypes as C
import os
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


DEFAULT_WRITE_CHUNK_BYTES = 64 << 20


def _block_size(block_size):
    block_size = int(block_size)
    if not 1 <= block_size <= 0xff00:
        raise ValueError("block_size must be in 1..0xff00")
    return block_size


def _device_bytes(scope, buf):
    """`buf` as a uint8 DeviceArray: one is taken as it is, bytes-like or a NumPy uint8 array is uploaded and owned by
    `scope`."""
    if isinstance(buf, _lib.DeviceArray):
        if buf.dtype.itemsize != 1:
            raise ValueError("a device buffer of bytes is uint8")
        return buf
    if not isinstance(buf, np.ndarray):
        buf = np.frombuffer(buf, dtype=np.uint8)
    if buf.dtype.itemsize != 1:
        raise ValueError("an array of bytes is uint8")
    return scope.on_device(buf.reshape(-1), np.uint8)


def deflate_on_device(buf, block_size=0xff00, n=None):
    """The first `n` bytes of `buf` (all of it by default) as BGZF members, deflated on the device (gki_bgzf_deflate,
    csrc/gki_bgzf_deflate.hip): (DeviceArray of uint8 holding the members back to back, their bytes).  One
    member per `block_size` bytes, the last one shorter, no end-of-file member; no bytes give no member.  `buf`: bytes-like,
    a NumPy uint8 array or a uint8 DeviceArray.  The caller owns the DeviceArray, which is as large as the bound, not as the
    members."""
    block_size = _block_size(block_size)
    if n is not None and int(n) < 0:
        raise ValueError("n must be >= 0")
    _lib.require_device()
    with _lib.DeviceScope() as s:
        d_in = _device_bytes(s, buf)
        n = d_in.n if n is None else int(n)
        if n > d_in.n:
            raise ValueError("n is %d, the buffer holds %d bytes" % (n, d_in.n))
        bound, n_out, n_members = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _lib.check(_lib.load().gki_bgzf_deflate_bound(n, block_size, C.byref(bound)))
        out = s.array(bound.value, np.uint8)
        _lib.check(_lib.load().gki_bgzf_deflate(d_in.ptr, n, block_size, out.ptr, bound.value, C.byref(n_out), C.byref(n_members),
                                                None))
        return s.release(out), n_out.value


class BgzfWriter:
    """A BGZF file written from text that is on the device: `write_device(d_array, n)` and `write(bytes_like)` add text,
    `close()` writes what is left and the end-of-file member.  Members are cut every `block_size` bytes of ALL the text
    written so far -- what is left below `block_size` after a write stays on the device and goes in front of the next -- so
    the file depends on the concatenated text and `block_size` only, not on how the text was cut into writes.  Only
    compressed bytes cross to the host.  A context manager: an exception inside the `with` block removes the file.
    `bytes_in`, `bytes_out` and `kernel_ms` count what went through."""

    def __init__(self, path, block_size=0xff00):
        self.block_size = _block_size(block_size)
        _lib.require_device()
        self.path, self.bytes_in, self.bytes_out, self.kernel_ms = path, 0, 0, 0.0
        self._scope = _lib.DeviceScope()
        self._rest = self._scope.array(self.block_size, np.uint8)      # the text below block_size that is not written yet
        self._rest_n = 0
        try:
            self._file = open(path, "wb")
        except BaseException:
            self._scope.__exit__(None, None, None)
            raise

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self.abandon()
        return False

    def _deflate(self, d_array, n):
        out, n_out = deflate_on_device(d_array, self.block_size, n)
        try:
            ms = C.c_float(0)
            _lib.check(_lib.load().gki_bgzf_deflate_kernel_ms(C.byref(ms)))
            self.kernel_ms += ms.value
            out.to_host(n_out).tofile(self._file)
            self.bytes_out += n_out
        finally:
            out.free()

    def write_device(self, d_array, n=None):
        """Adds the first `n` bytes (all by default) of a uint8 DeviceArray, which is the caller's again on return."""
        if self._file is None:
            raise ValueError("the writer is closed")
        if not isinstance(d_array, _lib.DeviceArray) or d_array.dtype.itemsize != 1:
            raise ValueError("write_device takes a uint8 DeviceArray")
        n = d_array.n if n is None else int(n)
        if not 0 <= n <= d_array.n:
            raise ValueError("n is %d, the buffer holds %d bytes" % (n, d_array.n))
        copy, at = _lib.load().gki_memcpy_d2d, 0
        self.bytes_in += n
        if self._rest_n:                                     # fill the member that is begun, and write it when it is whole
            at = min(n, self.block_size - self._rest_n)
            _lib.check(copy(C.c_void_p(self._rest.ptr.value + self._rest_n), d_array.ptr, at))
            self._rest_n += at
            if self._rest_n < self.block_size:
                return
            self._deflate(self._rest, self.block_size)
            self._rest_n = 0
        whole = (n - at) // self.block_size * self.block_size
        if whole:
            self._deflate(d_array.view(at, whole), whole)
        left = n - at - whole
        if left:
            _lib.check(copy(self._rest.ptr, C.c_void_p(d_array.ptr.value + at + whole), left))
            self._rest_n = left

    def write(self, data):
        """Adds bytes-like or NumPy uint8 host data (uploaded for the call)."""
        if self._file is None:
            raise ValueError("the writer is closed")
        view = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        if view.size == 0:
            return
        with _lib.DeviceScope() as s:
            self.write_device(_device_bytes(s, view))

    def close(self):
        """Writes the text that is left and the end-of-file member; closing twice is closing once."""
        if self._file is None:
            return
        try:
            if self._rest_n:
                self._deflate(self._rest, self._rest_n)
                self._rest_n = 0
            self._file.write(EOF_MEMBER)
            self.bytes_out += len(EOF_MEMBER)
        except BaseException:
            self.abandon()
            raise
        self._file.close()
        self._file = None
        self._scope.__exit__(None, None, None)

    def abandon(self):
        """Closes and removes the file and frees the device buffers."""
        if self._file is not None:
            self._file.close()
            self._file = None
            self._scope.__exit__(None, None, None)
        if os.path.exists(self.path):
            os.remove(self.path)


def write_bgzf_on_device(path, data, block_size=0xff00, chunk_bytes=DEFAULT_WRITE_CHUNK_BYTES):
    """Writes a BGZF file deflated on the device: `data` is the text (bytes-like, a NumPy uint8 array or a uint8
    DeviceArray) or the name of a plain file, which is streamed in reads of `chunk_bytes`.  The file is that of one
    `BgzfWriter` given all the text, whatever `chunk_bytes`.  Returns the bytes written.  `write_bgzf` is the host route."""
    block_size, chunk_bytes = _block_size(block_size), int(chunk_bytes)
    if chunk_bytes < 1:
        raise ValueError("chunk_bytes must be positive")
    if isinstance(data, (str, os.PathLike)) and not os.path.isfile(data):
        raise FileNotFoundError("no file %s" % data)
    with BgzfWriter(path, block_size) as writer:
        if isinstance(data, (str, os.PathLike)):
            with open(data, "rb") as f:
                while True:
                    piece = f.read(chunk_bytes)
                    if not piece:
                        break
                    writer.write(piece)
        elif isinstance(data, _lib.DeviceArray):
            writer.write_device(data)
        else:
            view = memoryview(data).cast("B")
            for a in range(0, len(view), chunk_bytes):
                writer.write(view[a:a + chunk_bytes])
    return writer.bytes_out


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
