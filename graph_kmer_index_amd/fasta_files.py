"""Reference FASTA files on the device: .fa and BGZF .fa.gz text -> the letters of the chosen records in HBM, without a
host pass over the text.

The text reaches HBM as the reads files' and the VCF's do -- `text_files.text_pieces`: pieces that end at a line end, a
BGZF file inflated on the device, any other gzip through Python's gzip -- and gki_fasta_parse_count / _names / _emit
(csrc/gki_fasta_parse.hip) give, per piece, the headers' names and letter counts and then the letters of the records the
host wants, line ends removed.  The rules are `snp_kmer_finder.read_fasta_records`' own, stated in include/gki.h ("FASTA
files") and DESIGN.md 4.16; that function is the host route and the tests' oracle.

`reference_from_file` is one loop over the pieces.  What is carried from piece to piece is the record the piece before
ended in and whether it is wanted: the bytes before a piece's first header continue it.  The host sees the names and the
counts, never the text; it decides which records are wanted (the first of a name, when the name is asked for), and after
the last piece the segments are laid out in the order asked for with device-to-device copies.
"""
import contextlib
import ctypes as C
import time

import numpy as np

from . import _lib
from .text_files import DEFAULT_CHUNK_BYTES, device_bytes, names_from, text_pieces

PARSE_CHOICES = ("auto", "host", "device")


def resolve_fasta_parse(fasta_parse):
    """'host' or 'device' for a caller's `fasta_parse`.  'auto' is the device route for every encoding: it is the faster
    one on the 3 Gbp reference as plain text, as BGZF and as other gzip (profiles/r14_fasta_parse.txt)."""
    if fasta_parse not in PARSE_CHOICES:
        raise ValueError("fasta_parse must be one of %s, not %r" % (", ".join(PARSE_CHOICES), fasta_parse))
    return "device" if fasta_parse == "auto" else fasta_parse


class DeviceReference:
    """The records `names` of a FASTA file on the device: `.letters` one uint8 DeviceArray, record i of `.names` at
    [bounds[i], bounds[i + 1]) (`.bounds` host int64); `.records_in_file` every header's name in file order, duplicates
    included; `.timings` seconds per stage of the call that made it, `parse_kernel_ms` the parse kernels' device time."""

    def __init__(self, names, bounds, letters, records_in_file, timings):
        self.names, self.bounds, self.letters = names, bounds, letters
        self.records_in_file, self.timings = records_in_file, timings

    def record(self, i):
        """Record i's letters as a window of `.letters` (no copy)."""
        return self.letters.view(int(self.bounds[i]), int(self.bounds[i + 1] - self.bounds[i]))

    def to_host(self):
        """The list of uint8 arrays `read_fasta_records` returns for the same names."""
        host = self.letters.to_host()
        return [np.ascontiguousarray(host[a:b]) for a, b in zip(self.bounds[:-1], self.bounds[1:])]

    def free(self):
        self.letters.free()


def fasta_count(text, n_bytes, kernel_ms):
    """(headers, name bytes, letters before the first header) of the device bytes text[:n_bytes]."""
    n_headers, n_name_bytes, n_lead, ms = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_float(0)
    _lib.check(_lib.load().gki_fasta_parse_count(text.ptr, n_bytes, C.byref(n_headers), C.byref(n_name_bytes),
                                                 C.byref(n_lead), C.byref(ms)))
    kernel_ms[0] += ms.value
    return n_headers.value, n_name_bytes.value, n_lead.value


def fasta_names(text, n_bytes, n_headers, n_name_bytes, kernel_ms):
    """(names list[str], letters int64 per header) of the device bytes text[:n_bytes]: a few bytes per record come back."""
    if n_headers == 0:
        return [], np.zeros(0, np.int64)
    ms = C.c_float(0)
    with _lib.DeviceScope() as s:
        name_start, body = s.array(n_headers + 1, np.int64), s.array(n_headers, np.int64)
        raw = s.array(max(n_name_bytes, 1), np.uint8)
        _lib.check(_lib.load().gki_fasta_parse_names(text.ptr, n_bytes, name_start.ptr, body.ptr, n_headers, raw.ptr,
                                                     n_name_bytes, C.byref(ms)))
        start, raw, body = name_start.to_host(), raw.to_host(n_name_bytes).tobytes(), body.to_host()
    kernel_ms[0] += ms.value
    return names_from(start, raw, "ascii", "replace"), body


def fasta_emit(scope, text, n_bytes, carry_wanted, wanted, n_letters, kernel_ms):
    """The letters of the wanted records of the device bytes text[:n_bytes], a DeviceArray of `scope` of n_letters."""
    ms, written = C.c_float(0), C.c_int64(0)
    letters = scope.array(n_letters, np.uint8)
    with _lib.DeviceScope() as t:
        flags = t.on_device(np.asarray(wanted, dtype=np.uint8), np.uint8) if len(wanted) else None
        _lib.check(_lib.load().gki_fasta_parse_emit(text.ptr, n_bytes, int(bool(carry_wanted)),
                                                    None if flags is None else flags.ptr, len(wanted), letters.ptr,
                                                    n_letters, C.byref(written), C.byref(ms)))
    if written.value != n_letters:
        raise RuntimeError("FASTA parse: the emit pass wrote %d letters, the count pass said %d" % (written.value, n_letters))
    kernel_ms[0] += ms.value
    return letters


class _Records:
    """The records of one stream, joined on the host from the pieces' names and counts (no device work here)."""

    def __init__(self, names):
        self.asked = None if names is None else set(names)
        self.found, self.first = [], {}                   # every header's name; name -> number of its first record
        self.segments = {}                                # wanted record -> [(chunk, offset in it, letters)]
        self.current, self.current_wanted = -1, False     # the record the stream is in: the carried state

    def plan_piece(self, names, body_letters, n_lead, chunk):
        """(carry_wanted, wanted flags, letters the piece gives); notes where each wanted record's letters will lie in
        the piece's output, which is chunk number `chunk`."""
        at, carry = 0, self.current_wanted
        if carry and n_lead:
            self.segments[self.current].append((chunk, 0, n_lead))
            at = n_lead
        wanted = np.zeros(len(names), dtype=np.uint8)
        for h, name in enumerate(names):
            self.current = len(self.found)
            self.found.append(name)
            self.current_wanted = name not in self.first and (self.asked is None or name in self.asked)
            self.first.setdefault(name, self.current)
            if self.current_wanted:
                wanted[h] = 1
                self.segments[self.current] = [(chunk, at, int(body_letters[h]))] if body_letters[h] else []
                at += int(body_letters[h])
        return carry, wanted, at


def _assemble(scope, records, chunks, names, file_name):
    """The final layout: (names, bounds, letters); `letters` belongs to `scope`."""
    names = [n for i, n in enumerate(records.found) if records.first[n] == i] if names is None else list(names)
    for name in names:
        if name not in records.first:
            raise KeyError("no record %r in %s (records: %s)" % (name, file_name, ", ".join(records.found)))
    bounds = np.zeros(len(names) + 1, dtype=np.int64)
    for i, name in enumerate(names):
        bounds[i + 1] = bounds[i] + sum(seg[2] for seg in records.segments[records.first[name]])
    letters = scope.array(int(bounds[-1]), np.uint8)
    lib = _lib.load()
    for i, name in enumerate(names):
        at = int(bounds[i])
        for chunk, offset, n in records.segments[records.first[name]]:
            _lib.check(lib.gki_memcpy_d2d(C.c_void_p(letters.ptr.value + at), C.c_void_p(chunks[chunk].ptr.value + offset), n))
            at += n
    return names, bounds, letters


def _reference_from_pieces(pieces, names, file_name):
    """The loop over a source of (text, n_bytes) pieces that `reference_from_file` and `parse_fasta_on_device` share."""
    records, chunks, kernel_ms = _Records(names), [], [0.0]
    timings = {"text": 0.0, "parse": 0.0, "assemble": 0.0}
    with _lib.DeviceScope() as s:
        t0 = time.perf_counter()
        for text, n_bytes in pieces:
            with _lib.DeviceScope() as t:
                t.keep(text)
                t1 = time.perf_counter()
                timings["text"] += t1 - t0                # reading, uploading and inflating happen inside the generator
                n_headers, n_name_bytes, n_lead = fasta_count(text, n_bytes, kernel_ms)
                piece_names, body = fasta_names(text, n_bytes, n_headers, n_name_bytes, kernel_ms)
                carry, wanted, n_letters = records.plan_piece(piece_names, body, n_lead, len(chunks))
                chunks.append(fasta_emit(s, text, n_bytes, carry, wanted, n_letters, kernel_ms) if n_letters else None)
                t0 = time.perf_counter()
                timings["parse"] += t0 - t1
        timings["text"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        names, bounds, letters = _assemble(s, records, chunks, names, file_name)
        _lib.check(_lib.load().gki_device_synchronize())
        timings["assemble"] = time.perf_counter() - t0
        timings["parse_kernel_ms"] = kernel_ms[0]
        return DeviceReference(names, bounds, s.release(letters), records.found, timings)


def reference_from_file(file_name, names=None, chunk_bytes=DEFAULT_CHUNK_BYTES, inflate="auto"):
    """`read_fasta_records(file_name, names)` with the text parsed on the device, streamed: one loop over the pieces of
    the text, about `chunk_bytes` each, that the file's route gives (`chunk_bytes` and `inflate` as in
    `text_files.text_pieces`).  names None: every distinct name in file order;
    of records that share a name the first is the one meant.  A name that is not in the file is read_fasta_records'
    KeyError.  Returns a DeviceReference; the caller frees its letters."""
    _lib.require_device()
    source = text_pieces(file_name, chunk_bytes, inflate)
    with contextlib.closing(source) as pieces:
        return _reference_from_pieces(pieces, names, file_name)


def parse_fasta_on_device(buf, names=None):
    """FASTA bytes (bytes, NumPy uint8 or a DeviceArray; the last line terminated or not) -> DeviceReference, as one
    piece.  A DeviceArray stays its owner's."""
    _lib.require_device()
    with _lib.DeviceScope() as s:
        d = device_bytes(s, buf)
        pieces = [(d.view(0, d.n), d.n)] if d.n else []   # a window: the loop frees what it is handed, `d` stays
        return _reference_from_pieces(iter(pieces), names, "<buffer>")
