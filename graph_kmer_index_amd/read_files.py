"""Reads files on the device: FASTA / FASTQ text -> node counts, without a host pass over the lines.

The text of a file reaches HBM in pieces that end at a line end (`text_files`: raw, BGZF inflated on the device, any other
gzip through Python's gzip); gki_reads_parse_count / _emit (csrc/gki_reads_parse.hip) find the lines, pick the sequence
lines, strip them and lay them out as (uint8 letters, int64 read_start), which `DeviceIndex.count_nodes_from_reads`
(gki_probe_reads_count_nodes) consumes unchanged.  The rules -- what a line, a header, a read and a malformed FASTQ record
are -- are stated in include/gki.h ("reads files") and DESIGN.md 4.12.

Every route is the one loop of `count_nodes_from_file` over `text_files.text_pieces`; `count_piece` parses and probes one
piece.  Device temporaries belong to a `_lib.DeviceScope`.  Tools and tests reach `text_files`' names through this module.
"""
import contextlib
import ctypes as C
import numpy as np

from . import _lib
from .collision_free_kmer_index import zeroed_counts
from .text_files import (DEFAULT_CHUNK_BYTES, INFLATE_CHOICES, bgzf_text_pieces, cut_at_line_end,  # noqa: F401
                         device_bytes, host_text_pieces, inflate_piece, iter_bgzf_pieces, iter_line_chunks,
                         open_reads_file, reads_file_route, text_pieces, upload_piece)

FORMATS = {"fasta": 0, "fastq": 1}            # GKI_READS_FASTA, GKI_READS_FASTQ


def detect_format(first_bytes):
    """'fasta' or 'fastq' from the first byte of a file: '>' / '@'; an empty file is FASTA with no reads."""
    head = bytes(first_bytes[:1])
    if head == b"" or head == b">":
        return "fasta"
    if head == b"@":
        return "fastq"
    raise ValueError("cannot tell FASTA from FASTQ: the file begins with %r, not '>' or '@'" % head)


def _format_code(fmt):
    if fmt not in FORMATS:
        raise ValueError("fmt must be 'fasta' or 'fastq', not %r" % (fmt,))
    return FORMATS[fmt]


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
        d = device_bytes(s, buf)
        return parse_count(d, d.n, code, line_phase)


def parse_reads_on_device(buf, fmt, line_phase=0):
    """File bytes (NumPy uint8, bytes or a DeviceArray; whole lines, the last one terminated or not) -> (letters
    DeviceArray uint8, read_start DeviceArray int64[n_reads + 1], n_reads, n_lines).  fmt: 'fasta' or 'fastq';
    line_phase: lines of the file before this buffer, mod 4 (FASTQ only)."""
    _lib.require_device()
    code = _format_code(fmt)
    with _lib.DeviceScope() as s:
        d = device_bytes(s, buf)
        return parse_piece(d, d.n, code, line_phase)[:4]


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


def count_nodes_from_file(device_index, file_name, k, n_nodes, strands=3, max_hits=2 ** 62, counts=None, fmt=None,
                          chunk_bytes=DEFAULT_CHUNK_BYTES, inflate="auto"):
    """Node hit counts of every k-mer of every read of a FASTA / FASTQ file, streamed: one loop over the pieces of the
    text, about `chunk_bytes` each, that the file's route gives (`text_files.text_pieces`, which states the `.gz` routes
    and `inflate`); each piece is parsed on the device and probed with `device_index.count_nodes_from_reads`
    (`count_piece`), all into one `counts`, and everything of it is freed before the next piece is made.
    fmt None: by the first byte of the text.  A FASTQ whose
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
