"""VCF files on the device: .vcf and BGZF .vcf.gz text -> VariantArrays, without a host pass over the lines.

The text reaches HBM as the reads files' does -- `text_files.text_pieces`: pieces that end at a line end, a BGZF file
inflated on the device -- and gki_vcf_parse_count / _emit (csrc/gki_vcf_parse.hip) turn each piece into POS, is_snp and
the chromosome of every data line, the chromosomes as runs of equal names.  The rules are stated in include/gki.h ("VCF
files") and DESIGN.md 4.14; they give what `VariantArrays.from_vcf` gives wherever that returns, except that POS must be
plain digits.

`variant_arrays_from_file` is one loop over the pieces; `VariantPieces` joins them on the host: data-line numbers go on
across pieces, and a piece's first run continues the last run of the piece before when the names are equal.

`allele_frequencies_from_file` / `allele_frequencies_on_device` give (ref_af, alt_af, route) per data line from INFO's AF=
entry or from the GT columns (gki_vcf_allele_frequencies, csrc/gki_vcf_af.hip; include/gki.h "VCF allele frequencies",
DESIGN.md 4.17).  `allele_frequencies_piece` is the step both and `graph_files` share: the kernel, then the host's
float() on the few value texts the device's grammar leaves out.
"""
import contextlib
import ctypes as C

import numpy as np

from . import _lib
from .text_files import DEFAULT_CHUNK_BYTES, device_bytes, names_from, text_pieces

BAD_TEXT = {1: "VCF data line %d has fewer than two columns",          # VariantArrays.from_vcf's own message
            2: "VCF data line %d: POS must be 1 to 18 plain digits (no sign, blank or underscore) for the device parser"}


AF_SOURCES = {"info": 0, "genotypes": 1}                  # GKI_AF_SOURCE_* of include/gki.h
ROUTE_DEVICE, ROUTE_ABSENT, ROUTE_HOST = 0, 1, 2
AF_KINDS = {1: "value", 2: "format", 3: "genotype"}       # first_bad_kind of gki_vcf_allele_frequencies
AF_KIND_TEXT = {"value": "INFO's AF is not a finite number in [0, 1]", "text": "INFO's AF is not a number",
                "format": "FORMAT does not begin with GT",
                "genotype": "a GT is not alleles ('.' or 1 to 9 digits) separated by '/' or '|'"}


class AlleleFrequencyError(ValueError):
    """A VCF whose allele frequencies cannot be read; `line` is the data line at fault, numbered from 0 in the file, `kind`
    a key of AF_KIND_TEXT."""

    def __init__(self, line, kind):
        super().__init__("VCF data line %d: %s" % (line, AF_KIND_TEXT[kind]))
        self.line, self.kind = int(line), kind


def bad_line_error(data_line, kind):
    """The ValueError for bad data line `data_line` (numbered from 0 in the file) of `kind` (include/gki.h)."""
    return ValueError(BAD_TEXT[kind] % data_line)


def vcf_count(text, n_bytes):
    """(n_lines, n_variants, n_runs, n_name_bytes, first_bad_variant, first_bad_kind) of the device bytes text[:n_bytes]."""
    n_lines, n_variants, n_runs, n_names, bad = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(-1)
    kind = C.c_int(0)
    _lib.check(_lib.load().gki_vcf_parse_count(text.ptr, n_bytes, C.byref(n_lines), C.byref(n_variants), C.byref(n_runs),
                                               C.byref(n_names), C.byref(bad), C.byref(kind)))
    return n_lines.value, n_variants.value, n_runs.value, n_names.value, bad.value, kind.value


def vcf_emit(scope, text, n_bytes, n_variants, n_runs, n_name_bytes):
    """(positions int64, is_snp int8, chrom_run int32, run_name_start int64[n_runs + 1], run_names uint8) of the device
    bytes text[:n_bytes], DeviceArrays of `scope` sized by what `vcf_count` said of them."""
    out = (scope.array(n_variants, np.int64), scope.array(n_variants, np.int8), scope.array(n_variants, np.int32),
           scope.array(n_runs + 1, np.int64), scope.array(n_name_bytes, np.uint8))
    _lib.check(_lib.load().gki_vcf_parse_emit(text.ptr, n_bytes, out[0].ptr, out[1].ptr, out[2].ptr, n_variants, out[3].ptr,
                                              n_runs, out[4].ptr, n_name_bytes))
    return out


def copy_back(positions, is_snp, chrom_run, run_name_start, run_names):
    """`vcf_emit`'s arrays on the host: (positions, is_snp, chrom_run, run_names list[str]); names are UTF-8."""
    names = names_from(run_name_start.to_host(), run_names.to_host().tobytes())
    return positions.to_host(), is_snp.to_host(), chrom_run.to_host(), names


def parse_piece(scope, text, n_bytes):
    """One piece: ((positions, is_snp, chrom_run, run_names, n_lines), None), or (None, (first bad data line of the piece,
    its kind)) when the piece has a bad line.  Host arrays; what the device holds for them on the way belongs to `scope`."""
    n_lines, n_variants, n_runs, n_name_bytes, bad, kind = vcf_count(text, n_bytes)
    if bad >= 0:
        return None, (bad, kind)
    return copy_back(*vcf_emit(scope, text, n_bytes, n_variants, n_runs, n_name_bytes)) + (n_lines,), None


def parse_vcf_on_device(buf):
    """VCF bytes (bytes, NumPy uint8 or a DeviceArray; whole lines, the last one terminated or not) -> (positions int64,
    is_snp int8, chrom_run int32, run_names list[str], n_lines), host arrays: chrom_run[v] is the number of the run of
    equal CHROM data line v belongs to, run_names[r] that run's name.  ValueError for a bad data line."""
    _lib.require_device()
    with _lib.DeviceScope() as s:
        d = device_bytes(s, buf)
        out, bad = parse_piece(s, d, d.n)
    if bad is not None:
        raise bad_line_error(*bad)
    return out


class VariantPieces:
    """The pieces of one file joined on the host (no device work here)."""

    def __init__(self):
        self.positions, self.is_snp, self.run_of_variant, self.run_names = [], [], [], []
        self.n_variants = self.n_lines = 0

    def add(self, positions, is_snp, chrom_run, run_names, n_lines):
        joined = bool(run_names) and bool(self.run_names) and run_names[0] == self.run_names[-1]
        shift = len(self.run_names) - (1 if joined else 0)
        self.run_names.extend(run_names[1:] if joined else run_names)
        self.positions.append(positions)
        self.is_snp.append(is_snp)
        self.run_of_variant.append(chrom_run.astype(np.int64) + shift)
        self.n_variants += len(positions)
        self.n_lines += n_lines

    def variant_arrays(self):
        from .unique_variant_kmers import VariantArrays

        def cat(parts, dtype):
            return np.concatenate(parts) if parts else np.zeros(0, dtype)
        run_of_variant = cat(self.run_of_variant, np.int64)
        chromosomes = np.array(self.run_names, dtype=object)[run_of_variant]
        return VariantArrays(cat(self.positions, np.int64), chromosomes, np.arange(self.n_variants),
                             cat(self.is_snp, np.int8))


def variant_arrays_from_file(file_name, chunk_bytes=DEFAULT_CHUNK_BYTES, inflate="auto"):
    """`VariantArrays.from_vcf(file_name)` with the lines parsed on the device, streamed: one loop over the pieces of the
    text, about `chunk_bytes` each, that the file's route gives (`chunk_bytes` and `inflate` as in
    `text_files.text_pieces`).  A bad data line raises ValueError after the piece that shows it, with its number in the
    file."""
    _lib.require_device()
    joined = VariantPieces()
    source = text_pieces(file_name, chunk_bytes, inflate)
    with contextlib.closing(source) as pieces:
        for text, n_bytes in pieces:
            with _lib.DeviceScope() as s:
                s.keep(text)
                out, bad = parse_piece(s, text, n_bytes)
            if bad is not None:
                raise bad_line_error(joined.n_variants + bad[0], bad[1])
            joined.add(*out)
    return joined.variant_arrays()


def af_source_code(source):
    if source not in AF_SOURCES:
        raise ValueError("the allele frequencies' source must be one of %s, not %r" % (", ".join(AF_SOURCES), source))
    return AF_SOURCES[source]


def allele_frequencies_piece(scope, text, n_bytes, source, n_variants):
    """One piece, the device bytes text[:n_bytes] with `n_variants` data lines (`vcf_count`'s): (ref_af, alt_af) float64
    DeviceArrays of `scope`, route as a host uint8 array, the device time of the kernel in ms, and the lowest line at
    fault as (data line of the piece, kind) or None.  The value texts of route 2 alone come back to the host; float()
    turns them into values that are written into the two device arrays."""
    lib, nv = _lib.load(), int(n_variants)
    ref_af, alt_af = scope.array(max(nv, 1), np.float64), scope.array(max(nv, 1), np.float64)
    with _lib.DeviceScope() as t:
        route, begin, length = t.array(max(nv, 1), np.uint8), t.array(max(nv, 1), np.int64), t.array(max(nv, 1), np.int32)
        found, bad, kind, ms = C.c_int64(0), C.c_int64(-1), C.c_int(0), C.c_float(0)
        _lib.check(lib.gki_vcf_allele_frequencies(text.ptr, n_bytes, af_source_code(source), nv, ref_af.ptr, alt_af.ptr,
                                                  route.ptr, begin.ptr, length.ptr, C.byref(found), C.byref(bad),
                                                  C.byref(kind), C.byref(ms)))
        fault = (bad.value, AF_KINDS[kind.value]) if bad.value >= 0 else None
        h_route = route.to_host(nv)
        host_lines = np.flatnonzero(h_route == ROUTE_HOST)
        if len(host_lines):
            h_begin, h_length = begin.to_host(nv), length.to_host(nv)
        for v in host_lines.tolist():                     # ascending: the first text at fault is the lowest
            if fault is not None and fault[0] < v:
                break
            raw = np.empty(int(h_length[v]), dtype=np.uint8)
            _lib.check(lib.gki_memcpy_d2h(_lib.hptr(raw), C.c_void_p(text.ptr.value + int(h_begin[v])), raw.nbytes))
            try:
                value = float(raw.tobytes())
            except ValueError:
                fault = (v, "text")
                break
            if not (np.isfinite(value) and 0.0 <= value <= 1.0):
                fault = (v, "value")
                break
            pair = np.array([1.0 - value, value], dtype=np.float64)
            for a, x in zip((ref_af, alt_af), (pair[0:1], pair[1:2])):
                _lib.check(lib.gki_memcpy_h2d(C.c_void_p(a.ptr.value + 8 * v), _lib.hptr(x), 8))
    return ref_af, alt_af, h_route, float(ms.value), fault


class _AfPieces:
    """The pieces' results joined on the host."""

    def __init__(self):
        self.ref_af, self.alt_af, self.route, self.n_variants = [], [], [], 0

    def add_piece(self, text, n_bytes, source):
        nv = vcf_count(text, n_bytes)[1]
        if nv == 0:
            return
        with _lib.DeviceScope() as s:
            ref_af, alt_af, route, _, fault = allele_frequencies_piece(s, text, n_bytes, source, nv)
            if fault is not None:
                raise AlleleFrequencyError(self.n_variants + fault[0], fault[1])
            self.ref_af.append(ref_af.to_host(nv))
            self.alt_af.append(alt_af.to_host(nv))
        self.route.append(route)
        self.n_variants += nv

    def arrays(self):
        def cat(parts, dtype):
            return np.concatenate(parts) if parts else np.zeros(0, dtype)
        return cat(self.ref_af, np.float64), cat(self.alt_af, np.float64), cat(self.route, np.uint8)


def allele_frequencies_on_device(buf, source):
    """VCF bytes (bytes, NumPy uint8 or a DeviceArray; whole lines, the last one terminated or not) -> (ref_af float64,
    alt_af float64, route uint8), one entry per data line, host arrays.  source: 'info' (INFO's AF= entry) or 'genotypes'
    (the GT columns).  route: 0 parsed on the device, 1 absent (both values 1.0), 2 the value text went through float()
    on the host.  AlleleFrequencyError (a ValueError) names the lowest data line at fault."""
    _lib.require_device()
    af_source_code(source)
    joined = _AfPieces()
    with _lib.DeviceScope() as s:
        d = device_bytes(s, buf)
        joined.add_piece(d, d.n, source)
    return joined.arrays()


def allele_frequencies_from_file(file_name, source, chunk_bytes=DEFAULT_CHUNK_BYTES, inflate="auto"):
    """`allele_frequencies_on_device` for every data line of a .vcf, a BGZF .vcf.gz (inflated on the device) or another
    gzip file, streamed in pieces of about `chunk_bytes` (`chunk_bytes` and `inflate` as in `text_files.text_pieces`);
    line numbers go on across pieces.  No reference and no graph is needed."""
    _lib.require_device()
    af_source_code(source)
    joined = _AfPieces()
    with contextlib.closing(text_pieces(file_name, chunk_bytes, inflate)) as pieces:
        for text, n_bytes in pieces:
            with _lib.DeviceScope() as s:
                s.keep(text)
                joined.add_piece(text, n_bytes, source)
    return joined.arrays()
