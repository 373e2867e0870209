"""VCF files on the device: .vcf and BGZF .vcf.gz text -> VariantArrays, without a host pass over the lines.

The text reaches HBM as the reads files' does -- `text_files.owned_pieces`: pieces that end at a line end, a BGZF file
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

`haplotype_matrix_from_file` / `haplotype_matrix_on_device` give the genotypes themselves as a `HaplotypeMatrix`: one code
per sample haplotype and data line, and on request the same as two bit planes (gki_vcf_haplotype_matrix,
gki_haplotype_planes, csrc/gki_vcf_gt.hip; include/gki.h "VCF haplotype matrix").  `MatrixPieces` appends
the pieces' rows on the device; the number of sample columns comes from the text in front of the first data line.
"""
import ctypes as C

import numpy as np

from . import _lib
from .text_files import DEFAULT_CHUNK_BYTES, device_bytes, names_from, owned_pieces

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


def cat(parts, dtype):
    """The pieces' host arrays as one, an empty one of `dtype` when there is no piece."""
    return np.concatenate(parts) if parts else np.zeros(0, dtype)


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
    for text, n_bytes in owned_pieces(file_name, chunk_bytes, inflate):
        with _lib.DeviceScope() as s:
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
    for text, n_bytes in owned_pieces(file_name, chunk_bytes, inflate):
        joined.add_piece(text, n_bytes, source)
    return joined.arrays()


# ---------------------------------------------------------------------------------------- the haplotype matrix

MAX_PLOIDY = 8
PLANES_TILE_SLOTS = 256                                    # PLANES_T of csrc/gki_vcf_gt.hip: the slots of a plane tile
STRIP = bytes([0x20]) + bytes(range(0x09, 0x0E)) + bytes(range(0x1C, 0x20))   # what a blank line is made of (include/gki.h)
HM_KIND_TEXT = {2: "FORMAT does not begin with GT", 3: AF_KIND_TEXT["genotype"],
                4: "the line does not have exactly %(n_samples)d sample fields",
                5: "a GT has more than %(ploidy)d alleles"}    # first_bad_kind of gki_vcf_haplotype_matrix


class HaplotypeMatrixError(ValueError):
    """A VCF whose haplotype matrix cannot be read; `line` is the data line at fault, numbered from 0 in the file, `kind`
    a key of HM_KIND_TEXT."""

    def __init__(self, line, kind, n_samples, ploidy):
        super().__init__("VCF data line %d: %s" % (line, HM_KIND_TEXT[kind] % {"n_samples": n_samples, "ploidy": ploidy}))
        self.line, self.kind = int(line), int(kind)


def haplotype_planes_on_device(scope, codes, n_variants, n_slots):
    """The device bytes codes[n_variants * n_slots] as two bit planes: (ref_bits, alt_bits) uint64 DeviceArrays of `scope`
    with n_slots * ceil(n_variants / 64) words each (one word where that is zero), and the kernel's device time in ms."""
    n_words = (n_variants + 63) // 64
    ref_bits, alt_bits = scope.array(max(n_slots * n_words, 1), np.uint64), scope.array(max(n_slots * n_words, 1), np.uint64)
    ms = C.c_float(0)
    _lib.check(_lib.load().gki_haplotype_planes(codes.ptr, n_variants, n_slots, ref_bits.ptr, alt_bits.ptr, C.byref(ms)))
    return ref_bits, alt_bits, float(ms.value)


class HaplotypeMatrix:
    """Which allele every sample haplotype carries at every data line of a VCF, host arrays: `codes` uint8[V, S * P] (0
    allele 0, 1 allele 1, 2 any other allele, 3 none; sample s has slots s * P .. s * P + P - 1), `phased` uint8[V] (1
    when no GT of the line holds a '/'), `n_samples` S, `ploidy` P, `sample_names` (list[str], or None when the file
    does not name S samples)."""

    def __init__(self, codes, phased, n_samples, ploidy, sample_names=None):
        self.n_samples, self.ploidy = int(n_samples), int(ploidy)
        self.phased = np.ascontiguousarray(phased, dtype=np.uint8).reshape(-1)
        self.codes = np.ascontiguousarray(codes, dtype=np.uint8).reshape(len(self.phased), self.n_samples * self.ploidy)
        self.sample_names = None if sample_names is None else [str(n) for n in sample_names]
        if self.sample_names is not None and len(self.sample_names) != self.n_samples:
            raise ValueError("a haplotype matrix of %d samples and %d names" % (self.n_samples, len(self.sample_names)))

    @property
    def n_variants(self):
        return len(self.phased)

    def planes(self):
        """(ref_bits, alt_bits) uint64[S * P, ceil(V / 64)], computed on the device: bit v % 64 of word [h][v // 64] is set
        in ref_bits where codes[v][h] == 0 and in alt_bits where it is 1."""
        n_variants, n_slots = self.n_variants, self.n_samples * self.ploidy
        shape = (n_slots, (n_variants + 63) // 64)
        if n_variants == 0 or n_slots == 0:
            return np.zeros(shape, dtype=np.uint64), np.zeros(shape, dtype=np.uint64)
        _lib.require_device()
        with _lib.DeviceScope() as s:
            ref_bits, alt_bits, _ = haplotype_planes_on_device(s, s.on_device(self.codes.reshape(-1), np.uint8), n_variants, n_slots)
            return tuple(a.to_host(shape[0] * shape[1]).reshape(shape) for a in (ref_bits, alt_bits))

    def to_file(self, file_name, planes=False):
        """np.savez with keys named after the attributes (sample_names left out when None), ref_bits and alt_bits too when
        `planes`."""
        arrays = {"codes": self.codes, "phased": self.phased, "n_samples": np.int64(self.n_samples),
                  "ploidy": np.int64(self.ploidy)}
        if self.sample_names is not None:
            arrays["sample_names"] = np.array(self.sample_names, dtype=np.str_)
        if planes:
            arrays["ref_bits"], arrays["alt_bits"] = self.planes()
        np.savez(file_name, **arrays)

    @classmethod
    def from_file(cls, file_name):
        file_name = str(file_name)
        d = np.load(file_name if file_name.endswith(".npz") else file_name + ".npz")
        return cls(d["codes"], d["phased"], int(d["n_samples"]), int(d["ploidy"]),
                   d["sample_names"].tolist() if "sample_names" in d.files else None)


class _SampleColumns:
    """Where S comes from: the text in front of the first data line, read on the host.  The caller's `n_samples` when
    given; else the last line beginning with #CHROM in front of the first data line, when it has 10 fields or more (S =
    fields - 9, fields 9 and up the sample names); else the first data line's field count - 9, at least 0; a file with
    neither has S = 0.  The names are kept only when they are S."""
    WINDOW = 1 << 16

    def __init__(self, n_samples):
        self.given = None if n_samples is None else int(n_samples)
        if self.given is not None and self.given < 0:
            raise ValueError("n_samples must be at least 0, not %d" % self.given)
        self.header = self.first = None
        self.done = False

    def feed(self, text, n_bytes):
        """The next piece (device bytes text[:n_bytes], whole lines): its lines up to the first data line, brought to the
        host a window at a time -- the header of a file, not its body."""
        at, window = 0, self.WINDOW
        while at < n_bytes and not self.done:
            raw = np.empty(min(window, n_bytes - at), dtype=np.uint8)
            _lib.check(_lib.load().gki_memcpy_d2h(_lib.hptr(raw), C.c_void_p(text.ptr.value + at), raw.nbytes))
            raw = raw.tobytes()
            cut = len(raw) if at + len(raw) == n_bytes else raw.rfind(b"\n") + 1
            if cut == 0:                                   # a line longer than the window
                window *= 2
                continue
            for line in raw[:cut].split(b"\n"):
                if line[:1] != b"#" and line.strip(STRIP):
                    self.first, self.done = line.rstrip(b"\r").split(b"\t"), True
                    break
                if line.startswith(b"#CHROM"):
                    self.header = line.rstrip(b"\r").split(b"\t")
            at += cut

    def resolve(self):
        """(S, sample names or None)"""
        names = None
        if self.header is not None and len(self.header) >= 10:
            names = [f.decode("utf-8") for f in self.header[9:]]
        if self.given is not None:
            n = self.given
        elif names is not None:
            n = len(names)
        else:
            n = max(len(self.first) - 9, 0) if self.first is not None else 0
        return n, names if names is not None and len(names) == n else None


def haplotype_matrix_piece(scope, text, n_bytes, n_variants, n_samples, ploidy):
    """One piece, the device bytes text[:n_bytes] with `n_variants` data lines (`vcf_count`'s): (codes uint8[n_variants *
    n_samples * ploidy], phased uint8[n_variants]) DeviceArrays of `scope`, the device time of the kernel in ms, and the
    lowest line at fault as (data line of the piece, kind) or None."""
    nv = int(n_variants)
    codes, phased = scope.array(max(nv * n_samples * ploidy, 1), np.uint8), scope.array(max(nv, 1), np.uint8)
    found, bad, kind, ms = C.c_int64(0), C.c_int64(-1), C.c_int(0), C.c_float(0)
    _lib.check(_lib.load().gki_vcf_haplotype_matrix(text.ptr, n_bytes, nv, n_samples, ploidy, codes.ptr, phased.ptr,
                                                    C.byref(found), C.byref(bad), C.byref(kind), C.byref(ms)))
    return codes, phased, float(ms.value), (bad.value, kind.value) if bad.value >= 0 else None


class MatrixPieces:
    """The pieces' rows appended on the device; everything there belongs to `scope`."""

    def __init__(self, scope, ploidy, n_samples):
        self.scope, self.ploidy = scope, int(ploidy)
        if not 1 <= self.ploidy <= MAX_PLOIDY:
            raise ValueError("ploidy must be 1 to %d, not %d" % (MAX_PLOIDY, self.ploidy))
        self.columns = _SampleColumns(n_samples)
        self.pieces, self.n_variants, self.kernel_ms = [], 0, 0.0      # [codes, phased] on the device with their bytes

    def add_piece(self, text, n_bytes):
        """The data lines of the device bytes text[:n_bytes] (whole lines) as rows, appended."""
        nv = vcf_count(text, n_bytes)[1]
        if not self.columns.done:
            self.columns.feed(text, n_bytes)
        if nv == 0:
            return
        n_samples = self.columns.resolve()[0]
        codes, phased, ms, fault = haplotype_matrix_piece(self.scope, text, n_bytes, nv, n_samples, self.ploidy)
        if fault is not None:
            raise HaplotypeMatrixError(self.n_variants + fault[0], fault[1], n_samples, self.ploidy)
        self.pieces.append([(codes, nv * n_samples * self.ploidy), (phased, nv)])
        self.n_variants += nv
        self.kernel_ms += ms

    def joined(self):
        """(codes, phased) of all pieces as one DeviceArray each, the pieces freed; None before the first data line."""
        if not self.pieces:
            return None, None
        if len(self.pieces) > 1:
            out = []
            for parts in zip(*self.pieces):
                whole, at = self.scope.array(max(sum(n for _, n in parts), 1), np.uint8), 0
                for a, n in parts:
                    if n:
                        _lib.check(_lib.load().gki_memcpy_d2d(C.c_void_p(whole.ptr.value + at), a.ptr, n))
                    a.free()
                    at += n
                out.append((whole, at))
            self.pieces = [out]
        return self.pieces[0][0][0], self.pieces[0][1][0]

    def finish(self):
        n_samples, names = self.columns.resolve()
        n_codes = self.n_variants * n_samples * self.ploidy
        d_codes, d_phased = self.joined()
        codes = d_codes.to_host(n_codes) if n_codes else np.zeros(0, np.uint8)
        phased = d_phased.to_host(self.n_variants) if self.n_variants else np.zeros(0, np.uint8)
        return HaplotypeMatrix(codes, phased, n_samples, self.ploidy, names)


def haplotype_matrix_on_device(buf, ploidy=2, n_samples=None):
    """VCF bytes (bytes, NumPy uint8 or a DeviceArray; whole lines, the last one terminated or not) -> HaplotypeMatrix of
    its GT columns, parsed on the device.  `ploidy` P: the slots of a sample, 1 to 8; a GT of fewer alleles leaves 3 in the
    others.  `n_samples`: None takes it from the #CHROM header line or the first data line.  HaplotypeMatrixError (a
    ValueError) names the lowest data line at fault."""
    _lib.require_device()
    with _lib.DeviceScope() as s:
        joined = MatrixPieces(s, ploidy, n_samples)
        d = device_bytes(s, buf)
        joined.add_piece(d, d.n)
        return joined.finish()


def haplotype_matrix_from_file(file_name, ploidy=2, n_samples=None, chunk_bytes=DEFAULT_CHUNK_BYTES, inflate="auto"):
    """`haplotype_matrix_on_device` for a .vcf, a BGZF .vcf.gz (inflated on the device) or another gzip file, streamed in
    pieces of about `chunk_bytes` (`chunk_bytes` and `inflate` as in `text_files.text_pieces`); the pieces' rows are
    appended on the device and line numbers go on across pieces."""
    _lib.require_device()
    with _lib.DeviceScope() as s:
        joined = MatrixPieces(s, ploidy, n_samples)
        for text, n_bytes in owned_pieces(file_name, chunk_bytes, inflate):
            joined.add_piece(text, n_bytes)
        return joined.finish()
