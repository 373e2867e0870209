"""Genotype a sample on the device: the node count model fitted once, a sample's node counts turned into a call and a
quality per VCF data line, and the calls written as a VCF with one sample column.

`HaplotypePaths.node_count_model` gives the model of the population's node counts, `map` (read_files.py) a sample's node
counts.  `Genotyper(model, variant_to_nodes)` uploads the model, fits it and keeps the fitted table on the device;
`.genotype(counts)` estimates the sample's coverage and calls every kept line; `write_genotyped_vcf` copies the first eight
fields of the input VCF's data lines and appends GT:GQ, the text made on the device piece by piece.  The rules are stated
in include/gki.h ("genotyping", "genotyped VCF text") and DESIGN.md 4.21; the kernels are csrc/gki_genotype.hip and
csrc/gki_vcf_write.hip.  A cohort -- the batch `.genotype` returns for counts with a leading axis of samples -- leaves as
one VCF with a column per sample through `write_cohort_vcf` ("genotyped cohort VCF text", DESIGN.md 4.23,
csrc/gki_vcf_cohort.hip).  This is this package's own model, not KAGE's.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _lib
from .bgzf import BgzfWriter
from .text_files import DEFAULT_CHUNK_BYTES, open_reads_file, owned_pieces

FIT_FAULTS = {1: "an allele has no populated entry", 2: "an allele's entries do not hold the model's individuals"}
TEXT_FAULTS = {1: "fewer than eight fields", 2: "a call outside -1 .. ploidy"}
FORMAT_LINES = [b'##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
                b'##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality, phred-scaled, at most 99">']
COLUMNS = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
STRIP = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"


def _positive_finite(value, name):
    value = float(value)
    if not (value > 0 and math.isfinite(value)):
        raise ValueError("%s must be positive and finite, not %r" % (name, value))
    return value


def _add_ms(timings, key, ms):
    if timings is not None:
        timings[key] = timings.get(key, 0.0) + ms.value


class Genotypes:
    """What `Genotyper.genotype` returns: `call` int8 (the number of alt copies, -1 for a line that is not kept), `gq`
    uint8, `loglik` float64 or None, each with a leading axis of samples when the counts had one, and `coverage`
    float64[n_samples]."""

    def __init__(self, call, gq, loglik, coverage):
        self.call, self.gq, self.loglik = call, gq, loglik
        self.coverage = np.ascontiguousarray(coverage, dtype=np.float64)

    def to_file(self, file_name):
        """np.savez with keys named after the attributes (no `loglik` key when there is none)."""
        arrays = {"call": self.call, "gq": self.gq, "coverage": self.coverage}
        if self.loglik is not None:
            arrays["loglik"] = self.loglik
        np.savez(file_name, **arrays)

    @classmethod
    def from_file(cls, file_name):
        file_name = str(file_name)
        d = np.load(file_name if file_name.endswith(".npz") else file_name + ".npz")
        return cls(d["call"], d["gq"], d["loglik"] if "loglik" in d else None, d["coverage"])


class Genotyper:
    """The fitted count model on the device.  A context manager: the device buffers go back when it is left (or on
    close()).  `.mean` float64[V][2][P + 1] and `.n_alt` uint32[V][P + 1] read the fitted table back; `.total` is the model
    total T and `.fit_ms` the fit kernel's device time."""

    def __init__(self, model, variant_to_nodes, error=0.01, pseudo_count=1.0):
        self.error = _positive_finite(error, "error")
        self.pseudo_count = _positive_finite(pseudo_count, "pseudo_count")
        ref_nodes = np.ascontiguousarray(variant_to_nodes.ref_nodes).astype(np.uint32)
        var_nodes = np.ascontiguousarray(variant_to_nodes.var_nodes).astype(np.uint32)
        self.n_lines, self.ploidy, self.n_bins = len(var_nodes), model.ploidy, model.n_bins
        self.n_individuals = len(model.samples)
        if len(ref_nodes) != self.n_lines or len(model.histogram) != self.n_lines:
            raise ValueError("the model has %d data lines, variant-to-nodes has %d ref and %d var nodes"
                             % (len(model.histogram), len(ref_nodes), self.n_lines))
        self._scope = _lib.DeviceScope()
        try:
            self._fit(model, ref_nodes, var_nodes)
        except BaseException:
            self.close()
            raise

    def _fit(self, model, ref_nodes, var_nodes):
        s, lib, V, E = self._scope, _lib.load(), self.n_lines, self.ploidy + 1
        self._ref_nodes = s.on_device(ref_nodes if V else np.zeros(1, np.uint32), np.uint32)
        self._var_nodes = s.on_device(var_nodes if V else np.zeros(1, np.uint32), np.uint32)
        self._mean = s.array(max(2 * E * V, 1), np.float64)
        self._n_alt = s.array(max(E * V, 1), np.uint32)
        total, line, kind, ms = C.c_uint64(0), C.c_int64(-1), C.c_int(0), C.c_float(0)
        with _lib.DeviceScope() as t:                      # the model itself leaves the device after the fit
            histogram = t.on_device(model.histogram.reshape(-1) if V else np.zeros(1, np.uint32), np.uint32)
            count_sum = t.on_device(model.count_sum.reshape(-1) if V else np.zeros(1, np.uint64), np.uint64)
            _lib.check(lib.gki_genotype_fit(histogram.ptr, count_sum.ptr, self._var_nodes.ptr, V, self.ploidy, self.n_bins,
                                            self.n_individuals, self._mean.ptr, self._n_alt.ptr, C.byref(total),
                                            C.byref(line), C.byref(kind), C.byref(ms)))
        self.fit_ms, self.total = ms.value, total.value
        if kind.value:
            raise ValueError("the model's data line %d: %s" % (line.value, FIT_FAULTS[kind.value]))
        if self.total == 0:
            raise ValueError("the model total is 0: no individual has a count on a kept line's node")

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def close(self):
        scope, self._scope = getattr(self, "_scope", None), None
        if scope is not None:
            scope.__exit__(None, None, None)

    @property
    def mean(self):
        E, V = self.ploidy + 1, self.n_lines
        return np.ascontiguousarray(self._mean.to_host(2 * E * V).reshape(2, E, V).transpose(2, 0, 1))

    @property
    def n_alt(self):
        E, V = self.ploidy + 1, self.n_lines
        return np.ascontiguousarray(self._n_alt.to_host(E * V).reshape(E, V).T)

    def scale(self, d_counts, n_samples, n_nodes, timings=None):
        """S of every row of a batch on the device: uint64[n_samples]."""
        sums, ms = np.zeros(n_samples, dtype=np.uint64), C.c_float(0)
        _lib.check(_lib.load().gki_genotype_scale(self._ref_nodes.ptr, self._var_nodes.ptr, self.n_lines, d_counts.ptr,
                                                  n_samples, n_nodes, _lib.hptr(sums), C.byref(ms)))
        _add_ms(timings, "scale_ms", ms)
        return sums

    def genotype(self, counts, coverage=None, loglik=False, timings=None):
        """The calls of one sample (`counts` uint32[n_nodes]) or of a batch (uint32[n_samples][n_nodes]) as `Genotypes`.
        coverage: the sample's lambda, a number or one per row; None estimates it from the counts, which takes the
        sample's genotypes to be spread as the population's are.  ValueError for a coverage that is not positive and
        finite, and for a sample without any count on a kept line's node when the coverage is to be estimated."""
        if self._scope is None:
            raise ValueError("the Genotyper is closed")
        counts = np.asarray(counts)
        single = counts.ndim == 1
        rows = np.ascontiguousarray(counts.reshape(1, -1) if single else counts, dtype=np.uint32)
        if rows.ndim != 2:
            raise ValueError("counts is uint32[n_nodes] or uint32[n_samples][n_nodes]")
        n_samples, n_nodes = rows.shape
        V, E = self.n_lines, self.ploidy + 1
        if coverage is not None:
            lam = np.ascontiguousarray(np.broadcast_to(np.asarray(coverage, dtype=np.float64), (n_samples,)))
            for x in lam:
                _positive_finite(x, "coverage")
        call, gq = np.full((n_samples, V), -1, dtype=np.int8), np.zeros((n_samples, V), dtype=np.uint8)
        ll = np.zeros((n_samples, V, E), dtype=np.float64) if loglik else None
        with _lib.DeviceScope() as s:
            d_counts = s.on_device(rows.reshape(-1) if rows.size else np.zeros(1, np.uint32), np.uint32)
            if coverage is None:
                sums = self.scale(d_counts, n_samples, n_nodes, timings)
                if n_samples and int(sums.min()) == 0:
                    raise ValueError("sample row %d has no count on a kept line's node: its coverage cannot be estimated"
                                     % int(np.argmin(sums)))
                lam = np.array([(float(x) * float(self.n_individuals)) / float(self.total) for x in sums], dtype=np.float64)
            if n_samples and V:
                d_call, d_gq = s.array(n_samples * V, np.int8), s.array(n_samples * V, np.uint8)
                d_ll = s.array(n_samples * V * E, np.float64) if loglik else None
                ms = C.c_float(0)
                _lib.check(_lib.load().gki_genotype_call(
                    self._mean.ptr, self._n_alt.ptr, self._ref_nodes.ptr, self._var_nodes.ptr, V, self.ploidy,
                    self.n_individuals, d_counts.ptr, n_samples, n_nodes, _lib.hptr(lam), self.error, self.pseudo_count,
                    d_call.ptr, d_gq.ptr, d_ll.ptr if loglik else None, C.byref(ms)))
                _add_ms(timings, "call_ms", ms)
                call, gq = d_call.to_host().reshape(n_samples, V), d_gq.to_host().reshape(n_samples, V)
                if loglik:
                    ll = d_ll.to_host().reshape(n_samples, V, E)
        if single:
            call, gq, ll = call[0], gq[0], ll[0] if loglik else None
        return Genotypes(call, gq, ll, lam)


def header_text(vcf_file_name, sample_name="sample"):
    """The header of the genotyped VCF, made on the host from the lines in front of the input's first data line: every ##
    line but FORMAT lines of GT and GQ, this package's two FORMAT lines, and the #CHROM line cut to eight columns (the
    standard one when the input has none) with the FORMAT and the sample's column."""
    kept, columns = [], None
    with open_reads_file(vcf_file_name) as f:
        for line in f:
            line = line.rstrip(b"\n").rstrip(b"\r")
            if line and not line.startswith(b"#") and line.strip(STRIP):
                break
            if line.startswith(b"##"):
                if not line.startswith((b"##FORMAT=<ID=GT,", b"##FORMAT=<ID=GQ,")):
                    kept.append(line)
            elif line.startswith(b"#CHROM") and columns is None:
                columns = b"\t".join(line.split(b"\t")[:8])
    columns = (COLUMNS if columns is None else columns) + b"\tFORMAT\t" + str(sample_name).encode()
    return b"".join(l + b"\n" for l in kept + FORMAT_LINES + [columns])


def genotyped_lines_on_device(scope, text, n_bytes, d_call, d_gq, first, n_calls, ploidy, timings=None):
    """The genotyped data lines of one piece of text on the device: (uint8 DeviceArray or None, bytes of it, data lines).
    `d_call` and `d_gq` hold `n_calls` entries; the piece's first data line is entry `first`.  ValueError for a line at
    fault, named by its number in the file, and for a piece with more data lines than there are calls left."""
    lib = _lib.load()
    left = n_calls - first
    call_at, gq_at = C.c_void_p(d_call.ptr.value + first), C.c_void_p(d_gq.ptr.value + first)
    n_data, n_out, line, kind, ms = C.c_int64(0), C.c_int64(0), C.c_int64(-1), C.c_int(0), C.c_float(0)
    try:
        _lib.check(lib.gki_vcf_genotypes_count(text.ptr, n_bytes, call_at, gq_at, left, ploidy, C.byref(n_data), C.byref(n_out),
                                               C.byref(line), C.byref(kind), C.byref(ms)))
    except _lib.GkiError:
        if n_data.value > left:
            raise ValueError("the VCF has more than the %d data lines there are calls for" % n_calls) from None
        raise
    _add_ms(timings, "lengths_ms", ms)
    if kind.value:
        raise ValueError("data line %d: %s" % (first + line.value, TEXT_FAULTS[kind.value]))
    if n_out.value == 0:
        return None, 0, n_data.value
    out = scope.array(n_out.value, np.uint8)
    written = C.c_int64(0)
    _lib.check(lib.gki_vcf_genotypes_emit(text.ptr, n_bytes, call_at, gq_at, left, ploidy, out.ptr, out.n, C.byref(written),
                                          C.byref(ms)))
    _add_ms(timings, "emit_call_ms", ms)
    return out, written.value, n_data.value


def write_genotyped_vcf(vcf_file_name, out_file_name, call, gq, ploidy, sample_name="sample",
                        chunk_bytes=DEFAULT_CHUNK_BYTES, inflate="auto", timings=None, compress="none"):
    """Write `out_file_name`: the header (`header_text`) and, per data line of `vcf_file_name` (.vcf, or .vcf.gz as BGZF or
    gzip), its first eight fields with GT:GQ of `call` int8[V] and `gq` uint8[V].  The input is streamed in pieces of about
    `chunk_bytes`; each piece's lines are made on the device and written.  `compress`: "none" writes plain text; "bgzf"
    sends the header and each piece's lines through a `bgzf.BgzfWriter`, so the lines are deflated where they were made
    and only compressed bytes are copied to the host -- the file inflates to the plain one's bytes, whatever `chunk_bytes`.
    ValueError when the file's data lines are not V, for a data line of fewer than eight fields and for a call outside
    -1 .. ploidy; the output file is then removed.  Returns the data lines written."""
    if compress not in ("none", "bgzf"):
        raise ValueError("compress must be 'none' or 'bgzf', not %r" % (compress,))
    call = np.ascontiguousarray(call, dtype=np.int8).reshape(-1)
    gq = np.ascontiguousarray(gq, dtype=np.uint8).reshape(-1)
    if len(call) != len(gq):
        raise ValueError("%d calls and %d qualities" % (len(call), len(gq)))
    if not 1 <= int(ploidy) <= 8:
        raise ValueError("ploidy must be in 1..8")
    V, done = len(call), 0
    header = header_text(vcf_file_name, sample_name)
    try:
        with _lib.DeviceScope() as s, (BgzfWriter(out_file_name) if compress == "bgzf" else open(out_file_name, "wb")) as out:
            d_call = s.on_device(call if V else np.zeros(1, np.int8), np.int8)
            d_gq = s.on_device(gq if V else np.zeros(1, np.uint8), np.uint8)
            out.write(header)
            for text, n_bytes in owned_pieces(vcf_file_name, chunk_bytes, inflate):
                with _lib.DeviceScope() as piece:
                    lines, n_out, n_data = genotyped_lines_on_device(piece, text, n_bytes, d_call, d_gq, done, V, int(ploidy),
                                                                     timings)
                    if n_out and compress == "bgzf":
                        out.write_device(lines, n_out)
                    elif n_out:
                        lines.to_host(n_out).tofile(out)
                    done += n_data
            if done != V:
                raise ValueError("%s has %d data lines, there are %d calls" % (vcf_file_name, done, V))
            if compress == "bgzf" and timings is not None:
                out.close()                                  # the last member's time too
                timings["deflate_ms"] = timings.get("deflate_ms", 0.0) + out.kernel_ms
    except BaseException:
        if os.path.exists(out_file_name):
            os.remove(out_file_name)
        raise
    return done


# ------------------------------------------------------------------------------------------------ a cohort

def check_sample_names(sample_names):
    """The names as a list of str.  ValueError unless they are non-empty, unique and free of tabs, spaces and line ends."""
    names = [str(n) for n in sample_names]
    for n in names:
        if not n or any(c in n for c in "\t \n\r"):
            raise ValueError("sample name %r: a name is not empty and holds no tab, space or line end" % (n,))
    if len(set(names)) != len(names):
        raise ValueError("the sample names are not unique")
    return names


def cohort_header_text(vcf_file_name, sample_names):
    """`header_text` with the #CHROM line carrying all the names, in order."""
    return header_text(vcf_file_name, "\t".join(check_sample_names(sample_names)))


def cohort_lines_on_device(text, n_bytes, d_call, d_gq, n_samples, row_stride, first, ploidy, max_out_bytes=1 << 30,
                           timings=None):
    """The genotyped data lines of one piece of text with `n_samples` sample columns, made on the device (include/gki.h,
    "genotyped cohort VCF text").  `d_call` int8 and `d_gq` uint8 are [n_samples][row_stride] as the call kernel writes
    them; the piece's first data line is entry `first` of every row.  A generator: yields (uint8 DeviceArray, bytes of it,
    data lines in it) for consecutive ranges of the piece's data lines, each of at most `max_out_bytes` bytes unless one
    line alone has more; a range's array lives until the next one is asked for.  A piece without data lines yields
    nothing.  ValueError for a line at fault, named by its number in the file, and for a piece with more data lines than
    there are calls left."""
    lib = _lib.load()
    left = row_stride - first
    batch = (text.ptr, n_bytes, d_call.ptr, d_gq.ptr, row_stride, first, n_samples, left, ploidy)
    n_data, n_out, line, kind, ms = C.c_int64(0), C.c_int64(0), C.c_int64(-1), C.c_int(0), C.c_float(0)
    with _lib.DeviceScope() as piece:
        try:
            _lib.check(lib.gki_vcf_cohort_count(*batch, C.byref(n_data), C.byref(n_out), C.byref(line), C.byref(kind), None, 0,
                                                C.byref(ms)))
        except _lib.GkiError:
            if n_data.value > left:
                raise ValueError("the VCF has more than the %d data lines there are calls for" % row_stride) from None
            raise
        _add_ms(timings, "lengths_ms", ms)
        if kind.value:
            raise ValueError("data line %d: %s" % (first + line.value, TEXT_FAULTS[kind.value]))
        V = n_data.value
        cuts = [0, V]
        if n_out.value > max(int(max_out_bytes), 1):         # cut where the line starts say, at least a line a range
            d_start = piece.array(V + 1, np.int64)
            _lib.check(lib.gki_vcf_cohort_count(*batch, C.byref(n_data), C.byref(n_out), C.byref(line), C.byref(kind),
                                                d_start.ptr, V + 1, C.byref(ms)))
            _add_ms(timings, "lengths_ms", ms)
            start = d_start.to_host(V + 1)
            cuts = [0]
            while cuts[-1] < V:
                fit = int(np.searchsorted(start, start[cuts[-1]] + int(max_out_bytes), side="right")) - 1
                cuts.append(min(V, max(fit, cuts[-1] + 1)))
    for line_from, line_to in zip(cuts[:-1], cuts[1:]):
        if line_to == line_from:
            continue
        with _lib.DeviceScope() as part:
            capacity = n_out.value if len(cuts) == 2 else int(start[line_to] - start[line_from])
            out, written = part.array(capacity, np.uint8), C.c_int64(0)
            _lib.check(lib.gki_vcf_cohort_emit(*batch, line_from, line_to, out.ptr, out.n, C.byref(written), C.byref(ms)))
            _add_ms(timings, "emit_call_ms", ms)
            yield out, written.value, line_to - line_from


def write_cohort_vcf(vcf_file_name, out_file_name, call, gq, ploidy, sample_names, chunk_bytes=None, inflate="auto",
                     compress="none", max_out_bytes=1 << 30, timings=None):
    """Write `out_file_name`: the header (`cohort_header_text`) and, per data line of `vcf_file_name` (.vcf, or .vcf.gz as
    BGZF or gzip), its first eight fields, GT:GQ and one column per sample s of `call` int8[S][V] and `gq` uint8[S][V]
    (a quality above 99 is written as 99).  The batch is uploaded once, as it is; the input is streamed in pieces of
    about `chunk_bytes` (default: text_files' own, divided by the number of 64-column groups so that a piece's tables stay
    small), each piece's lines are made on the device in ranges of at most `max_out_bytes` output bytes (a line alone may
    have more) and written, or with `compress` "bgzf" sent through a `bgzf.BgzfWriter` where they were made.  The file's
    bytes depend on the input's text and the calls alone.  ValueError as `write_genotyped_vcf`, and when the names do not
    match the rows or break `check_sample_names`' rule; the output file is then removed.  Returns the data lines written."""
    if compress not in ("none", "bgzf"):
        raise ValueError("compress must be 'none' or 'bgzf', not %r" % (compress,))
    call, gq = np.ascontiguousarray(call, dtype=np.int8), np.ascontiguousarray(gq, dtype=np.uint8)
    if call.ndim != 2 or call.shape != gq.shape:
        raise ValueError("call is int8[S][V] and gq uint8[S][V], not %r and %r" % (call.shape, gq.shape))
    S, V = call.shape
    names = check_sample_names(sample_names)
    if len(names) != S or S < 1:
        raise ValueError("%d sample names for %d rows of calls (at least one)" % (len(names), S))
    if not 1 <= int(ploidy) <= 8:
        raise ValueError("ploidy must be in 1..8")
    if int(max_out_bytes) < 1:
        raise ValueError("max_out_bytes must be positive")
    if chunk_bytes is None:
        chunk_bytes = max(1 << 20, DEFAULT_CHUNK_BYTES // ((S + 63) // 64))
    header, done = cohort_header_text(vcf_file_name, names), 0
    try:
        with _lib.DeviceScope() as s, (BgzfWriter(out_file_name) if compress == "bgzf" else open(out_file_name, "wb")) as out:
            d_call = s.on_device(call.reshape(-1) if V else np.zeros(1, np.int8), np.int8)
            d_gq = s.on_device(gq.reshape(-1) if V else np.zeros(1, np.uint8), np.uint8)
            out.write(header)
            for text, n_bytes in owned_pieces(vcf_file_name, chunk_bytes, inflate):
                for lines, n_out, n_lines in cohort_lines_on_device(text, n_bytes, d_call, d_gq, S, V, done, int(ploidy),
                                                                    max_out_bytes, timings):
                    if compress == "bgzf":
                        out.write_device(lines, n_out)
                    else:
                        lines.to_host(n_out).tofile(out)
                    done += n_lines
            if done != V:
                raise ValueError("%s has %d data lines, there are %d calls" % (vcf_file_name, done, V))
            if compress == "bgzf" and timings is not None:
                out.close()                                  # the last member's time too
                timings["deflate_ms"] = timings.get("deflate_ms", 0.0) + out.kernel_ms
    except BaseException:
        if os.path.exists(out_file_name):
            os.remove(out_file_name)
        raise
    return done
