"""The graph and its variant-to-nodes table from a reference FASTA and a VCF, built on the device.

The chosen chromosomes' letters go to HBM one record at a time and lie there concatenated; the VCF text reaches HBM as it
does for `vcf_files` (`text_files.text_pieces`: plain, BGZF inflated on the device, other gzip on the host).  Per piece the
existing parse gives the chromosome runs, the host maps the few run names to their chromosomes' bounds, and
gki_graph_sites_count / _emit (csrc/gki_graph_build.hip) turn every data line into a site.  Over all lines
gki_graph_build_count / _emit decide which sites are kept and write the arrays of graph.py, `ref_nodes` / `var_nodes`
and the sequence.  The rules are stated in include/gki.h ("graph build") and DESIGN.md 4.15.  With a source of allele
frequencies ('info' or 'genotypes') `vcf_files.allele_frequencies_piece` runs on every piece while it is on the device, and
its two arrays go to the emit call as device pointers.

The layout is the bubble chain of `graph.synthetic_snp_graph` / `synthetic_indel_graph` with every id shifted by one; it
is this package's own construction and not claimed equal to obgraph's node numbering, so a
variant-to-nodes table is only valid with the graph it was built with.
"""
import contextlib
import ctypes as C
import time

import numpy as np

from . import _lib
from .graph import GraphArrays
from .text_files import device_bytes, names_from, text_pieces
from .vcf_files import AlleleFrequencyError, af_source_code, allele_frequencies_piece, vcf_count, vcf_emit

STATUS_TEXT = {0: "kept", 1: "REF or ALT is not plain letters", 2: "no base before the site", 3: "overlaps an earlier site"}
# kinds 1 to 4 are those of gki_graph_sites_count (include/gki.h)
KIND_TEXT = {1: "fewer than five fields", 2: "POS is not 1 .. the chromosome's length", 3: "REF differs from the reference",
             4: "REF runs past the chromosome's end", "digits": "POS must be 1 to 18 plain digits",
             "unknown": "CHROM %r is not among the chosen chromosomes", "twice": "chromosome %r appears in two runs",
             "order": "chromosome %r comes out of graph order", "decreasing": "POS decreases inside a chromosome"}


class GraphBuildError(ValueError):
    """A VCF the graph cannot be built from; `line` is the data line at fault, numbered from 0 in the file."""

    def __init__(self, line, kind, name=None):
        text = KIND_TEXT[kind] % name if name is not None else KIND_TEXT[kind]
        super().__init__("VCF data line %d: %s" % (line, text))
        self.line, self.kind = int(line), kind


class GraphBuild:
    """`.graph` GraphArrays, `.variant_to_nodes` VariantToNodesArrays, `.line_status` uint8 per data line (STATUS_TEXT);
    `.route` uint8 per data line when the allele frequencies came from the VCF (vcf_files.ROUTE_*: 0 parsed on the device,
    1 absent, 2 parsed by the host), else None;
    `.timings`: seconds per stage of the call that made it, `sequence_kernel_ms` the device time of the sequence kernel."""

    def __init__(self, graph, variant_to_nodes, line_status, timings, route=None):
        self.graph, self.variant_to_nodes, self.line_status, self.timings = graph, variant_to_nodes, line_status, timings
        self.route = route


def _letters(x):
    if isinstance(x, str):
        x = x.encode("ascii", "replace")
    if isinstance(x, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(x), dtype=np.uint8)
    x = np.ascontiguousarray(x)
    if x.dtype != np.uint8:
        raise TypeError("reference letters are bytes or uint8, not %s" % x.dtype)
    return x


def _array(scope, n, dtype):
    return scope.array(max(int(n), 1), dtype)             # never a zero-byte allocation; only the first n entries count


class _Builder:
    """One build: the reference on the device, the pieces' sites appended, then the assembly.  Everything on the device
    belongs to `scope`.  `records` is one array of letters per name, uploaded here, or a reference that is on the device
    already (`.letters` one uint8 DeviceArray, `.bounds` int64[len(names) + 1], as `fasta_files.DeviceReference` has
    them), which the scope takes over and uses in place.  `af_source`: None, or where the pieces' allele frequencies come
    from ('info' or 'genotypes')."""

    def __init__(self, scope, names, records, af_source=None):
        self.scope, self.names, self.timings = scope, list(names), {}
        self.af_source = af_source
        if af_source is not None:
            af_source_code(af_source)
            self.timings["allele_frequencies"] = self.timings["allele_frequencies_kernel_ms"] = 0.0
        self.af_pieces, self.routes = [], []              # (ref_af, alt_af, n_variants) on the device; route on the host
        t0 = time.perf_counter()
        on_device = hasattr(records, "letters") and hasattr(records, "bounds")
        if on_device:
            scope.keep(records.letters)
        if not self.names or len(set(self.names)) != len(self.names):
            raise ValueError("the chromosomes must be at least one and distinct: %r" % (self.names,))
        if on_device:
            self.bounds = np.ascontiguousarray(records.bounds, dtype=np.int64)
            if len(self.bounds) != len(self.names) + 1 or int(self.bounds[-1]) != records.letters.n:
                raise ValueError("the device reference's bounds do not fit its %d names and %d letters"
                                 % (len(self.names), records.letters.n))
            for c in np.flatnonzero(np.diff(self.bounds) < 1)[:1]:
                raise ValueError("chromosome %r has no letters" % (self.names[c],))
            self.reference = records.letters
        else:
            self.bounds = np.zeros(len(self.names) + 1, dtype=np.int64)
            records = [_letters(r) for r in records]
            for c, r in enumerate(records):
                if len(r) < 1:
                    raise ValueError("chromosome %r has no letters" % (self.names[c],))
                self.bounds[c + 1] = self.bounds[c] + len(r)
            self.reference = scope.array(int(self.bounds[-1]), np.uint8)
            for c, r in enumerate(records):               # one upload per chromosome, concatenated on the device
                _lib.check(_lib.load().gki_memcpy_h2d(C.c_void_p(self.reference.ptr.value + int(self.bounds[c])),
                                                      _lib.hptr(r), len(r)))
        self.timings["upload_reference"] = time.perf_counter() - t0
        self.timings["site_pass"] = 0.0
        self.index_of = {n: c for c, n in enumerate(self.names)}
        self.pieces = []                                  # (gpos, lo, ref_len, alt_len, status, pool, n_variants, n_alt)
        self.n_lines = 0
        self.last_name, self.last_chrom, self.seen = None, -1, set()

    def _run_bounds(self, run_names, first_line_of_run):
        """(C0, C1) of every run of a piece; the checks on runs, which carry on from the piece before."""
        c0, c1 = np.zeros(len(run_names), np.int64), np.zeros(len(run_names), np.int64)
        for r, name in enumerate(run_names):
            if not (r == 0 and name == self.last_name):
                if name not in self.index_of:
                    raise GraphBuildError(first_line_of_run(r), "unknown", name)
                if name in self.seen:
                    raise GraphBuildError(first_line_of_run(r), "twice", name)
                if self.index_of[name] < self.last_chrom:
                    raise GraphBuildError(first_line_of_run(r), "order", name)
                self.seen.add(name)
                self.last_name, self.last_chrom = name, self.index_of[name]
            c0[r], c1[r] = self.bounds[self.last_chrom], self.bounds[self.last_chrom + 1]
        return c0, c1

    def add_piece(self, text, n_bytes):
        """The data lines of the device bytes text[:n_bytes] (whole lines) as sites, appended."""
        t0 = time.perf_counter()
        _, nv, n_runs, n_name_bytes, bad, kind = vcf_count(text, n_bytes)
        t1 = time.perf_counter()
        af_error = self._allele_frequencies(text, n_bytes, nv) if self.af_source is not None and nv else None
        t0 += time.perf_counter() - t1                    # the site pass's clock leaves the allele frequencies out
        try:
            if bad >= 0:                                  # kind 1: no tab at all; kind 2: POS is not plain digits
                raise GraphBuildError(self.n_lines + bad, 1 if kind == 1 else "digits")
            if nv:
                self._sites(text, n_bytes, nv, n_runs, n_name_bytes)
        except GraphBuildError as e:                      # of two lines at fault the lowest is reported
            raise (af_error if af_error is not None and af_error.line < e.line else e) from None
        if af_error is not None:
            raise af_error
        self.n_lines += nv
        self.timings["site_pass"] += time.perf_counter() - t0

    def _allele_frequencies(self, text, n_bytes, nv):
        """The piece's allele frequencies, appended; returns the error of its lowest line at fault, or None."""
        t0 = time.perf_counter()
        ref_af, alt_af, route, ms, fault = allele_frequencies_piece(self.scope, text, n_bytes, self.af_source, nv)
        self.af_pieces.append((ref_af, alt_af, nv))
        self.routes.append(route)
        self.timings["allele_frequencies"] += time.perf_counter() - t0
        self.timings["allele_frequencies_kernel_ms"] += ms
        return None if fault is None else AlleleFrequencyError(self.n_lines + fault[0], fault[1])

    def _sites(self, text, n_bytes, nv, n_runs, n_name_bytes):
        s, lib = self.scope, _lib.load()
        with _lib.DeviceScope() as t:
            _, _, chrom_run, run_name_start, run_names = vcf_emit(t, text, n_bytes, nv, n_runs, n_name_bytes)
            names = names_from(run_name_start.to_host(), run_names.to_host().tobytes(), errors="replace")
            c0, c1 = self._run_bounds(
                names, lambda r: self.n_lines + int(np.searchsorted(chrom_run.to_host(), r, side="left")))
            run_c0, run_c1 = t.on_device(c0, np.int64), t.on_device(c1, np.int64)
            args = (text.ptr, n_bytes, chrom_run.ptr, nv, run_c0.ptr, run_c1.ptr, n_runs, self.reference.ptr)
            n_alt, bad, kind = C.c_int64(0), C.c_int64(-1), C.c_int(0)
            _lib.check(lib.gki_graph_sites_count(*args, C.byref(n_alt), C.byref(bad), C.byref(kind)))
            if bad.value >= 0:
                raise GraphBuildError(self.n_lines + bad.value, kind.value)
            out = (s.array(nv, np.int64), s.array(nv, np.int64), s.array(nv, np.int32), s.array(nv, np.int32),
                   s.array(nv, np.uint8), _array(s, n_alt.value, np.uint8))
            _lib.check(lib.gki_graph_sites_emit(*args, *(a.ptr for a in out), n_alt.value))
        self.pieces.append(out + (nv, n_alt.value))

    def _joined(self, parts, dtype):
        """The pieces' arrays [(DeviceArray, entries)] as one on the device, the pieces freed; a single piece as it is."""
        if len(parts) == 1:
            return parts[0][0]
        out, at = _array(self.scope, sum(n for _, n in parts), dtype), 0
        size = out.dtype.itemsize
        for a, n in parts:
            if n:
                _lib.check(_lib.load().gki_memcpy_d2d(C.c_void_p(out.ptr.value + at * size), a.ptr, n * size))
            a.free()
            at += n
        return out

    def _appended(self):
        """The pieces' arrays as one set: (gpos, lo, ref_len, alt_len, status, pool)."""
        dtypes = (np.int64, np.int64, np.int32, np.int32, np.uint8, np.uint8)
        return tuple(self._joined([(p[j], p[7] if j == 5 else p[6]) for p in self.pieces], dt)
                     for j, dt in enumerate(dtypes))

    def finish(self, allele_frequencies=None):
        from .unique_variant_kmers import VariantToNodesArrays
        s, lib, n = self.scope, _lib.load(), self.n_lines
        t0 = time.perf_counter()
        ref_af = alt_af = route = None
        if self.af_source is not None:                    # on the device already, one value per data line
            ref_af, alt_af = (self._joined([(p[j], p[2]) for p in self.af_pieces], np.float64) for j in (0, 1))
            route = np.concatenate(self.routes) if self.routes else np.zeros(0, np.uint8)
        elif allele_frequencies is not None:
            ref_af, alt_af = (np.ascontiguousarray(a, dtype=np.float64) for a in allele_frequencies)
            if len(ref_af) != n or len(alt_af) != n:
                raise ValueError("allele_frequencies: %d and %d values for %d data lines" % (len(ref_af), len(alt_af), n))
        gpos, lo, ref_len, alt_len, status, pool = self._appended()
        n_nodes, n_edges, n_bases, n_alt, unordered = (C.c_int64(0) for _ in range(5))
        plan = C.c_void_p()
        _lib.check(lib.gki_graph_build_count(gpos.ptr, lo.ptr, ref_len.ptr, alt_len.ptr, status.ptr, n, _lib.hptr(self.bounds),
                                             len(self.names), C.byref(n_nodes), C.byref(n_edges), C.byref(n_bases),
                                             C.byref(n_alt), C.byref(unordered), C.byref(plan)))
        if unordered.value >= 0:
            raise GraphBuildError(unordered.value, "decreasing")
        try:
            if n_alt.value != sum(p[7] for p in self.pieces):
                raise RuntimeError("graph build: the alt pool has %d letters, the lines count %d"
                                   % (sum(p[7] for p in self.pieces), n_alt.value))
            self.timings["assembly_count"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            nn, ne, nb = n_nodes.value, n_edges.value, n_bases.value
            out = {"node_size": s.array(nn, np.int32), "seq": _array(s, nb, np.uint8),
                   "edge_start": s.array(nn + 1, np.int64), "edges": _array(s, ne, np.int32),
                   "rev_start": s.array(nn + 1, np.int64), "rev_edges": _array(s, ne, np.int32),
                   "is_ref": s.array(nn, np.uint8), "allele_freq": s.array(nn, np.float64), "exists": s.array(nn, np.uint8),
                   "node_to_ref_offset": s.array(nn + 1, np.int64), "chromosome_start_nodes": s.array(len(self.names), np.int64),
                   "ref_nodes": _array(s, n, np.uint32), "var_nodes": _array(s, n, np.uint32)}
            d_ref_af = None if ref_af is None else s.on_device(ref_af, np.float64).ptr
            d_alt_af = None if alt_af is None else s.on_device(alt_af, np.float64).ptr
            ms = C.c_float(0)
            _lib.check(lib.gki_graph_build_emit(plan, self.reference.ptr, pool.ptr, d_ref_af, d_alt_af,
                                                *(out[k].ptr for k in ("node_size", "seq", "edge_start", "edges",
                                                                       "rev_start", "rev_edges", "is_ref", "allele_freq",
                                                                       "exists", "node_to_ref_offset",
                                                                       "chromosome_start_nodes", "ref_nodes", "var_nodes")),
                                                C.byref(ms)))
            self.timings["assembly_emit"] = time.perf_counter() - t0
            self.timings["sequence_kernel_ms"] = float(ms.value)
        finally:
            lib.gki_graph_build_destroy(plan)
        t0 = time.perf_counter()
        sizes = {"seq": nb, "edges": ne, "rev_edges": ne, "ref_nodes": n, "var_nodes": n}
        h = {k: a.to_host(sizes.get(k)) for k, a in out.items()}
        line_status = status.to_host(n) if n else np.zeros(0, np.uint8)
        self.timings["copy_back"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        graph = GraphArrays(h["node_size"], h["seq"], h["edge_start"], h["edges"], h["is_ref"], h["allele_freq"], h["exists"],
                            first_node=1, chromosome_start_nodes=h["chromosome_start_nodes"].tolist(),
                            node_to_ref_offset=h["node_to_ref_offset"], rev_start=h["rev_start"], rev_edges=h["rev_edges"])
        self.timings["graph_arrays"] = time.perf_counter() - t0
        return GraphBuild(graph, VariantToNodesArrays(h["ref_nodes"], h["var_nodes"]), line_status, self.timings, route)


def _af_argument(allele_frequencies):
    """(source, values) of the `allele_frequencies` argument: a source's name, or None / the two host arrays."""
    if isinstance(allele_frequencies, str):
        af_source_code(allele_frequencies)
        return allele_frequencies, None
    return None, allele_frequencies


def build_graph(reference, text, chromosomes=None, allele_frequencies=None):
    """The build from in-memory inputs: `reference` a {name: letters} mapping (bytes or uint8), `text` the VCF as bytes
    (or NumPy uint8, or a uint8 DeviceArray).  `chromosomes`: the names in graph order, None = the mapping's order.
    `allele_frequencies`: None (every node 1.0), (ref_af, alt_af), float64 with one value per data line, or the source
    they are read from on the device: 'info' (INFO's AF= entry) or 'genotypes' (the GT columns); a line without a value
    keeps 1.0 on both nodes.
    Returns a GraphBuild; GraphBuildError and vcf_files.AlleleFrequencyError (both ValueError) name the data line a faulty
    VCF is refused at."""
    _lib.require_device()
    names = list(reference) if chromosomes is None else list(chromosomes)
    source, values = _af_argument(allele_frequencies)
    with _lib.DeviceScope() as s:
        builder = _Builder(s, names, [reference[n] for n in names], source)
        d = device_bytes(s, text)
        builder.add_piece(d, d.n)
        return builder.finish(values)


def build_graph_from_files(fasta, vcf, chromosomes=None, allele_frequencies=None, chunk_bytes=None, inflate="auto",
                           fasta_parse="auto"):
    """The graph of the FASTA records `chromosomes` (None: every record, in file order) with the variants of `vcf`: a
    .vcf, a BGZF .vcf.gz inflated on the device, any other .gz through Python's gzip (`inflate` and `chunk_bytes` as in
    `text_files.text_pieces`).  The VCF is streamed in pieces of about `chunk_bytes`; line numbers and the order check
    carry across pieces.  `allele_frequencies` as in `build_graph`; a source is read from every piece while it is on the
    device.
    fasta_parse: 'device' the FASTA (plain, BGZF or gzip) is parsed on the device (`fasta_files.reference_from_file`) and
    its letters stay there; 'host' `read_fasta_records` and one upload per chromosome; 'auto' the faster of the two."""
    from .fasta_files import reference_from_file, resolve_fasta_parse
    from .snp_kmer_finder import read_fasta_records
    _lib.require_device()
    device = resolve_fasta_parse(fasta_parse) == "device"
    af_source, af_values = _af_argument(allele_frequencies)
    source = text_pieces(vcf, chunk_bytes, inflate)
    with _lib.DeviceScope() as s, contextlib.closing(source) as pieces:
        t0 = time.perf_counter()
        if device:                                        # `chunk_bytes` is the VCF's: the FASTA's pieces keep their size
            records = reference_from_file(fasta, chromosomes)
            s.keep(records.letters)
            names, parse_ms = records.names, records.timings["parse_kernel_ms"]
        else:
            names, records = read_fasta_records(fasta, chromosomes)  # one read of the file for every record
            parse_ms = 0.0
        read_seconds = time.perf_counter() - t0
        builder = _Builder(s, names, records, af_source)
        del records
        builder.timings["read_reference"] = read_seconds
        builder.timings["parse_reference_kernel_ms"] = parse_ms
        t0 = time.perf_counter()
        for text, n_bytes in pieces:
            with _lib.DeviceScope() as t:
                t.keep(text)
                builder.add_piece(text, n_bytes)
        # reading, uploading and inflating the VCF happen inside the loop, between the site passes
        builder.timings["vcf_text"] = (time.perf_counter() - t0 - builder.timings["site_pass"]
                                       - builder.timings.get("allele_frequencies", 0.0))
        return builder.finish(af_values)
