"""UniqueVariantKmersFinder with the reference's constructor (unique_variant_kmers.py:10-41), dense path only
(`use_dense_kmer_finder=True`, unique_variant_kmers.py:114-270), on MI355X.

For every variant (skipped when its ref or alt node is 0) the reference tries P = len(range(2, k-2)[::4]) start
positions POS-26, POS-22, ..., POS-2 (k=31), farthest first; at each it runs a fresh DenseKmerFinder limited to the
variant's nodes not yet taken by an earlier variant of the same finder (`_nodes_found`), rejects a position whose first
500 windows share a hash between ref and alt (the last position is always accepted), stops after a position whose
maximum k-mer frequency is <= 1, and keeps the first position of lowest maximum frequency.

Here all start positions of all variants run as one batch (csrc/gki_variant_kmers.hip, include/gki.h gki_uvk_*): the
search with no store filter, one summary per start position (records and maximum frequency per node, shared-hash flag),
one selection per variant.  Variants whose ref or alt node also belongs to another variant of the same chunk depend on
what was chosen before them; those are resolved in order on the host from their summaries (`last_serial_variants`).

The positional accessors obgraph would supply are restated from the graph's arrays (unpinned):
  * graph ref offset = node_to_ref_offset[chromosome_start_nodes[chromosome]] + chromosome offset
  * the node at a ref offset is the linear-ref node of nonzero size that covers it, the offset is the distance into it
A start before 0 or past the linear path is a ValueError naming the variant (the reference's answer there depends on
obgraph's arrays).  When the graph object has obgraph's accessors, a sample of starts is checked against them.

Simple selection (`use_simple=True` of the reference, unique_variant_kmers.py:66-111): find_kmers_over_variants below.  For
every variant one search for its ref node and one for its alt node, each with only_store_nodes = only_follow_nodes =
{node}; no frequency source, no choice among start positions, no `_nodes_found`.  All searches run as one batch of the
per-node search (include/gki.h gki_uvk_simple_starts, gki_forward_node_*), which writes the FlatKmers columns itself.
"""
import logging
import time

import numpy as np

from . import _lib
from .collision_free_kmer_index import CollisionFreeKmerIndex
from .device_graph import DeviceGraph
from .flat_kmers import DeviceFlatKmers, FlatKmers
from .graph import GraphArrays
from .kmer_counter import KmerCounter

WINDOW_CAP = 500          # kmer_finder.py:137-160
SUMMARY_DTYPE = np.dtype([("n_ref", np.uint32), ("n_alt", np.uint32), ("f_ref", np.uint32), ("f_alt", np.uint32),
                          ("flags", np.uint32)])          # gki_uvk_summary


def start_distances(k):
    """[i for i in range(2, k-2)][::4][::-1]: start j of a variant is POS - start_distances(k)[j]."""
    return [i for i in range(2, k - 2)][::4][::-1]


class VariantArrays:
    """Variants as arrays: VCF POS (1-based), chromosome (as in the VCF), line number (data lines from 0), and
    optionally is_snp (1 SNP, 0 another type, -1 type not set), which only simple selection reads."""

    def __init__(self, positions, chromosomes, line_numbers, is_snp=None):
        self.positions = np.ascontiguousarray(positions, dtype=np.int64)
        n = len(self.positions)
        if np.isscalar(chromosomes) or isinstance(chromosomes, str):
            chromosomes = np.full(n, chromosomes, dtype=object)
        self.chromosomes = np.asarray(chromosomes)
        self.line_numbers = np.ascontiguousarray(line_numbers, dtype=np.int64)
        if len(self.chromosomes) != n or len(self.line_numbers) != n:
            raise ValueError("positions, chromosomes and line numbers differ in length")
        self.is_snp = None if is_snp is None else np.ascontiguousarray(is_snp, dtype=np.int8)
        if self.is_snp is not None and len(self.is_snp) != n:
            raise ValueError("positions and is_snp differ in length")

    def __len__(self):
        return len(self.positions)

    @classmethod
    def from_objects(cls, variants):
        variants = list(variants)
        for v in variants:
            assert v.vcf_line_number is not None, "Variant line number must be specified"     # :251
        types = [getattr(v, "type", None) for v in variants]
        return cls([v.position for v in variants], np.array([v.chromosome for v in variants], dtype=object),
                   [v.vcf_line_number for v in variants], [-1 if t is None else int(t == "SNP") for t in types])

    @classmethod
    def from_vcf(cls, file_name):
        """CHROM, POS and line number of every data line (lines not starting with '#'), numbered from 0; is_snp from REF
        and ALT, a SNP when both are one base long (as obgraph types a variant), not set on a line without them."""
        import gzip
        opener = gzip.open if str(file_name).endswith(".gz") else open
        chroms, positions, is_snp = [], [], []
        with opener(file_name, "rt") as f:
            for line in f:
                if line.startswith("#") or not line.strip():
                    continue
                fields = line.rstrip("\r\n").split("\t", 5)
                if len(fields) < 2:
                    raise ValueError("VCF data line %d has fewer than two columns" % len(positions))
                chroms.append(fields[0])
                positions.append(int(fields[1]))
                is_snp.append(-1 if len(fields) < 5 else int(len(fields[3]) == 1 and len(fields[4]) == 1))
        return cls(positions, np.array(chroms, dtype=object), np.arange(len(positions)), is_snp)

    @classmethod
    def from_vcf_on_device(cls, file_name, chunk_bytes=None, inflate="auto"):
        """What `from_vcf` returns, with the lines parsed on the device (vcf_files.py): a .vcf, a BGZF .vcf.gz inflated on
        the device, any other .gz through Python's gzip.  POS must be plain digits there."""
        from .vcf_files import variant_arrays_from_file
        return variant_arrays_from_file(file_name, chunk_bytes=chunk_bytes, inflate=inflate)


def load_variant_to_nodes(file_name):
    """(ref_nodes, var_nodes) of a VariantToNodes file: an .npz with `ref_nodes` and `var_nodes`, or obgraph's own
    format through obgraph when it is installed.  A missing file is a FileNotFoundError."""
    import os
    name = str(file_name)
    path = name if os.path.exists(name) else name + ".npz"
    if not os.path.exists(path):
        raise FileNotFoundError("variant-to-nodes file not found: %s" % name)
    try:
        d = np.load(path)
        return VariantToNodesArrays(d["ref_nodes"], d["var_nodes"])
    except (KeyError, ValueError, TypeError, AttributeError):
        from obgraph.variant_to_nodes import VariantToNodes    # the reference's loader (needs obgraph installed)
        return VariantToNodes.from_file(name)


class VariantToNodesArrays:
    def __init__(self, ref_nodes, var_nodes):
        self.ref_nodes = np.asarray(ref_nodes)
        self.var_nodes = np.asarray(var_nodes)

    def to_file(self, file_name):
        np.savez(file_name, ref_nodes=self.ref_nodes, var_nodes=self.var_nodes)


class LinearReference:
    """The linear path's nonzero-size nodes and their graph ref offsets (node_to_ref_offset), for the positional
    accessors of obgraph (unpinned)."""

    def __init__(self, arrays, graph):
        ntro = getattr(graph, "node_to_ref_offset", None)
        if ntro is None:
            ntro = arrays.node_to_ref_offset
        if ntro is None:
            raise ValueError("the graph has no node_to_ref_offset: ref offsets of the linear path are unknown")
        self.node_to_ref_offset = np.asarray(ntro).astype(np.int64)
        sel = (arrays.is_ref != 0) & (arrays.node_size > 0) & (arrays.exists != 0)
        nodes = np.nonzero(sel)[0]
        starts = self.node_to_ref_offset[nodes]
        o = np.argsort(starts, kind="stable")
        self.nodes = np.ascontiguousarray(nodes[o], dtype=np.int32)
        self.starts = np.ascontiguousarray(starts[o], dtype=np.int64)
        self.end = int((self.starts + arrays.node_size[self.nodes]).max()) if len(self.nodes) else 0
        self._sizes = arrays.node_size
        self.chromosome_start_nodes = dict(graph.chromosome_start_nodes)

    def chromosome_offset(self, chromosome):
        """convert_chromosome_ref_offset_to_graph_ref_offset(0, chromosome)."""
        d = self.chromosome_start_nodes
        for key in (chromosome, _as_int(chromosome), str(chromosome)):
            if key is not None and key in d:
                return int(self.node_to_ref_offset[int(d[key])])
        raise ValueError("chromosome %r is not among the graph's chromosome start nodes %s" % (chromosome, sorted(d)))

    def node_and_offset(self, ref_offsets):
        """Host form of gki_uvk_starts (for checks): (node, offset) at every graph ref offset, ValueError outside."""
        x = np.asarray(ref_offsets, dtype=np.int64)
        i = np.searchsorted(self.starts, x, side="right") - 1
        bad = (i < 0) | (x >= self.end)
        i = np.maximum(i, 0)
        nodes = self.nodes[i] if len(self.nodes) else np.zeros(len(x), np.int32)
        off = x - (self.starts[i] if len(self.nodes) else 0)
        bad |= off >= (self._sizes[nodes] if len(self.nodes) else 0)
        if np.any(bad):
            raise ValueError("ref offset %d lies outside the linear reference [0, %d)" % (int(x[bad][0]), self.end))
        return nodes.astype(np.int32), off.astype(np.int32)


def _as_int(x):
    try:
        return int(x)
    except (TypeError, ValueError):
        return None


def _graph_ref_offsets(lin, va, active):
    """Graph ref offset of POS of every active variant: its chromosome's start offset + POS."""
    chrom = va.chromosomes[active]
    uniq, inv = np.unique(chrom.astype(str), return_inverse=True) if chrom.dtype == object else \
        np.unique(chrom, return_inverse=True)
    first_of = np.zeros(len(uniq), np.int64)
    first_of[inv[::-1]] = np.arange(len(inv))[::-1]
    base = np.array([lin.chromosome_offset(chrom[i]) for i in first_of], dtype=np.int64)
    return np.ascontiguousarray(base[inv] + va.positions[active])


def _graph_on_device(arrays, position_id_index):
    """The graph in HBM with the position ids of `position_id_index` (None: the default ones): the package's cached upload
    when they are the default ones, otherwise a new upload."""
    if position_id_index is None:
        return DeviceGraph.of(arrays)
    n = arrays.n_nodes
    base = np.asarray(position_id_index.get(np.arange(n), np.zeros(n, dtype=np.int64))).astype(np.int64)
    return DeviceGraph.of(arrays) if np.array_equal(base, arrays.position_id_base()) else \
        DeviceGraph(arrays, position_base=base)


def _outside_linear_reference(va, src):
    return ValueError("variant %d (line %d, chromosome %s, POS %d): a start position lies before 0 or past the "
                      "linear reference (the reference's answer is undefined there)"
                      % (src, int(va.line_numbers[src]), va.chromosomes[src], int(va.positions[src])))


def choose_position(summaries, mask, lowest):
    """Rules 5-6 for one variant (host form of k_uvk_select): summaries = P gki_uvk_summary records, mask bit 0/1 = ref /
    alt stored.  Returns (chosen start, nodes of the chosen flat as a set of 'ref' / 'alt')."""
    P = len(summaries)
    best, best_score, first = P - 1, None, None
    for j in range(P):
        s = summaries[j]
        shared = (s["flags"] & 1) and (mask & 1) and ((mask & 2) or (s["flags"] & 2))
        if shared and j != P - 1:
            continue
        score = max(int(s["f_ref"]) if mask & 1 else 0, int(s["f_alt"]) if mask & 2 else 0)
        if first is None:
            first = j
        if best_score is None or score < best_score:
            best, best_score = j, score
        if score <= 1:
            break
    return best if lowest else first


class UniqueVariantKmersFinder:
    def __init__(self, graph, variant_to_nodes, variants, k=31, max_variant_nodes=6,
                 kmer_index_with_frequencies=None, haplotype_matrix=None, node_to_variants=None,
                 do_not_choose_lowest_frequency_kmers=False, use_dense_kmer_finder=False, position_id_index=None,
                 use_simple=False, chunk_size=None):
        """The reference's signature.  `variants`: objects with .position, .chromosome, .vcf_line_number, or a
        VariantArrays.  chunk_size (port only): `_nodes_found` restarts every chunk_size variants (counted with the
        skipped ones), as the CLI's one finder per `-c` chunk does; None = one chunk, as for one reference object."""
        if not use_dense_kmer_finder:
            raise NotImplementedError("only the dense path is supported: UniqueVariantKmersFinder(..., "
                                      "use_dense_kmer_finder=True, position_id_index=...) (SnpKmerFinder is not ported)")
        if use_simple:
            raise NotImplementedError("use_simple=True is not accepted by the constructor: simple selection is "
                                      "find_kmers_over_variants(graph, variant_to_nodes, variants, k, max_variant_nodes, "
                                      "position_id_index) of this module, and make_unique_variant_kmers -S True")
        if not isinstance(kmer_index_with_frequencies, (CollisionFreeKmerIndex, KmerCounter)):
            raise NotImplementedError("the frequency source must be graph_kmer_index_amd's CollisionFreeKmerIndex or "
                                      "KmerCounter (got %s); the reference's npstructures-backed KmerCounter is not "
                                      "supported" % type(kmer_index_with_frequencies).__name__)
        assert position_id_index is not None, "Position id index must be set when using dense kmer finder"
        self.graph = graph
        self.variant_to_nodes = variant_to_nodes
        self.variants = variants
        self.k = int(k)
        self._max_variant_nodes = int(max_variant_nodes)
        self._kmer_index_with_frequencies = kmer_index_with_frequencies
        self._position_id_index = position_id_index
        self._choose_kmers_with_lowest_frequencies = not do_not_choose_lowest_frequency_kmers
        self._chunk_size = chunk_size
        self._use_dense_kmer_finder = True
        self.n_failed_variants = 0
        self.last_serial_variants = 0
        self.last_timings = {}
        self.last_counts = {}
        self._dg = None

    # ------------------------------------------------------------------ inputs
    def _variant_arrays(self):
        v = self.variants
        return v if isinstance(v, VariantArrays) else VariantArrays.from_objects(v)

    def _device_graph(self, arrays):
        """The graph in HBM with the position ids of `position_id_index`: the package's cached upload when they are the
        default ones, otherwise an upload of this finder's own."""
        if self._dg is not None and self._dg[0] is arrays:
            return self._dg[1]
        dg = _graph_on_device(arrays, self._position_id_index)
        self._dg = (arrays, dg)
        return dg

    def _check_against_obgraph(self, lin, va, active, ref_offsets, d_nodes, d_offsets, P):
        """With obgraph's accessors on the graph object, a sample of starts must agree with them (the pattern of
        GraphArrays._first_disagreement)."""
        g = self.graph
        names = ("convert_chromosome_ref_offset_to_graph_ref_offset", "get_node_at_ref_offset",
                 "get_node_offset_at_ref_offset")
        if isinstance(g, GraphArrays) or not all(hasattr(g, n) for n in names) or len(active) == 0:
            return
        nodes, offsets = d_nodes.to_host(), d_offsets.to_host()
        rng = np.random.default_rng(len(active))
        sample = np.unique(np.concatenate([rng.integers(0, len(active) * P, size=min(len(active) * P, 2000)),
                                           [0, len(active) * P - 1]]))
        dist = start_distances(self.k)
        for i in sample.tolist():
            v, j = divmod(i, P)
            src = int(active[v])
            pos = int(va.positions[src]) - dist[j]
            x = int(g.convert_chromosome_ref_offset_to_graph_ref_offset(pos, va.chromosomes[src]))
            if x != int(ref_offsets[v]) - dist[j] or int(g.get_node_at_ref_offset(x)) != int(nodes[i]) or \
                    int(g.get_node_offset_at_ref_offset(x)) != int(offsets[i]):
                raise ValueError("start position %d of variant %d (line %d): the graph's accessors disagree with the "
                                 "positional assumptions of graph_kmer_index_amd (INTEGRATION.md)"
                                 % (j, src, int(va.line_numbers[src])))

    # ------------------------------------------------------------------ device path
    def find_unique_kmers_on_device(self):
        """find_unique_kmers() with the columns left in HBM: DeviceFlatKmers (uint64, uint32, uint64, float32)."""
        _lib.require_device()
        lib = _lib.load()
        t = {}
        t0 = time.perf_counter()
        dist = start_distances(self.k)
        if not dist:
            raise ValueError("k=%d leaves no start position per variant (range(2, k-2) is empty); the reference breaks "
                             "in FlatKmers.from_multiple_flat_kmers(None) there" % self.k)
        P = len(dist)
        arrays = GraphArrays.from_obgraph(self.graph)
        va = self._variant_arrays()
        ref_all = np.asarray(self.variant_to_nodes.ref_nodes)
        alt_all = np.asarray(self.variant_to_nodes.var_nodes)
        ref = ref_all[va.line_numbers].astype(np.int64) if len(va) else np.zeros(0, np.int64)
        alt = alt_all[va.line_numbers].astype(np.int64) if len(va) else np.zeros(0, np.int64)
        active = np.nonzero((ref != 0) & (alt != 0))[0]                     # :254-255
        n_var = len(active)
        self.n_failed_variants = 0
        self.last_serial_variants = 0
        if n_var == 0:
            self.last_timings, self.last_counts = {}, dict(variants=len(va), active=0, starts=0, records=0, chosen=0)
            return DeviceFlatKmers.allocate(0)
        ref, alt = np.ascontiguousarray(ref[active], np.int32), np.ascontiguousarray(alt[active], np.int32)
        lin = LinearReference(arrays, self.graph)
        ref_offsets = _graph_ref_offsets(lin, va, active)
        dg = self._device_graph(arrays)
        t["host_prepare"] = time.perf_counter() - t0

        def sync_time(name, t_start):
            _lib.check(lib.gki_device_synchronize())
            t[name] = time.perf_counter() - t_start

        with _lib.DeviceScope() as s:
            # 1. start positions
            t1 = time.perf_counter()
            h = lambda a: s.on_device(a, a.dtype)
            d_lin_start, d_lin_node, d_ro = h(lin.starts), h(lin.nodes), h(ref_offsets)
            n_pos = n_var * P
            d_nodes, d_offs, d_var = (s.array(n_pos, np.int32) for _ in range(3))
            bad = _lib._I64(-1)
            _lib.check(lib.gki_uvk_starts(dg.handle, d_lin_start.ptr, d_lin_node.ptr, len(lin.nodes), d_ro.ptr, n_var, P,
                                          d_nodes.ptr, d_offs.ptr, d_var.ptr, _lib.C.byref(bad)))
            sync_time("starts", t1)
            if bad.value >= 0:
                raise _outside_linear_reference(va, int(active[bad.value]))
            self._check_against_obgraph(lin, va, active, ref_offsets, d_nodes, d_offs, P)
            # 2. the forward search over all starts, no store filter
            t2 = time.perf_counter()
            d_rec = s.array(n_pos + 1, np.int64)
            n_rec = _lib._I64(0)
            args = (dg.handle, self.k, self._max_variant_nodes, 0, None, d_nodes.ptr, d_offs.ptr, n_pos)
            _lib.check(lib.gki_forward_count(*args, d_rec.ptr, _lib.C.byref(n_rec)))
            cols = [s.array(n_rec.value, d) for d in (np.int64, np.int32, np.int16, np.int32, np.float64)]
            if n_rec.value:
                _lib.check(lib.gki_forward_emit(*args, d_rec.ptr, *[c.ptr for c in cols]))
            sync_time("search", t2)
            d_hashes, d_snodes, d_soffs, d_rnodes, d_af = cols
            # 3. summaries with the fused frequency probe
            t3 = time.perf_counter()
            d_ref, d_alt = h(ref), h(alt)
            d_summ = s.array(n_pos * SUMMARY_DTYPE.itemsize, np.uint8)
            source = self._kmer_index_with_frequencies
            cols_and_nodes = (d_rec.ptr, n_var, P, d_hashes.ptr, d_snodes.ptr, d_soffs.ptr, d_rnodes.ptr, d_ref.ptr, d_alt.ptr,
                              d_summ.ptr)
            if isinstance(source, KmerCounter):              # the count of the hash alone: no reverse complement added
                _lib.check(lib.gki_uvk_summarize_counter(dg.handle, source._device_counter().handle, *cols_and_nodes))
            else:
                view = source._device_index().view()
                _lib.check(lib.gki_uvk_summarize(dg.handle, _lib.C.byref(view), *cols_and_nodes))
            t["summarize"] = time.perf_counter() - t3
            # 4. selection; variants sharing a node with another variant of their chunk resolved in order on the host
            t4 = time.perf_counter()
            mask = self._store_masks(active, ref, alt, d_summ, n_var, P)
            d_mask = None if mask is None else h(mask)
            d_choice = s.array(n_var, np.int32)
            d_out_start = s.array(n_var + 1, np.int64)
            n_out = _lib._I64(0)
            _lib.check(lib.gki_uvk_select(d_summ.ptr, n_var, P, int(self._choose_kmers_with_lowest_frequencies),
                                          None if d_mask is None else d_mask.ptr, d_choice.ptr, d_out_start.ptr,
                                          _lib.C.byref(n_out)))
            t["select"] = time.perf_counter() - t4
            # 5. gather
            t5 = time.perf_counter()
            out = s.keep(DeviceFlatKmers.allocate(n_out.value))
            out.n = n_out.value
            if n_out.value:
                _lib.check(lib.gki_uvk_emit(dg.handle, d_rec.ptr, n_var, P, d_choice.ptr,
                                            None if d_mask is None else d_mask.ptr, d_ref.ptr, d_alt.ptr, d_out_start.ptr,
                                            d_hashes.ptr, d_snodes.ptr, d_soffs.ptr, d_rnodes.ptr, d_af.ptr, out.hashes.ptr,
                                            out.nodes.ptr, out.ref_offsets.ptr, out.allele_frequencies.ptr))
            t["emit"] = time.perf_counter() - t5
            s.release(out)
        self.last_timings = t
        self.last_counts = dict(variants=len(va), active=n_var, starts=n_pos, search_records=int(n_rec.value),
                                chosen=int(n_out.value), serial=self.last_serial_variants)
        return out

    def _store_masks(self, active, ref, alt, d_summ, n_var, P):
        """uint8 store set per active variant (bit 0 ref, bit 1 alt), or None when every variant stores both: only
        variants that share a node with another variant of their chunk can lose one (`_nodes_found`, :156-158, :265-268);
        they are resolved here in variant order from their summaries."""
        chunk = active // self._chunk_size if self._chunk_size else np.zeros(n_var, np.int64)
        span = int(max(ref.max(), alt.max())) + 1
        key_ref = chunk * span + ref
        key_alt = chunk * span + alt
        keys = np.sort(np.concatenate([key_ref, key_alt[alt != ref]]))
        dup = np.unique(keys[1:][keys[1:] == keys[:-1]])       # a (chunk, node) held by two variants
        involved = np.nonzero(np.isin(key_ref, dup) | np.isin(key_alt, dup))[0] if len(dup) else dup
        self.last_serial_variants = len(involved)
        if len(involved) == 0:
            return None
        summ = d_summ.to_host().view(SUMMARY_DTYPE).reshape(n_var, P)
        mask = np.full(n_var, 3, dtype=np.uint8)
        found = set()                                   # (chunk, node) taken by an earlier variant
        lowest = self._choose_kmers_with_lowest_frequencies
        for v in involved.tolist():
            c, r, a = int(chunk[v]), int(ref[v]), int(alt[v])
            m = (0 if (c, r) in found else 1) | (0 if (a == r or (c, a) in found) else 2)
            mask[v] = m
            j = choose_position(summ[v], m, lowest)
            s = summ[v, j]
            if m & 1 and s["n_ref"]:
                found.add((c, r))
            if m & 2 and s["n_alt"]:
                found.add((c, a))
        return mask

    # ------------------------------------------------------------------ reference API
    def find_unique_kmers(self):
        """unique_variant_kmers.py:243-270: the chosen k-mers of every variant, in variant order (FlatKmers)."""
        t0 = time.perf_counter()
        with _lib.DeviceScope() as s:
            flat = s.keep(self.find_unique_kmers_on_device()).to_flat_kmers()
        self.last_timings["end_to_end"] = time.perf_counter() - t0
        logging.info("N variants with kmers found: %d" % self.last_counts.get("active", 0))
        return flat

    # ------------------------------------------------------------------ simple selection, one variant at a time
    def find_kmers_over_variant_node(self, variant, node):
        """unique_variant_kmers.py:66-98: the k-mers of one search for `node` of `variant` (FlatKmers)."""
        return self.find_kmers_over_variant(variant, node, None)

    def find_kmers_over_variant(self, variant, ref_node, variant_node):
        """unique_variant_kmers.py:107-111: the search for the ref node, then the one for the variant node (FlatKmers).
        Nodes are taken as given (the skip of node 0 belongs to the loop over all variants)."""
        va = VariantArrays([variant.position], np.array([variant.chromosome], dtype=object), [0],
                           [-1 if getattr(variant, "type", None) is None else int(variant.type == "SNP")])
        one = variant_node is None
        with _lib.DeviceScope() as s:
            return s.keep(_simple_selection(
                self.graph, va, np.array([ref_node], np.int64), np.array([ref_node if one else variant_node], np.int64),
                self.k, self._max_variant_nodes, self._position_id_index, n_searches=1 if one else 2,
                skip_zero_nodes=False)[0]).to_flat_kmers()


def _simple_selection(graph, va, ref_all, alt_all, k, max_variant_nodes, position_id_index, n_searches=None,
                      skip_zero_nodes=True):
    """The batch behind find_kmers_over_variants: (DeviceFlatKmers, facts).  ref_all / alt_all: the nodes of every variant
    of `va`.  n_searches: only the first so many of the 2 * active searches are run (the one-node call of the finder)."""
    t, t0 = {}, time.perf_counter()
    ref, alt = np.asarray(ref_all).astype(np.int64), np.asarray(alt_all).astype(np.int64)
    active = np.nonzero((ref != 0) & (alt != 0))[0] if skip_zero_nodes else np.arange(len(va))         # :254-255
    n_var = len(active)
    assert n_var == 0 or (va.is_snp is not None and not np.any(va.is_snp[active] < 0)), "Variant type must be set"  # :73
    _lib.require_device()
    lib = _lib.load()
    arrays = GraphArrays.from_obgraph(graph)
    facts = dict(variants=len(va), active=n_var, searches=0, records=0, timings=t)
    if n_var == 0:
        return DeviceFlatKmers.allocate(0), facts
    ref, alt = ref[active], alt[active]
    outside = np.nonzero((np.minimum(ref, alt) < 0) | (np.maximum(ref, alt) >= arrays.n_nodes))[0]
    if len(outside):
        src = int(active[outside[0]])
        raise ValueError("variant %d (line %d): node %d / %d is not a node of the graph (%d nodes)"
                         % (src, int(va.line_numbers[src]), int(ref[outside[0]]), int(alt[outside[0]]), arrays.n_nodes))
    ref, alt = np.ascontiguousarray(ref, np.int32), np.ascontiguousarray(alt, np.int32)
    is_snp = np.ascontiguousarray(va.is_snp[active] != 0, np.uint8)
    lin = LinearReference(arrays, graph)
    ref_offsets = _graph_ref_offsets(lin, va, active)
    dg = _graph_on_device(arrays, position_id_index)
    t["host_prepare"] = time.perf_counter() - t0
    with _lib.DeviceScope() as s:
        # 1. the start and the target of both searches of every variant
        t1 = time.perf_counter()
        h = lambda a: s.on_device(a, a.dtype)
        d_lin_start, d_lin_node, d_ro = h(lin.starts), h(lin.nodes), h(ref_offsets)
        d_snp, d_ref, d_alt = h(is_snp), h(ref), h(alt)
        n_pos = 2 * n_var
        d_nodes, d_offs, d_targets = (s.array(n_pos, np.int32) for _ in range(3))
        bad = _lib._I64(-1)
        _lib.check(lib.gki_uvk_simple_starts(dg.handle, d_lin_start.ptr, d_lin_node.ptr, len(lin.nodes), d_ro.ptr, d_snp.ptr,
                                             d_ref.ptr, d_alt.ptr, n_var, d_nodes.ptr, d_offs.ptr, d_targets.ptr,
                                             _lib.C.byref(bad)))
        t["starts"] = time.perf_counter() - t1
        if bad.value >= 0:
            raise _outside_linear_reference(va, int(active[bad.value]))
        if n_searches is not None:
            n_pos = min(n_pos, int(n_searches))
        # 2. the per-node search: count, then the FlatKmers columns straight from the walk
        t2 = time.perf_counter()
        d_rec = s.array(n_pos + 1, np.int64)
        n_rec = _lib._I64(0)
        args = (dg.handle, int(k), int(max_variant_nodes), d_targets.ptr, d_nodes.ptr, d_offs.ptr, n_pos, d_rec.ptr)
        _lib.check(lib.gki_forward_node_count(*args, _lib.C.byref(n_rec)))
        t["count"] = time.perf_counter() - t2
        t3 = time.perf_counter()
        out = s.keep(DeviceFlatKmers.allocate(n_rec.value))
        if n_rec.value:
            _lib.check(lib.gki_forward_node_emit(*args, out.hashes.ptr, out.nodes.ptr, out.ref_offsets.ptr,
                                                 out.allele_frequencies.ptr))
        t["emit"] = time.perf_counter() - t3
        s.release(out)
    facts.update(searches=n_pos, records=int(n_rec.value))
    return out, facts


def find_kmers_over_variants_on_device(graph, variant_to_nodes, variants, k=31, max_variant_nodes=6, position_id_index=None):
    """find_kmers_over_variants with the columns left in HBM: DeviceFlatKmers (uint64, uint32, uint64, float32)."""
    va = variants if isinstance(variants, VariantArrays) else VariantArrays.from_objects(variants)
    ref_all, alt_all = np.asarray(variant_to_nodes.ref_nodes), np.asarray(variant_to_nodes.var_nodes)
    lines = va.line_numbers
    out, _ = _simple_selection(graph, va, ref_all[lines] if len(va) else np.zeros(0, np.int64),
                               alt_all[lines] if len(va) else np.zeros(0, np.int64), k, max_variant_nodes, position_id_index)
    return out


def find_kmers_over_variants(graph, variant_to_nodes, variants, k=31, max_variant_nodes=6, position_id_index=None):
    """What the reference's UniqueVariantKmersFinder(..., use_simple=True).find_unique_kmers() returns
    (unique_variant_kmers.py:66-111, 241-269): for every variant in order (skipped when its ref or alt node is 0) the
    k-mers of the search for its ref node, then of the search for its alt node -- FlatKmers, hash / node / position id of
    the k-mer's end / minimum allele frequency of its path.  position_id_index None: the graph's default position ids
    (PositionId.from_graph).  One device batch; no frequency source."""
    with _lib.DeviceScope() as s:
        return s.keep(find_kmers_over_variants_on_device(graph, variant_to_nodes, variants, k, max_variant_nodes,
                                                         position_id_index)).to_flat_kmers()
