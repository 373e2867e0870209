"""Sample haplotypes spelled through the graph on the device: a slot's sequence, the variant nodes every slot carries,
and the node hit counts of a slot's k-mers.

`graph_files.build_graph` gives a graph and, per VCF data line, its two allele nodes; `vcf_files.haplotype_matrix_from_file`
gives, for the same data lines, which allele every sample haplotype carries.  `HaplotypePaths` joins the two.  The rules
are stated in include/gki.h ("haplotype paths") and DESIGN.md 4.19; the kernels are csrc/gki_haplotype_paths.hip.

The graph must be a bubble chain (`bubble_chain_plan` checks it on the host, once per graph): node ids then ascend along
every path and a kept line's two allele nodes lie side by side in `seq`, so a haplotype's sequence is `seq` with one allele
node per kept line cut out -- an output-dense gather.  `.sequence(slot)` returns a `fasta_files.DeviceReference`, so
`linear_kmers_on_device`, `ReferenceKmerIndex` and the graph build's `records` take a haplotype where they take a reference;
`.node_counts` composes the spelling with `linear_kmers_on_device` and `DeviceIndex.count_nodes`.

`.node_counts_by_difference` gives the same rows without probing what a slot shares with the linear reference, and
`.node_count_model` sums them per sampled individual into a `NodeCountModel` (the kernels are
csrc/gki_haplotype_counts.hip and k_probe_segments of csrc/gki_probe.hip).
"""
import collections
import ctypes as C
import time

import numpy as np

from . import _lib
from .collision_free_kmer_index import zeroed_counts
from .fasta_files import DeviceReference
from .vcf_files import haplotype_planes_on_device

# An alt plane that is on the device already, in place of a HaplotypeMatrix: `alt_bits` a uint64 DeviceArray
# [n_slots][ceil(n_variants / 64)] as gki_haplotype_planes lays it out.  It stays its owner's.
AltPlane = collections.namedtuple("AltPlane", "alt_bits n_variants n_slots")


def bubble_chain_plan(graph, variant_to_nodes):
    """The host arrays of gki_haplotype_paths_create for `graph` and `variant_to_nodes`, as a dict, after the bubble-chain
    check: ValueError naming the first line or node at fault.  NumPy only; no device."""
    ref_nodes = np.asarray(variant_to_nodes.ref_nodes).astype(np.int64)
    var_nodes = np.asarray(variant_to_nodes.var_nodes).astype(np.int64)
    if len(ref_nodes) != len(var_nodes):
        raise ValueError("variant-to-nodes has %d ref nodes and %d var nodes" % (len(ref_nodes), len(var_nodes)))
    n_lines, n_nodes = len(var_nodes), graph.n_nodes
    kept_line = np.flatnonzero(var_nodes != 0)
    ref, var = ref_nodes[kept_line], var_nodes[kept_line]

    def first_bad(bad, what):
        if np.any(bad):
            j = int(np.argmax(bad))
            raise ValueError("not a bubble chain: data line %d (ref node %d, var node %d) %s"
                             % (kept_line[j], ref[j], var[j], what))
    first_bad((ref < 0) | (var >= n_nodes), "names a node outside the graph")
    first_bad(var != ref + 1, "does not have var_nodes == ref_nodes + 1")
    first_bad(np.concatenate([[False], np.diff(ref) <= 0]), "does not ascend: its ref node is not above the line's before")
    starts = np.array([graph.chromosome_start_nodes[c] for c in sorted(graph.chromosome_start_nodes)], dtype=np.int64)
    if len(starts) < 1 or np.any(np.diff(starts) <= 0) or starts[0] < 0 or starts[-1] >= max(n_nodes, 1):
        raise ValueError("not a bubble chain: the chromosome start nodes %s do not ascend inside the graph" % starts.tolist())
    first_bad(ref < starts[0], "lies in front of the first chromosome's start node")
    plain = np.ones(n_nodes, dtype=bool)
    plain[ref], plain[var] = False, False
    bad_nodes = plain & (graph.exists != 0) & (graph.is_ref == 0)
    if np.any(bad_nodes):
        raise ValueError("not a bubble chain: node %d is no allele node of a kept line and is not on the linear reference"
                         % int(np.argmax(bad_nodes)))
    kept_bits = np.zeros((n_lines + 63) // 64, dtype=np.uint64)
    np.bitwise_or.at(kept_bits, kept_line >> 6, np.uint64(1) << (kept_line & 63).astype(np.uint64))
    seq_start, node_size = graph.seq_start, graph.node_size
    return {"seq": np.ascontiguousarray(graph.seq, dtype=np.uint8), "n_lines": n_lines,
            "var_nodes": np.ascontiguousarray(var_nodes, dtype=np.uint32), "kept_bits": kept_bits,
            "kept_line": np.ascontiguousarray(kept_line, dtype=np.int64),
            "ref_start": np.ascontiguousarray(seq_start[ref], dtype=np.int64),
            "ref_size": np.ascontiguousarray(node_size[ref], dtype=np.int32),
            "alt_start": np.ascontiguousarray(seq_start[var], dtype=np.int64),
            "alt_size": np.ascontiguousarray(node_size[var], dtype=np.int32),
            "chrom_seq_start": np.ascontiguousarray(np.append(seq_start[starts], seq_start[-1]), dtype=np.int64),
            "chrom_first_kept": np.ascontiguousarray(np.append(np.searchsorted(ref, starts, side="left"), len(ref)),
                                                     dtype=np.int64)}


def check_slot(slot, n_slots):
    """`slot` as an int; IndexError outside 0 .. n_slots - 1."""
    if not 0 <= int(slot) < n_slots:
        raise IndexError("haplotype slot %d is outside 0 .. %d" % (int(slot), n_slots - 1))
    return int(slot)


def nodes_of_index(index, n_nodes):
    """The `n_nodes` default of the count routes: the index's highest node + 1."""
    return int(index.max_node_id()) + 1 if n_nodes is None else n_nodes


def strands_of(include_reverse_complement):
    """The `strands` of the segment probe: 3 both strands, 1 forward only."""
    return 3 if include_reverse_complement else 1


def kmer_passes(bounds, k, chunk_kmers):
    """The k-mers of every record [bounds[c], bounds[c + 1]) as passes of (seg_first, seg_count) lists, each pass of at
    most `chunk_kmers` k-mers: no k-mer crosses a record's end, a record shorter than k has none, and a pass may end
    anywhere inside a record."""
    if chunk_kmers < 1:
        raise ValueError("chunk_kmers must be at least 1")
    passes, first, count, room = [], [], [], chunk_kmers
    for a, b in zip(bounds[:-1], bounds[1:]):
        at, left = int(a), int(b) - int(a) - k + 1
        while left > 0:
            n = min(left, room)
            first.append(at), count.append(n)
            at, left, room = at + n, left - n, room - n
            if room == 0:
                passes.append((first, count))
                first, count, room = [], [], chunk_kmers
    if first:
        passes.append((first, count))
    return passes


def whole_segments(bounds, k, windows=4096):
    """All windows of every record [bounds[c], bounds[c + 1]) as segments of at most `windows` windows, in order: (start
    int64[], windows int64[]).  A record shorter than k has none.  A loop over the records, not over their letters."""
    starts, counts = [], []
    for a, b in zip(bounds[:-1], bounds[1:]):
        n = int(b) - int(a) - k + 1
        if n > 0:
            first = np.arange(int(a), int(a) + n, windows, dtype=np.int64)
            starts.append(first)
            counts.append(np.minimum(int(a) + n - first, windows))
    if not starts:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(starts), np.concatenate(counts).astype(np.int64)


class NodeCountModel:
    """Per data line, allele (0 the ref node, 1 the var node) and number of copies of that allele an individual carries
    (0 .. ploidy): how the node's count is spread over the sampled individuals.  `histogram` uint32[V][2][ploidy + 1][n_bins]
    counts the individuals by min(count, n_bins - 1), `count_sum` uint64[V][2][ploidy + 1] sums their counts.  Lines that
    are not kept are all zero.  `samples` are the individuals that went in, in the order given."""

    def __init__(self, histogram, count_sum, k, ploidy, n_bins, samples):
        self.k, self.ploidy, self.n_bins = int(k), int(ploidy), int(n_bins)
        histogram, count_sum = np.asarray(histogram), np.asarray(count_sum)
        per_line = 2 * (self.ploidy + 1)
        self.histogram = np.ascontiguousarray(histogram, dtype=np.uint32).reshape(
            histogram.size // (per_line * self.n_bins), 2, self.ploidy + 1, self.n_bins)
        self.count_sum = np.ascontiguousarray(count_sum, dtype=np.uint64).reshape(
            count_sum.size // per_line, 2, self.ploidy + 1)
        self.samples = np.ascontiguousarray(samples, dtype=np.int64)
        if len(self.histogram) != len(self.count_sum):
            raise ValueError("the histogram has %d lines, count_sum has %d" % (len(self.histogram), len(self.count_sum)))

    def mean(self):
        """float64[V][2][ploidy + 1]: count_sum over the individuals of the entry, NaN where there is none."""
        n = self.histogram.sum(axis=3, dtype=np.int64)
        out = np.full(n.shape, np.nan)
        np.divide(self.count_sum, n, out=out, where=n > 0)
        return out

    def to_file(self, file_name):
        """np.savez with keys named after the attributes."""
        np.savez(file_name, histogram=self.histogram, count_sum=self.count_sum, k=np.int64(self.k),
                 ploidy=np.int64(self.ploidy), n_bins=np.int64(self.n_bins), samples=self.samples)

    @classmethod
    def from_file(cls, file_name):
        file_name = str(file_name)
        d = np.load(file_name if file_name.endswith(".npz") else file_name + ".npz")
        return cls(d["histogram"], d["count_sum"], int(d["k"]), int(d["ploidy"]), int(d["n_bins"]), d["samples"])


class HaplotypeToNodes:
    """The variant nodes every haplotype slot carries: slot h's are nodes[start[h]:start[h + 1]], in line order (`start`
    int64[H + 1], `nodes` uint32).  Valid only with the graph and variant-to-nodes it was made from; slots are numbered
    as in `vcf_files.HaplotypeMatrix` (sample s has slots s * ploidy .. s * ploidy + ploidy - 1)."""

    def __init__(self, start, nodes, n_samples=None, ploidy=None, sample_names=None):
        self.start = np.ascontiguousarray(start, dtype=np.int64)
        self.nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        self.n_samples = None if n_samples is None else int(n_samples)
        self.ploidy = None if ploidy is None else int(ploidy)
        self.sample_names = None if sample_names is None else [str(n) for n in sample_names]

    @property
    def n_slots(self):
        return len(self.start) - 1

    def nodes_of(self, h):
        h = check_slot(h, self.n_slots)
        return self.nodes[self.start[h]:self.start[h + 1]]

    def to_file(self, file_name):
        """np.savez with keys named after the attributes; those that are None are left out."""
        arrays = {"start": self.start, "nodes": self.nodes}
        if self.n_samples is not None:
            arrays["n_samples"] = np.int64(self.n_samples)
        if self.ploidy is not None:
            arrays["ploidy"] = np.int64(self.ploidy)
        if self.sample_names is not None:
            arrays["sample_names"] = np.array(self.sample_names, dtype=np.str_)
        np.savez(file_name, **arrays)

    @classmethod
    def from_file(cls, file_name):
        file_name = str(file_name)
        d = np.load(file_name if file_name.endswith(".npz") else file_name + ".npz")
        return cls(d["start"], d["nodes"], int(d["n_samples"]) if "n_samples" in d.files else None,
                   int(d["ploidy"]) if "ploidy" in d.files else None,
                   d["sample_names"].tolist() if "sample_names" in d.files else None)


class HaplotypePaths:
    """The plan of one graph (gki_haplotype_paths_create) and the alt plane of `matrix` on the device.  `matrix` is a
    `vcf_files.HaplotypeMatrix` or an `AltPlane`.  A context manager; `close()` frees everything it holds."""

    def __init__(self, graph, variant_to_nodes, matrix):
        self._plan, self._alt_bits, self._owns_plane = None, None, False
        self._ref_path, self._base_rows = None, {}         # the all-ref path's (letters, bounds); key -> (device index, base row)
        n_lines = len(np.asarray(variant_to_nodes.var_nodes))
        if isinstance(matrix, AltPlane):
            n_variants, self.n_slots = int(matrix.n_variants), int(matrix.n_slots)
            if matrix.alt_bits.n < self.n_slots * ((n_variants + 63) // 64):
                raise ValueError("the alt plane holds %d words, %d slots of %d lines need more" % (matrix.alt_bits.n, self.n_slots, n_variants))
            self.n_samples = self.ploidy = self.sample_names = None
        else:
            n_variants, self.n_slots = matrix.n_variants, matrix.n_samples * matrix.ploidy
            self.n_samples, self.ploidy, self.sample_names = matrix.n_samples, matrix.ploidy, matrix.sample_names
        if n_variants != n_lines:
            raise ValueError("the haplotype matrix has %d data lines, variant-to-nodes has %d" % (n_variants, n_lines))
        a = bubble_chain_plan(graph, variant_to_nodes)
        self.n_lines, self.n_chromosomes = n_lines, len(a["chrom_seq_start"]) - 1
        _lib.require_device()
        with _lib.DeviceScope() as s:
            if isinstance(matrix, AltPlane):
                alt_bits = matrix.alt_bits
            elif n_lines == 0 or self.n_slots == 0:
                alt_bits = s.array(1, np.uint64)
                alt_bits.zero()
            else:
                codes = s.on_device(matrix.codes.reshape(-1), np.uint8)
                ref_bits, alt_bits, _ = haplotype_planes_on_device(s, codes, n_lines, self.n_slots)
                ref_bits.free()
                codes.free()
            plan = C.c_void_p()
            _lib.check(_lib.load().gki_haplotype_paths_create(
                _lib.hptr(a["seq"]), len(a["seq"]), n_lines, _lib.hptr(a["var_nodes"]), _lib.hptr(a["kept_bits"]),
                len(a["kept_line"]), _lib.hptr(a["kept_line"]), _lib.hptr(a["ref_start"]), _lib.hptr(a["ref_size"]),
                _lib.hptr(a["alt_start"]), _lib.hptr(a["alt_size"]), self.n_chromosomes, _lib.hptr(a["chrom_seq_start"]),
                _lib.hptr(a["chrom_first_kept"]), C.byref(plan)))
            self._plan = plan
            self._owns_plane = not isinstance(matrix, AltPlane)
            self._alt_bits = s.release(alt_bits) if self._owns_plane else alt_bits

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
        if self._plan is not None:
            plan, self._plan = self._plan, None
            _lib.load().gki_haplotype_paths_destroy(plan)
        if self._alt_bits is not None:
            if self._owns_plane:
                self._alt_bits.free()
            self._alt_bits = None
        if self._ref_path is not None:
            self._ref_path[0].free()
            self._ref_path = None
        while self._base_rows:
            self._base_rows.popitem()[1][1].free()

    def _open(self):
        if self._plan is None:
            raise ValueError("the HaplotypePaths is closed")
        return _lib.load()

    def _slots(self, slots):
        """`slots` as ints on an open plan; IndexError for one outside 0 .. H - 1."""
        self._open()
        return [check_slot(h, self.n_slots) for h in slots]

    def _spell(self, plane, n_slots, slot):
        """Slot `slot` of `plane` spelled: (letters, which the caller frees, bounds, count ms, spell ms)."""
        lib = self._open()
        n_out, ms_count, ms_spell = C.c_int64(0), C.c_float(0), C.c_float(0)
        bounds = np.zeros(self.n_chromosomes + 1, dtype=np.int64)
        _lib.check(lib.gki_haplotype_spell_count(self._plan, plane.ptr, n_slots, slot, C.byref(n_out),
                                                 _lib.hptr(bounds), C.byref(ms_count)))
        with _lib.DeviceScope() as s:
            letters = s.array(max(n_out.value, 1), np.uint8)
            letters.n = n_out.value
            _lib.check(lib.gki_haplotype_spell_emit(self._plan, letters.ptr, C.byref(ms_spell)))
            s.release(letters)
        return letters, bounds, float(ms_count.value), float(ms_spell.value)

    def sequence(self, slot):
        """Slot `slot`'s sequence as a DeviceReference: `.letters` upper-case ACGT, record c (named str(c + 1)) the
        haplotype's chromosome c.  `.timings` holds the count pass' and the spelling kernel's device time in ms.  The
        caller frees it.  IndexError for a slot outside 0 .. H - 1."""
        slot, = self._slots([slot])
        letters, bounds, ms_count, ms_spell = self._spell(self._alt_bits, self.n_slots, slot)
        names = [str(c + 1) for c in range(self.n_chromosomes)]
        return DeviceReference(names, bounds, letters, list(names), {"count_kernel_ms": ms_count, "spell_kernel_ms": ms_spell})

    def alt_nodes(self, kernel_ms=None):
        """The alt nodes of all slots as a HaplotypeToNodes.  kernel_ms: a list that receives (count ms, emit ms)."""
        lib = self._open()
        n_nodes, ms_count, ms_emit = C.c_int64(0), C.c_float(0), C.c_float(0)
        with _lib.DeviceScope() as s:
            start = s.array(self.n_slots + 1, np.int64)
            _lib.check(lib.gki_haplotype_alt_nodes_count(self._plan, self._alt_bits.ptr, self.n_slots, start.ptr,
                                                         C.byref(n_nodes), C.byref(ms_count)))
            nodes = s.array(max(n_nodes.value, 1), np.uint32)
            _lib.check(lib.gki_haplotype_alt_nodes_emit(self._plan, self._alt_bits.ptr, self.n_slots, nodes.ptr,
                                                        C.byref(ms_emit)))
            if kernel_ms is not None:
                kernel_ms[:] = [float(ms_count.value), float(ms_emit.value)]
            return HaplotypeToNodes(start.to_host(), nodes.to_host(n_nodes.value), self.n_samples, self.ploidy,
                                    self.sample_names)

    def node_counts(self, slots, index, k, n_nodes=None, include_reverse_complement=True, chunk_kmers=1 << 28, timings=None):
        """uint32[len(slots), n_nodes] on the host: row i holds the node hit counts of all k-mers of slot slots[i]'s
        sequence (none across a chromosome boundary) and, by default, of their reverse complements -- what
        `index.map_reads([one string per chromosome], k, n_nodes)` gives for that haplotype.  `index` is a
        CollisionFreeKmerIndex; n_nodes None: index.max_node_id() + 1.  Per slot: spell, then passes of at most
        `chunk_kmers` k-mers through `linear_kmers_on_device` and `DeviceIndex.count_nodes`.
        timings: a list that receives one dict per slot (seconds per stage, synchronised)."""
        from .snp_kmer_finder import linear_kmers_on_device
        slots, n_nodes = self._slots(slots), nodes_of_index(index, n_nodes)
        device_index = index._device_index()
        out = np.zeros((len(slots), int(n_nodes)), dtype=np.uint32)
        for i, slot in enumerate(slots):
            with _lib.DeviceScope() as s:
                t0 = time.perf_counter()
                ref = s.keep(self.sequence(slot))
                t1 = time.perf_counter()
                row = zeroed_counts(s, n_nodes)
                hash_s = probe_s = 0.0
                for seg_first, seg_count in kmer_passes(ref.bounds, k, chunk_kmers):
                    with _lib.DeviceScope() as p:
                        t2 = time.perf_counter()
                        hashes, _ = linear_kmers_on_device(ref.letters, k, 1, seg_first, seg_count,
                                                           with_reverse_complement=include_reverse_complement,
                                                           hashes_only=True)
                        p.keep(hashes)
                        _lib.check(_lib.load().gki_device_synchronize())
                        t3 = time.perf_counter()
                        device_index.count_nodes(hashes, n_nodes, max_hits=2 ** 62, counts=row)
                        _lib.check(_lib.load().gki_device_synchronize())
                        hash_s, probe_s = hash_s + t3 - t2, probe_s + time.perf_counter() - t3
                out[i] = row.to_host(int(n_nodes))
                if timings is not None:
                    timings.append({"slot": slot, "letters": ref.letters.n, "spell_s": t1 - t0, "hash_s": hash_s,
                                    "probe_s": probe_s, "total_s": time.perf_counter() - t0, **ref.timings})
        return out

    # ------------------------------------------------------------------ counts by difference from the all-ref path
    def _reference_path(self):
        """(letters, bounds) of the all-ref path -- a slot whose plane is all zero -- spelled once and kept."""
        self._open()
        if self._ref_path is None:
            with _lib.DeviceScope() as s:
                zero = s.array(max((self.n_lines + 63) // 64, 1), np.uint64)
                zero.zero()
                letters, bounds, _, _ = self._spell(zero, 1, 0)
            self._ref_path = (letters, bounds)
        return self._ref_path

    def _base_row(self, index, k, n_nodes, strands):
        """The all-ref path's node counts as a uint32 DeviceArray, made once per (index, k, n_nodes, strands) and kept.
        The key is the index's DeviceIndex, which the entry holds on to: an index that drops its device copy and makes
        another (remove_frequencies and the like) gets a new base row, never the stale one."""
        self._open()
        device_index = index._device_index()
        key = (id(device_index), int(k), int(n_nodes), int(strands))
        if key not in self._base_rows:
            letters, bounds = self._reference_path()
            start, windows = whole_segments(bounds, k)
            with _lib.DeviceScope() as s:
                row = zeroed_counts(s, n_nodes)
                device_index.count_nodes_from_segments(letters, start, windows, k, row, n_nodes, strands)
                self._base_rows[key] = (device_index, s.release(row))
        return self._base_rows[key][1]

    def reference_node_counts(self, index, k, n_nodes=None, include_reverse_complement=True):
        """uint32[n_nodes] on the host: the node hit counts of the all-ref path, what `node_counts` gives for a slot that
        takes no alt allele.  The path's letters and this row stay on the device until close(), for
        `node_counts_by_difference` and `node_count_model` to start from."""
        n_nodes = nodes_of_index(index, n_nodes)
        return self._base_row(index, k, n_nodes, strands_of(include_reverse_complement)).to_host(int(n_nodes))

    def _list_segments(self, s, slot, k):
        """Slot `slot` spelled, which leaves its path in the plan, and its segments listed, all owned by `s`: (the sequence,
        [ref start, ref windows, slot start, slot windows], the five totals, kernel ms, the host clock at the three stages)."""
        lib = self._open()
        t0 = time.perf_counter()
        seq = s.keep(self.sequence(slot))
        t1 = time.perf_counter()
        totals = [C.c_int64(0) for _ in range(5)]
        ms_count, ms_emit = C.c_float(0), C.c_float(0)
        _lib.check(lib.gki_haplotype_segments_count(self._plan, self._alt_bits.ptr, self.n_slots, slot, int(k),
                                                    *[C.byref(t) for t in totals], C.byref(ms_count)))
        totals = [t.value for t in totals]
        arrays = [s.array(max(n, 1), np.int64) for n in (totals[1], totals[1], totals[3], totals[3])]
        _lib.check(lib.gki_haplotype_segments_emit(self._plan, *[a.ptr for a in arrays], C.byref(ms_emit)))
        return seq, arrays, totals, float(ms_count.value) + float(ms_emit.value), (t0, t1, time.perf_counter())

    def _apply_slot(self, slot, row, device_index, k, n_nodes, strands):
        """row += counts(slot) - counts(all-ref path), by the two segment passes; returns the slot's timing dict."""
        ref_letters, _ = self._reference_path()
        with _lib.DeviceScope() as s:
            seq, (ref_start, ref_n, slot_start, slot_n), totals, kernel_ms, (t0, t1, t2) = self._list_segments(s, slot, k)
            n_taken, n_ref, ref_windows, n_slot, slot_windows = totals
            device_index.count_nodes_from_segments(ref_letters, ref_start, ref_n, k, row, n_nodes, strands, sign=-1,
                                                   n_segs=n_ref)
            t3 = time.perf_counter()
            device_index.count_nodes_from_segments(seq.letters, slot_start, slot_n, k, row, n_nodes, strands, sign=1,
                                                   n_segs=n_slot)
            t4 = time.perf_counter()
            return {"slot": slot, "letters": seq.letters.n, "taken_lines": n_taken, "ref_segments": n_ref,
                    "ref_windows": ref_windows, "slot_segments": n_slot, "slot_windows": slot_windows,
                    "spell_s": t1 - t0, "segments_s": t2 - t1, "subtract_s": t3 - t2, "add_s": t4 - t3, "total_s": t4 - t0,
                    "segments_kernel_ms": kernel_ms, **seq.timings}

    def segments(self, slot, k):
        """The segments of slot `slot` read back: ((start, windows) in the all-ref path, (start, windows)
        in the slot's sequence), int64 arrays.  For inspection and tests; the count routes keep them on the device."""
        with _lib.DeviceScope() as s:
            _, arrays, totals, _, _ = self._list_segments(s, slot, k)
            out = [a.to_host(n) for a, n in zip(arrays, (totals[1], totals[1], totals[3], totals[3]))]
        return (out[0], out[1]), (out[2], out[3])

    def node_counts_by_difference(self, slots, index, k, n_nodes=None, include_reverse_complement=True, timings=None):
        """What `node_counts` returns, by another route: counts(slot) = counts(all-ref path) - counts(the all-ref path's
        segments) + counts(the slot's segments), the segments being the windows that touch an allele the slot replaces or
        takes.  Per slot: spell, list the segments, copy the base row, one signed probe pass over each segment list.
        timings: a list that receives one dict per slot (seconds per stage, synchronised, and the windows probed)."""
        slots, n_nodes, strands = self._slots(slots), nodes_of_index(index, n_nodes), strands_of(include_reverse_complement)
        device_index = index._device_index()
        base = self._base_row(index, k, n_nodes, strands)
        out = np.zeros((len(slots), int(n_nodes)), dtype=np.uint32)
        for i, slot in enumerate(slots):
            with _lib.DeviceScope() as s:
                row = s.array(base.n, np.uint32)
                _lib.check(_lib.load().gki_memcpy_d2d(row.ptr, base.ptr, base.nbytes))
                t = self._apply_slot(slot, row, device_index, k, n_nodes, strands)
                out[i] = row.to_host(int(n_nodes))
                if timings is not None:
                    timings.append(t)
        return out

    def node_count_model(self, index, k, samples=None, n_bins=5, n_nodes=None, include_reverse_complement=True,
                         route="difference", ploidy=None, timings=None):
        """The NodeCountModel of the individuals `samples` (default: all): sample s owns the slots s * ploidy ..
        s * ploidy + ploidy - 1 and its row is the sum of its slots' node counts.  route "difference" starts every row from
        ploidy x the base row and applies each slot's two segment passes; "whole" sums `node_counts` rows instead, for
        comparison.  With an AltPlane the caller passes `ploidy`.  ValueError for n_bins < 2, IndexError for a sample
        outside the matrix.  timings: a list that receives one dict per slot of the difference route."""
        lib = self._open()
        if self.ploidy is not None and ploidy is not None and int(ploidy) != self.ploidy:
            raise ValueError("ploidy %d was given, the matrix has %d" % (int(ploidy), self.ploidy))
        ploidy = self.ploidy if self.ploidy is not None else ploidy
        if ploidy is None:
            raise ValueError("an AltPlane has no ploidy: pass ploidy=")
        ploidy = int(ploidy)
        if not 1 <= ploidy <= 8:
            raise ValueError("ploidy must be in 1..8")
        if int(n_bins) < 2:
            raise ValueError("n_bins must be at least 2")
        if route not in ("difference", "whole"):
            raise ValueError("route must be 'difference' or 'whole'")
        n_samples, n_bins = self.n_slots // ploidy, int(n_bins)
        samples = list(range(n_samples)) if samples is None else [int(x) for x in samples]
        for x in samples:
            if not 0 <= x < n_samples:
                raise IndexError("sample %d is outside 0 .. %d" % (x, n_samples - 1))
        n_nodes, strands = nodes_of_index(index, n_nodes), strands_of(include_reverse_complement)
        entries = self.n_lines * 2 * (ploidy + 1)
        with _lib.DeviceScope() as s:
            histogram, count_sum = s.array(max(entries * n_bins, 1), np.uint32), s.array(max(entries, 1), np.uint64)
            histogram.zero(), count_sum.zero()
            row = s.array(max(int(n_nodes), 1), np.uint32)
            if route == "difference":
                device_index = index._device_index()
                base = self._base_row(index, k, n_nodes, strands)
            for x in samples:
                slots = range(x * ploidy, x * ploidy + ploidy)
                if route == "difference":
                    _lib.check(lib.gki_node_count_model_row_start(base.ptr, int(n_nodes), ploidy, row.ptr))
                    for slot in slots:
                        t = self._apply_slot(slot, row, device_index, k, n_nodes, strands)
                        if timings is not None:
                            timings.append(t)
                else:
                    whole = self.node_counts(list(slots), index, k, n_nodes, include_reverse_complement)
                    host = np.zeros(row.n, dtype=np.uint32)
                    host[:int(n_nodes)] = whole.sum(axis=0, dtype=np.uint32)
                    _lib.check(lib.gki_memcpy_h2d(row.ptr, _lib.hptr(host), host.nbytes))
                _lib.check(lib.gki_node_count_model_accumulate(self._plan, self._alt_bits.ptr, self.n_slots, x * ploidy, ploidy,
                                                               row.ptr, int(n_nodes), n_bins, histogram.ptr, count_sum.ptr,
                                                               None))
            return NodeCountModel(histogram.to_host(entries * n_bins), count_sum.to_host(entries), k, ploidy, n_bins, samples)


def write_fasta(file_name, names, records, width=60):
    """Host FASTA writer: record i as '>' + names[i] and its letters (uint8 arrays) in lines of `width`."""
    with open(file_name, "wb") as f:
        for name, letters in zip(names, records):
            f.write(b">" + str(name).encode() + b"\n")
            n = len(letters)
            if n:
                # the letters with a line end behind every `width` of them and behind the last
                lines = -(-n // width)
                out = np.full(n + lines, ord("\n"), dtype=np.uint8)
                at = np.arange(n)
                out[at + at // width] = letters
                f.write(out.tobytes())
