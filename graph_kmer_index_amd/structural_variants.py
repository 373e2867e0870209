"""sample_kmers_from_structural_variants with the reference's signature (structural_variants.py:6-43), on MI355X.

For every (ref_node, var_node) pair of `variant_to_nodes`, ref first, a node longer than k + 5 bases gives the k-mers of
its own sequence (windows 0 .. size - k) whose `kmer_index_with_frequencies.get_frequency` (a CollisionFreeKmerIndex: the
k-mer plus its 31-mer reverse complement; a KmerCounter: the k-mer alone) is below `max_frequency`,
thinned from the left so that two chosen windows never overlap; every chosen window is one record (hash, node, 0).  A
node listed twice gives its records twice.  The reference asks get_frequency once per base of every big node; here all
windows of all nodes are one device batch (csrc/gki_sv_kmers.hip, include/gki.h gki_sv_sample_*): a probe pass that
leaves one valid bit per window, and a greedy pass over the bits, run once to count and once to emit.
"""
import time

import numpy as np

from . import _lib
from .collision_free_kmer_index import CollisionFreeKmerIndex
from .device_graph import DeviceGraph
from .flat_kmers import DeviceFlatKmers, FlatKmers
from .graph import GraphArrays
from .kmer_counter import KmerCounter

last_timings = {}          # of the latest call: seconds per stage, kernel milliseconds per pass
last_counts = {}


def candidate_nodes(variant_to_nodes):
    """The nodes in visiting order: every (ref_node, var_node) pair flattened, ref first (int64)."""
    if hasattr(variant_to_nodes, "ref_nodes") and hasattr(variant_to_nodes, "var_nodes"):
        ref = np.asarray(variant_to_nodes.ref_nodes).astype(np.int64).ravel()
        var = np.asarray(variant_to_nodes.var_nodes).astype(np.int64).ravel()
        if len(ref) != len(var):
            raise ValueError("variant_to_nodes: %d ref nodes, %d var nodes" % (len(ref), len(var)))
        pairs = np.stack([ref, var], axis=1)
    else:
        pairs = np.array([(int(r), int(v)) for r, v in variant_to_nodes], dtype=np.int64).reshape(-1, 2)
    return np.ascontiguousarray(pairs.reshape(-1))


def sample_kmers_from_structural_variants_on_device(graph, variant_to_nodes, kmer_index_with_frequencies, k,
                                                    max_frequency=2):
    """sample_kmers_from_structural_variants with the columns left in HBM: DeviceFlatKmers in the merged layout
    (uint64, uint32, uint64 zeros, float32 ones), ready for DeviceFlatKmers.from_multiple_flat_kmers."""
    global last_timings, last_counts
    if not isinstance(kmer_index_with_frequencies, (CollisionFreeKmerIndex, KmerCounter)):
        raise NotImplementedError("the frequency source must be graph_kmer_index_amd's CollisionFreeKmerIndex or "
                                  "KmerCounter (got %s); the reference's npstructures-backed KmerCounter is not supported"
                                  % type(kmer_index_with_frequencies).__name__)
    k, max_frequency = int(k), int(max_frequency)
    if not 1 <= k <= 31:
        raise ValueError("k must be in 1..31 (got %d)" % k)
    if max_frequency < 0:
        raise ValueError("max_frequency must not be negative (got %d)" % max_frequency)
    _lib.require_device()
    lib = _lib.load()
    t = {}
    t0 = time.perf_counter()
    arrays = GraphArrays.from_obgraph(graph)
    nodes = candidate_nodes(variant_to_nodes)
    if len(nodes) and (nodes.min() < 0 or nodes.max() >= arrays.n_nodes):
        bad = nodes[(nodes < 0) | (nodes >= arrays.n_nodes)][0]
        raise ValueError("variant_to_nodes names node %d, the graph has nodes 0..%d" % (int(bad), arrays.n_nodes - 1))
    # nodes that fail the size test give nothing (node 0 / "no node" entries among them): dropped here, order kept
    cand = np.ascontiguousarray(nodes[arrays.node_size[nodes] > k + 5], dtype=np.int32)
    dg = DeviceGraph.of(arrays)
    # a KmerCounter answers with the count of the hash alone, the index adds its 31-mer reverse complement's
    if isinstance(kmer_index_with_frequencies, KmerCounter):
        counter, view = kmer_index_with_frequencies._device_counter(), None
    else:
        counter, view = None, kmer_index_with_frequencies._device_index().view()
    t["host_prepare"] = time.perf_counter() - t0
    t1 = time.perf_counter()
    n_rec, plan = _lib._I64(0), _lib.C.c_void_p()
    ms, ms_emit = (_lib.C.c_float * 2)(), (_lib.C.c_float * 1)()
    with _lib.DeviceScope() as s:
        d_cand = s.on_device(cand, np.int32)
        try:
            if counter is not None:
                _lib.check(lib.gki_sv_sample_count_counter(dg.handle, counter.handle, d_cand.ptr, len(cand), k, max_frequency,
                                                           None, _lib.C.byref(n_rec), _lib.C.byref(plan), ms))
            else:
                _lib.check(lib.gki_sv_sample_count(dg.handle, _lib.C.byref(view), d_cand.ptr, len(cand), k, max_frequency,
                                                   None, _lib.C.byref(n_rec), _lib.C.byref(plan), ms))
            t["count"] = time.perf_counter() - t1
            t2 = time.perf_counter()
            out = s.keep(DeviceFlatKmers.allocate(n_rec.value))
            _lib.check(lib.gki_sv_sample_emit(plan, out.hashes.ptr, out.nodes.ptr, out.ref_offsets.ptr,
                                              out.allele_frequencies.ptr, ms_emit))
            t["emit"] = time.perf_counter() - t2
        finally:
            if plan.value:
                lib.gki_sv_sample_destroy(plan)
        s.release(out)
    t["kernel_ms"] = {"probe": float(ms[0]), "greedy_count": float(ms[1]), "greedy_emit_and_records": float(ms_emit[0])}
    last_timings = t
    last_counts = dict(pairs=len(nodes) // 2, candidates=int(len(cand)), records=int(n_rec.value),
                       windows=int((arrays.node_size[cand].astype(np.int64) - k + 1).sum()))
    return out


def sample_kmers_from_structural_variants(graph, variant_to_nodes, kmer_index_with_frequencies, k, max_frequency=2):
    """structural_variants.py:6-43: FlatKmers(hashes uint64, nodes uint32, ref_offsets uint32 all 0)."""
    t0 = time.perf_counter()
    with _lib.DeviceScope() as s:
        d = s.keep(sample_kmers_from_structural_variants_on_device(graph, variant_to_nodes, kmer_index_with_frequencies, k,
                                                                   max_frequency))
        flat = FlatKmers(d.hashes.to_host(d.n), d.nodes.to_host(d.n), np.zeros(d.n, dtype=np.uint32))
    last_timings["end_to_end"] = time.perf_counter() - t0
    return flat
