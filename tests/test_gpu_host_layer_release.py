"""-m gpu: the Python host layer leaves no device buffer behind on any error path.

Every entry point below is called with host NumPy inputs, so that every upload is its own.  The library object is replaced
by a proxy that passes every call through, except that the i-th call to an entry point whose status the host layer checks
is not made and returns GKI_ERR_BAD_ARG (2): a host-side error return, no kernel is launched at the failure.  The calls
that are passed through uncounted are gki_malloc, gki_free, gki_memcpy_*, gki_memset, gki_last_error and gki_device_count,
and the gki_*_destroy calls of the plan handles, which release like gki_free and whose status nobody reads (a failure put
there raises nothing).  `DeviceArray.__init__` and `DeviceArray.free` are wrapped to keep the set of live device pointers.

Per entry point: one untouched run warms the legitimate caches (probe table, DeviceGraph.of, finder handle); a second
untouched run counts the library calls N and must leave exactly the returned buffers new; then, for every i < N, the run
with call i failing must raise GkiError and, while the exception with its traceback (and so every frame) is still held,
the live set must equal the baseline."""
import gc
import gzip

import numpy as np
import pytest

import graphgen
import read_file_cases as cases
from graph_kmer_index_amd import (CollisionFreeKmerIndex, DenseKmerFinder, DeviceFlatKmers, FlatKmers, KmerCounter,
                                  ReverseKmerIndex, _lib, bgzf, read_files)
from graph_kmer_index_amd.collision_free_kmer_index import PartitionedDeviceIndex
from test_gpu_read_files import N_NODES, golden_queries, small_index
from uvk_cases import bubble_variants

pytestmark = pytest.mark.gpu
K = 31
PASSED_THROUGH = {"gki_malloc", "gki_free", "gki_memset", "gki_last_error", "gki_device_count"}


class FailingLibrary:
    """The loaded library with the `fail_at`-th counted call replaced by `return 2`."""

    def __init__(self, real):
        self._real, self.calls, self.fail_at, self.failed = real, 0, None, None

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("gki_") or name in PASSED_THROUGH or name.startswith("gki_memcpy_") \
                or name.endswith("_destroy") or _lib.SYMBOLS[name][0] is not _lib._I32:      # (or returns no status)
            return fn

        def call(*args):
            i, self.calls = self.calls, self.calls + 1
            if i == self.fail_at:
                self.failed = name
                return 2
            return fn(*args)
        return call


@pytest.fixture
def live(monkeypatch):
    """The set of device pointers that DeviceArrays made from here on hold."""
    live = set()
    init, free = _lib.DeviceArray.__init__, _lib.DeviceArray.free

    def tracked_init(self, n, dtype):
        init(self, n, dtype)
        live.add(self.ptr.value)

    def tracked_free(self):
        if self.ptr is not None and self.ptr.value:
            live.discard(self.ptr.value)
        free(self)

    monkeypatch.setattr(_lib.DeviceArray, "__init__", tracked_init)
    monkeypatch.setattr(_lib.DeviceArray, "free", tracked_free)
    return live


def device_arrays_of(result):
    if isinstance(result, _lib.DeviceArray):
        return [result]
    if isinstance(result, DeviceFlatKmers):
        return [result.hashes, result.nodes, result.ref_offsets, result.allele_frequencies]
    if isinstance(result, (tuple, list)):
        return [a for r in result for a in device_arrays_of(r)]
    return []


# ------------------------------------------------------------------ inputs, made once
class _Pid:
    def __init__(self, base):
        self._base = np.asarray(base, dtype=np.int64)

    def get(self, nodes, offsets):
        return self._base[np.asarray(nodes, dtype=np.int64)] + np.asarray(offsets, dtype=np.int64)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from graph_kmer_index_amd.graph import GraphArrays
    from graph_kmer_index_amd.unique_variant_kmers import UniqueVariantKmersFinder, VariantArrays, VariantToNodesArrays
    w = type("World", (), {})()
    rng = np.random.default_rng(2024)
    index, _ = small_index(K, 0)
    w.index = index._device_index()
    w.queries = golden_queries("stream", K, False)[:60].copy()
    w.letters = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=8 * 40)        # 8 reads of 40 bases
    w.read_start = np.arange(0, 8 * 40 + 1, 40, dtype=np.int64)
    w.flat = FlatKmers(np.asarray(index._kmers), np.asarray(index._nodes), np.asarray(index._ref_offsets),
                       np.asarray(index._allele_frequencies))
    w.dflat = DeviceFlatKmers.from_flat_kmers(w.flat)
    w.partitioned = PartitionedDeviceIndex.build(w.dflat, 10007, n_parts=2)
    w.counter = KmerCounter.from_kmers(np.concatenate([w.queries, w.queries[::3]]), 0)
    # a chain of 100 SNP bubbles (301 nodes) between two long nodes; a handful of its variants
    seqs, edges, linear, _ = graphgen.random_bubble_graph(rng, n_var=100, min_ref=4, max_ref=14, p_indel=0.0,
                                                          first_ref=80, last_ref=80)
    g = w.graph = GraphArrays.from_dicts(seqs, edges, linear)
    assert 200 < g.n_nodes < 400
    w.finder = DenseKmerFinder(g, K, max_variant_nodes=6)
    w.starts = [int(n) for n in linear[10:14]]
    w.finder.find()
    w.graph_index = CollisionFreeKmerIndex.from_flat_kmers(w.finder.get_flat_kmers(v="1"), modulo=100003)
    refs, alts, pos = bubble_variants(g, K)
    pick = np.nonzero((pos > 150) & (pos < int(g.node_size[g.is_ref != 0].sum()) - 150))[0][:6]
    assert len(pick) == 6
    refs, alts, pos = refs[pick], alts[pick], pos[pick]
    w.variant_to_nodes = VariantToNodesArrays(refs, alts)
    w.variants = VariantArrays(pos, 1, np.arange(len(pos)), np.ones(len(pos), np.int8))
    w.uvk = UniqueVariantKmersFinder(g, w.variant_to_nodes, w.variants, K, 6, kmer_index_with_frequencies=w.graph_index,
                                     use_dense_kmer_finder=True, position_id_index=_Pid(g.position_id_base()))
    w.sv_pairs = [(int(linear[0]), 0), (0, int(linear[-1]))]
    assert all(g.node_size[n] > K + 5 for n in (linear[0], linear[-1]))
    # the reads files: pieces of 64 bytes and members of 100 end inside lines, so that a tail is alive between pieces
    data = cases.GOLDEN_CASES["stream"]
    tmp = tmp_path_factory.mktemp("release")
    w.text = data
    w.raw, w.gz, w.bgzf = str(tmp / "stream.fa"), str(tmp / "plain.fa.gz"), str(tmp / "blocked.fa.gz")
    with open(w.raw, "wb") as fh:
        fh.write(data)
    with open(w.gz, "wb") as fh:
        fh.write(gzip.compress(data))
    bgzf.write_bgzf(w.bgzf, data, block_size=100)
    assert [read_files.reads_file_route(p) for p in (w.raw, w.gz, w.bgzf)] == ["raw", "gzip-host", "bgzf-device"]
    with open(w.bgzf, "rb") as fh:
        w.packed = fh.read()
    w.members = bgzf.scan_all(w.packed)[0]
    assert len(w.members) > 50
    yield w
    w.partitioned.free()
    w.dflat.free()


def _from_file(w, path):
    return read_files.count_nodes_from_file(w.index, path, K, N_NODES, chunk_bytes=64)


def _sv(w):
    from graph_kmer_index_amd.structural_variants import sample_kmers_from_structural_variants_on_device
    return sample_kmers_from_structural_variants_on_device(w.graph, w.sv_pairs, w.graph_index, K)


def _simple(w):
    from graph_kmer_index_amd.unique_variant_kmers import find_kmers_over_variants_on_device
    return find_kmers_over_variants_on_device(w.graph, w.variant_to_nodes, w.variants, K, 6)


def _hash_reads(w):
    from graph_kmer_index_amd.read_kmers import hash_reads
    return hash_reads((w.letters, w.read_start), K)


def _reverse_complement(w):
    from graph_kmer_index_amd.kmer_hashing import kmer_hashes_to_reverse_complement_hash
    return kmer_hashes_to_reverse_complement_hash(w.queries, K)


def _unique_counts(w):
    from graph_kmer_index_amd.kmer_counter import unique_counts
    return unique_counts(np.concatenate([w.queries, w.queries[::3]]))


ENTRY_POINTS = {
    "lookup_positions_probe_table": lambda w: w.index.lookup_positions(w.queries, use_probe_table=True),
    "lookup_positions_reference_layout": lambda w: w.index.lookup_positions(w.queries, use_probe_table=False),
    "contains": lambda w: w.index.contains(w.queries),
    "count_nodes": lambda w: w.index.count_nodes(w.queries, N_NODES),
    "count_nodes_from_reads": lambda w: w.index.count_nodes_from_reads(w.letters, w.read_start, K, N_NODES),
    "partitioned_count_nodes": lambda w: w.partitioned.count_nodes(w.queries, N_NODES),
    "partitioned_count_nodes_from_reads": lambda w: w.partitioned.count_nodes_from_reads(w.letters, w.read_start, K, N_NODES),
    "counter_get_frequencies": lambda w: w.counter.get_frequencies(w.queries),
    "unique_counts": _unique_counts,
    "hash_reads": _hash_reads,
    "reverse_complement_hashes": _reverse_complement,
    "without_singletons": lambda w: w.dflat.get_new_without_singletons(),
    "finder_find": lambda w: w.finder.find(),
    "finder_find_kmers_starting_at_positions": lambda w: w.finder.find_kmers_starting_at_positions(w.starts, [0] * len(w.starts)),
    "unique_variant_kmers": lambda w: w.uvk.find_unique_kmers_on_device(),
    "kmers_over_variants": _simple,
    "structural_variant_sampler": _sv,
    "reverse_index": lambda w: ReverseKmerIndex.from_flat_kmers(w.flat),
    "bgzf_inflate": lambda w: bgzf.inflate_on_device(w.packed, w.members),
    "parse_reads": lambda w: read_files.parse_reads_on_device(w.text, "fasta"),
    "file_raw": lambda w: _from_file(w, w.raw),
    "file_gzip_host": lambda w: _from_file(w, w.gz),
    "file_bgzf_device": lambda w: _from_file(w, w.bgzf),
}


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_nothing_stays_on_the_device_after_a_failed_library_call(name, world, live, monkeypatch):
    run = lambda: ENTRY_POINTS[name](world)
    for a in device_arrays_of(run()):                    # warms the caches
        a.free()
    gc.collect()
    baseline = set(live)
    proxy = FailingLibrary(_lib.load())
    monkeypatch.setattr(_lib, "_lib", proxy)
    returned = device_arrays_of(run())
    assert live - baseline == {a.ptr.value for a in returned} and baseline <= live, "more than the result is new"
    for a in returned:
        a.free()
    assert live == baseline
    n_calls = proxy.calls
    assert n_calls > 0
    for i in range(n_calls):
        proxy.calls, proxy.fail_at, proxy.failed = 0, i, None
        with pytest.raises(_lib.GkiError) as e:
            run()
        assert e.value.code == 2 and proxy.failed is not None
        assert live == baseline, "call %d of %d (%s): %d buffers are still on the device while the exception is held" \
            % (i, n_calls, proxy.failed, len(live - baseline))
