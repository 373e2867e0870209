"""Node counts by difference from the all-ref path and the count model on the device (graph_kmer_index_amd.haplotype_paths,
csrc/gki_haplotype_counts.hip, k_probe_segments of csrc/gki_probe.hip) against the spec
(tests/spec_haplotype_count_model.py, tests/spec_haplotype_paths.py) on the cases of tests/haplotype_count_model_cases.py.
Every comparison is exact integer equality."""
import functools

import numpy as np
import pytest

import spec_graph_build
import spec_haplotype_count_model as spec
import spec_haplotype_paths
from graph_build_cases import random_reference, vcf
from haplotype_count_model_cases import CASE_NAMES, KS, case, model_case
from haplotype_path_cases import graph_of
from graph_kmer_index_amd import CollisionFreeKmerIndex, DenseKmerFinder, _lib
from graph_kmer_index_amd.haplotype_paths import AltPlane, HaplotypePaths, NodeCountModel
from graph_kmer_index_amd.unique_variant_kmers import VariantToNodesArrays
from graph_kmer_index_amd.vcf_files import HaplotypeMatrix

pytestmark = pytest.mark.gpu
MODULO = 2_000_003


def the_case(name):
    return model_case() if name == "model" else case(name)


def paths_of(c, ploidy=1):
    matrix = HaplotypeMatrix(c.codes, np.ones(len(c.codes), np.uint8), c.n_slots // ploidy, ploidy)
    return HaplotypePaths(c.graph, VariantToNodesArrays(c.ref_nodes, c.var_nodes), matrix)


@functools.lru_cache(maxsize=None)
def index_of(name, k):
    """The case's variant index by the package's own route: find() into from_flat_kmers."""
    finder = DenseKmerFinder(the_case(name).graph, k, max_variant_nodes=4)
    finder.find()
    return CollisionFreeKmerIndex.from_flat_kmers(finder.get_flat_kmers(v="1"), modulo=MODULO)


@functools.lru_cache(maxsize=None)
def spelled(name, slot):
    c = the_case(name)
    return spec_haplotype_paths.spell(c.graph, c.ref_nodes, c.var_nodes, c.codes, slot, c.starts)


@functools.lru_cache(maxsize=None)
def spec_counts(name, slot, k, rc):
    """The slot's row by the spec, computed once and shared; read only."""
    c = the_case(name)
    row = spec_haplotype_paths.node_counts(spelled(name, slot), index_of(name, k), k, c.graph.n_nodes, rc)
    row.setflags(write=False)
    return row


def spec_segments(c, slot, k):
    """((start, windows) in the all-ref path, (start, windows) in the slot's sequence) as int64 arrays, by the spec."""
    out = []
    for along in (False, True):
        bounds, intervals = spec.walk(c.graph, c.ref_nodes, c.var_nodes, c.codes, slot, c.starts, along)
        segs = spec.segments(bounds, intervals, k)
        out.append((np.array([s for s, _ in segs], dtype=np.int64), np.array([n for _, n in segs], dtype=np.int64)))
    return out


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_counts_by_difference_equal_the_whole_route_and_the_spec(name, k):
    c = case(name)
    index, n_nodes, slots = index_of(name, k), c.graph.n_nodes, list(range(c.n_slots))
    with paths_of(c) as paths:
        for slot in slots:
            got, want = paths.segments(slot, k), spec_segments(c, slot, k)
            for which in (0, 1):
                assert got[which][0].dtype == np.int64 and got[which][1].dtype == np.int64
                assert np.array_equal(got[which][0], want[which][0]), (name, k, slot, which)
                assert np.array_equal(got[which][1], want[which][1]), (name, k, slot, which)
        for rc in (True, False):
            timings = []
            got = paths.node_counts_by_difference(slots, index, k, n_nodes, include_reverse_complement=rc, timings=timings)
            assert got.shape == (len(slots), n_nodes) and got.dtype == np.uint32
            whole = paths.node_counts(slots, index, k, n_nodes, include_reverse_complement=rc)
            assert np.array_equal(got, whole), (name, k, rc)
            for slot in slots:
                assert np.array_equal(got[slot], spec_counts(name, slot, k, rc)), (name, k, slot, rc)
            base = paths.reference_node_counts(index, k, n_nodes, include_reverse_complement=rc)
            assert base.dtype == np.uint32 and not c.codes[:, 0].any()
            assert np.array_equal(base, whole[0]) and np.array_equal(base, got[0]), (name, k, rc)
            assert [t["slot"] for t in timings] == slots
            for t in timings:
                want = spec_segments(c, t["slot"], k)
                assert (t["ref_segments"], t["ref_windows"]) == (len(want[0][0]), int(want[0][1].sum())), (name, k, t)
                assert (t["slot_segments"], t["slot_windows"]) == (len(want[1][0]), int(want[1][1].sum())), (name, k, t)
                assert t["taken_lines"] == int(np.sum(c.codes[np.asarray(c.var_nodes) != 0, t["slot"]] == 1))
                assert all(t[key] >= 0 for key in ("spell_s", "segments_s", "subtract_s", "add_s"))
        # n_nodes left out: the index's highest node + 1; reverse complements are the default
        assert np.array_equal(paths.node_counts_by_difference([1], index, k)[0],
                              spec_counts(name, 1, k, True)[:int(index.max_node_id()) + 1])


def assert_segments(got, want, where):
    for which in (0, 1):
        for g, w in zip(got[which], want[which]):
            assert g.dtype == np.int64 and np.array_equal(g, w), (where, which)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["indels", "lines_63", "lines_64", "lines_65", "lines_129", "short_chromosome_4"])
def test_a_plans_first_segments_call_is_of_a_slot_that_takes_every_alt_allele(name, k):
    """The all-ref path is built inside the plan's first segments call, behind the slot's own path and through the same
    scratch.  The test above starts every plan with slot 0, whose path IS the all-ref path; here it differs at every line."""
    c = case(name)
    assert c.codes[:, 1].all() and not c.codes[:, 0].any()
    with paths_of(c) as paths:
        first = paths.segments(1, k)
        assert_segments(first, spec_segments(c, 1, k), (name, k, "first"))
        for slot in (2, 1, 0):
            got = paths.segments(slot, k)
            assert_segments(got, spec_segments(c, slot, k), (name, k, slot))
            if slot == 1:
                assert_segments(got, first, (name, k, "again"))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["indels", "merge_edges"])
def test_paths_do_not_leak_into_one_another(name, k):
    import ctypes as C
    c = case(name)
    index, n_nodes, lib = index_of(name, k), c.graph.n_nodes, _lib.load()
    with paths_of(c) as paths, _lib.DeviceScope() as s:
        totals = [C.c_int64(0) for _ in range(5)]
        args = [C.byref(t) for t in totals] + [None]
        s.keep(paths.sequence(1))
        # the all-ref letters are spelled as slot 0 of a zeroed plane: another slot between the two calls, as sequence(2) is
        base = paths.reference_node_counts(index, k, n_nodes)
        assert np.array_equal(base, spec_counts(name, 0, k, True))
        assert lib.gki_haplotype_segments_count(paths._plan, paths._alt_bits.ptr, paths.n_slots, 1, k, *args) == 5   # GKI_ERR_STATE
        got = paths.node_counts_by_difference([1, 2, 1], index, k, n_nodes)
        assert np.array_equal(got[0], got[2])
        for row, slot in zip(got, (1, 2, 1)):
            assert np.array_equal(row, spec_counts(name, slot, k, True)), (name, k, slot)


def test_a_chain_without_a_kept_line():
    """Two chromosomes and a VCF with no data line: no path drops anything, no line is taken, the model has no entry."""
    k, ploidy, n_bins = 5, 2, 3
    reference = {"a": random_reference(40, 71), "b": random_reference(33, 72)}
    build = spec_graph_build.build(reference, vcf([]))
    graph, codes = graph_of(build), np.zeros((0, 4), np.uint8)
    assert len(build.var_nodes) == 0 and len(graph.chromosome_start_nodes) == 2
    finder = DenseKmerFinder(graph, k, max_variant_nodes=4)
    finder.find()
    index = CollisionFreeKmerIndex.from_flat_kmers(finder.get_flat_kmers(v="1"), modulo=MODULO)
    starts = [graph.chromosome_start_nodes[x] for x in sorted(graph.chromosome_start_nodes)]
    want = spec_haplotype_paths.node_counts(spec_haplotype_paths.spell(graph, build.ref_nodes, build.var_nodes, codes, 0, starts),
                                            index, k, graph.n_nodes, True)
    assert want.any()
    matrix = HaplotypeMatrix(codes, np.ones(0, np.uint8), 4 // ploidy, ploidy)
    with HaplotypePaths(graph, VariantToNodesArrays(build.ref_nodes, build.var_nodes), matrix) as paths:
        for pair in paths.segments(0, k):
            for a in pair:
                assert a.dtype == np.int64 and a.shape == (0,)
        base = paths.reference_node_counts(index, k, graph.n_nodes)
        assert np.array_equal(base, paths.node_counts([0], index, k, graph.n_nodes)[0]) and np.array_equal(base, want)
        assert np.array_equal(paths.node_counts_by_difference([3], index, k, graph.n_nodes)[0], want)
        m = paths.node_count_model(index, k, None, n_bins, graph.n_nodes)
        assert m.histogram.shape == (0, 2, ploidy + 1, n_bins) and m.count_sum.shape == (0, 2, ploidy + 1)
        assert m.samples.tolist() == [0, 1]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_adding_then_taking_away_the_same_segments_leaves_zero(name, k):
    c = case(name)
    device_index, n_nodes = index_of(name, k)._device_index(), c.graph.n_nodes
    with paths_of(c) as paths, _lib.DeviceScope() as s:
        start, windows = paths.segments(1, k)[1]
        assert len(start) > 0
        seq = s.keep(paths.sequence(1))
        row = s.array(n_nodes, np.uint32)
        row.zero()
        for strands in (3, 1):
            probed, hits = device_index.count_nodes_from_segments(seq.letters, start, windows, k, row, n_nodes, strands, sign=1)
            assert probed == int(windows.sum()) * (2 if strands == 3 else 1) and hits >= 0
            added = row.to_host()
            assert int(added.sum(dtype=np.int64)) == hits
            assert device_index.count_nodes_from_segments(seq.letters, start, windows, k, row, n_nodes, strands, sign=-1) == (probed, hits)
            assert not row.to_host().any(), (name, k, strands)
        # taking away first wraps and adding brings it back
        _, hits = device_index.count_nodes_from_segments(seq.letters, start, windows, k, row, n_nodes, sign=-1)
        assert hits == 0 or row.to_host().max() > 2 ** 31
        if name in ("long_insertions", "taken_300", "merge_edges"):
            assert hits > 0
        device_index.count_nodes_from_segments(seq.letters, start, windows, k, row, n_nodes, sign=1)
        assert not row.to_host().any()


def test_segments_that_reach_outside_the_letters_are_cut_and_reported():
    c, k = case("long_insertions"), 31
    device_index, n_nodes = index_of("long_insertions", k)._device_index(), c.graph.n_nodes
    with paths_of(c) as paths, _lib.DeviceScope() as s:
        seq = s.keep(paths.sequence(1))
        n = seq.letters.n
        row = s.array(n_nodes, np.uint32)
        row.zero()
        device_index.count_nodes_from_segments(seq.letters, [0], [n - k + 1], k, row, n_nodes)
        whole = row.to_host()
        assert whole.any()
        for start, windows in (([-3], [10]), ([n - k], [2]), ([n + 5], [1]), ([0], [-1]), ([0], [2 ** 62]), ([2 ** 62], [1]),
                               ([-2 ** 62], [2 ** 62])):
            with pytest.raises(_lib.GkiError) as e:
                device_index.count_nodes_from_segments(seq.letters, start, windows, k, row, n_nodes)
            assert e.value.code == 2, (start, windows)
        # a segment cut at the end keeps the windows that lie inside: the whole sequence asked for with too many windows
        row.zero()
        with pytest.raises(_lib.GkiError):
            device_index.count_nodes_from_segments(seq.letters, [0], [n], k, row, n_nodes)
        assert np.array_equal(row.to_host(), whole)
        for bad in ({"sign": 0}, {"sign": 2}, {"strands": 0}, {"strands": 4}):
            with pytest.raises(_lib.GkiError):
                device_index.count_nodes_from_segments(seq.letters, [0], [1], k, row, n_nodes, **bad)
        with pytest.raises(_lib.GkiError):
            device_index.count_nodes_from_segments(seq.letters, [0], [1], 32, row, n_nodes)


def test_the_segment_calls_keep_their_order():
    import ctypes as C
    c = case("indels")
    lib = _lib.load()
    with paths_of(c) as paths, _lib.DeviceScope() as s:
        totals = [C.c_int64(0) for _ in range(5)]
        args = [C.byref(t) for t in totals] + [None]
        out = [s.array(16, np.int64) for _ in range(4)]
        assert lib.gki_haplotype_segments_emit(paths._plan, *[a.ptr for a in out], None) == 5          # GKI_ERR_STATE
        assert lib.gki_haplotype_segments_count(paths._plan, paths._alt_bits.ptr, paths.n_slots, 1, 5, *args) == 5
        s.keep(paths.sequence(2))
        assert lib.gki_haplotype_segments_count(paths._plan, paths._alt_bits.ptr, paths.n_slots, 1, 5, *args) == 5
        assert lib.gki_haplotype_segments_count(paths._plan, paths._alt_bits.ptr, paths.n_slots, 2, 0, *args) == 2
        assert lib.gki_haplotype_segments_count(paths._plan, paths._alt_bits.ptr, paths.n_slots, 2, 32, *args) == 2
        assert lib.gki_haplotype_segments_count(paths._plan, paths._alt_bits.ptr, paths.n_slots, 2, 5, *args) == 0
        s.keep(paths.sequence(1))
        assert lib.gki_haplotype_segments_emit(paths._plan, *[a.ptr for a in out], None) == 5
        assert lib.gki_haplotype_segments_emit(paths._plan, *[a.ptr for a in out], None) == 5          # the count is used up
        # the same slot number spelled from another plane between the two calls
        s.keep(paths.sequence(2))
        assert lib.gki_haplotype_segments_count(paths._plan, paths._alt_bits.ptr, paths.n_slots, 2, 5, *args) == 0
        other = s.array(paths._alt_bits.n, np.uint64)
        _lib.check(lib.gki_memcpy_d2d(other.ptr, paths._alt_bits.ptr, other.nbytes))
        n_out, bounds = C.c_int64(0), np.zeros(paths.n_chromosomes + 1, dtype=np.int64)
        assert lib.gki_haplotype_spell_count(paths._plan, other.ptr, paths.n_slots, 2, C.byref(n_out), _lib.hptr(bounds), None) == 0
        assert lib.gki_haplotype_segments_emit(paths._plan, *[a.ptr for a in out], None) == 5
        s.keep(paths.sequence(2))                          # and in order again it works
        assert lib.gki_haplotype_segments_count(paths._plan, paths._alt_bits.ptr, paths.n_slots, 2, 5, *args) == 0
        assert lib.gki_haplotype_segments_emit(paths._plan, *[a.ptr for a in out], None) == 0


def sample_rows(name, samples, ploidy, k, rc=True):
    return [sum(spec_counts(name, s * ploidy + i, k, rc).astype(np.uint32) for i in range(ploidy)) for s in samples]


def assert_model(m, want, k, ploidy, n_bins, samples):
    assert m.histogram.dtype == np.uint32 and m.count_sum.dtype == np.uint64
    assert np.array_equal(m.histogram, want[0]) and np.array_equal(m.count_sum, want[1]), (k, ploidy, n_bins, samples)
    assert (m.k, m.ploidy, m.n_bins, m.samples.tolist()) == (k, ploidy, n_bins, list(samples))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ploidy", [1, 2])
def test_the_model_equals_the_spec(ploidy, k, tmp_path):
    c = model_case()
    index, n_nodes, n_samples = index_of("model", k), c.graph.n_nodes, c.n_slots // ploidy
    everyone, subset = list(range(n_samples)), [2, 0, 3]
    with paths_of(c, ploidy) as paths:
        for n_bins in (2, 5):
            want = spec.model(sample_rows("model", everyone, ploidy, k), c.codes, c.ref_nodes, c.var_nodes, everyone, ploidy, n_bins)
            assert want[0].sum() == 2 * n_samples * int(np.count_nonzero(c.var_nodes))
            if k == 5:                                      # counts in the hundreds: nearly everything is clipped
                assert want[0][..., -1].sum() > 0.9 * want[0].sum()
            elif n_bins == 5:
                assert want[0][..., :-1].sum() > 0 and want[0][..., -1].sum() > 0
            m = paths.node_count_model(index, k, None, n_bins, n_nodes)
            assert_model(m, want, k, ploidy, n_bins, everyone)
        want = spec.model(sample_rows("model", subset, ploidy, k), c.codes, c.ref_nodes, c.var_nodes, subset, ploidy, 5)
        by_difference = paths.node_count_model(index, k, subset, 5, n_nodes)
        assert_model(by_difference, want, k, ploidy, 5, subset)
        assert_model(paths.node_count_model(index, k, subset, 5, n_nodes, route="whole"), want, k, ploidy, 5, subset)
        want = spec.model(sample_rows("model", subset, ploidy, k, False), c.codes, c.ref_nodes, c.var_nodes, subset, ploidy, 5)
        assert_model(paths.node_count_model(index, k, subset, 5, n_nodes, include_reverse_complement=False), want, k, ploidy, 5, subset)
        mean = by_difference.mean()
        n = by_difference.histogram.sum(axis=3)
        assert np.array_equal(np.isnan(mean), n == 0) and np.array_equal(mean[n > 0] * n[n > 0], by_difference.count_sum[n > 0])
        with pytest.raises(ValueError):
            paths.node_count_model(index, k, subset, 1, n_nodes)
        with pytest.raises(IndexError):
            paths.node_count_model(index, k, [n_samples], 5, n_nodes)
    by_difference.to_file(str(tmp_path / "model"))
    back = NodeCountModel.from_file(str(tmp_path / "model"))
    assert_model(back, (by_difference.histogram, by_difference.count_sum), k, ploidy, 5, subset)


def test_the_model_over_a_plane_on_the_device_takes_its_ploidy_from_the_caller():
    c, k = model_case(), 31
    index, n_nodes = index_of("model", k), c.graph.n_nodes
    v, h = len(c.var_nodes), c.n_slots
    plane = np.zeros((h, (v + 63) // 64), dtype=np.uint64)
    for slot in range(h):
        for line_no in np.flatnonzero(c.codes[:, slot] == 1):
            plane[slot, line_no >> 6] |= np.uint64(1) << np.uint64(line_no & 63)
    plane[:, -1] |= ~((np.uint64(1) << np.uint64(v & 63)) - np.uint64(1))      # tail bits are masked, not relied on
    want = spec.model(sample_rows("model", [1, 3], 2, k), c.codes, c.ref_nodes, c.var_nodes, [1, 3], 2, 5)
    with _lib.DeviceScope() as s:
        alt_bits = s.on_device(plane.reshape(-1), np.uint64)
        with HaplotypePaths(c.graph, VariantToNodesArrays(c.ref_nodes, c.var_nodes), AltPlane(alt_bits, v, h)) as paths:
            with pytest.raises(ValueError, match="ploidy="):
                paths.node_count_model(index, k, [1, 3], 5, n_nodes)
            assert_model(paths.node_count_model(index, k, [1, 3], 5, n_nodes, ploidy=2), want, k, 2, 5, [1, 3])


def test_the_sub_commands_write_the_same_arrays(tmp_path):
    from graph_kmer_index_amd.command_line_interface import main
    c, k = model_case(), 31
    index = index_of("model", k)
    n_nodes = int(index.max_node_id()) + 1
    files = {n: str(tmp_path / n) for n in ("graph", "v2n", "matrix", "index", "model", "counts")}
    c.graph.to_file(files["graph"])
    VariantToNodesArrays(c.ref_nodes, c.var_nodes).to_file(files["v2n"])
    HaplotypeMatrix(c.codes, np.ones(len(c.codes), np.uint8), 4, 2).to_file(files["matrix"])
    index.to_file(files["index"])
    common = ["-g", files["graph"] + ".npz", "-V", files["v2n"], "-m", files["matrix"], "-i", files["index"], "-k", str(k)]
    assert main(["make_node_count_model"] + common + ["-s", "3,1", "-b", "4", "-o", files["model"]]) == 0
    back = NodeCountModel.from_file(files["model"])
    rows = [r[:n_nodes] for r in sample_rows("model", [3, 1], 2, k)]
    assert_model(back, spec.model(rows, c.codes, c.ref_nodes, c.var_nodes, [3, 1], 2, 4), k, 2, 4, [3, 1])
    assert main(["haplotype_node_counts"] + common + ["-s", "5,2", "--route", "difference", "-o", files["counts"]]) == 0
    counts = np.load(files["counts"] + ".npy")
    assert counts.shape == (2, n_nodes) and counts.dtype == np.uint32
    for row, slot in zip(counts, (5, 2)):
        assert np.array_equal(row, spec_counts("model", slot, k, True)[:n_nodes]), slot


class FailingLibrary:
    """The loaded library with the `fail_at`-th call to an entry point whose status the host layer checks replaced by
    `return 2` (GKI_ERR_BAD_ARG); allocation, copies, destroy calls and calls without a status pass through uncounted."""

    def __init__(self, real):
        self._real, self.calls, self.fail_at, self.failed = real, 0, None, None

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name in ("gki_malloc", "gki_free", "gki_memset", "gki_last_error", "gki_device_count") or name.startswith("gki_memcpy_") \
                or name.endswith("_destroy") or _lib.SYMBOLS[name][0] is not _lib._I32:
            return fn

        def call(*args):
            i, self.calls = self.calls, self.calls + 1
            if i == self.fail_at:
                self.failed = name
                return 2
            return fn(*args)
        return call


def test_nothing_stays_on_the_device_after_a_failed_library_call(monkeypatch):
    """Every library call of the two new routes fails once; whatever the route had made by then is freed."""
    c, k = model_case(), 31
    index, n_nodes = index_of("model", k), c.graph.n_nodes
    with paths_of(c, 2) as paths:
        runs = {"by_difference": lambda: paths.node_counts_by_difference([3], index, k, n_nodes),
                "model": lambda: paths.node_count_model(index, k, [1], 3, n_nodes),
                "model_whole": lambda: paths.node_count_model(index, k, [1], 3, n_nodes, route="whole")}
        for run in runs.values():                          # the probe table, the all-ref path and the base row are kept
            run()
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
        proxy = FailingLibrary(_lib.load())
        monkeypatch.setattr(_lib, "_lib", proxy)
        for name, run in runs.items():
            proxy.calls, proxy.fail_at = 0, None
            run()
            n_calls = proxy.calls
            assert not live and n_calls >= 5, (name, n_calls)
            for i in range(n_calls):
                proxy.calls, proxy.fail_at, proxy.failed = 0, i, None
                with pytest.raises(_lib.GkiError) as e:
                    run()
                assert e.value.code == 2 and proxy.failed is not None
                assert not live, "%s, call %d of %d (%s): %d buffers are still on the device" % (name, i, n_calls, proxy.failed, len(live))
            proxy.fail_at = None
            run()                                          # and the route works again behind a failure
        monkeypatch.undo()


def live_allocations():
    mallocs, frees = _lib.pool_stats()[:2]
    return mallocs - frees


def test_close_gives_everything_back():
    c, k = model_case(), 5
    index, n_nodes = index_of("model", k), c.graph.n_nodes
    index._device_index().probe_table()
    with paths_of(c, 2) as warm:                           # whatever the first use of a route parks stays out of the count
        warm.node_counts_by_difference([0], index, k, n_nodes)
        warm.node_count_model(index, k, [0], 2, n_nodes)
        warm.node_count_model(index, k, [0], 2, n_nodes, route="whole")
        warm.segments(1, k)
    _lib.check(_lib.load().gki_trim())
    before = live_allocations()
    paths = paths_of(c, 2)
    paths.reference_node_counts(index, k, n_nodes)
    paths.reference_node_counts(index, k, n_nodes, include_reverse_complement=False)
    paths.node_counts_by_difference([2, 3], index, k, n_nodes)
    paths.segments(1, k)
    paths.node_count_model(index, k, [1, 0], 3, n_nodes)
    paths.node_count_model(index, k, [1], 3, n_nodes, route="whole")
    with pytest.raises(IndexError):
        paths.node_counts_by_difference([0, 8], index, k, n_nodes)
    with pytest.raises(IndexError):
        paths.node_count_model(index, k, [4], 3, n_nodes)
    paths.close()
    paths.close()
    with pytest.raises(ValueError, match="closed"):
        paths.node_counts_by_difference([0], index, k, n_nodes)
    _lib.check(_lib.load().gki_trim())
    assert live_allocations() == before
