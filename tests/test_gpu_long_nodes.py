"""-m gpu: every k-mer route on graphs with nodes longer than 32 767 and 65 535 bases (tests/long_node_cases.py).

The rule under test: a column the reference types as int16 holds the end offset modulo 2^16; every
64-bit position the product hands out is `position base of the end node + TRUE end offset`.  All expectations come from
the oracle's full-width column (`start_offsets_wide`, pinned on the CPU in tests/test_long_nodes_oracle.py) or from the
Python specs; where two product routes are also compared with each other, that is in addition."""
import ctypes as C

import numpy as np
import pytest

import long_node_cases as cases
import spec_unique_variant_kmers as uvk_spec
from gpu_util import assert_same_records, finder_cols
from oracle import oracle

pytestmark = pytest.mark.gpu
K = cases.K
MASK64 = (1 << 64) - 1
FIND_CASES = cases.ALL
EARLY_STOP_CASES = ("linear_row", "bubbles", "indel", "nested_bubbles", "not_topological", "deep_after_long")


class _Pid:
    """A caller's position_id object: any int64 base per node, plus the offset."""

    def __init__(self, base):
        self._base = np.asarray(base, dtype=np.int64)

    def get(self, nodes, offsets):
        return self._base[np.asarray(nodes, dtype=np.int64)] + np.asarray(offsets, dtype=np.int64)


def _finder(name, one=True, **kw):
    from graph_kmer_index_amd import DenseKmerFinder
    return DenseKmerFinder(cases.graph(name), K, only_save_one_node_per_kmer=one,
                           max_variant_nodes=cases.max_variant_nodes(name), **kw)


def _flat_cols(flat):
    return (np.asarray(flat._hashes).astype(np.uint64), np.asarray(flat._nodes).astype(np.uint32),
            np.asarray(flat._ref_offsets).astype(np.int64), np.asarray(flat._allele_frequencies).astype(np.float32))


def _expected_flat(g, rec, base=None):
    return (rec["kmers"].astype(np.uint64), rec["nodes"].astype(np.uint32), cases.expected_positions(g, rec, base),
            rec["allele_frequencies"].astype(np.float32))


def _assert_same_flat(got, exp, exact_order=False):
    assert len(got[0]) == len(exp[0]), "%d records, %d expected" % (len(got[0]), len(exp[0]))
    if not exact_order:
        og, oe = (np.lexsort((c[3], c[0], c[1], c[2])) for c in (got, exp))
        got, exp = [c[og] for c in got], [c[oe] for c in exp]
    for name, a, b in zip(("hashes", "nodes", "ref_offsets", "allele_frequencies"), got, exp):
        assert np.array_equal(a, b), "column %s differs" % name


def _device_flat(f, split_layout):
    d = f.find_flat_on_device(split_layout=split_layout)
    f.synchronize()
    flat = d.to_flat_kmers()
    d.free()
    return flat


# ------------------------------------------------------------------ find() and the positions made from it
@pytest.mark.parametrize("one", [True, False])
@pytest.mark.parametrize("name", FIND_CASES)
def test_find_v2_columns_equal_the_oracle(name, one):
    g, exp = cases.graph(name), cases.oracle_records(name, one)
    f = _finder(name, one)
    f.find()
    got = finder_cols(f)
    assert got["start_offsets"].dtype == np.int16
    assert_same_records(got, exp, exact_order=name in cases.LINEAR)
    # rule 1 said on the wide column: the int16 column is the true offset modulo 2^16
    o = np.lexsort((got["nodes"], got["kmers"], got["start_offsets"], got["start_nodes"]))
    e = np.lexsort((exp["nodes"], exp["kmers"], exp["start_offsets"], exp["start_nodes"]))
    assert np.array_equal(got["start_offsets"][o], exp["start_offsets_wide"][e].astype(np.int16))
    f.close()


@pytest.mark.parametrize("one", [True, False])
@pytest.mark.parametrize("name", FIND_CASES)
def test_host_positions_after_find_are_true_positions(name, one):
    from graph_kmer_index_amd import DenseKmerFinder
    g, exp = cases.graph(name), cases.oracle_records(name, one)
    f = _finder(name, one)
    f.find()
    v1 = _flat_cols(f.get_flat_kmers(v="1"))
    _assert_same_flat(v1, _expected_flat(g, exp), exact_order=name in cases.LINEAR)
    v0 = _flat_cols(f.get_flat_kmers(v="0"))
    _assert_same_flat(v0, _expected_flat(g, exp, np.asarray(g.node_to_ref_offset)[:g.n_nodes]), exact_order=name in cases.LINEAR)
    # record for record the device route of the same finder, by-node layout
    by_node = _flat_cols(_device_flat(f, split_layout=False))
    _assert_same_flat(v1, by_node, exact_order=True)
    f.close()
    # a caller's position_id object gets the true offsets too
    base = g.position_id_base() * 2 + 11
    fp = DenseKmerFinder(g, K, position_id=_Pid(base), only_save_one_node_per_kmer=one,
                         max_variant_nodes=cases.max_variant_nodes(name))
    fp.find()
    _assert_same_flat(_flat_cols(fp.get_flat_kmers(v="1")), _expected_flat(g, exp, base), exact_order=name in cases.LINEAR)
    fp.close()


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", FIND_CASES)
def test_find_flat_on_device_equals_the_oracle(name, split):
    from graph_kmer_index_amd import _lib
    g, exp = cases.graph(name), cases.oracle_records(name, True)
    f = _finder(name, True)
    got = _flat_cols(_device_flat(f, split))
    _assert_same_flat(got, _expected_flat(g, exp))
    if name in cases.LINEAR and not split:
        _assert_same_flat(got, _expected_flat(g, exp), exact_order=True)
    n_int = f.interior_records()
    assert 0 < n_int <= len(got[0])
    if split:
        # interior section: one window per position, written by position, every one inside its node
        pos = got[2][:n_int]
        assert np.all(np.diff(pos) > 0)
        node_of = np.searchsorted(g.seq_start, pos, side="right") - 1
        assert np.array_equal(got[1][:n_int], node_of.astype(np.uint32))
        assert np.all(pos - g.seq_start[node_of] >= K - 1)
        assert np.count_nonzero(pos - g.seq_start[node_of] >= 32768) == np.count_nonzero(exp["start_offsets_wide"] >= 32768)
    # the partial-column form (hashes and positions only) of the same layout
    n = f._count(layout=1 if split else 0)
    assert n == len(got[0])
    d_h, d_r = _lib.DeviceArray(n, np.uint64), _lib.DeviceArray(n, np.uint64)
    _lib.check(_lib.load().gki_finder_emit_flat(f._finder_handle(), d_h.ptr, None, d_r.ptr, None))
    f.synchronize()
    h, r = d_h.to_host(), d_r.to_host().view(np.int64)
    d_h.free(); d_r.free()
    if split:           # the boundary section's order inside a node is the walk's; the interior section's is by position
        assert np.array_equal(h[:n_int], got[0][:n_int]) and np.array_equal(r[:n_int], got[2][:n_int])
    o1, o2 = np.lexsort((h, r)), np.lexsort((got[0], got[2]))
    assert np.array_equal(h[o1], got[0][o2]) and np.array_equal(r[o1], got[2][o2])
    f.close()


# ------------------------------------------------------------------ chunks, shards, store sets, whitelist
@pytest.mark.parametrize("name", ["snp", "indel", "bubbles"])
def test_every_chunk_of_critical_paths(name):
    from graph_kmer_index_amd import CriticalGraphPaths
    g, M = cases.graph(name), cases.max_variant_nodes(name)
    cp = CriticalGraphPaths.from_graph(g, K)
    crit = cases.critical(name)
    assert np.array_equal(cp.nodes, crit[0]) and np.array_equal(cp.offsets, crit[1]) and len(cp) >= 4
    f = _finder(name, True, critical_graph_paths=cp, start_at_critical_path_number=0, stop_at_critical_path_number=len(cp))
    total = far = 0
    for a in range(len(cp)):
        f.set_critical_path_range(a, a + 1)
        exp = oracle.find(g, K, crit, True, M, start_at_critical_path_number=a, stop_at_critical_path_number=a + 1)
        f.find()
        assert_same_records(finder_cols(f), exp)
        _assert_same_flat(_flat_cols(f.get_flat_kmers(v="1")), _expected_flat(g, exp))
        for split in (True, False):
            _assert_same_flat(_flat_cols(_device_flat(f, split)), _expected_flat(g, exp))
        total += len(exp["kmers"])
        far += int(np.count_nonzero(exp["start_offsets_wide"] >= 65536))
    assert total >= len(cases.oracle_records(name, True)["kmers"]) and far > 0
    f.close()


@pytest.mark.parametrize("name", ["bubbles", "snp", "not_topological"])
def test_eight_shards_sum_to_the_whole(name):
    from graph_kmer_index_amd import CriticalGraphPaths
    from graph_kmer_index_amd.sharding import critical_path_cuts
    g = cases.graph(name)
    cp = CriticalGraphPaths.from_graph(g, K)

    def checksums(flat):
        return [c.checksum(flat.n) for c in (flat.hashes, flat.nodes, flat.ref_offsets, flat.allele_frequencies)]

    full = _finder(name, True, critical_graph_paths=cp)
    flat = full.find_flat_on_device()
    full.synchronize()
    n, want = flat.n, checksums(flat)
    exp = cases.oracle_records(name, True)
    assert n == len(exp["kmers"])
    pos = cases.expected_positions(g, exp).astype(np.uint64)
    assert want[2][0] == int(pos.sum(dtype=np.uint64)) and want[2][1] == int(np.bitwise_xor.reduce(pos))
    flat.free()
    full.close()
    cuts = critical_path_cuts(g, cp, 8)
    total, sums, xors = 0, [0] * 4, [0] * 4
    for a, b in zip(cuts[:-1], cuts[1:]):
        f = _finder(name, True, critical_graph_paths=cp, start_at_critical_path_number=a, stop_at_critical_path_number=b)
        part = f.find_flat_on_device()
        f.synchronize()
        total += part.n
        for i, (s, x) in enumerate(checksums(part)):
            sums[i] = (sums[i] + s) & MASK64
            xors[i] ^= x
        part.free()
        f.close()
    assert total == n
    assert [(s, x) for s, x in zip(sums, xors)] == want


@pytest.mark.parametrize("name", ["bubbles", "nested_bubbles"])
def test_only_store_nodes_with_a_long_node_inside_and_outside_the_set(name):
    g, M = cases.graph(name), cases.max_variant_nodes(name)
    long_ = cases.long_nodes(g).tolist()
    assert len(long_) >= 2
    short = np.nonzero(g.node_size < K)[0].tolist()
    for store in (set(long_[:1] + short[::2]), set(long_[1:] + short[1::3]), set(short)):
        for one in (True, False):
            exp = oracle.find(g, K, cases.critical(name), one, M, only_store_nodes=store)
            f = _finder(name, one, only_store_nodes=store)
            f.find()
            assert_same_records(finder_cols(f), exp)
            _assert_same_flat(_flat_cols(f.get_flat_kmers(v="1")), _expected_flat(g, exp))
            _assert_same_flat(_flat_cols(_device_flat(f, True)), _expected_flat(g, exp))
            f.close()


@pytest.mark.parametrize("name", ["bubbles", "planted_repeats"])
def test_whitelist(name):
    g, M = cases.graph(name), cases.max_variant_nodes(name)
    every = cases.oracle_records(name, True)
    white = set(every["kmers"][every["kmers"] % 7 == 0].tolist()) | {h for h, _, _ in cases.planted_hashes(g)} | {1, 2, 3}
    exp = oracle.find(g, K, cases.critical(name), True, M, whitelist=white)
    assert 0 < len(exp["kmers"]) < len(every["kmers"]) and np.count_nonzero(exp["start_offsets_wide"] >= 65536) > 0
    f = _finder(name, True, whitelist=white)
    f.find()
    assert_same_records(finder_cols(f), exp)
    _assert_same_flat(_flat_cols(f.get_flat_kmers(v="1")), _expected_flat(g, exp))
    _assert_same_flat(_flat_cols(_device_flat(f, True)), _expected_flat(g, exp))
    f.close()


# ------------------------------------------------------------------ critical paths, node classes, topological rank
@pytest.mark.parametrize("name", cases.VARIANT + ("linear_row", "linear_1000003"))
def test_critical_paths_classes_and_rank(name):
    from graph_kmer_index_amd import CriticalGraphPaths, _lib
    from graph_kmer_index_amd.kmer_finder import classify_nodes
    g, M = cases.graph(name), cases.max_variant_nodes(name)
    want = cases.critical(name)
    for dev in (True, False):
        cp = CriticalGraphPaths.from_graph(g, K, on_device=dev)
        assert np.array_equal(np.asarray(cp.nodes).astype(np.int64), want[0].astype(np.int64))
        assert np.array_equal(np.asarray(cp.offsets).astype(np.int64), want[1].astype(np.int64))
    assert np.all(want[1].astype(np.int64) < K)                   # why a uint16 critical offset is safe at any node size
    host = classify_nodes(g, K, M, None, want[0], on_device=False)
    device = classify_nodes(g, K, M, None, want[0], on_device=True)
    assert device[1] == host[1] and np.array_equal(device[0], host[0])
    rank = np.zeros(g.n_nodes, dtype=np.int32)
    _lib.check(_lib.load().gki_topological_rank(g.n_nodes, _lib.hptr(g.edge_start), _lib.hptr(g.edges), _lib.hptr(rank)))
    src = np.repeat(np.arange(g.n_nodes), np.diff(g.edge_start))
    assert np.all(rank[src] < rank[g.edges])


# ------------------------------------------------------------------ early-stop search
def _follow_sets(g):
    """None, and the non-linear successors of the long nodes (unique_variant_kmers.py:91-96 follows the variant's node)."""
    alts = [int(s) for n in cases.long_nodes(g).tolist() for s in g.edges[g.edge_start[n]:g.edge_start[n + 1]].tolist()
            if not g.is_ref[s]]
    return [None] + ([set(alts)] if alts else [])


@pytest.mark.parametrize("one", [False, True])
@pytest.mark.parametrize("name", EARLY_STOP_CASES)
def test_early_stop_search_from_deep_inside_long_nodes(name, one):
    from graph_kmer_index_amd import DenseKmerFinder
    g, M = cases.graph(name), cases.max_variant_nodes(name)
    nodes, offs = cases.early_stop_starts(g)
    for follow in _follow_sets(g):
        exp = oracle.find_from_positions(g, K, nodes, offs, one, M, only_follow_nodes=follow, with_records=True)
        assert np.count_nonzero(exp["start_offsets_wide"] >= 32768) >= 16
        f = DenseKmerFinder(g, K, only_save_one_node_per_kmer=one, max_variant_nodes=M, only_follow_nodes=follow)
        f.find_kmers_starting_at_positions(nodes, offs)
        assert_same_records(finder_cols(f), exp, exact_order=True)
        _assert_same_flat(_flat_cols(f.get_flat_kmers(v="1")), _expected_flat(g, exp), exact_order=True)
        _assert_same_flat(_flat_cols(f.get_flat_kmers(v="0")),
                          _expected_flat(g, exp, np.asarray(g.node_to_ref_offset)[:g.n_nodes]), exact_order=True)
        f.close()
        base = g.position_id_base() * 3 + 5
        fp = DenseKmerFinder(g, K, position_id=_Pid(base), only_save_one_node_per_kmer=one, max_variant_nodes=M,
                             only_follow_nodes=follow)
        half = len(nodes) // 2                    # records accumulate over calls
        fp.find_kmers_starting_at_positions(nodes[:half], offs[:half])
        fp.find_kmers_starting_at_positions(nodes[half:], offs[half:])
        _assert_same_flat(_flat_cols(fp.get_flat_kmers(v="1")), _expected_flat(g, exp, base), exact_order=True)
        fp.close()


@pytest.mark.parametrize("name", EARLY_STOP_CASES)
def test_early_stop_emit_from_the_script_and_walking_emit(name):
    # gki_forward_count leaves finished k-mers in a script (end offset packed into 16 bits) that the first emit call
    # expands; a second emit call with the same arguments walks again.  Both fill the int16 column with the true offset
    # modulo 2^16, and everything else as the oracle does.
    from graph_kmer_index_amd import DenseKmerFinder, _lib
    lib = _lib.load()
    g, M = cases.graph(name), cases.max_variant_nodes(name)
    nodes, offs = cases.early_stop_starts(g)
    dt = [np.int64, np.int32, np.int16, np.int32, np.float64]
    for follow in _follow_sets(g):
        f = DenseKmerFinder(g, K, only_save_one_node_per_kmer=False, max_variant_nodes=M)
        d_nodes, d_offs = _lib.DeviceArray.from_host(nodes), _lib.DeviceArray.from_host(offs)
        d_start = _lib.DeviceArray(len(nodes) + 1, np.int64)
        d_follow = None
        if follow is not None:
            mask = np.zeros(g.n_nodes, dtype=np.uint8)
            mask[sorted(follow)] = 1
            d_follow = _lib.DeviceArray.from_host(mask)
        n = C.c_int64(0)
        args = (f._device_graph().handle, K, M, 0, None if d_follow is None else d_follow.ptr, d_nodes.ptr, d_offs.ptr, len(nodes))
        _lib.check(lib.gki_forward_count(*args, d_start.ptr, C.byref(n)))
        exp = oracle.find_from_positions(g, K, nodes, offs, False, M, only_follow_nodes=follow, with_records=True)
        assert n.value == len(exp["kmers"]) > 0
        first = [_lib.DeviceArray(n.value, d) for d in dt]
        second = [_lib.DeviceArray(n.value, d) for d in dt]
        _lib.check(lib.gki_forward_emit(*args, d_start.ptr, *[b.ptr for b in first]))      # expands the script
        _lib.check(lib.gki_forward_emit(*args, d_start.ptr, *[b.ptr for b in second]))     # no script left: walks
        for cols in (first, second):
            a = [x.to_host() for x in cols]
            got = dict(kmers=a[0], start_nodes=a[1], start_offsets=a[2], nodes=a[3], allele_frequencies=a[4])
            assert_same_records(got, exp, exact_order=True)
            assert np.array_equal(a[2], exp["start_offsets_wide"].astype(np.int16))
        for x in first + second + [d_nodes, d_offs, d_start] + ([] if d_follow is None else [d_follow]):
            x.free()
        f.close()


# ------------------------------------------------------------------ UniqueVariantKmersFinder
def _planted_variant_graph(seed):
    """A chromosome whose variants lie more than 32 767, more than 65 536 and more than 131 072 bases into the linear node
    before them, one of them a 70 000-base deletion (its ref node is itself long).  Returns (graph, ref nodes, alt nodes,
    POS)."""
    from graph_kmer_index_amd.graph import GraphArrays
    rng = np.random.default_rng(seed)
    seq = "".join(rng.choice(list("acgt"), 620_000))
    other = lambda b: "acgt"[("acgt".index(b) + 1 + int(rng.integers(0, 3))) % 4]
    # (offset, ref allele length, alt allele)
    sites = [(60, 1, None), (40_000, 1, None), (40_050, 1, ""), (110_100, 1, None), (110_140, 70_000, ""), (180_200, 1, None),
             (320_000, 1, None), (320_020, 1, "gg"), (320_031, 1, None), (500_000, 1, None)]
    ns, ed, lin, refs, alts, pos = {}, {}, [], [], [], []
    nid = prev = 0
    for p, ref_len, alt in sites:
        ns[nid], ns[nid + 1] = seq[prev:p], seq[p:p + ref_len]
        ns[nid + 2] = other(seq[p]) if alt is None else alt
        ed[nid], ed[nid + 1], ed[nid + 2] = [nid + 1, nid + 2], [nid + 3], [nid + 3]
        lin += [nid, nid + 1]
        refs.append(nid + 1); alts.append(nid + 2); pos.append(p + 1)
        nid, prev = nid + 3, p + ref_len
    ns[nid] = seq[prev:]
    lin.append(nid)
    return GraphArrays.from_dicts(ns, ed, lin), np.array(refs), np.array(alts), np.array(pos)


@pytest.mark.parametrize("lowest,chunk_size", [(True, None), (False, None), (True, 3)])
def test_unique_variant_kmers_far_into_long_nodes(lowest, chunk_size):
    from graph_kmer_index_amd import CollisionFreeKmerIndex, DenseKmerFinder, _lib
    from graph_kmer_index_amd.device_graph import DeviceGraph
    from graph_kmer_index_amd.unique_variant_kmers import (LinearReference, UniqueVariantKmersFinder, VariantArrays,
                                                           VariantToNodesArrays)
    k, m = K, 6
    g, refs, alts, pos = _planted_variant_graph(3)
    assert g.node_size[refs].max() == 70_000
    # the frequency index, from true positions
    ff = DenseKmerFinder(g, k, max_variant_nodes=12)
    index = CollisionFreeKmerIndex.from_flat_kmers(_device_flat(ff, True), modulo=1_000_003)
    ff.close()
    # gki_uvk_starts against the host form
    dist = uvk_spec.start_distances(k)
    P, n_var = len(dist), len(pos)
    lin = LinearReference(g, g)
    ro = np.ascontiguousarray(pos.astype(np.int64))                          # one chromosome: graph ref offset = POS
    h = _lib.DeviceArray.from_host
    d_ls, d_ln, d_ro = h(lin.starts), h(lin.nodes), h(ro)
    d_nodes, d_offs, d_var = (_lib.DeviceArray(n_var * P, np.int32) for _ in range(3))
    bad = _lib._I64(-1)
    _lib.check(_lib.load().gki_uvk_starts(DeviceGraph.of(g).handle, d_ls.ptr, d_ln.ptr, len(lin.nodes), d_ro.ptr, n_var, P,
                                          d_nodes.ptr, d_offs.ptr, d_var.ptr, C.byref(bad)))
    _lib.check(_lib.load().gki_device_synchronize())
    assert bad.value == -1
    want_nodes, want_offs = lin.node_and_offset((ro[:, None] - np.asarray(dist)[None, :]).ravel())
    got_nodes, got_offs = d_nodes.to_host(), d_offs.to_host()
    for x in (d_ls, d_ln, d_ro, d_nodes, d_offs, d_var):
        x.free()
    assert np.array_equal(got_nodes, want_nodes) and np.array_equal(got_offs, want_offs)
    assert np.count_nonzero((want_offs > 32767) & (want_offs < 65536)) >= P
    assert np.count_nonzero(want_offs > 65536) >= P and np.count_nonzero(want_offs > 131072) >= P
    # the invariant k_uvk_emit relies on when it adds its int16 offset column to the position base: a record that is kept
    # touches the variant's node, the search stops at the first k-mer, so the window ends fewer than k bases into its node
    kept = 0
    for v in range(n_var):
        for j in range(P):
            rec = oracle.find_from_position(g, k, int(want_nodes[v * P + j]), int(want_offs[v * P + j]), False, m)
            keep = np.isin(rec["nodes"], [refs[v], alts[v]])
            assert np.all(rec["start_offsets_wide"][keep] < k)
            kept += int(keep.sum())
    assert kept > n_var
    # all four output columns against the spec
    ref_nodes, var_nodes = np.zeros(2 * n_var + 1, np.int64), np.zeros(2 * n_var + 1, np.int64)
    ref_nodes[1::2], var_nodes[1::2] = refs, alts
    lines = np.arange(n_var) * 2 + 1
    pid = _Pid(g.position_id_base())
    finder = UniqueVariantKmersFinder(g, VariantToNodesArrays(ref_nodes, var_nodes), VariantArrays(pos, 1, lines), k, m,
                                      kmer_index_with_frequencies=index, do_not_choose_lowest_frequency_kmers=not lowest,
                                      use_dense_kmer_finder=True, position_id_index=pid, chunk_size=chunk_size)
    got = finder.find_unique_kmers()
    exp = uvk_spec.unique_variant_kmers(g, ref_nodes, var_nodes, pos, lines, k, m, index.get_frequency, lowest, chunk_size)
    assert len(exp[0]) > n_var
    for a, b in zip((got._hashes, got._nodes, got._ref_offsets, got._allele_frequencies), exp):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    d = finder.find_unique_kmers_on_device()
    back = d.to_flat_kmers()
    d.free()
    for a, b in zip((back._hashes, back._nodes, back._ref_offsets, back._allele_frequencies), exp):
        assert np.array_equal(a, b)
    # positions of the kept records: beyond the first 65 536 bases of the graph, i.e. true positions were needed
    assert np.count_nonzero(got._ref_offsets > 131072) > 0


# ------------------------------------------------------------------ what flows into the indexes
def _reverse_index_numpy(nodes, kmers, refs):
    """the reference's ReverseKmerIndex.from_flat_kmers with a stable argsort (as tests/test_gpu_hash_index.py)"""
    order = np.argsort(nodes, kind="stable")
    snodes = nodes[order].astype(np.int64)
    first = np.flatnonzero(np.ediff1d(snodes, to_begin=1))
    uniq = snodes[first]
    index = np.zeros(int(nodes.max()) + 1, np.uint32)
    counts = np.zeros(int(nodes.max()) + 1, np.uint16)
    index[uniq] = first
    counts[uniq] = np.ediff1d(first, to_end=len(nodes) - first[-1]).astype(np.uint16)
    return index, counts, kmers[order], refs[order]


@pytest.mark.parametrize("route", ["device", "host_v1"])
def test_indexes_of_the_planted_repeats_count_two_positions(route):
    from graph_kmer_index_amd import CollisionFreeKmerIndex, FlatKmers, ReverseKmerIndex
    g = cases.graph("planted_repeats")
    exp = cases.oracle_records("planted_repeats", True)
    f = _finder("planted_repeats", True)
    if route == "device":
        flat = _device_flat(f, split_layout=False)
    else:
        f.find()
        flat = f.get_flat_kmers(v="1")
    f.close()
    cols = _flat_cols(flat)
    _assert_same_flat(cols, _expected_flat(g, exp), exact_order=True)
    modulo = 1_000_003
    flat = FlatKmers(cols[0], cols[1], cols[2].astype(np.uint64), cols[3])
    idx = CollisionFreeKmerIndex.from_flat_kmers(flat, modulo=modulo)
    want = oracle.index_build(exp["kmers"].astype(np.uint64), exp["nodes"].astype(np.uint32),
                              cases.expected_positions(g, exp).astype(np.uint64),
                              exp["allele_frequencies"].astype(np.float32), modulo=modulo)
    assert np.array_equal(idx._hashes_to_index, want["_hashes_to_index"]) and np.array_equal(idx._n_kmers, want["_n_kmers"])
    assert np.array_equal(idx._kmers, want["_kmers"]) and np.array_equal(idx._frequencies, want["_frequencies"])
    # inside a bucket the order is not contractual: compare the payload bucket by bucket as sets of rows
    rows = lambda i: np.lexsort((i["_ref_offsets"] if isinstance(i, dict) else i._ref_offsets,
                                 i["_kmers"] if isinstance(i, dict) else i._kmers))
    og, ow = rows(idx), rows(want)
    assert np.array_equal(np.asarray(idx._ref_offsets)[og].astype(np.uint64), want["_ref_offsets"][ow].astype(np.uint64))
    assert np.array_equal(np.asarray(idx._nodes)[og].astype(np.uint32), want["_nodes"][ow].astype(np.uint32))
    assert np.array_equal(np.asarray(idx._allele_frequencies)[og], want["_allele_frequencies"][ow])
    for h, first, second in cases.planted_hashes(g):
        assert np.asarray(idx._frequencies)[np.asarray(idx._kmers) == np.uint64(h)].tolist() == [2, 2]
        hits = np.asarray(idx._ref_offsets)[np.asarray(idx._kmers) == np.uint64(h)]
        assert sorted(int(x) for x in hits) == [first, second]
    r = ReverseKmerIndex.from_flat_kmers(flat)
    index, counts, skm, srf = _reverse_index_numpy(cols[1], cols[0], cols[2].astype(np.uint64))
    assert np.array_equal(r.nodes_to_index_positions, index) and np.array_equal(r.nodes_to_n_hashes, counts)
    assert np.array_equal(r.hashes, skm) and np.array_equal(r.ref_positions, srf)
