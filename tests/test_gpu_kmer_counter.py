"""The k-mer counter on the device: unique keys with counts (csrc/gki_count.hip) at the sort's tile boundaries, the
counter's batched lookup, KmerCounter / KmerFrequencyIndex, the counter as frequency source of the variant-signature
finders, and the command line.  Everything is compared exactly, values and dtypes, with tests/spec_kmer_counter.py and
the outputs recorded from the reference (tests/golden/kmer_counter_reference.json.gz)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import spec_kmer_counter as spec
import spec_structural_variants as spec_sv
import uvk_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SV = {c["name"]: c for c in spec_sv.load_cases()}
UVK = {c["name"]: c for c in uvk_golden.load_cases()}


def _tile():
    from graph_kmer_index_amd.kmer_counter import SORT_TILE
    src = open(os.path.join(ROOT, "graph_kmer_index_amd", "csrc", "gki_count.hip")).read()
    assert "constexpr int CB = 256;" in src and "constexpr int CI = 16;" in src and SORT_TILE == 256 * 16
    return SORT_TILE


def _check(kmers, stride=1, key_bits=None, device=False):
    """unique_counts of the package against the spec; the input must come back unchanged."""
    from graph_kmer_index_amd import _lib
    from graph_kmer_index_amd.kmer_counter import unique_counts
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
    before = kmers.copy()
    if device:
        d = _lib.DeviceArray.from_host(kmers) if len(kmers) else _lib.DeviceArray(0, np.uint64)
        u, c = unique_counts(d, stride, key_bits)
        assert np.array_equal(d.to_host(), before)
        d.free()
    else:
        u, c = unique_counts(kmers, stride, key_bits)
    assert np.array_equal(kmers, before)
    eu, ec = spec.unique_counts(before, stride)
    assert u.dtype == np.uint64 and c.dtype == np.int64
    assert len(u) == len(eu) and np.array_equal(u, eu) and np.array_equal(c, ec)
    assert int(c.sum()) == len(before[::stride])
    return u, c


# ------------------------------------------------------------------ unique keys with counts
def _sizes():
    T = 4096
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 3]


@pytest.mark.parametrize("n", _sizes())
def test_sizes_at_the_tile_boundaries(n):
    assert _tile() == 4096
    rng = np.random.default_rng(n)
    _check(rng.integers(0, 1 << 62, size=n, dtype=np.uint64), key_bits=62, device=True)       # (almost) all distinct
    _check(rng.integers(0, 50, size=n, dtype=np.uint64))                                      # long runs, key_bits from the maximum
    _check(rng.integers(0, max(1, n // 3), size=n, dtype=np.uint64) << np.uint64(30), key_bits=64, device=True)


def test_one_run_across_tiles_counts_above_65535():
    u, c = _check(np.full(70000, 0x2AAAAAAAAAAAAAAA, dtype=np.uint64), key_bits=62, device=True)
    assert u.tolist() == [0x2AAAAAAAAAAAAAAA] and c.tolist() == [70000]


def test_all_keys_distinct():
    T = _tile()
    rng = np.random.default_rng(3)
    keys = rng.permutation(5 * T + 17).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15 >> 3) % np.uint64(1 << 62)
    assert len(np.unique(keys)) == len(keys)
    u, c = _check(keys, key_bits=62)
    assert (c == 1).all()


def test_a_run_from_the_last_lane_of_a_tile_to_the_first_lane_of_the_next():
    T = _tile()
    rng = np.random.default_rng(4)
    sorted_keys = np.concatenate([np.arange(T - 1), [T + 5, T + 5], T + 10 + np.arange(T - 1)]).astype(np.uint64)
    assert sorted_keys[T - 1] == sorted_keys[T] and sorted_keys[T - 2] != sorted_keys[T - 1] != sorted_keys[T + 1]
    u, c = _check(rng.permutation(sorted_keys), device=True)
    assert c[T - 1] == 2 and c.sum() == 2 * T


def test_keys_that_differ_in_one_digit_only():
    rng = np.random.default_rng(5)
    base = np.uint64(0x00AB_CDEF_0123_4500)
    top = base | (rng.integers(0, 64, size=6000, dtype=np.uint64) << np.uint64(56))           # bits 56..61: the top digit of 62
    u, _ = _check(top, key_bits=62, device=True)
    assert len(u) == 64
    bottom = base | rng.integers(0, 256, size=6000, dtype=np.uint64)
    u, _ = _check(bottom, key_bits=62)
    assert len(u) == 256


@pytest.mark.parametrize("key_bits", [2, 8, 9, 62, 64])
def test_key_bits_with_both_extremes_present(key_bits):
    rng = np.random.default_rng(key_bits)
    top = (1 << key_bits) - 1
    keys = rng.integers(0, top, size=9000, dtype=np.uint64, endpoint=True)
    keys[[17, 4500, 8999]] = top
    keys[[0, 4096]] = 0
    for device in (False, True):
        u, _ = _check(keys, key_bits=key_bits, device=device)
        assert int(u[0]) == 0 and int(u[-1]) == top


def test_a_key_outside_key_bits_is_refused():
    from graph_kmer_index_amd import _lib
    from graph_kmer_index_amd.kmer_counter import unique_counts
    with pytest.raises(_lib.GkiError, match="key_bits"):
        unique_counts(np.array([1, 2, 1 << 9, 3], dtype=np.uint64), key_bits=9)
    for bad in (0, 65):
        with pytest.raises(_lib.GkiError):
            unique_counts(np.array([1], dtype=np.uint64), key_bits=bad)


@pytest.mark.parametrize("stride", [1, 2, 3, 7])
def test_stride_with_a_remainder(stride):
    T = _tile()
    rng = np.random.default_rng(stride)
    n = stride * (T + 5) + (stride - 1 if stride > 1 else 0)
    assert stride == 1 or n % stride
    keys = rng.integers(0, 3000, size=n, dtype=np.uint64) * np.uint64(0x1_0000_0001)
    _check(keys, stride=stride, device=True)
    _check(keys, stride=stride, key_bits=64)
    with pytest.raises(ValueError):
        _check(keys, stride=0)


# ------------------------------------------------------------------ the counter's lookup
def _lookup(keys, counts, queries):
    from graph_kmer_index_amd import KmerCounter
    c = KmerCounter(keys, counts)
    got = c.get_frequencies(np.asarray(queries, dtype=np.uint64))
    table = dict(zip(np.asarray(keys).tolist(), np.asarray(counts).tolist()))
    assert got.dtype == np.int64
    assert got.tolist() == [table.get(int(q), 0) for q in queries]
    return c


def test_lookup_empty_counter_and_no_queries():
    c = _lookup(np.zeros(0, np.uint64), np.zeros(0, np.int64), [0, 5, (1 << 64) - 1])
    assert len(c.get_frequencies(np.zeros(0, np.uint64))) == 0
    assert c.get_frequency(7) == 0 and c.score_kmers([1, 2]) == 1
    c = _lookup(np.array([9], np.uint64), np.array([4], np.int64), [])
    assert c.get_frequencies(np.array([9, 8, 10], np.uint64)).tolist() == [4, 0, 0]


def test_lookup_around_the_keys():
    keys = np.array([100, 101, 5000, 1 << 40, (1 << 61) + 12345], dtype=np.uint64)
    counts = np.array([3, 1, 70000, 1 << 35, 2], dtype=np.int64)
    _lookup(keys, counts, [0, 99, 100, 101, 102, 4999, 5000, 5001, (1 << 40) - 1, 1 << 40, (1 << 61) + 12345,
                           (1 << 61) + 12346, (1 << 62) - 1, 1 << 62, (1 << 64) - 1])


def test_lookup_one_crowded_bucket_beside_sparse_ones():
    rng = np.random.default_rng(8)
    dense = (np.uint64(1) << np.uint64(50)) + np.arange(0, 10000, 2, dtype=np.uint64)          # 5 000 keys, one directory bucket
    sparse = rng.integers(0, 1 << 62, size=3000, dtype=np.uint64)
    keys = np.unique(np.concatenate([dense, sparse]))
    counts = rng.integers(1, 1 << 40, size=len(keys), dtype=np.int64)
    queries = np.concatenate([keys, dense + np.uint64(1), sparse + np.uint64(1), rng.integers(0, 1 << 62, size=2000, dtype=np.uint64)])
    _lookup(keys, counts, rng.permutation(queries))


# ------------------------------------------------------------------ KmerCounter
class _Flat:
    def __init__(self, hashes):
        self._hashes = hashes


@pytest.mark.parametrize("ratio", [1, 3])
def test_kmer_counter_from_flat_and_accessors(ratio, tmp_path):
    from graph_kmer_index_amd import KmerCounter
    from graph_kmer_index_amd.kmer_counter import choose_modulo
    rng = np.random.default_rng(20 + ratio)
    hashes = rng.integers(0, 4000, size=20001, dtype=np.uint64) * np.uint64(0x3_0000_0007)
    flat = _Flat(hashes)
    c = KmerCounter.from_flat_kmersv2(flat, 0, subsample_ratio=ratio) if ratio > 1 else KmerCounter.from_flat_kmersv2(flat, 0)
    eu, ec = spec.unique_counts(hashes, ratio)
    assert c._kmers.dtype == np.uint64 and c._counts.dtype == np.int64
    assert np.array_equal(c._kmers, eu) and np.array_equal(c._counts, ec)
    assert c._modulo == choose_modulo(len(eu)) == 2000003
    assert KmerCounter.from_flat_kmersv2(flat, 1000003, ratio)._modulo == 1000003
    table = spec.DictCounter(eu, ec)
    probes = [int(eu[0]), int(eu[-1]), int(eu[len(eu) // 2]), int(eu[0]) + 1, 0, (1 << 62) - 1]
    assert [c.get_frequency(q) for q in probes] == [table.get_frequency(q) for q in probes]
    assert isinstance(c.get_frequency(probes[0]), int)
    q = np.concatenate([hashes[:500], hashes[:500] + np.uint64(1)])
    assert c.get_frequencies(q).tolist() == [table.get_frequency(x) for x in q]
    present = [int(x) for x in eu[:7]]
    assert c.score_kmers(present + [1, 2]) == -max(table.get_frequency(x) for x in present)
    assert c.score_kmers([1, 2, 4]) == 1 and c.score_kmers([]) == 1
    if ratio == 1:
        same = KmerCounter.from_flat_kmers(flat, 0)
        assert np.array_equal(same._kmers, eu) and np.array_equal(same._counts, ec)
        assert not os.path.exists("debugging.npy")
    c.to_file(str(tmp_path / "counter"))
    assert sorted(np.load(tmp_path / "counter.npz").files) == ["counts", "kmers", "modulo"]
    for name in ("counter", "counter.npz"):
        back = KmerCounter.from_file(str(tmp_path / name))
        assert np.array_equal(back._kmers, eu) and np.array_equal(back._counts, ec) and back._modulo == c._modulo
        assert back._kmers.dtype == np.uint64 and back._counts.dtype == np.int64
    with pytest.raises(FileNotFoundError):
        KmerCounter.from_file(str(tmp_path / "missing"))


def test_choose_modulo_values():
    from graph_kmer_index_amd.kmer_counter import choose_modulo
    assert [choose_modulo(n) for n in (0, 999999, 1000000, 9999999, 10000000)] == \
        [2000003, 2000003, 19999999, 19999999, 200000003]


# ------------------------------------------------------------------ KmerFrequencyIndex
def test_kmer_frequency_index_equals_the_recorded_reference(tmp_path):
    from graph_kmer_index_amd import KmerFrequencyIndex, _lib
    rec = spec.golden()["frequency_index"]
    for name, kmers in spec.frequency_index_inputs().items():
        idx = KmerFrequencyIndex.from_kmers(kmers)
        assert (str(idx._kmers.dtype), str(idx._frequencies.dtype)) == (rec[name]["dtypes"]["kmers"], rec[name]["dtypes"]["frequencies"])
        assert idx._kmers.tolist() == rec[name]["kmers"] and idx._frequencies.tolist() == rec[name]["frequencies"]
        d = _lib.DeviceArray.from_host(kmers)
        from_device = KmerFrequencyIndex.from_kmers(d)
        assert np.array_equal(from_device._kmers, idx._kmers) and np.array_equal(from_device._frequencies, idx._frequencies)
        # get: as the reference's on the same arrays (side="right": a present k-mer is a miss; past the end an IndexError)
        for q, want in zip(rec[name]["probes"], rec[name]["get"]):
            if want == "IndexError":
                with pytest.raises(IndexError):
                    idx.get(np.uint64(q))
            else:
                assert int(idx.get(np.uint64(q))) == want
        table = spec.DictCounter(idx._kmers, idx._frequencies)
        assert idx.get_frequencies(rec[name]["probes"][:-1]).tolist() == [table.get_frequency(q) for q in rec[name]["probes"][:-1]]
        idx.to_file(str(tmp_path / name))
        assert sorted(np.load(tmp_path / (name + ".npz")).files) == ["frequencies", "kmers"]
        for fn in (name, name + ".npz"):
            back = KmerFrequencyIndex.from_file(str(tmp_path / fn))
            assert np.array_equal(back._kmers, idx._kmers) and np.array_equal(back._frequencies, idx._frequencies)
            assert back._kmers.dtype == np.uint64 and back._frequencies.dtype == np.int64


# ------------------------------------------------------------------ the counter as frequency source
def _counter_of(case):
    from graph_kmer_index_amd import KmerCounter
    return KmerCounter(np.array(case["index"]["hashes"], dtype=np.uint64), np.array(case["index"]["counts"], dtype=np.int64))


def _same(flat, exp):
    got = (flat._hashes, flat._nodes, flat._ref_offsets, flat._allele_frequencies)
    for name, a, b in zip(("hashes", "nodes", "ref_offsets", "allele_frequencies"), got, exp):
        assert a.dtype == b.dtype, name
        assert len(a) == len(b) and np.array_equal(a, b), name


@pytest.mark.parametrize("name", spec.SV_CASES)
def test_sv_with_a_kmer_counter_equals_the_recorded_reference(name):
    from graph_kmer_index_amd.structural_variants import (sample_kmers_from_structural_variants,
                                                          sample_kmers_from_structural_variants_on_device)
    case = SV[name]
    exp = spec.flat_columns(spec.golden()["sv"][name])
    g, counter = spec_sv.case_graph(case), _counter_of(case)
    pairs = [tuple(p) for p in case["pairs"]]
    _same(sample_kmers_from_structural_variants(g, pairs, counter, case["k"], case["max_frequency"]), exp)
    d = sample_kmers_from_structural_variants_on_device(g, pairs, counter, case["k"], case["max_frequency"])
    flat = d.to_flat_kmers()
    d.free()
    assert np.array_equal(flat._hashes, exp[0]) and np.array_equal(flat._nodes, exp[1])


def test_sv_case_where_the_missing_reverse_complement_decides():
    """max_frequency_2 has windows whose own count is 0 while their reverse complement's is >= max_frequency: valid for a
    KmerCounter, not for a CollisionFreeKmerIndex of the same (hash, count) table."""
    from graph_kmer_index_amd import CollisionFreeKmerIndex
    from graph_kmer_index_amd.structural_variants import sample_kmers_from_structural_variants
    case = SV["max_frequency_2"]
    g, t = spec_sv.case_graph(case), spec_sv.case_table(case)
    deciding = []
    for node in np.asarray(case["pairs"]).reshape(-1).tolist():
        if g.get_node_size(node) > case["k"] + 5:
            h = spec_sv.window_hashes(g.get_numeric_node_sequence(node), case["k"])
            deciding += h[(t.first_hit(h) == 0) & (t.first_hit(spec_sv.revcomp(h, 31)) >= case["max_frequency"])].tolist()
    assert deciding
    with_counter = sample_kmers_from_structural_variants(g, case["pairs"], _counter_of(case), case["k"], case["max_frequency"])
    index = CollisionFreeKmerIndex.from_flat_kmers(spec_sv.case_index_flat(case), modulo=case["index"]["modulo"])
    with_index = sample_kmers_from_structural_variants(g, case["pairs"], index, case["k"], case["max_frequency"])
    _same(with_counter, spec.flat_columns(spec.golden()["sv"]["max_frequency_2"]))
    _same(with_index, spec_sv.expected(case))
    assert with_counter._hashes.tolist() != with_index._hashes.tolist()
    assert set(with_counter._hashes.tolist()) & set(deciding) and not set(with_index._hashes.tolist()) & set(deciding)


class _Pid:
    def __init__(self, base):
        self._base = np.asarray(base, dtype=np.int64)

    def get(self, nodes, offsets):
        return self._base[np.asarray(nodes, dtype=np.int64)] + np.asarray(offsets, dtype=np.int64)


@pytest.mark.parametrize("name", spec.UVK_CASES)
def test_uvk_with_a_kmer_counter_equals_the_recorded_reference(name):
    from graph_kmer_index_amd.unique_variant_kmers import UniqueVariantKmersFinder, VariantArrays, VariantToNodesArrays
    case = UVK[name]
    g = uvk_golden.case_graph(case)
    v = case["variants"]
    f = UniqueVariantKmersFinder(g, VariantToNodesArrays(case["ref_nodes"], case["var_nodes"]),
                                 VariantArrays(v["positions"], v["chromosomes"], v["lines"]), case["k"],
                                 case["max_variant_nodes"], kmer_index_with_frequencies=_counter_of(case),
                                 do_not_choose_lowest_frequency_kmers=not case["lowest"], use_dense_kmer_finder=True,
                                 position_id_index=_Pid(g.position_id_base()), chunk_size=case["chunk_size"])
    exp = spec.flat_columns(spec.golden()["uvk"][name])
    want = (exp[0].astype(np.uint64), exp[1].astype(np.uint32), exp[2].astype(np.uint64), exp[3].astype(np.float32))
    _same(f.find_unique_kmers(), want)


def test_other_frequency_sources_are_still_refused():
    from graph_kmer_index_amd.structural_variants import sample_kmers_from_structural_variants
    from graph_kmer_index_amd.unique_variant_kmers import UniqueVariantKmersFinder
    case = SV["greedy_rule"]
    with pytest.raises(NotImplementedError):
        sample_kmers_from_structural_variants(spec_sv.case_graph(case), case["pairs"], spec.DictCounter([], []), 31)
    with pytest.raises(NotImplementedError):
        UniqueVariantKmersFinder(spec_sv.case_graph(case), None, [], kmer_index_with_frequencies=spec.DictCounter([], []),
                                 use_dense_kmer_finder=True, position_id_index=object())


# ------------------------------------------------------------------ command line
def _run_cli(args, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, "-m", "graph_kmer_index_amd.command_line_interface"] + args, check=True, env=env,
                   cwd=str(tmp_path))


def test_cli_count_kmers_then_both_consumers_equal_the_api(tmp_path):
    from graph_kmer_index_amd import DenseKmerFinder, FlatKmers, KmerCounter
    from graph_kmer_index_amd.graph import synthetic_snp_graph
    from graph_kmer_index_amd.structural_variants import sample_kmers_from_structural_variants
    from graph_kmer_index_amd.unique_variant_kmers import UniqueVariantKmersFinder, VariantArrays, VariantToNodesArrays
    from uvk_cases import bubble_variants
    g = synthetic_snp_graph(4000, 50, k=31, seed=7)
    refs, alts, pos = bubble_variants(g, 31)
    f = DenseKmerFinder(g, 31, max_variant_nodes=4)
    f.find()
    flat = f.get_flat_kmers(v="1")
    h = np.asarray(flat._hashes).astype(np.uint64)
    keep = h % np.uint64(3) != 0
    flat = FlatKmers(np.concatenate([h[keep], h[keep][::2]]), np.zeros(keep.sum() + len(h[keep][::2]), np.uint32),
                     np.zeros(keep.sum() + len(h[keep][::2]), np.uint64))
    flat.to_file(str(tmp_path / "flat"))
    g.to_file(str(tmp_path / "graph.npz"))
    VariantToNodesArrays(refs, alts).to_file(str(tmp_path / "v2n.npz"))
    big = np.nonzero(g.node_size > 31 + 5)[0]
    sv_pairs = VariantToNodesArrays(big, np.concatenate([big[1:], [0]]))
    sv_pairs.to_file(str(tmp_path / "sv_v2n.npz"))
    with open(tmp_path / "v.vcf", "w") as fh:
        fh.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n")
        for p in pos:
            fh.write("1\t%d\t.\tA\tC\n" % p)
    _run_cli(["count_kmers", "-f", "flat.npz", "-o", "counter", "-s", "2"], tmp_path)
    counter = KmerCounter.from_file(str(tmp_path / "counter"))
    eu, ec = spec.unique_counts(flat._hashes, 2)
    assert np.array_equal(counter._kmers, eu) and np.array_equal(counter._counts, ec) and counter._modulo == 2000003
    _run_cli(["make_unique_variant_kmers", "-g", "graph.npz", "-V", "v2n.npz", "-k", "31", "-D", "True", "-I", "counter",
              "-v", "v.vcf", "-o", "uvk"], tmp_path)
    _run_cli(["sample_kmers_from_structural_variants", "-g", "graph.npz", "-V", "sv_v2n.npz", "-k", "31", "-I", "counter.npz",
              "-o", "sv"], tmp_path)
    api_uvk = UniqueVariantKmersFinder(g, VariantToNodesArrays(refs, alts), VariantArrays(pos, "1", np.arange(len(pos))), 31,
                                       kmer_index_with_frequencies=counter, use_dense_kmer_finder=True,
                                       position_id_index=_Pid(g.position_id_base()), chunk_size=10000).find_unique_kmers()
    api_sv = sample_kmers_from_structural_variants(g, sv_pairs, counter, 31)
    assert len(api_uvk._hashes) > 0 and len(api_sv._hashes) > 0
    for name, api in (("uvk", api_uvk), ("sv", api_sv)):
        cli = np.load(tmp_path / (name + ".npz"))
        for key, a in (("hashes", api._hashes), ("nodes", api._nodes), ("ref_offsets", api._ref_offsets),
                       ("allele_frequencies", api._allele_frequencies)):
            assert cli[key].dtype == a.dtype and np.array_equal(cli[key], a), (name, key)
    exp = spec_sv.sample_kmers(g, np.stack([sv_pairs.ref_nodes, sv_pairs.var_nodes], axis=1),
                               spec.NoReverseComplementTable(eu, ec), 31, 2)
    assert np.array_equal(api_sv._hashes, exp[0]) and np.array_equal(api_sv._nodes, exp[1])
