"""The index build at the edges of its tiles (csrc/gki_index_rows.hip): record counts one below, at and one above a tile
(512 x 8 rows in the build's passes, 256 x 8 in the bucket-range partition into columns), a chunk seam on a tile edge, and
the segmented tiles of the grouped build with a group of exactly one finish's capacity, an empty group and a group of one
row; and the pair-sorting form's 8-bit passes (csrc/gki_radix_tile.h, 256 x 16 pairs a tile) on keys crafted so that a digit's
run spans all tiles of a pass.  Every case is a few thousand records and compares element by element with the oracle's stable build or with a NumPy
stable argsort."""
import numpy as np
import pytest

from graph_kmer_index_amd import ReverseKmerIndex
from graph_kmer_index_amd.flat_kmers import FlatKmers, DeviceFlatKmers
from graph_kmer_index_amd.collision_free_kmer_index import (DeviceIndex, PartitionedDeviceIndex, bucket_range,
                                                            partition_by_bucket_range, partition_rows_by_bucket_range)
from oracle import oracle

pytestmark = pytest.mark.gpu

COLS = (("_hashes_to_index", "hashes_to_index"), ("_n_kmers", "n_kmers"), ("_kmers", "kmers"), ("_nodes", "nodes"),
        ("_ref_offsets", "ref_offsets"), ("_allele_frequencies", "allele_frequencies"), ("_frequencies", "frequencies"))


def _payload(kmers, rng):
    n = len(kmers)
    nodes = rng.integers(0, 1 << 24, size=n).astype(np.uint32)
    refs = (kmers % np.uint64(50)) + rng.integers(0, 30, size=n).astype(np.uint64)
    return nodes, refs, rng.uniform(0, 1, size=n).astype(np.float32)


def _records(n, seed, n_distinct=3000):
    """n records over exactly n_distinct k-mers (every one of them present), in random order"""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, 4 ** 31, size=n_distinct + 1000, dtype=np.uint64))[:n_distinct]
    kmers = rng.permutation(np.concatenate([pool, pool[rng.integers(0, n_distinct, size=n - n_distinct)]]))
    assert len(kmers) == n and len(np.unique(kmers)) == n_distinct
    return (kmers,) + _payload(kmers, rng)


def _check(dev, o, n, perm=None):
    for name, attr in COLS:
        got = getattr(dev, attr).to_host(len(o[name]) if name in ("_hashes_to_index", "_n_kmers") else n)
        assert np.array_equal(got, o[name]), name
    if perm is not None:
        assert np.array_equal(dev.permutation.to_host(n), perm)


# 1009: a 10-bit key, all but three bits of it sorted inside LDS; 65537: one pass; 1 << 21: two passes
@pytest.mark.parametrize("modulo", [1009, 65537, 1 << 21])
@pytest.mark.parametrize("n", [4095, 4096, 4097, 8192])
def test_build_from_columns_at_the_tile_edges(n, modulo):
    kmers, nodes, refs, af = _records(n, seed=n + modulo % 1000)
    o = oracle.index_build(kmers, nodes, refs, af, modulo=modulo)
    order = np.argsort(kmers % np.uint64(modulo), kind="stable").astype(np.uint32)
    d = DeviceFlatKmers.from_flat_kmers(FlatKmers(kmers, nodes, refs, af))
    for pairs in (False, True):
        for want_perm in (False, True):
            dev = DeviceIndex.build(d, modulo, want_permutation=want_perm, pairs_form=pairs)
            _check(dev, o, n, order if want_perm else None)
            dev.free()
    d.free()


def _one_run_keys(n, rng):
    """one low byte, five second bytes: pass 1 of the pair sort is ONE run across all tiles, pass 2 has to keep its order"""
    return np.uint64(0x5A) | (rng.choice(np.array([0x00, 0x01, 0x7F, 0x80, 0xFF], dtype=np.uint64), size=n) << np.uint64(8))


def _digit_255_keys(n, rng):
    """low byte 0xFF everywhere: in the partial last tile the real digit 255 sits beside the padding lanes"""
    return np.uint64(0xFF) | (rng.integers(0, 256, size=n).astype(np.uint64) << np.uint64(8))


# 4097 = a tile and one record, 3 * 4096 + 3 = three tiles and three records: the last tile is partial in both
@pytest.mark.parametrize("make_keys", [_one_run_keys, _digit_255_keys])
@pytest.mark.parametrize("n", [4097, 3 * 4096 + 3])
def test_pair_sort_is_stable_across_tiles_within_a_pass(n, make_keys):
    modulo = 65537                                              # every k-mer is below it: bucket = k-mer, three 8-bit passes
    rng = np.random.default_rng(n)
    kmers = make_keys(n, rng)
    assert kmers.max() < modulo
    nodes, refs, af = _payload(kmers, rng)
    o = oracle.index_build(kmers, nodes, refs, af, modulo=modulo)
    d = DeviceFlatKmers.from_flat_kmers(FlatKmers(kmers, nodes, refs, af))
    dev = DeviceIndex.build(d, modulo, want_permutation=True, pairs_form=True)
    _check(dev, o, n, np.argsort(kmers, kind="stable").astype(np.uint32))
    dev.free()
    d.free()


@pytest.mark.parametrize("form", ["rows", "pairs"])
@pytest.mark.parametrize("n_nodes", [1, 5000])
@pytest.mark.parametrize("n", [4095, 4096, 4097, 8192])
def test_reverse_index_at_the_tile_edges(n, n_nodes, form, monkeypatch):
    monkeypatch.setenv("GKI_REVERSE_FORM", form)              # read by the library per call
    rng = np.random.default_rng(n + n_nodes)
    nodes = rng.integers(0, n_nodes, size=n).astype(np.uint32)
    nodes[n // 2] = n_nodes - 1                                # the directory has exactly n_nodes entries
    kmers = rng.integers(0, 4 ** 31, size=n, dtype=np.uint64)
    refs = rng.integers(0, 2 ** 40, size=n, dtype=np.uint64)
    r = ReverseKmerIndex.from_flat_kmers(FlatKmers(kmers, nodes, refs))
    order = np.argsort(nodes, kind="stable")
    counts = np.bincount(nodes, minlength=n_nodes)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    assert np.array_equal(r.nodes_to_index_positions, np.where(counts > 0, first, 0).astype(np.uint32))
    assert np.array_equal(r.nodes_to_n_hashes, counts.astype(np.uint16))
    assert np.array_equal(r.hashes, kmers[order]) and np.array_equal(r.ref_positions, refs[order])


def _owner(buckets, modulo, n_parts):
    begins = np.array([bucket_range(modulo, n_parts, p)[0] for p in range(n_parts)], dtype=np.uint64)
    return begins, np.searchsorted(begins, buckets, side="right") - 1


# 8 parts: a power of two (no table, the few-digit histogram); 3 parts: the part table in LDS.  max_rows_per_pass = 2048: a
# chunk seam on a tile edge
@pytest.mark.parametrize("max_rows_per_pass", [0, 2048])
@pytest.mark.parametrize("n_parts", [8, 3])
@pytest.mark.parametrize("n", [2047, 2048, 2049, 4096])
def test_partition_into_columns_at_the_tile_edges(n, n_parts, max_rows_per_pass):
    modulo = 100003
    kmers, nodes, refs, af = _records(n, seed=n + n_parts, n_distinct=1500)
    _, owner = _owner(kmers % np.uint64(modulo), modulo, n_parts)
    order = np.argsort(owner, kind="stable")
    d = DeviceFlatKmers.from_flat_kmers(FlatKmers(kmers, nodes, refs, af))
    part, start = partition_by_bucket_range(d, modulo, n_parts, max_rows_per_pass=max_rows_per_pass)
    got = part.to_flat_kmers()
    for name, col in (("_hashes", kmers), ("_nodes", nodes), ("_ref_offsets", refs), ("_allele_frequencies", af)):
        assert np.array_equal(getattr(got, name), col[order]), name
    assert start == np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n_parts))]).tolist()
    part.free()
    d.free()


@pytest.mark.parametrize("group_bits", [0, 4])
@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_partition_into_rows_at_the_tile_edges(n, group_bits):
    modulo, n_parts = 100003, 8
    kmers, nodes, refs, af = _records(n, seed=n + group_bits)
    buckets = kmers % np.uint64(modulo)
    begins, owner = _owner(buckets, modulo, n_parts)
    digit = np.zeros(n, dtype=np.int64)
    for p in range(n_parts):
        lo, hi = bucket_range(modulo, n_parts, p)
        sel = owner == p
        kb = int(hi - lo - 1).bit_length()
        digit[sel] = (p << group_bits) | ((buckets[sel] - np.uint64(lo)) >> np.uint64(max(0, kb - group_bits))).astype(np.int64)
    order = np.argsort(digit, kind="stable")
    d = DeviceFlatKmers.from_flat_kmers(FlatKmers(kmers, nodes, refs, af))
    rows, start = partition_rows_by_bucket_range(d, modulo, n_parts, group_bits=group_bits)
    assert start == np.concatenate([[0], np.cumsum(np.bincount(digit, minlength=n_parts << group_bits))]).tolist()
    r = rows.rows.to_host(3 * n).reshape(n, 3)
    assert np.array_equal(r[:, 0], kmers[order]) and np.array_equal(r[:, 1], refs[order])
    assert np.array_equal(r[:, 2], nodes[order].astype(np.uint64) | (af[order].view(np.uint32).astype(np.uint64) << np.uint64(32)))
    assert np.array_equal(rows.keys.to_host(n), (buckets - begins[owner])[order].astype(np.uint32))
    rows.free()
    d.free()


# rows of the four groups (bucket >> 10 of a 12-bit key).  4096: exactly what one finish workgroup of the grouped build
# holds and exactly one tile; 0: a group without a tile; 1: a tile of one row.  An ordinary group of 3000 rows leaves
# nothing to sort between the grouping and the finish (from columns: one pass that only packs the rows; from rows: none);
# one of 12000 makes the records dense enough that one key bit is left to a real segmented pass in both
@pytest.mark.parametrize("sizes", [(3000, 4096, 0, 1), (4096, 0, 1, 3000), (0, 1, 3000, 4096), (1, 4096, 0, 12000),
                                   (12000, 0, 4096, 1)])
def test_grouped_build_with_crafted_group_sizes(sizes):
    modulo, g = 4093, 2                                         # buckets 0 .. 4092: a 12-bit key, groups of 1024 buckets
    rng = np.random.default_rng(sum(s * (i + 1) for i, s in enumerate(sizes)))
    buckets = np.concatenate([rng.integers(1024 * i, min(1024 * (i + 1), modulo), size=s) for i, s in enumerate(sizes)])
    buckets = rng.permutation(buckets).astype(np.uint64)
    kmers = buckets + np.uint64(modulo) * rng.integers(0, 3, size=len(buckets)).astype(np.uint64)     # k-mers repeat
    nodes, refs, af = _payload(kmers, rng)
    n = len(kmers)
    full = oracle.index_build(kmers, nodes, refs, af, modulo=modulo)
    want_start = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    d = DeviceFlatKmers.from_flat_kmers(FlatKmers(kmers, nodes, refs, af))
    part, start = partition_by_bucket_range(d, modulo, 1, group_bits=g)
    rows, start_r = partition_rows_by_bucket_range(d, modulo, 1, group_bits=g)
    assert start == want_start and start_r == want_start
    for src in (part, rows):
        for skip in (False, True):
            dev = PartitionedDeviceIndex.build_slice(src, start, modulo, 1, 0, g, skip_frequencies=skip)
            assert dev.n == n
            for name, attr in COLS:
                if skip and name == "_frequencies":
                    continue
                got = getattr(dev, attr).to_host(len(full[name]) if name in ("_hashes_to_index", "_n_kmers") else n)
                assert np.array_equal(got, full[name]), (name, skip)
            dev.free()
    # from columns with the permutation wanted: the row's input index rides through the segmented pass
    dev = DeviceIndex.build(part, modulo, want_permutation=True, group_start=start)
    _check(dev, full, n, np.argsort(part.to_flat_kmers()._hashes % np.uint64(modulo), kind="stable").astype(np.uint32))
    dev.free()
    rows.free()
    part.free()
    d.free()
