"""CPU tests of the linear-reference path: the NumPy spec (tests/spec_linear_reference.py) against the golden file and,
where the reference checkout is present, against the reference itself; the three readings of the reference that decide
the format of `make -R`, each asserted once; and the host-only parts of the product (segment table, FASTA reader,
ReferenceKmerIndex.from_flat_kmers, the sub-commands' options)."""
import logging
import os
import sys

import numpy as np
import pytest

import conftest
import spec_linear_reference as spec
from linref_cases import load_golden, random_sequence

from graph_kmer_index_amd import FlatKmers, ReferenceKmerIndex, SnpKmerFinder
from graph_kmer_index_amd import snp_kmer_finder as skf
from graph_kmer_index_amd.command_line_interface import build_parser, main


@pytest.fixture(scope="module")
def reference():
    """The reference's modules (Bio and friends come from tests/standins)."""
    paths = [os.path.join(conftest.ROOT, "tests", "standins"), conftest.REFERENCE]
    sys.path[:0] = paths
    logging.disable(logging.CRITICAL)
    try:
        from graph_kmer_index.snp_kmer_finder import SnpKmerFinder as RefFinder
        from graph_kmer_index.flat_kmers import FlatKmers as RefFlat
        from graph_kmer_index.reference_kmer_index import ReferenceKmerIndex as RefIndex
        yield dict(SnpKmerFinder=RefFinder, FlatKmers=RefFlat, ReferenceKmerIndex=RefIndex)
    finally:
        logging.disable(logging.NOTSET)
        for p in paths:
            sys.path.remove(p)


def _text(seq):
    return seq.tobytes().decode("ascii")


# ------------------------------------------------------------------------------------------ spec against the golden file
def test_spec_equals_golden_reference_outputs():
    cases, index = load_golden()
    assert len(cases) >= 24
    for c in cases:
        got = spec.make_columns(c["seq"], c["k"], c["spacing"], c["G"], c["t"], c["rc"])
        for col in ("hashes", "nodes", "allele_frequencies"):
            assert got[col].dtype == c[col].dtype, (c["name"], col)
            assert np.array_equal(got[col], c[col]), (c["name"], col)
    for k in (16, 17):
        kmers = spec.window_hashes(index[k]["seq"], k)
        assert np.array_equal(kmers.astype(index[k]["kmers"].dtype), index[k]["kmers"])
        assert index[k]["kmers"].dtype == (np.uint32 if k <= 16 else np.uint64)
        assert np.array_equal(index[k]["ref_position_to_index"], np.arange(len(index[k]["seq"]), dtype=np.uint32))


def test_spec_shift_form_equals_convolution():
    rng = np.random.default_rng(5)
    for k in (1, 2, 15, 16, 31):
        seq = random_sequence(rng, 500)
        assert np.array_equal(spec.window_hashes(seq, k), spec.window_hashes_by_shifts(seq, k))


# ------------------------------------------------------------------------------------------ against the live reference
@pytest.mark.reference
def test_spec_equals_reference_on_random_cases(reference):
    rng = np.random.default_rng(11)
    for _ in range(40):
        k = int(rng.choice([1, 3, 8, 16, 17, 31]))
        spacing = int(rng.choice([1, 2, 5, 31, 40]))
        seq = random_sequence(rng, int(rng.integers(k + 40, 1500)))
        start = int(rng.integers(0, len(seq) - k))
        end = int(rng.integers(start, len(seq) + 50))
        ref = reference["SnpKmerFinder"](None, k=k, spacing=spacing, start_position=start, end_position=end,
                                         reference=_text(seq)).find_kmers()
        hashes, positions = spec.interval_records(seq, k, spacing, start, end)
        assert np.array_equal(ref._hashes, hashes) and ref._hashes.dtype == np.uint64
        assert np.array_equal(ref._nodes, np.ones(len(hashes), dtype=np.uint32)) and ref._nodes.dtype == np.uint32
        assert np.array_equal(ref._allele_frequencies, np.ones(len(hashes), dtype=np.float32))
        assert ref._allele_frequencies.dtype == np.float32
        rc = ref.get_reverse_complement_flat_kmers(k)
        assert np.array_equal(np.asarray(rc._hashes, dtype=np.uint64), spec.reverse_complement_hashes(hashes, k))
        # where the reference's offsets are aligned with its hashes (their common prefix) they are the positions
        assert np.array_equal(ref._ref_offsets[:len(positions)], positions)


@pytest.mark.reference
def test_reference_single_thread_make_cannot_work(reference):
    """`make -t 1 -R`: interval=None leaves end_position=None (command_line_interface.py:44-49) and the finder adds k to it."""
    with pytest.raises(TypeError):
        reference["SnpKmerFinder"](None, k=5, spacing=1, start_position=None, end_position=None,
                                   reference="ACGTACGTACGTACGTACGT").find_kmers()


@pytest.mark.reference
def test_reference_ref_offsets_are_longer_than_hashes(reference):
    seq = _text(random_sequence(np.random.default_rng(3), 60))
    flat = reference["SnpKmerFinder"](None, k=5, spacing=1, start_position=0, end_position=40, reference=seq).find_kmers()
    assert (len(flat._hashes), len(flat._ref_offsets)) == (41, 45)
    flat = reference["SnpKmerFinder"](None, k=7, spacing=3, start_position=6, end_position=36, reference=seq).find_kmers()
    length = 36 + 7 - 6
    assert len(flat._hashes) == -(-(length - 7 + 1) // 3) and len(flat._ref_offsets) == -(-length // 3)


@pytest.mark.reference
def test_reference_chunks_repeat_their_boundary_record_and_clip(reference):
    """Each interval ends on the position the next one starts with, so that k-mer is emitted twice; an interval whose end
    lies past the sequence stops at the last whole k-mer."""
    seq = random_sequence(np.random.default_rng(4), 400)
    k, spacing = 6, 2
    intervals = spec.chunk_intervals(330, spacing, 1)
    assert intervals[0][1] == intervals[1][0]
    chunks = [reference["SnpKmerFinder"](None, k=k, spacing=spacing, start_position=a, end_position=b,
                                         reference=_text(seq)).find_kmers() for a, b in intervals]
    for left, right in zip(chunks[:-1], chunks[1:]):
        assert left._hashes[-1] == right._hashes[0]
    assert sum(len(c._hashes) for c in chunks) == len(intervals) * (intervals[0][1] // spacing + 1)
    clipped = reference["SnpKmerFinder"](None, k=31, spacing=1, start_position=10, end_position=200,
                                         reference=_text(seq[:90])).find_kmers()
    assert len(clipped._hashes) == 50
    with pytest.raises(AssertionError):
        reference["SnpKmerFinder"](None, k=31, spacing=1, start_position=90, end_position=200,
                                   reference=_text(seq[:90])).find_kmers()


@pytest.mark.reference
def test_reference_kmer_index_from_flat_kmers_matches_reference(reference):
    """Per reference position as multisets: the reference's argsort is not stable.  The offsets are int64 here: on a
    uint64 column the reference's np.ediff1d(..., to_begin=0) raises under NumPy 2."""
    rng = np.random.default_rng(8)
    n = 300
    offsets = np.sort(rng.integers(0, 90, n)).astype(np.int64)
    perm = rng.permutation(n)
    hashes = rng.integers(0, 2 ** 40, n).astype(np.uint64)
    nodes = rng.integers(1, 50, n).astype(np.uint32)
    ours = ReferenceKmerIndex.from_flat_kmers(FlatKmers(hashes[perm], nodes[perm], offsets[perm]))
    theirs = reference["ReferenceKmerIndex"].from_flat_kmers(reference["FlatKmers"](hashes[perm], nodes[perm], offsets[perm]))
    assert np.array_equal(ours.ref_position_to_index, theirs.ref_position_to_index)
    assert ours.ref_position_to_index.dtype == theirs.ref_position_to_index.dtype
    assert np.array_equal(ours.ref_positions, theirs.ref_positions)
    assert ours.kmers.dtype == theirs.kmers.dtype and ours.nodes.dtype == theirs.nodes.dtype
    for a in np.unique(offsets):
        sel_o, sel_t = ours.ref_positions == a, theirs.ref_positions == a
        assert sorted(zip(ours.kmers[sel_o].tolist(), ours.nodes[sel_o].tolist())) == \
            sorted(zip(theirs.kmers[sel_t].tolist(), theirs.nodes[sel_t].tolist()))


# ------------------------------------------------------------------------------------------ host-only parts of the product
def test_segment_table_follows_the_interval_rule():
    assert skf.chunk_intervals(1000, 3, 2) == spec.chunk_intervals(1000, 3, 2)
    first, count = skf.segments_of_intervals([(10, 200)], 90, 31, 1)
    assert (first.tolist(), count.tolist()) == ([10], [50])                 # clipped at the last whole k-mer
    first, count = skf.segments_of_intervals(skf.chunk_intervals(330, 2, 1), 400, 6, 2)
    assert count.tolist() == [17] * 10 and first.tolist() == [32 * i for i in range(10)]
    for start, end in ((90, 200), (95, 200), (70, 200)):                     # at, past the end; fewer than k bases left
        with pytest.raises(skf.NoReferenceSequence) as e:
            skf.segments_of_intervals([(start, end)], 90, 31, 1)
        assert isinstance(e.value, AssertionError) and "-G" in str(e.value) and "90" in str(e.value)


def test_snp_kmer_finder_modes_without_a_device():
    import inspect
    params = list(inspect.signature(SnpKmerFinder.__init__).parameters)
    assert params[1:6] == ["graph", "k", "spacing", "include_reverse_complements", "pruning"]
    assert params[-4:] == ["reference", "variant_to_nodes", "node_to_variants", "haplotype_matrix"]
    assert SnpKmerFinder(None, k=7, reference="ACGT").spacing == 7           # spacing defaults to k
    with pytest.raises(NotImplementedError):
        SnpKmerFinder(object(), k=5).find_kmers()
    with pytest.raises(NotImplementedError):
        SnpKmerFinder(object(), k=5).find_kmers_on_device()


def test_reference_to_letters_forms():
    want = np.frombuffer(b"ACgtN", dtype=np.uint8)
    for form in ("ACgtN", b"ACgtN", want.copy(), np.array(list("ACgtN"))):
        assert np.array_equal(skf.reference_to_letters(form), want)

    class Record:                                                            # a FASTA record: slicing gives text
        def __getitem__(self, s):
            return "ACgtN"[s]
    assert np.array_equal(skf.reference_to_letters(Record()), want)


def test_fasta_reader(tmp_path):
    path = str(tmp_path / "ref.fa")
    with open(path, "wb") as f:
        f.write(b">chr1 first record\r\nACGT\r\nacgtNN\r\n\r\n>chr2\nGG>CC\nTT\n>chr3 empty\n>chr4\nA")
    assert skf.read_fasta_record(path, "chr1").tobytes() == b"ACGTacgtNN"
    assert skf.read_fasta_record(path, "chr2").tobytes() == b"GG>CCTT"       # a `>` inside a line is no header
    assert skf.read_fasta_record(path, "chr3").tobytes() == b""
    assert skf.read_fasta_record(path, "chr4").tobytes() == b"A"
    assert skf.read_fasta_record(path, "chr1").dtype == np.uint8
    with pytest.raises(KeyError) as e:
        skf.read_fasta_record(path, "chrX")
    assert all(name in str(e.value) for name in ("chr1", "chr2", "chr3", "chr4"))


def test_reference_kmer_index_host_forms(tmp_path):
    offsets = np.array([5, 2, 2, 9, 5, 2], dtype=np.uint64)
    hashes = np.array([50, 20, 21, 90, 51, 22], dtype=np.uint64)
    nodes = np.array([1, 2, 3, 4, 5, 6], dtype=np.uint32)
    idx = ReferenceKmerIndex.from_flat_kmers(FlatKmers(hashes, nodes, offsets))
    assert idx.kmers.tolist() == [20, 21, 22, 50, 51, 90] and idx.kmers.dtype == np.uint32     # stable inside a position
    assert idx.nodes.tolist() == [2, 3, 6, 1, 5, 4]
    # what the reference returns on this input (int64 offsets): index 0 of the first position counts as "no k-mer
    # here" in its zero fill (reference_kmer_index.py:91-112), so positions up to the first one map to the second
    assert idx.ref_position_to_index.tolist() == [3, 3, 3, 3, 3, 3, 5, 5, 5, 5]
    k, p, n = idx.get_all_between(2, 9)
    assert k.tolist() == [50, 51] and p.tolist() == [5, 5] and n.tolist() == [1, 5]
    big = ReferenceKmerIndex.from_flat_kmers(FlatKmers(hashes + np.uint64(2 ** 40), nodes, offsets))
    assert big.kmers.dtype == np.uint64
    # the three file shapes
    full = str(tmp_path / "full")
    idx.to_file(full)
    assert sorted(np.load(full + ".npz").files) == ["kmers", "nodes", "ref_position_to_index", "ref_positions"]
    back = ReferenceKmerIndex.from_file(full)
    assert all(np.array_equal(getattr(back, a), getattr(idx, a)) for a in ReferenceKmerIndex.properties)
    linear = ReferenceKmerIndex(np.arange(6, dtype=np.uint32), np.arange(10, 14, dtype=np.uint32))
    linear.to_file(str(tmp_path / "linear"))
    assert sorted(np.load(str(tmp_path / "linear.npz")).files) == ["kmers", "ref_position_to_index"]
    back = ReferenceKmerIndex.from_file(str(tmp_path / "linear.npz"))
    assert back.ref_positions is None and back.nodes is None
    assert back.get_between(1, 3).tolist() == [11, 12] and back.get_between(2, 99).tolist() == [12, 13]
    assert back.get_between_except(0, 4, 2).tolist() == [10, 11, 13]
    with pytest.raises(Exception):
        back.get_all_between(0, 2)
    only = ReferenceKmerIndex(None, np.arange(4, dtype=np.uint64))
    only.to_file(str(tmp_path / "only"))
    assert np.load(str(tmp_path / "only.npz")).files == ["kmers"]
    assert ReferenceKmerIndex.from_file(str(tmp_path / "only")).ref_position_to_index is None


def test_new_sub_commands_parse_and_merge(tmp_path):
    p = build_parser()
    a = p.parse_args("make -t 16 -s 1 -k 31 -r True -R ref.fa -n chr1 -G 1000 -o out".split())
    assert (a.threads, a.spacing, a.kmer_size, a.include_reverse_complement, a.genome_size) == (16, 1, 31, True, 1000)
    assert p.parse_args("make -r False -R r -n c -o o".split()).include_reverse_complement is False
    d = p.parse_args("make -R r -n c -o o".split())
    assert (d.kmer_size, d.spacing, d.threads, d.genome_size) == (31, 31, 1, 3000000000)
    with pytest.raises(NotImplementedError):
        main("make -g graph.npz -o out".split())
    a = p.parse_args("make_reference_kmer_index -r ref.fa -n chr1 -o out".split())
    assert a.kmer_size == 16 and a.only_store_kmers is False and a.flat_index is None
    one = FlatKmers(np.array([1, 2], np.uint64), np.array([1, 1], np.uint32), np.array([0, 1], np.uint64))
    two = FlatKmers(np.array([3], np.uint64), np.array([1], np.uint32), np.array([7], np.uint64))
    one.to_file(str(tmp_path / "a"))
    two.to_file(str(tmp_path / "b"))
    assert main(["merge_flat_kmers", "-f", "%s,%s" % (tmp_path / "a.npz", tmp_path / "b"), "-o", str(tmp_path / "m")]) == 0
    merged = FlatKmers.from_file(str(tmp_path / "m"))
    assert merged._hashes.tolist() == [1, 2, 3] and merged._ref_offsets.tolist() == [0, 1, 7]
    assert merged._hashes.dtype == np.uint64 and merged._nodes.dtype == np.uint32
    assert merged._allele_frequencies.dtype == np.float32
    # make_reference_kmer_index -f: host only
    assert main(["make_reference_kmer_index", "-f", str(tmp_path / "m"), "-o", str(tmp_path / "rki")]) == 0
    assert ReferenceKmerIndex.from_file(str(tmp_path / "rki")).kmers.tolist() == [1, 2, 3]
