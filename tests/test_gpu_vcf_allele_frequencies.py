"""Allele frequencies from the VCF on the device (vcf_files.py, graph_files.py, csrc/gki_vcf_af.hip) against the plain-Python
rules of tests/spec_vcf_allele_frequencies.py: ref_af, alt_af and route of every data line of every named case, bit for
bit, through the in-memory and the file form; the refused inputs with their line; pieces cut anywhere, from plain, BGZF
and gzip files; the graph build with a source against the build that is handed the spec's values; and the command line."""
import gzip
from collections import Counter

import numpy as np
import pytest

import spec_graph_build
import spec_vcf_allele_frequencies as spec
from graph_build_cases import GOOD_CASES as GRAPH_CASES, line, other_base, random_reference, snp, vcf
from vcf_af_cases import ERROR_CASES, GOOD_CASES, GT_FORMS, gt_line, info_line, random_value_text, text_of

pytestmark = pytest.mark.gpu

SOURCES = ("genotypes", "info")
CASES = [(source, name) for source in SOURCES for name in sorted(GOOD_CASES[source])]
_SPEC = {}


def spec_of(source, name):
    if (source, name) not in _SPEC:
        _SPEC[source, name] = spec.allele_frequencies(GOOD_CASES[source][name], source)
    return _SPEC[source, name]


def assert_equals_spec(got, want):
    for key, g, w in zip(("ref_af", "alt_af"), got, want):
        assert g.dtype == np.float64 and np.array_equal(g.view(np.uint64), w.view(np.uint64)), key
    assert got[2].dtype == np.uint8 and np.array_equal(got[2], want[2]), "route"


@pytest.mark.parametrize("source,name", CASES)
def test_case_equals_spec_in_memory_and_from_file(source, name, tmp_path):
    from graph_kmer_index_amd.vcf_files import allele_frequencies_from_file, allele_frequencies_on_device
    text = GOOD_CASES[source][name]
    assert_equals_spec(allele_frequencies_on_device(text, source), spec_of(source, name))
    path = str(tmp_path / "v.vcf")
    with open(path, "wb") as f:
        f.write(text)
    assert_equals_spec(allele_frequencies_from_file(path, source), spec_of(source, name))


def test_device_buffer_and_the_other_source_on_one_text():
    from graph_kmer_index_amd import _lib
    from graph_kmer_index_amd.vcf_files import allele_frequencies_on_device
    text = text_of([info_line(b"AF=0.125", b"\tGT\t0|1\t1|1"), info_line(b"NS=2", b"\tGT:DP\t0|0:3\t.:1"), gt_line([b"1|1"])])
    with _lib.DeviceScope() as s:
        d = s.on_device(np.frombuffer(text, dtype=np.uint8), np.uint8)
        for source in SOURCES:
            assert_equals_spec(allele_frequencies_on_device(d, source), spec.allele_frequencies(text, source))
    with pytest.raises(ValueError):
        allele_frequencies_on_device(text, "format")


@pytest.mark.parametrize("name", sorted(ERROR_CASES))
def test_error_case_names_the_lowest_line(name, tmp_path):
    from graph_kmer_index_amd.vcf_files import AlleleFrequencyError, allele_frequencies_from_file, allele_frequencies_on_device
    source, text, at, kind = ERROR_CASES[name]
    with pytest.raises(spec.AfError) as want:
        spec.allele_frequencies(text, source)
    assert (want.value.line, want.value.kind) == (at, kind)
    path = str(tmp_path / "v.vcf")
    with open(path, "wb") as f:
        f.write(text)
    for call in (lambda: allele_frequencies_on_device(text, source), lambda: allele_frequencies_from_file(path, source),
                 lambda: allele_frequencies_from_file(path, source, chunk_bytes=1)):
        with pytest.raises(ValueError) as e:
            call()
        assert isinstance(e.value, AlleleFrequencyError) and (e.value.line, e.value.kind) == (at, kind)
        assert "data line %d:" % at in str(e.value)


@pytest.fixture(scope="module", params=[("genotypes", "mixed_file"), ("genotypes", "line_lengths_around_w"),
                                        ("info", "host_and_device_mixed"), ("info", "random_values")])
def case_files(request, tmp_path_factory):
    from graph_kmer_index_amd import bgzf
    source, name = request.param
    d = tmp_path_factory.mktemp("vcf_af_%s_%s" % (source, name))
    text = GOOD_CASES[source][name]
    paths = {"plain": str(d / "v.vcf"), "bgzf": str(d / "v_bgzf.vcf.gz"), "gzip": str(d / "v_gzip.vcf.gz")}
    with open(paths["plain"], "wb") as f:
        f.write(text)
    bgzf.write_bgzf(paths["bgzf"], text, block_size=777)                # lines span members
    with open(paths["gzip"], "wb") as f:
        f.write(gzip.compress(text))
    return source, name, paths


@pytest.mark.parametrize("encoding", ["plain", "bgzf", "gzip"])
@pytest.mark.parametrize("chunk_bytes", [64, 1])                        # 1: a cut after every line of the host routes
def test_pieces_cut_anywhere(case_files, encoding, chunk_bytes):
    from graph_kmer_index_amd.vcf_files import allele_frequencies_from_file
    source, name, paths = case_files
    assert_equals_spec(allele_frequencies_from_file(paths[encoding], source, chunk_bytes=chunk_bytes), spec_of(source, name))


def test_error_line_numbers_carry_across_pieces(tmp_path):
    from graph_kmer_index_amd import bgzf
    from graph_kmer_index_amd.vcf_files import AlleleFrequencyError, allele_frequencies_from_file
    good = [gt_line([b"0|1", b"1|1"], pos=i + 1) for i in range(100)]
    for source, bad, kind in (("genotypes", gt_line([b"0|1", b"0|"]), "genotype"), ("info", info_line(b"AF=abc"), "text"),
                              ("info", info_line(b"AF=1.5"), "value")):
        text = text_of(good + [bad, good[0], bad])
        bgzf.write_bgzf(str(tmp_path / "v.vcf.gz"), text, block_size=500)
        with open(str(tmp_path / "v.vcf"), "wb") as f:
            f.write(text)
        for path in ("v.vcf", "v.vcf.gz"):
            with pytest.raises(AlleleFrequencyError) as e:
                allele_frequencies_from_file(str(tmp_path / path), source, chunk_bytes=64)
            assert (e.value.line, e.value.kind) == (100, kind)


# ---------------------------------------------------------------------------------------------------- the graph build

def with_columns(text, seed):
    """The VCF text with INFO, FORMAT and sample columns in place of whatever follows ALT on every data line of five
    fields or more: an AF= entry of any route or none, and 1 to 40 samples, sometimes all of them missing."""
    rng = np.random.default_rng([seed, 41])
    out = []
    for raw in text.split(b"\n"):
        fields = raw.split(b"\t")
        if raw[:1] != b"#" and len(fields) >= 5:
            pick = rng.random()
            info = b"NS=3;AF=%s;DP=9" % random_value_text(rng) if pick < 0.8 else (b"DP=9", b"AF=.", b".")[int(rng.integers(0, 3))]
            n = int(rng.integers(1, 41))
            samples = [b"./."] * n if rng.random() < 0.1 else [GT_FORMS[i] for i in rng.integers(0, len(GT_FORMS), size=n)]
            raw = b"\t".join(fields[:5] + [b".", b"PASS", info, b"GT:DP"] + samples)
        out.append(raw)
    return b"\n".join(out)


GRAPH_ARRAYS = ("node_size", "seq", "edge_start", "edges", "rev_start", "rev_edges", "is_ref", "allele_freq", "exists",
                "node_to_ref_offset", "seq_start")


def assert_same_build(got, want, but=()):
    for key in GRAPH_ARRAYS:
        if key not in but:
            a, b = np.asarray(getattr(got.graph, key)), np.asarray(getattr(want.graph, key))
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                                         b.view(np.uint64) if b.dtype == np.float64 else b), key
    assert got.graph._chromosome_start_nodes == want.graph._chromosome_start_nodes
    for key in ("ref_nodes", "var_nodes"):
        assert np.array_equal(getattr(got.variant_to_nodes, key), getattr(want.variant_to_nodes, key)), key
    assert np.array_equal(got.line_status, want.line_status)


@pytest.mark.parametrize("name", sorted(GRAPH_CASES))
def test_graph_build_with_a_source_equals_the_build_given_the_spec_values(name):
    from graph_kmer_index_amd.graph_files import build_graph
    reference, text = GRAPH_CASES[name]
    text = with_columns(text, len(name))
    plain = build_graph(reference, text)
    assert plain.route is None and np.all(plain.graph.allele_freq == 1.0)
    for source in SOURCES:
        want = spec.allele_frequencies(text, source)
        built = build_graph(reference, text, allele_frequencies=source)
        assert_same_build(built, build_graph(reference, text, allele_frequencies=want[:2]))
        assert built.route.dtype == np.uint8 and np.array_equal(built.route, want[2])
        assert_same_build(built, plain, but=("allele_freq",))


def write_fasta(path, reference, width=61):
    with open(path, "wb") as f:
        for name, letters in reference.items():
            f.write(b">%s some description\n" % name.encode())
            for a in range(0, len(letters), width):
                f.write(letters[a:a + width] + b"\n")


@pytest.mark.parametrize("encoding", ["plain", "bgzf"])
def test_graph_build_from_files_in_pieces(tmp_path, encoding):
    from graph_kmer_index_amd import bgzf
    from graph_kmer_index_amd.graph_files import build_graph, build_graph_from_files
    reference, text = GRAPH_CASES["mixed_random_two_chromosomes"]
    text = with_columns(text, 5)
    fasta, path = str(tmp_path / "ref.fa"), str(tmp_path / ("v.vcf" if encoding == "plain" else "v.vcf.gz"))
    write_fasta(fasta, reference)
    if encoding == "plain":
        with open(path, "wb") as f:
            f.write(text)
    else:
        bgzf.write_bgzf(path, text, block_size=777)
    for source in SOURCES:
        want = spec.allele_frequencies(text, source)
        built = build_graph_from_files(fasta, path, allele_frequencies=source, chunk_bytes=64)
        assert_same_build(built, build_graph(reference, text, allele_frequencies=want[:2]))
        assert np.array_equal(built.route, want[2]) and set(want[2].tolist()) >= {0, 1}


def test_graph_build_reports_the_lowest_line_of_either_pass():
    from graph_kmer_index_amd.graph_files import GraphBuildError, build_graph
    from graph_kmer_index_amd.vcf_files import AlleleFrequencyError
    r = random_reference(60, 3)
    tail = b"\t.\tPASS\t.\tGT\t"
    good, bad_gt = snp("1", r, 5)[:-1], line("1", 9, r[8:9], other_base(r[8]), tail + b"0|")[:-1]
    bad_ref = line("1", 20, other_base(r[19]), r[19:20])[:-1]
    with pytest.raises(AlleleFrequencyError) as e:
        build_graph({"1": r}, vcf([l + b"\n" for l in (good, bad_gt, bad_ref)]), allele_frequencies="genotypes")
    assert (e.value.line, e.value.kind) == (1, "genotype")
    bad_gt_later = line("1", 30, r[29:30], other_base(r[29]), tail + b"x")[:-1]
    with pytest.raises(GraphBuildError) as e:
        build_graph({"1": r}, vcf([l + b"\n" for l in (good, bad_ref, bad_gt_later)]), allele_frequencies="genotypes")
    assert (e.value.line, e.value.kind) == (1, 3)
    with pytest.raises(ValueError):
        build_graph({"1": r}, vcf([good + b"\n"]), allele_frequencies="samples")


def test_command_line_allele_frequencies_reach_the_index(tmp_path):
    from graph_kmer_index_amd.command_line_interface import build_parser, load_graph
    from graph_kmer_index_amd.critical_graph_paths import CriticalGraphPaths
    from graph_kmer_index_amd.flat_kmers import FlatKmers
    from graph_kmer_index_amd.graph import GraphArrays
    from graph_kmer_index_amd.unique_variant_kmers import load_variant_to_nodes
    from spec_bruteforce import spec_rows
    k, r = 15, random_reference(500, 77)
    rng = np.random.default_rng(78)
    text = vcf([line("1", pos, r[pos - 1:pos], other_base(r[pos - 1]), b"\t.\tPASS\tAF=0.5\tGT\t" +
                     b"\t".join(GT_FORMS[i] for i in rng.integers(0, len(GT_FORMS), size=30)))
                for pos in range(20, 480, 23)])
    fasta, vcf_path, out = str(tmp_path / "ref.fa"), str(tmp_path / "v.vcf"), str(tmp_path / "graph")
    write_fasta(fasta, {"1": r})
    with open(vcf_path, "wb") as f:
        f.write(text)

    def graph_of(want):
        return GraphArrays(want.node_size, want.seq, want.edge_start, want.edges, want.is_ref, want.allele_freq, want.exists,
                           1, want.chromosome_start_nodes, want.node_to_ref_offset)
    for flags, values in (([], None), (["-a", "genotypes"], spec.allele_frequencies(text, "genotypes")[:2])):
        parser = build_parser()
        args = parser.parse_args(["make_graph", "-r", fasta, "-v", vcf_path, "-o", out] + flags)
        args.func(args)
        want = spec_graph_build.build({"1": r}, text, allele_frequencies=values)
        graph, v2n = load_graph(out), load_variant_to_nodes(out + ".variant_to_nodes")
        for key in ("node_size", "seq", "edge_start", "edges", "is_ref", "exists", "node_to_ref_offset"):
            assert np.array_equal(np.asarray(getattr(graph, key)), getattr(want, key)), key
        assert np.array_equal(np.asarray(graph.allele_freq).view(np.uint64), want.allele_freq.view(np.uint64))
        assert np.array_equal(v2n.ref_nodes, want.ref_nodes) and np.array_equal(v2n.var_nodes, want.var_nodes)
        assert np.all(want.allele_freq == 1.0) == (values is None)
    args = parser.parse_args(["index", "-g", out, "-k", str(k), "-o", str(tmp_path / "flat")])
    args.func(args)
    flat = FlatKmers.from_file(str(tmp_path / "flat"))
    want_graph = graph_of(want)
    cp = CriticalGraphPaths.from_graph(want_graph, k)
    rows = spec_rows(want_graph, k, 5, True, {int(a): int(b) for a, b in zip(cp.nodes, cp.offsets)})
    expected = Counter()
    for (h, _, _, node, af), count in rows.items():       # af: the minimum over the window's nodes, in Python
        expected[h, node, float(np.float32(af))] += count
    got = Counter(zip(flat._hashes.tolist(), flat._nodes.tolist(), flat._allele_frequencies.astype(np.float64).tolist()))
    assert got == expected
    assert flat._allele_frequencies.dtype == np.float32 and not np.all(flat._allele_frequencies == 1.0)
