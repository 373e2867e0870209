"""-m gpu: the device route of the reference FASTA (fasta_files.py, csrc/gki_fasta_parse.hip) equals the rules' plain
restatement (spec_fasta_files.py) -- names, bounds, letters and records_in_file -- on every case of fasta_cases.py, cut
into pieces of every size and from every encoding; the callers give the same from the device route as from the host's.

Note on `> desc`: the rules are read_fasta_records', where the name is the first word behind the '>' as bytes.split()
finds it, so `> desc` is named "desc" and only a header line without any word has the empty name."""
import gc
import gzip

import numpy as np
import pytest

import spec_fasta_files as spec
from fasta_cases import CASES, MISSING, PIECE_CASES, SELECTIONS
from graph_build_cases import GOOD_CASES
from graph_kmer_index_amd import _lib, bgzf, read_files
from test_gpu_host_layer_release import FailingLibrary, live  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def assert_equals_spec(ref, data, names, file_name="<buffer>"):
    """`ref` (a DeviceReference, freed here) against the spec for the same request."""
    try:
        found = spec.records(data)[0]
        want_names, want, _ = spec.read(data, spec.distinct(found) if names is None else names, file_name)
        assert ref.records_in_file == found
        assert ref.names == want_names
        assert ref.bounds.dtype == np.int64
        assert ref.bounds.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.int64).tolist()
        assert ref.letters.dtype == np.uint8 and ref.letters.n == ref.bounds[-1]
        assert ref.letters.to_host().tobytes() == b"".join(want)
        got = ref.to_host()
        assert len(got) == len(want) and all(g.dtype == np.uint8 and g.tobytes() == w for g, w in zip(got, want))
        assert ref.timings["parse_kernel_ms"] >= 0.0 and {"text", "parse", "assemble"} <= set(ref.timings)
    finally:
        ref.free()


@pytest.mark.parametrize("name", list(CASES))
def test_buffer_equals_spec(name):
    from graph_kmer_index_amd.fasta_files import parse_fasta_on_device
    data = CASES[name]
    for names in [None] + SELECTIONS.get(name, []):
        assert_equals_spec(parse_fasta_on_device(data, names), data, names)


def test_buffer_forms_and_alignment():
    """NumPy bytes, a DeviceArray (which stays its owner's) and a window that is not 16-byte aligned."""
    from graph_kmer_index_amd.fasta_files import parse_fasta_on_device
    data = CASES["many_records"]
    assert_equals_spec(parse_fasta_on_device(np.frombuffer(data, dtype=np.uint8)), data, None)
    with _lib.DeviceScope() as s:
        d = s.on_device(np.frombuffer(b"\n\n\n" + data, dtype=np.uint8), np.uint8)
        assert_equals_spec(parse_fasta_on_device(d), b"\n\n\n" + data, None)
        assert_equals_spec(parse_fasta_on_device(d.view(3, len(data)), ["r4", "r2"]), data, ["r4", "r2"])
        assert d.to_host().tobytes() == b"\n\n\n" + data


@pytest.fixture(scope="module")
def piece_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("fasta_pieces")
    files = {}
    for name in PIECE_CASES:
        paths = {"plain": str(d / (name + ".fa")), "bgzf": str(d / (name + "_bgzf.fa.gz")),
                 "gzip": str(d / (name + "_gzip.fa.gz"))}
        with open(paths["plain"], "wb") as f:
            f.write(CASES[name])
        bgzf.write_bgzf(paths["bgzf"], CASES[name], block_size=41)     # members end mid-line and mid-header
        with open(paths["gzip"], "wb") as f:
            f.write(gzip.compress(CASES[name]))
        assert [read_files.reads_file_route(paths[k]) for k in ("plain", "bgzf", "gzip")] == ["raw", "bgzf-device", "gzip-host"]
        files[name] = paths
    return files


@pytest.mark.parametrize("encoding", ["plain", "bgzf", "gzip"])
@pytest.mark.parametrize("chunk_bytes", [1, 64, None])
@pytest.mark.parametrize("name", PIECE_CASES)
def test_file_in_pieces_equals_spec(piece_files, name, chunk_bytes, encoding):
    from graph_kmer_index_amd.fasta_files import reference_from_file
    path, data = piece_files[name][encoding], CASES[name]
    for names in [None] + SELECTIONS.get(name, [])[:2]:
        assert_equals_spec(reference_from_file(path, names, chunk_bytes=chunk_bytes), data, names, path)


def test_inflate_choices(piece_files):
    from graph_kmer_index_amd.fasta_files import reference_from_file
    paths, data = piece_files["many_records"], CASES["many_records"]
    assert_equals_spec(reference_from_file(paths["bgzf"], ["r2"], chunk_bytes=64, inflate="host"), data, ["r2"])
    assert_equals_spec(reference_from_file(paths["bgzf"], ["r2"], chunk_bytes=64, inflate="device"), data, ["r2"])
    with pytest.raises(ValueError):
        reference_from_file(paths["gzip"], inflate="device")


@pytest.mark.parametrize("name", list(MISSING))
def test_missing_name_is_the_host_routes_key_error(name, tmp_path):
    from graph_kmer_index_amd.fasta_files import reference_from_file
    from graph_kmer_index_amd.snp_kmer_finder import read_fasta_records
    path = str(tmp_path / "ref.fa")
    with open(path, "wb") as f:
        f.write(CASES[name])
    with pytest.raises(KeyError) as want:
        read_fasta_records(path, [MISSING[name]])
    with pytest.raises(KeyError) as got:
        reference_from_file(path, [MISSING[name]], chunk_bytes=64)
    assert got.value.args == want.value.args
    assert "records: " + ", ".join(spec.records(CASES[name])[0]) in got.value.args[0]


@pytest.mark.parametrize("encoding", ["plain", "bgzf"])
def test_key_error_mid_stream_leaves_nothing_on_the_device(piece_files, live, encoding):  # noqa: F811
    """The wanted records' letters of the pieces so far are alive when the missing name is found out."""
    from graph_kmer_index_amd.fasta_files import reference_from_file
    path = piece_files["many_records"][encoding]
    reference_from_file(path, ["r4"], chunk_bytes=64).free()
    gc.collect()
    baseline = set(live)
    with pytest.raises(KeyError) as e:
        reference_from_file(path, ["r4", "r9", "r0"], chunk_bytes=64)
    assert live == baseline, "%d buffers are still on the device while the exception is held" % len(live - baseline)
    del e


@pytest.mark.parametrize("encoding", ["plain", "bgzf"])
def test_nothing_stays_on_the_device_after_a_failed_library_call(piece_files, live, monkeypatch, encoding):  # noqa: F811
    """test_gpu_host_layer_release.py's check for the new route: every library call of a streamed parse fails in turn."""
    from graph_kmer_index_amd.fasta_files import reference_from_file
    path = piece_files["name_twice"][encoding]
    run = lambda: reference_from_file(path, ["z", "x"], chunk_bytes=16)
    run().free()
    gc.collect()
    baseline = set(live)
    proxy = FailingLibrary(_lib.load())
    monkeypatch.setattr(_lib, "_lib", proxy)
    ref = run()
    assert live - baseline == {ref.letters.ptr.value}, "more than the result is new"
    ref.free()
    n_calls = proxy.calls
    assert n_calls > 6
    for i in range(n_calls):
        proxy.calls, proxy.fail_at, proxy.failed = 0, i, None
        with pytest.raises(_lib.GkiError) as e:
            run()
        assert e.value.code == 2 and proxy.failed is not None
        assert live == baseline, "call %d of %d (%s): %d buffers are still on the device while the exception is held" \
            % (i, n_calls, proxy.failed, len(live - baseline))


# ------------------------------------------------------------------ callers
def write_fasta(path, reference, width=61, end=b"\n"):
    with open(path, "wb") as f:
        for name, letters in reference.items():
            f.write(b">%s some description" % name.encode() + end)
            for a in range(0, len(letters), width):
                f.write(letters[a:a + width] + end)


@pytest.fixture(scope="module")
def graph_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("fasta_graph")
    reference, text = GOOD_CASES["mixed_random_two_chromosomes"]
    paths = {"plain": str(d / "ref.fa"), "bgzf": str(d / "ref_bgzf.fa.gz"), "gzip": str(d / "ref_gzip.fa.gz"),
             "vcf": str(d / "v.vcf")}
    write_fasta(paths["plain"], reference)
    with open(paths["plain"], "rb") as f:
        data = f.read()
    bgzf.write_bgzf(paths["bgzf"], data, block_size=4001)
    with open(paths["gzip"], "wb") as f:
        f.write(gzip.compress(data))
    with open(paths["vcf"], "wb") as f:
        f.write(text)
    return list(reference), paths


GRAPH_ARRAYS = ("node_size", "seq", "edge_start", "edges", "rev_start", "rev_edges", "is_ref", "allele_freq", "exists",
                "node_to_ref_offset")


def assert_same_build(a, b):
    for key in GRAPH_ARRAYS:
        x, y = getattr(a.graph, key), getattr(b.graph, key)
        assert x.dtype == y.dtype and np.array_equal(x, y), key
    assert list(a.graph.chromosome_start_nodes) == list(b.graph.chromosome_start_nodes)
    assert np.array_equal(a.variant_to_nodes.ref_nodes, b.variant_to_nodes.ref_nodes)
    assert np.array_equal(a.variant_to_nodes.var_nodes, b.variant_to_nodes.var_nodes)
    assert np.array_equal(a.line_status, b.line_status)


@pytest.mark.parametrize("encoding", ["plain", "bgzf", "gzip"])
def test_graph_build_device_equals_host(graph_files, encoding):
    from graph_kmer_index_amd.graph_files import build_graph_from_files
    names, paths = graph_files
    host = build_graph_from_files(paths["plain"], paths["vcf"], fasta_parse="host")
    assert len(host.graph.seq) > 9000 and int((host.line_status == 0).sum()) > 100
    for route in ("device", "auto", "host"):
        got = build_graph_from_files(paths[encoding], paths["vcf"], fasta_parse=route)
        assert_same_build(got, host)
        assert {"read_reference", "upload_reference", "parse_reference_kernel_ms"} <= set(got.timings)
    got = build_graph_from_files(paths[encoding], paths["vcf"], names, chunk_bytes=64, fasta_parse="device")
    assert_same_build(got, host)


def run_command(argv):
    from graph_kmer_index_amd.command_line_interface import build_parser
    args = build_parser().parse_args(argv)
    args.func(args)


def same_npz(a, b):
    x, y = np.load(a, allow_pickle=True), np.load(b, allow_pickle=True)
    assert sorted(x.files) == sorted(y.files)
    for key in x.files:
        assert x[key].dtype == y[key].dtype and np.array_equal(x[key], y[key]), key


@pytest.mark.parametrize("route", ["device", "host"])
def test_commands_from_compressed_fasta_equal_plain(graph_files, tmp_path, route):
    names, paths = graph_files
    name = names[-1]
    outs = {}
    for encoding in ("plain", "bgzf", "gzip"):
        flat, index, graph = (str(tmp_path / ("%s_%s" % (kind, encoding))) for kind in ("flat", "index", "graph"))
        run_command(["make", "-o", flat, "-R", paths[encoding], "-n", name, "-k", "31", "-s", "7", "-G", "4000", "-t", "2",
                     "--fasta-parse", route])
        run_command(["make_reference_kmer_index", "-o", index, "-r", paths[encoding], "-n", name, "-k", "16",
                     "--fasta-parse", route])
        run_command(["make_graph", "-o", graph, "-r", paths[encoding], "-v", paths["vcf"], "--fasta-parse", route])
        outs[encoding] = (flat + ".npz", index + ".npz", graph + ".npz", graph + ".variant_to_nodes.npz")
    for encoding in ("bgzf", "gzip"):
        for a, b in zip(outs["plain"], outs[encoding]):
            same_npz(a, b)


def test_commands_device_equals_host(graph_files, tmp_path):
    names, paths = graph_files
    outs = {}
    for route in ("host", "device"):
        flat, index = str(tmp_path / ("flat_" + route)), str(tmp_path / ("index_" + route))
        run_command(["make", "-o", flat, "-R", paths["bgzf"], "-n", names[0], "-k", "31", "-s", "5", "-G", "5000",
                     "-r", "True", "--fasta-parse", route])
        run_command(["make_reference_kmer_index", "-o", index, "-r", paths["bgzf"], "-n", names[0], "-k", "31",
                     "--fasta-parse", route])
        outs[route] = (flat + ".npz", index + ".npz")
    for a, b in zip(outs["host"], outs["device"]):
        same_npz(a, b)
