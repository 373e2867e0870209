"""Graph build from files at full size: a 3 Gbp reference and 5e6 SNPs (the shape of bench.py's graph), written once from
`synthetic_snp_graph` with unsplit segments as a FASTA and a VCF, plain and BGZF.

    python tools/bench_graph_build.py [--bases 3e9] [--sites 5e6] [--dir DIR] [--runs 3]

Reports, per VCF encoding, the whole `build_graph_from_files` call and its stages (GraphBuild.timings): reading the FASTA
records (one read), uploading them, the VCF text, the site pass, the assembly (count and emit), the sequence stage's
device time, the copy back and the host's GraphArrays construction; `unattributed` is what of the call no stage covers.
The VCF text's own steps -- file read, upload, inflate with the line cut -- are timed in a pass of their own over the
same step functions the call uses (`vcf_text_stages`).  The first run of each encoding is checked against the
generator's graph (every id + 1); every time quoted is the median of the runs after it.  Beside them, measured in the
same process: a device-to-device copy of as many bytes as the sequence has (median of three), the store ceiling of this
device (gki_measure_store_bw), and the time `synthetic_snp_graph` itself takes in NumPy (drawing the bases included)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graph_kmer_index_amd import _lib, bgzf, read_files                         # noqa: E402
from graph_kmer_index_amd.graph import synthetic_snp_graph                      # noqa: E402
from graph_kmer_index_amd.graph_files import build_graph_from_files             # noqa: E402

LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def write_inputs(g, directory, width=80):
    """ref.fa, v.vcf and v.vcf.gz (BGZF) of a synthetic_snp_graph with unsplit segments; returns (paths, ref_af, alt_af)."""
    alt = np.flatnonzero(g.is_ref == 0)
    ref = alt - 1
    alt_slot = g.seq_start[alt]
    reference = LETTERS[np.delete(g.seq, alt_slot)]
    paths = {"fasta": os.path.join(directory, "ref.fa"), "plain": os.path.join(directory, "v.vcf"),
             "bgzf": os.path.join(directory, "v.vcf.gz")}
    with open(paths["fasta"], "wb") as f:
        f.write(b">1 synthetic\n")
        whole = len(reference) // width * width
        rows = np.empty((whole // width, width + 1), dtype=np.uint8)
        rows[:, :width] = reference[:whole].reshape(-1, width)
        rows[:, width] = 10
        f.write(rows.tobytes())
        del rows
        if whole < len(reference):
            f.write(reference[whole:].tobytes() + b"\n")
    pos = (g.node_to_ref_offset[ref] + 1).tolist()
    ref_letter = LETTERS[g.seq[g.seq_start[ref]]].tolist()
    alt_letter = LETTERS[g.seq[alt_slot]].tolist()
    text = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" + b"".join(
        b"1\t%d\t.\t%c\t%c\t.\tPASS\t.\n" % t for t in zip(pos, ref_letter, alt_letter))
    with open(paths["plain"], "wb") as f:
        f.write(text)
    bgzf.write_bgzf(paths["bgzf"], text, threads=8)
    return paths, g.allele_freq[ref], g.allele_freq[alt]


def assert_equals_generator(built, g):
    b = built.graph
    alt = np.flatnonzero(g.is_ref == 0)
    checks = {"node_size": np.array_equal(b.node_size[1:], g.node_size), "seq": np.array_equal(b.seq, g.seq),
              "edge_start": np.array_equal(b.edge_start[1:], g.edge_start), "edges": np.array_equal(b.edges, g.edges + 1),
              "is_ref": np.array_equal(b.is_ref[1:], g.is_ref), "allele_freq": np.array_equal(b.allele_freq[1:], g.allele_freq),
              "node_to_ref_offset": np.array_equal(np.asarray(b.node_to_ref_offset)[1:], g.node_to_ref_offset),
              "var_nodes": np.array_equal(built.variant_to_nodes.var_nodes, alt + 1),
              "ref_nodes": np.array_equal(built.variant_to_nodes.ref_nodes, alt),
              "line_status": not built.line_status.any()}
    bad = [k for k, ok in checks.items() if not ok]
    if bad:
        raise AssertionError("the built graph differs from the generator's in %s" % ", ".join(bad))


def vcf_text_stages(path, chunk_bytes=read_files.DEFAULT_CHUNK_BYTES):
    """Seconds of the VCF text's way to the device, step by step, with a synchronise behind each device step: the steps
    of `read_files.host_text_pieces` / `bgzf_text_pieces`, nothing parsed."""
    lib = _lib.load()
    sync = lambda: _lib.check(lib.gki_device_synchronize())
    st = dict(vcf_file_read=0.0, vcf_upload=0.0, vcf_inflate=0.0)
    bgzf_route = read_files.reads_file_route(path) == "bgzf-device"
    with _lib.DeviceScope() as run, (open(path, "rb") if bgzf_route else read_files.open_reads_file(path)) as f:
        pieces = read_files.iter_bgzf_pieces(f, chunk_bytes, path) if bgzf_route else read_files.iter_line_chunks(f, chunk_bytes)
        tail = None
        while True:
            t = time.perf_counter()
            item = next(pieces, None)
            st["vcf_file_read"] += time.perf_counter() - t
            if item is None:
                break
            with _lib.DeviceScope() as s:
                t = time.perf_counter()
                d = s.keep(read_files.upload_piece(item[0] if bgzf_route else item)); sync()
                st["vcf_upload"] += time.perf_counter() - t
                if bgzf_route:
                    t = time.perf_counter()
                    text = s.keep(read_files.inflate_piece(d, item[1], item[2], tail, path))
                    _, tail = read_files.cut_at_line_end(text); sync()
                    st["vcf_inflate"] += time.perf_counter() - t
                    if tail is not None:
                        run.keep(tail)
    return st


def device_yardsticks(n_bytes):
    """(seconds of a device-to-device copy of n_bytes, median of three; store ceiling in bytes/s)."""
    lib = _lib.load()
    with _lib.DeviceScope() as s:
        a, b = s.array(n_bytes, np.uint8), s.array(n_bytes, np.uint8)
        a.zero()
        times = []
        for _ in range(3):
            _lib.check(lib.gki_device_synchronize())
            t0 = time.perf_counter()
            _lib.check(lib.gki_memcpy_d2d(b.ptr, a.ptr, n_bytes))
            _lib.check(lib.gki_device_synchronize())
            times.append(time.perf_counter() - t0)
    with _lib.DeviceScope() as s:
        n = max(1 << 20, n_bytes // 24)                  # the measure wants at least 2^20 records
        cols = s.array(n, np.uint64), s.array(n, np.uint32), s.array(n, np.uint64), s.array(n, np.float32)
        rate = C.c_double(0)
        _lib.check(lib.gki_measure_store_bw(cols[0].ptr, cols[1].ptr, cols[2].ptr, cols[3].ptr, n, C.byref(rate)))
    return statistics.median(times), rate.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=3e9)
    ap.add_argument("--sites", type=float, default=5e6)
    ap.add_argument("--runs", type=int, default=3, help="timed runs per encoding after the checked one")
    ap.add_argument("--fasta-parse", default="auto", choices=("auto", "host", "device"),
                    help="where the reference FASTA is parsed (build_graph_from_files' fasta_parse)")
    ap.add_argument("--dir", default=None, help="where the input files go (default: a temporary directory)")
    args = ap.parse_args()
    _lib.require_device()
    t0 = time.perf_counter()
    g = synthetic_snp_graph(int(args.bases), int(args.sites), 31, 1234, max_node_len=2 ** 31 - 1)
    numpy_seconds = time.perf_counter() - t0
    print("generated %d nodes in %.1f s" % (g.n_nodes, numpy_seconds), flush=True)
    with tempfile.TemporaryDirectory(prefix="gki_graph_build_", dir=args.dir) as d:
        paths, ref_af, alt_af = write_inputs(g, d)
        print("wrote the input files", flush=True)
        result = {"fasta_parse": args.fasta_parse, "bases": int(args.bases), "sites": int(np.sum(g.is_ref == 0)),
                  "nodes": g.n_nodes + 1,
                  "synthetic_snp_graph_numpy_s": round(numpy_seconds, 3),
                  "file_bytes": {k: os.path.getsize(p) for k, p in paths.items()}}
        for encoding in ("plain", "bgzf"):
            runs = []
            for i in range(args.runs + 1):
                t0 = time.perf_counter()
                built = build_graph_from_files(paths["fasta"], paths[encoding], allele_frequencies=(ref_af, alt_af),
                                               fasta_parse=args.fasta_parse)
                whole = time.perf_counter() - t0
                if i == 0:
                    assert_equals_generator(built, g)
                    print("%s: equals the generator's graph (ids + 1)" % encoding, flush=True)
                else:
                    stages = dict(built.timings, whole_call=whole, **vcf_text_stages(paths[encoding]))
                    stages["unattributed"] = whole - sum(v for k, v in built.timings.items() if not k.endswith("_ms"))
                    runs.append(stages)
                del built
            result[encoding] = {k: round(statistics.median(r[k] for r in runs), 4) for k in runs[0]} if runs else {}
    copy_s, store_rate = device_yardsticks(len(g.seq))
    result["device_copy_of_seq_bytes_ms"] = round(copy_s * 1e3, 3)
    result["store_ceiling_GBps"] = round(store_rate / 1e9, 1)
    for encoding in ("plain", "bgzf"):
        ms = result[encoding].get("sequence_kernel_ms")
        if ms:
            result[encoding]["sequence_kernel_GBps_read_plus_written"] = round(2 * len(g.seq) / ms / 1e6, 1)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
