#!/usr/bin/env python3
"""Secondary benchmark (not the headline): the genotyper and the genotyped VCF's text on MI355X.
  python tools/bench_genotype.py --bases 3e9 --sites 5e6 --samples 16
The 3 Gbp + 5 M SNP graph, the variant index and the alt plane of tools/bench_haplotype_count_model.py; the count model of
its `--samples` diploid individuals (node_count_model, difference route); the sample to genotype is individual 1's own row;
the VCF is one sites-only line per SNP, written to `--dir`.  In one run, medians of `--reps` after a warm-up, kernels by
device events:
  genotyper   the model's upload with the fit (host clock) and the fit kernel; per sample the scale and the call kernel, with
              the bytes each kernel moves and their rate as a share of the 8 TB/s peak; the whole genotype() call (host clock)
  writer      the whole text as one piece: the lengths kernel with its scan, the emit kernels, and a device copy of the
              output's bytes measured in the same run, which the text kernels are set beside
  command     the stages of the `genotype` sub-command from files to the VCF, host clock: the files loaded, the fit, the calls,
              the VCF written (with the host's write of the same bytes to a second file measured alone)
  host        the same rules as vectorised NumPy for the fit and the calls, a Python line loop for the text; the device's
              means, calls and text are compared with them
Prints one JSON object; every section is also printed as soon as it is measured."""
import argparse, ctypes as C, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from graph_kmer_index_amd import _lib, DenseKmerFinder, DeviceFlatKmers, CriticalGraphPaths
from graph_kmer_index_amd.collision_free_kmer_index import DeviceIndex
from graph_kmer_index_amd.genotyper import Genotyper, genotyped_lines_on_device, header_text, write_genotyped_vcf
from graph_kmer_index_amd.graph import synthetic_snp_graph
from graph_kmer_index_amd.haplotype_paths import AltPlane, HaplotypePaths, NodeCountModel
from graph_kmer_index_amd.unique_variant_kmers import VariantToNodesArrays, load_variant_to_nodes
from bench_haplotype_paths import IndexOnDevice, plane_row, section

PEAK_BYTES_PER_MS = 8e12 / 1e3
PHRED = 4.342944819032518


def median(values):
    return round(statistics.median(values), 5)


def kernel_line(ms, moved):
    return {"ms": ms, "bytes": int(moved), "share_of_8TBs": round(moved / ms / PEAK_BYTES_PER_MS, 4) if ms > 0 else None}


def numpy_fit(model, var_nodes):
    """The fit's rule, vectorised over the lines: (mean [V][2][E], n_alt [V][E])."""
    n = model.histogram.sum(axis=3, dtype=np.int64)
    kept = (var_nodes != 0)[:, None, None]
    populated = (n > 0) & kept
    own = np.zeros(n.shape)
    np.divide(model.count_sum.astype(np.float64), n.astype(np.float64), out=own, where=populated)
    mean, found, entries = own.copy(), populated.copy(), n.shape[2]
    for c in range(entries):
        for d in range(1, entries):
            for near in (c - d, c + d):
                if 0 <= near < entries:
                    take = ~found[:, :, c] & populated[:, :, near]
                    mean[:, :, c] = np.where(take, np.maximum(0.0, own[:, :, near] + float(c - near)), mean[:, :, c])
                    found[:, :, c] |= take
    return mean, np.where(kept[:, :, 0], n[:, 1, :], 0).astype(np.uint32)


def numpy_call(mean, n_alt, n_individuals, ref_nodes, var_nodes, x, lam, error, alpha):
    entries = n_alt.shape[1]
    ploidy = entries - 1
    kept = var_nodes != 0
    x0, x1 = x[ref_nodes].astype(np.float64), x[var_nodes].astype(np.float64)
    L = np.empty((len(var_nodes), entries))
    with np.errstate(divide="ignore", invalid="ignore"):
        for g in range(entries):
            m0, m1 = lam * (mean[:, 0, ploidy - g] + error), lam * (mean[:, 1, g] + error)
            prior = (n_alt[:, g].astype(np.float64) + alpha) / (float(n_individuals) + float(entries) * alpha)
            L[:, g] = x0 * np.log(m0) - m0 + x1 * np.log(m1) - m1 + np.log(prior)
    best = np.argmax(L, axis=1)
    top = L[np.arange(len(L)), best]
    rest = L.copy()
    rest[np.arange(len(L)), best] = -np.inf
    q = PHRED * (top - rest.max(axis=1))
    gq = np.where(q >= 99, 99, np.floor(np.minimum(q, 99))).astype(np.uint8)
    return np.where(kept, best, -1).astype(np.int8), np.where(kept, gq, 0).astype(np.uint8)


def python_lines(text, call, gq, ploidy):
    out, v = [], 0
    for line in text.split(b"\n"):
        line = line.rstrip(b"\r")
        if not line or line.startswith(b"#") or not line.strip():
            continue
        c = int(call[v])
        gt = b"/".join([b"."] * ploidy) + b":." if c < 0 else b"/".join([b"0"] * (ploidy - c) + [b"1"] * c) + b":%d" % gq[v]
        out.append(b"\t".join(line.split(b"\t")[:8]) + b"\tGT:GQ\t" + gt + b"\n")
        v += 1
    return b"".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=3e9)
    ap.add_argument("--sites", type=float, default=5e6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--bins", type=int, default=5)
    ap.add_argument("--modulo", type=int, default=452930477)
    ap.add_argument("--dir", default=None, help="where the files of the command go (default: a temporary directory)")
    args = ap.parse_args()
    lib = _lib.load(); _lib.require_device()
    k, ploidy = 31, 2
    t0 = time.perf_counter()
    g = synthetic_snp_graph(int(args.bases), int(args.sites), k=k, seed=1234)
    alts = np.flatnonzero(g.is_ref == 0)
    v2n = VariantToNodesArrays(alts - 1, alts)
    n_lines, n_slots, n_nodes = len(alts), args.samples * ploidy, g.n_nodes
    result = {"bases": int(args.bases), "sites": n_lines, "nodes": n_nodes, "samples": args.samples, "ploidy": ploidy,
              "bins": args.bins, "reps": args.reps}
    print("generated %d nodes in %.1f s" % (n_nodes, time.perf_counter() - t0), flush=True)
    rng = np.random.default_rng(17)
    rows = [plane_row(rng, n_lines, 0.5 if slot == 0 else 0.05) for slot in range(n_slots)]
    with _lib.DeviceScope() as s:
        plane = s.on_device(np.concatenate(rows), np.uint64)
        del rows
        cp = CriticalGraphPaths.from_graph(g, k)
        f = DenseKmerFinder(g, k, critical_graph_paths=cp, only_save_one_node_per_kmer=True, max_variant_nodes=5)
        flat = f.find_flat_on_device(); f.synchronize()
        n_int = f.interior_records()
        nb = flat.n - n_int
        bnd = DeviceFlatKmers(nb, flat.hashes.view(n_int, nb), flat.nodes.view(n_int, nb), flat.ref_offsets.view(n_int, nb),
                              flat.allele_frequencies.view(n_int, nb))
        idx = DeviceIndex.build(bnd, args.modulo)
        _lib.check(lib.gki_device_synchronize())
        flat.free()
        del bnd, flat, f
        index = IndexOnDevice(idx, n_nodes)
        idx.probe_table()
        with HaplotypePaths(g, v2n, AltPlane(plane, n_lines, n_slots)) as paths:
            t0 = time.perf_counter()
            model = paths.node_count_model(index, k, None, args.bins, n_nodes, ploidy=ploidy)
            model_s = time.perf_counter() - t0
            own = paths.node_counts_by_difference([ploidy, ploidy + 1], index, k, n_nodes)
            counts = (own[0] + own[1]).astype(np.uint32)
            del own
        idx.free()
    del g, cp
    section(result, "inputs", {"node_count_model_s": round(model_s, 4), "histogram_bytes": model.histogram.nbytes,
                               "count_sum_bytes": model.count_sum.nbytes, "sample_hits": int(counts.sum(dtype=np.int64))})
    ref_nodes, var_nodes = v2n.ref_nodes.astype(np.int64), v2n.var_nodes.astype(np.int64)
    V, E = n_lines, ploidy + 1

    # ---- the genotyper
    t0 = time.perf_counter()
    genotyper = Genotyper(model, v2n)
    upload_and_fit_s = time.perf_counter() - t0
    with genotyper:
        fit_bytes = model.histogram.nbytes + model.count_sum.nbytes + 4 * V + 2 * E * 8 * V + E * 4 * V
        scale_bytes = 8 * V + 8 * V
        call_bytes = 2 * E * 8 * V + E * 4 * V + 8 * V + 8 * V + 2 * V
        genotyper.genotype(counts)                         # warm-up
        timings, walls = [], []
        for _ in range(args.reps):
            t = {}
            t0 = time.perf_counter()
            calls = genotyper.genotype(counts, timings=t)
            walls.append(time.perf_counter() - t0)
            timings.append(t)
        t = {}
        with_loglik = genotyper.genotype(counts, loglik=True, timings=t)
        section(result, "genotyper", {
            "upload_and_fit_s": round(upload_and_fit_s, 4), "total": genotyper.total, "coverage": float(calls.coverage[0]),
            "fit": kernel_line(round(genotyper.fit_ms, 5), fit_bytes),
            "scale": kernel_line(median([t["scale_ms"] for t in timings]), scale_bytes),
            "call": kernel_line(median([t["call_ms"] for t in timings]), call_bytes),
            "call_with_loglik": kernel_line(round(t["call_ms"], 5), call_bytes + E * 8 * V),
            "genotype_call_s": median(walls), "genotype_call_all_s": [round(w, 5) for w in walls],
            "not_called": int(np.count_nonzero(calls.call < 0)), "alt_calls": int(np.count_nonzero(calls.call > 0)),
            "gq99": int(np.count_nonzero(calls.gq == 99))})
        device_mean, device_n_alt = genotyper.mean, genotyper.n_alt
        del with_loglik

    # ---- the writer: the whole text as one piece
    work = args.dir or tempfile.mkdtemp(prefix="bench_genotype_")
    files = {n: os.path.join(work, n) for n in ("in.vcf", "out.vcf", "again.vcf", "model.npz", "v2n.npz", "counts.npy")}
    head = b"##fileformat=VCFv4.2\n##contig=<ID=1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
    text = head + b"".join(b"1\t%d\t.\tA\tC\t.\tPASS\t.\n" % (600 * i + 1) for i in range(V))
    open(files["in.vcf"], "wb").write(text)
    with _lib.DeviceScope() as s:
        d_text = s.on_device(np.frombuffer(text, dtype=np.uint8), np.uint8)
        d_call, d_gq = s.on_device(calls.call, np.int8), s.on_device(calls.gq, np.uint8)
        lengths, both, copies = [], [], []
        n_out = 0
        for rep in range(args.reps + 1):
            with _lib.DeviceScope() as piece:
                t = {}
                out, n_out, n_data = genotyped_lines_on_device(piece, d_text, len(text), d_call, d_gq, 0, V, ploidy, t)
                ms = C.c_float(0)
                twin = piece.array(n_out, np.uint8)
                _lib.check(lib.gki_measure_copy_ms(twin.ptr, out.ptr, n_out, C.byref(ms)))
                if rep:                                    # the first is the warm-up
                    lengths.append(t["lengths_ms"]); both.append(t["emit_call_ms"]); copies.append(ms.value)
                if rep == args.reps:
                    device_text = out.to_host(n_out).tobytes()
        lengths_ms, emit_ms, copy_ms = median(lengths), median([b - a for a, b in zip(lengths, both)]), median(copies)
        section(result, "writer", {"in_bytes": len(text), "out_bytes": int(n_out), "data_lines": int(n_data),
                                   "lengths_and_scan_ms": lengths_ms, "emit_ms": emit_ms, "device_copy_of_out_bytes_ms": copy_ms,
                                   "lengths_over_copy": round(lengths_ms / copy_ms, 2), "emit_over_copy": round(emit_ms / copy_ms, 2)})

    # ---- the command's stages from files
    model.to_file(files["model.npz"]); v2n.to_file(files["v2n.npz"]); np.save(files["counts.npy"], counts)
    stages = {}
    t_all = time.perf_counter()
    t0 = time.perf_counter()
    m2, v2, c2 = NodeCountModel.from_file(files["model.npz"]), load_variant_to_nodes(files["v2n.npz"]), np.load(files["counts.npy"])
    stages["load_files_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    with Genotyper(m2, v2) as again:
        stages["upload_and_fit_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        calls2 = again.genotype(c2)
        stages["genotype_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    kernels = {}
    write_genotyped_vcf(files["in.vcf"], files["out.vcf"], calls2.call, calls2.gq, ploidy, "sample", timings=kernels)
    stages["write_vcf_s"] = time.perf_counter() - t0
    stages["total_s"] = time.perf_counter() - t_all
    written = open(files["out.vcf"], "rb").read()
    t0 = time.perf_counter()
    with open(files["again.vcf"], "wb") as out_file:
        out_file.write(written)
    stages["host_write_of_the_same_bytes_s"] = time.perf_counter() - t0
    stages = {key: round(v, 4) for key, v in stages.items()}
    stages["write_vcf_kernel_ms"] = round(kernels["emit_call_ms"], 3)
    stages["vcf_bytes"] = len(written)
    assert np.array_equal(calls2.call, calls.call) and written == header_text(files["in.vcf"]) + device_text
    section(result, "command", stages)

    # ---- the host's baseline, and the device's results against it
    t0 = time.perf_counter()
    host_mean, host_n_alt = numpy_fit(model, var_nodes)
    fit_s = time.perf_counter() - t0
    lam = float(calls.coverage[0])
    t0 = time.perf_counter()
    host_call, host_gq = numpy_call(host_mean, host_n_alt, args.samples, ref_nodes, var_nodes, counts, lam, 0.01, 1.0)
    call_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    host_text = python_lines(text, calls.call, calls.gq, ploidy)
    lines_s = time.perf_counter() - t0
    section(result, "host", {"numpy_fit_s": round(fit_s, 4), "numpy_call_s": round(call_s, 4), "python_line_loop_s": round(lines_s, 4),
                             "means_bit_equal": bool(np.array_equal(host_mean.view(np.uint64), device_mean.view(np.uint64))),
                             "n_alt_equal": bool(np.array_equal(host_n_alt, device_n_alt)),
                             "calls_that_differ": int(np.count_nonzero(host_call != calls.call)),
                             "qualities_that_differ": int(np.count_nonzero(host_gq != calls.gq)),
                             "text_equal": host_text == device_text})
    if args.dir is None:
        for name in files.values():
            if os.path.exists(name):
                os.remove(name)
        os.rmdir(work)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
