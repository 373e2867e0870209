#!/usr/bin/env python3
"""Secondary benchmark (not the headline): the genotyped cohort VCF's text on MI355X.
  python tools/bench_genotype_cohort.py --sites 5e6 --samples 64 --few-sites 2e4 --many-samples 2504
Two shapes on the sites-only VCF text of tools/bench_genotype.py (one line per SNP): `--samples` columns on `--sites` lines,
and `--many-samples` columns on `--few-sites` lines.  The calls are drawn, not genotyped (2 % no-calls, 70 % of the
qualities 99, the rest uniform in 0..98): the writer's work depends on the text and the calls' widths alone.  In one run
per shape, medians of `--reps` after a warm-up, kernels by device events:
  cohort      the text as one piece: the pack pass, the lengths kernel with its scan, the tile search with the emit kernel,
              and a device copy of the output's bytes measured in the same run, which they are set beside
  single      k_vcf_gt_emit on the same text with sample 0's calls, and a device copy of ITS output: the yardstick ratio
  files       write_cohort_vcf from the file to a plain and to a BGZF file (host clock, once each), and `--single-runs`
              runs of write_genotyped_vcf, whose time times the samples is what the same data costs without this writer
  host        the spec's Python loop over the first `--host-lines` lines (its text compared with the device's), scaled to
              the shape by lines
Prints one JSON object; every section is also printed as soon as it is measured."""
import argparse, ctypes as C, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from graph_kmer_index_amd import _lib
from graph_kmer_index_amd.genotyper import genotyped_lines_on_device, write_cohort_vcf, write_genotyped_vcf
import spec_genotype_cohort as spec

HEAD = b"##fileformat=VCFv4.2\n##contig=<ID=1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def median(values):
    return round(statistics.median(values), 5)


def section(result, name, values):
    result[name] = values
    print(name, json.dumps(values), flush=True)


def shape(lib, args, S, V, work, result, name):
    ploidy = 2
    rng = np.random.default_rng([S, V])
    text = HEAD + b"".join(b"1\t%d\t.\tA\tC\t.\tPASS\t.\n" % (600 * i + 1) for i in range(V))
    call = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(S, V), p=[0.02, 0.6, 0.25, 0.13])
    gq = np.where(rng.random((S, V)) < 0.7, 99, rng.integers(0, 99, size=(S, V))).astype(np.uint8)
    out = {"samples": S, "lines": V, "in_bytes": len(text), "reps": args.reps}
    with _lib.DeviceScope() as s:
        d_text = s.on_device(np.frombuffer(text, dtype=np.uint8), np.uint8)
        d_call, d_gq = s.on_device(call.reshape(-1), np.int8), s.on_device(gq.reshape(-1), np.uint8)
        batch = (d_text.ptr, len(text), d_call.ptr, d_gq.ptr, V, 0, S, V, ploidy)
        n_data, n_out, line, kind = C.c_int64(0), C.c_int64(0), C.c_int64(-1), C.c_int(0)
        _lib.check(lib.gki_vcf_cohort_count(*batch, C.byref(n_data), C.byref(n_out), C.byref(line), C.byref(kind), None, 0, None))
        assert n_data.value == V and kind.value == 0
        packs, lengths, emits, copies = [], [], [], []
        for rep in range(args.reps + 1):
            with _lib.DeviceScope() as piece:
                lines, twin = piece.array(n_out.value, np.uint8), piece.array(n_out.value, np.uint8)
                written, ms = C.c_int64(0), [C.c_float(0), C.c_float(0), C.c_float(0), C.c_float(0)]
                _lib.check(lib.gki_vcf_cohort_emit(*batch, 0, V, lines.ptr, lines.n, C.byref(written), None))
                _lib.check(lib.gki_vcf_cohort_kernel_ms(C.byref(ms[0]), C.byref(ms[1]), C.byref(ms[2])))
                _lib.check(lib.gki_measure_copy_ms(twin.ptr, lines.ptr, n_out.value, C.byref(ms[3])))
                if rep:                                    # the first is the warm-up
                    for values, m in zip((packs, lengths, emits, copies), ms):
                        values.append(m.value)
                if rep == args.reps:
                    head_lines = min(args.host_lines, V)
                    t0 = time.perf_counter()
                    first_lines = b"\n".join(text[len(HEAD):].split(b"\n", head_lines)[:head_lines])
                    want = spec.data_lines_text(first_lines, call[:, :head_lines], gq[:, :head_lines], ploidy)
                    host_s = time.perf_counter() - t0
                    text_equal = lines.to_host(len(want)).tobytes() == want
        copy_ms = median(copies)
        out.update({"out_bytes": n_out.value, "pack_ms": median(packs), "lengths_and_scan_ms": median(lengths),
                    "tile_search_and_emit_ms": median(emits), "device_copy_of_out_bytes_ms": copy_ms,
                    "pack_over_copy": round(median(packs) / copy_ms, 2), "lengths_over_copy": round(median(lengths) / copy_ms, 2),
                    "emit_over_copy": round(median(emits) / copy_ms, 2),
                    "emit_GBps": round(n_out.value / median(emits) / 1e6, 1)})
        # the yardstick: the single-sample emit kernel on the same text, and a copy of its output
        lengths, both, copies = [], [], []
        for rep in range(args.reps + 1):
            with _lib.DeviceScope() as piece:
                t, ms = {}, C.c_float(0)
                one, n_one, _ = genotyped_lines_on_device(piece, d_text, len(text), d_call, d_gq, 0, V, ploidy, t)
                twin = piece.array(n_one, np.uint8)
                _lib.check(lib.gki_measure_copy_ms(twin.ptr, one.ptr, n_one, C.byref(ms)))
                if rep:
                    lengths.append(t["lengths_ms"]); both.append(t["emit_call_ms"]); copies.append(ms.value)
        single_emit = median([b - a for a, b in zip(lengths, both)])
        out["single_sample"] = {"out_bytes": int(n_one), "emit_ms": single_emit, "device_copy_of_its_out_bytes_ms": median(copies),
                                "emit_over_copy": round(single_emit / median(copies), 2)}
    out["host"] = {"python_loop_lines": head_lines, "python_loop_s": round(host_s, 4),
                   "python_loop_scaled_to_the_shape_s": round(host_s * V / head_lines, 2), "text_equal": bool(text_equal)}
    section(result, name, out)
    if not args.files:
        return
    files = {n: os.path.join(work, n) for n in ("in.vcf", "cohort.vcf", "cohort.vcf.gz", "single.vcf")}
    open(files["in.vcf"], "wb").write(text)
    names = ["s%d" % i for i in range(S)]
    stages = {}
    for key, target, compress in (("plain", "cohort.vcf", "none"), ("bgzf", "cohort.vcf.gz", "bgzf")):
        kernels = {}
        t0 = time.perf_counter()
        write_cohort_vcf(files["in.vcf"], files[target], call, gq, ploidy, names, compress=compress, timings=kernels)
        stages["write_cohort_vcf_%s_s" % key] = round(time.perf_counter() - t0, 4)
        stages["%s_file_bytes" % key] = os.path.getsize(files[target])
        stages["%s_kernel_ms" % key] = {k: round(v, 3) for k, v in kernels.items()}
        os.remove(files[target])
    runs = []
    for r in range(min(args.single_runs, S)):
        t0 = time.perf_counter()
        write_genotyped_vcf(files["in.vcf"], files["single.vcf"], call[r], gq[r], ploidy, names[r])
        runs.append(time.perf_counter() - t0)
    stages["write_genotyped_vcf_runs_s"] = [round(x, 4) for x in runs]
    stages["one_run_times_the_samples_s"] = round(statistics.median(runs) * S, 2)
    for name_ in ("in.vcf", "single.vcf"):
        os.remove(files[name_])
    section(result, name + "_files", stages)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=float, default=5e6)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--few-sites", type=float, default=2e4)
    ap.add_argument("--many-samples", type=int, default=2504)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-lines", type=int, default=2000)
    ap.add_argument("--single-runs", type=int, default=2)
    ap.add_argument("--files", type=int, default=1, help="0: leave the whole calls from and to files out")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    args = ap.parse_args()
    lib = _lib.load(); _lib.require_device()
    work = args.dir or tempfile.mkdtemp(prefix="bench_genotype_cohort_")
    result = {}
    shape(lib, args, args.samples, int(args.sites), work, result, "many_lines")
    shape(lib, args, args.many_samples, int(args.few_sites), work, result, "many_samples")
    if args.dir is None:
        os.rmdir(work)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
