#!/usr/bin/env python3
"""Secondary benchmark (not the headline): allele frequencies from a VCF FILE on one MI355X.
  python tools/bench_vcf_allele_frequencies.py --sites 5e6 --multi-lines 2e4 --samples 2504 --graph-bases 3e9 --graph-sites 5e6
Inputs, written to a temporary directory, each as plain text and as BGZF, and taken whole (nothing is scaled from a prefix):
  multi   tools/bench_vcf_parse.py's multi-sample VCF: --multi-lines data lines x --samples phased GT columns, every
          allele 1 with probability 0.1 (2e4 x 2504: about 200 MB of text); source genotypes
  sites   that tool's sites-only VCF of --sites data lines with an AF= entry of 1 to 9 digits behind AC=; source info
From ONE run, per file:
  (a) host     the same rule stated on the host over the whole file, once: a loop over the lines with split("\\t") (the
               spec's byte loop is not what is timed).
  (b) device   vcf_files.allele_frequencies_from_file end to end: one warm-up pass, then --reps passes, the median.
  (c) kernel   per pass, the device time of the source's kernel over all pieces (events around the launch), and in the same
               pass and process a device-to-device copy of every piece's text: the kernel as a multiple of that copy.
Every device result is checked bit-equal to the host's.
  graph   DESIGN 4.15's input (tools/bench_graph_build.py's reference and SNPs, --graph-bases / --graph-sites) with an AF=
          entry on every line: build_graph_from_files without a source and with source info, --reps runs each after a
          warm-up, alternating, the medians and the difference; the graphs' allele_freq is checked against the host rule.
Prints one JSON object and a few summary lines."""
import argparse, contextlib, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from graph_kmer_index_amd import _lib, bgzf, text_files, vcf_files
from bench_vcf_parse import HEADER, site_columns, write_multi


def write_sites_with_af(path, rng, n, rows_per_write=500_000):
    chrom, pos, ref, alt = site_columns(rng, n)
    digits = rng.integers(1, 10, size=n)
    af = rng.integers(0, 10 ** 9, size=n) // 10 ** (9 - digits)
    with open(path, "wb") as f:
        f.write(HEADER + b"\n")
        for a in range(0, n, rows_per_write):
            b = min(n, a + rows_per_write)
            f.write(b"".join([b"%d\t%d\t.\t%s\t%s\t.\tPASS\tAC=1;AF=0.%0*d;NS=2504\n" % row
                              for row in zip(chrom[a:b].tolist(), pos[a:b].tolist(), ref[a:b], alt[a:b], digits[a:b].tolist(),
                                             af[a:b].tolist())]))


def host_rule(path, source):
    """The rule of DESIGN 4.17 on well-formed input, as a host program would write it: (ref_af, alt_af) per data line."""
    ref_af, alt_af = [], []
    with open(path, "rb") as f:
        for raw in f:
            if raw[:1] == b"#":
                continue
            fields = raw.rstrip(b"\r\n").split(b"\t")
            value = None
            if source == "info":
                for entry in fields[7].split(b";") if len(fields) > 7 else ():
                    if entry[:3] == b"AF=":
                        text = entry[3:].split(b",")[0]
                        value = None if text in (b"", b".") else float(text)
                        break
                ref_af.append(1.0 if value is None else 1.0 - value)
                alt_af.append(1.0 if value is None else value)
            else:
                n_called = n_ref = n_alt = 0
                for sample in fields[9:]:
                    for allele in sample.split(b":", 1)[0].replace(b"|", b"/").split(b"/"):
                        if allele != b".":
                            n_called += 1
                            n_ref += allele == b"0"
                            n_alt += allele == b"1"
                ref_af.append(n_ref / n_called if n_called else 1.0)
                alt_af.append(n_alt / n_called if n_called else 1.0)
    return np.array(ref_af, dtype=np.float64), np.array(alt_af, dtype=np.float64)


def kernel_pass(path, source, chunk_bytes):
    """One pass over the file's pieces: (kernel ms summed, device-copy seconds summed, text bytes, ref_af, alt_af)."""
    lib = _lib.load()
    sync = lambda: _lib.check(lib.gki_device_synchronize())
    ms, copy_s, n_text, ref_af, alt_af = 0.0, 0.0, 0, [], []
    with contextlib.closing(text_files.text_pieces(path, chunk_bytes)) as pieces:
        for text, n in pieces:
            with _lib.DeviceScope() as s:
                s.keep(text)
                nv = vcf_files.vcf_count(text, n)[1]
                r, a, _, piece_ms, fault = vcf_files.allele_frequencies_piece(s, text, n, source, nv)
                assert fault is None
                ms, n_text = ms + piece_ms, n_text + n
                ref_af.append(r.to_host(nv)); alt_af.append(a.to_host(nv))
                other = s.array(n, np.uint8); sync()
                t = time.perf_counter()
                _lib.check(lib.gki_memcpy_d2d(other.ptr, text.ptr, n)); sync()
                copy_s += time.perf_counter() - t
    return ms, copy_s, n_text, np.concatenate(ref_af), np.concatenate(alt_af)


def same_bits(a, b):
    return bool(len(a) == len(b) and np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def measure(path, source, chunk_bytes, reps, want):
    lib = _lib.load()
    row = {"file_bytes": os.path.getsize(path), "data_lines": len(want[0])}
    passes, end_to_end, same = [], [], True
    for rep in range(reps + 1):                                    # the first pass warms the pool and the code up
        ms, copy_s, n_text, ref_af, alt_af = kernel_pass(path, source, chunk_bytes)
        same = same and same_bits(ref_af, want[0]) and same_bits(alt_af, want[1])
        t = time.perf_counter()
        got = vcf_files.allele_frequencies_from_file(path, source, chunk_bytes=chunk_bytes)
        _lib.check(lib.gki_device_synchronize())
        dt = time.perf_counter() - t
        same = same and same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        if rep:
            passes.append((ms, copy_s)); end_to_end.append(dt)
    kernel_s = statistics.median(p[0] for p in passes) / 1e3
    copy_s = statistics.median(p[1] for p in passes)
    row.update({"text_bytes": n_text, "kernel_s": kernel_s, "kernel_all_ms": [p[0] for p in passes], "device_copy_s": copy_s,
                "kernel_over_device_copy": kernel_s / copy_s, "kernel_text_bytes_per_s": n_text / kernel_s,
                "device_copy_bytes_per_s": 2 * n_text / copy_s, "device_end_to_end_s": statistics.median(end_to_end),
                "device_end_to_end_all_s": end_to_end, "routes": np.bincount(got[2], minlength=3).tolist(),
                "equal_to_host": same})
    return row


def measure_graph(tmp, bases, sites, reps):
    from bench_graph_build import write_inputs
    from graph_kmer_index_amd.graph import synthetic_snp_graph
    from graph_kmer_index_amd.graph_files import build_graph_from_files
    g = synthetic_snp_graph(bases, sites, 31, 1234, max_node_len=2 ** 31 - 1)
    print("graph: generated", file=sys.stderr, flush=True)
    paths, _, _ = write_inputs(g, tmp)
    print("graph: inputs written", file=sys.stderr, flush=True)
    del g
    with open(paths["plain"], "rb") as f:
        lines = f.read().split(b"\n")
    text = b"\n".join(l if l[:1] == b"#" or not l else l[:-1] + b"AF=0.%04d" % (i % 9973) for i, l in enumerate(lines))
    del lines
    with open(paths["plain"], "wb") as f:
        f.write(text)
    bgzf.write_bgzf(paths["bgzf"], text, threads=16)
    del text
    want = host_rule(paths["plain"], "info")
    res = {"bases": bases, "sites": sites}
    for encoding in ("plain", "bgzf"):
        times, same = {None: [], "info": []}, True
        for rep in range(reps + 1):
            for source in (None, "info"):
                t = time.perf_counter()
                built = build_graph_from_files(paths["fasta"], paths[encoding], allele_frequencies=source)
                dt = time.perf_counter() - t
                if rep:
                    times[source].append(dt)
                if source == "info":
                    v2n, af = built.variant_to_nodes, built.graph.allele_freq
                    kept = v2n.var_nodes > 0
                    same = same and same_bits(af[v2n.ref_nodes[kept]], want[0][kept]) and same_bits(af[v2n.var_nodes[kept]], want[1][kept])
                    stage = built.timings["allele_frequencies"], built.timings["allele_frequencies_kernel_ms"]
                del built
        res[encoding] = {"without_s": statistics.median(times[None]), "with_info_s": statistics.median(times["info"]),
                         "without_all_s": times[None], "with_info_all_s": times["info"],
                         "allele_frequencies_stage_s": stage[0], "allele_frequencies_kernel_ms": stage[1], "equal_to_host": same}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=float, default=5e6)
    ap.add_argument("--multi-lines", type=float, default=2e4)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--graph-bases", type=float, default=3e9, help="0: leave the graph comparison out")
    ap.add_argument("--graph-sites", type=float, default=5e6)
    ap.add_argument("--chunk-bytes", type=int, default=text_files.DEFAULT_CHUNK_BYTES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tmp", default=None, help="directory for the files (default: the system's temporary directory)")
    args = ap.parse_args()
    _lib.load(); _lib.require_device()
    rng = np.random.default_rng(2025)
    res = {"sites": int(args.sites), "multi_lines": int(args.multi_lines), "samples": args.samples,
           "chunk_bytes": args.chunk_bytes, "reps": args.reps}
    ok = True
    with tempfile.TemporaryDirectory(prefix="gki_bench_vcf_af_", dir=args.tmp) as tmp:
        for name, source, write in (("multi", "genotypes", lambda p: write_multi(p, rng, int(args.multi_lines), args.samples)),
                                    ("sites", "info", lambda p: write_sites_with_af(p, rng, int(args.sites)))):
            paths = {"plain": os.path.join(tmp, name + ".vcf"), "bgzf": os.path.join(tmp, name + "_bgzf.vcf.gz")}
            write(paths["plain"])
            with open(paths["plain"], "rb") as fh:
                bgzf.write_bgzf(paths["bgzf"], fh.read(), level=6, threads=16)
            t = time.perf_counter()
            want = host_rule(paths["plain"], source)
            host_s = time.perf_counter() - t                       # a single run
            for encoding in ("plain", "bgzf"):
                m = measure(paths[encoding], source, args.chunk_bytes, args.reps, want)
                m["host_rule_s"], m["host_over_device"] = host_s, host_s / m["device_end_to_end_s"]
                res["%s_%s" % (name, encoding)] = m
                ok = ok and m["equal_to_host"]
                print("%s %s (source %s): %.0f MB file, %d data lines, routes %s; host rule %.2f s (one run, plain file); device "
                      "%.3f s end to end (%.1f x); kernel %.4f s = %.2f x a device copy of the %.0f MB of text (%.4f s), "
                      "%.0f GB/s of text; equal: %s"
                      % (name, encoding, source, m["file_bytes"] / 1e6, m["data_lines"], m["routes"], host_s,
                         m["device_end_to_end_s"], m["host_over_device"], m["kernel_s"], m["kernel_over_device_copy"],
                         m["text_bytes"] / 1e6, m["device_copy_s"], m["kernel_text_bytes_per_s"] / 1e9, m["equal_to_host"]),
                      flush=True)
            for p in paths.values():
                os.remove(p)
        if args.graph_bases:
            res["graph"] = g = measure_graph(tmp, int(args.graph_bases), int(args.graph_sites), args.reps)
            for encoding in ("plain", "bgzf"):
                m = g[encoding]
                ok = ok and m["equal_to_host"]
                print("graph %s: %d bases, %d sites; build_graph_from_files %.3f s without a source, %.3f s with source info "
                      "(+%.3f s; its stage %.3f s, kernel %.2f ms); equal: %s"
                      % (encoding, g["bases"], g["sites"], m["without_s"], m["with_info_s"], m["with_info_s"] - m["without_s"],
                         m["allele_frequencies_stage_s"], m["allele_frequencies_kernel_ms"], m["equal_to_host"]), flush=True)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
