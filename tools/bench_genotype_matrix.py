#!/usr/bin/env python3
"""Secondary benchmark (not the headline): the haplotype matrix of a multi-sample VCF FILE on one MI355X.
  python tools/bench_genotype_matrix.py --multi-lines 2e4 --samples 2504
Input, written to a temporary directory as plain text and as BGZF and taken whole (nothing is scaled from a prefix):
tools/bench_vcf_parse.py's multi-sample VCF, --multi-lines data lines x --samples phased GT columns, every allele 1 with
probability 0.1 (2e4 x 2504: about 200 MB of text).
From ONE run, per file:
  (a) host     the rule of DESIGN 4.18 stated on the host over the whole file, once: a loop over the lines with
               split("\\t") and a table from GT text to codes (the spec's byte loop is not what is timed).
  (b) device   vcf_files.haplotype_matrix_from_file end to end, the matrix on the host at its end: one warm-up pass, then
               --reps passes, the median.
  (c) kernels  per pass and in the same process, over all pieces: the device time of k_gt_matrix (events around the
               launch), the device time of k_af_genotypes on the same text (its own events), and a device-to-device copy of
               the text (a host clock around the copy and a synchronise); then, once per pass over the appended rows, the
               device time of k_haplotype_planes and a device-to-device copy of the codes it reads.
Every device result is checked equal to the host's, the planes against NumPy's packbits.
Prints one JSON object and a few summary lines."""
import argparse, contextlib, ctypes as C, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from graph_kmer_index_amd import _lib, bgzf, text_files, vcf_files
from bench_vcf_parse import write_multi

CODE = {b"0": 0, b"1": 1, b".": 3}


def host_rule(path, ploidy):
    """The rule of DESIGN 4.18 on well-formed input, as a host program would write it: (codes uint8[V, S * P], phased)."""
    rows, phased, table = [], [], {}
    with open(path, "rb") as f:
        for raw in f:
            if raw[:1] == b"#":
                continue
            row, all_phased = bytearray(), 1
            for sample in raw.rstrip(b"\r\n").split(b"\t")[9:]:
                gt = sample.split(b":", 1)[0]
                entry = table.get(gt)
                if entry is None:
                    alleles = gt.replace(b"|", b"/").split(b"/")
                    entry = table[gt] = (bytes(([CODE.get(a, 2) for a in alleles] + [3] * ploidy)[:ploidy]), b"/" not in gt)
                row += entry[0]
                all_phased &= entry[1]
            rows.append(bytes(row))
            phased.append(all_phased)
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1), np.array(phased, dtype=np.uint8)


def planes_by_packbits(codes):
    out = []
    for value in (0, 1):
        bits = np.zeros((codes.shape[1], -(-codes.shape[0] // 64) * 64), dtype=np.uint8)
        bits[:, :codes.shape[0]] = (codes == value).T
        out.append(np.packbits(bits, axis=1, bitorder="little").view("<u8"))
    return out


def timed_copy(dst, src, n):
    lib = _lib.load()
    _lib.check(lib.gki_device_synchronize())
    t = time.perf_counter()
    _lib.check(lib.gki_memcpy_d2d(dst.ptr, src.ptr, n))
    _lib.check(lib.gki_device_synchronize())
    return time.perf_counter() - t


def kernel_pass(path, ploidy, chunk_bytes, want, want_planes):
    """One pass over the file's pieces: the device times and whether every result equals the host's."""
    out = {"af_ms": 0.0, "text_copy_s": 0.0, "text_bytes": 0}
    with _lib.DeviceScope() as s:
        joined = vcf_files.MatrixPieces(s, ploidy, None)
        with contextlib.closing(text_files.text_pieces(path, chunk_bytes)) as pieces:
            for text, n in pieces:
                with _lib.DeviceScope() as t:
                    t.keep(text)
                    joined.add_piece(text, n)
                    nv = vcf_files.vcf_count(text, n)[1]
                    if nv:
                        out["af_ms"] += vcf_files.allele_frequencies_piece(t, text, n, "genotypes", nv)[3]
                    out["text_copy_s"] += timed_copy(t.array(n, np.uint8), text, n)
                    out["text_bytes"] += n
        out["matrix_ms"] = joined.kernel_ms
        d_codes, d_phased = joined.joined()
        n_variants, n_slots = want[0].shape
        ref_bits, alt_bits, out["planes_ms"] = vcf_files.haplotype_planes_on_device(s, d_codes, n_variants, n_slots)
        out["codes_copy_s"] = timed_copy(s.array(want[0].size, np.uint8), d_codes, want[0].size)
        out["equal"] = bool(joined.n_variants == n_variants and
                            np.array_equal(d_codes.to_host(want[0].size).reshape(want[0].shape), want[0]) and
                            np.array_equal(d_phased.to_host(n_variants), want[1]) and
                            all(np.array_equal(p.to_host(w.size).reshape(w.shape), w)
                                for p, w in zip((ref_bits, alt_bits), want_planes)))
    return out


def measure(path, ploidy, chunk_bytes, reps, want, want_planes):
    lib = _lib.load()
    passes, end_to_end, same = [], [], True
    for rep in range(reps + 1):                                    # the first pass warms the pool and the code up
        p = kernel_pass(path, ploidy, chunk_bytes, want, want_planes)
        t = time.perf_counter()
        got = vcf_files.haplotype_matrix_from_file(path, ploidy, chunk_bytes=chunk_bytes)
        _lib.check(lib.gki_device_synchronize())
        dt = time.perf_counter() - t
        same = same and p["equal"] and np.array_equal(got.codes, want[0]) and np.array_equal(got.phased, want[1])
        if rep:
            passes.append(p); end_to_end.append(dt)
    med = lambda key: statistics.median(p[key] for p in passes)
    matrix_s, af_s, copy_s, planes_s, codes_copy_s = med("matrix_ms") / 1e3, med("af_ms") / 1e3, med("text_copy_s"), \
        med("planes_ms") / 1e3, med("codes_copy_s")
    n_text = passes[0]["text_bytes"]
    return {"file_bytes": os.path.getsize(path), "data_lines": int(want[0].shape[0]), "slots": int(want[0].shape[1]),
            "text_bytes": n_text, "k_gt_matrix_s": matrix_s, "k_gt_matrix_all_ms": [p["matrix_ms"] for p in passes],
            "k_af_genotypes_s": af_s, "k_af_genotypes_all_ms": [p["af_ms"] for p in passes], "text_copy_s": copy_s,
            "matrix_over_text_copy": matrix_s / copy_s, "matrix_over_af_genotypes": matrix_s / af_s,
            "matrix_text_bytes_per_s": n_text / matrix_s, "text_copy_bytes_per_s": 2 * n_text / copy_s,
            "k_haplotype_planes_s": planes_s, "k_haplotype_planes_all_ms": [p["planes_ms"] for p in passes],
            "codes_copy_s": codes_copy_s, "planes_over_codes_copy": planes_s / codes_copy_s,
            "planes_codes_bytes_per_s": want[0].size / planes_s, "device_end_to_end_s": statistics.median(end_to_end),
            "device_end_to_end_all_s": end_to_end, "equal_to_host": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--multi-lines", type=float, default=2e4)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--ploidy", type=int, default=2)
    ap.add_argument("--chunk-bytes", type=int, default=text_files.DEFAULT_CHUNK_BYTES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tmp", default=None, help="directory for the files (default: the system's temporary directory)")
    args = ap.parse_args()
    _lib.load(); _lib.require_device()
    rng = np.random.default_rng(2025)
    res = {"multi_lines": int(args.multi_lines), "samples": args.samples, "ploidy": args.ploidy,
           "chunk_bytes": args.chunk_bytes, "reps": args.reps}
    ok = True
    with tempfile.TemporaryDirectory(prefix="gki_bench_gt_matrix_", dir=args.tmp) as tmp:
        paths = {"plain": os.path.join(tmp, "multi.vcf"), "bgzf": os.path.join(tmp, "multi_bgzf.vcf.gz")}
        write_multi(paths["plain"], rng, int(args.multi_lines), args.samples)
        with open(paths["plain"], "rb") as fh:
            bgzf.write_bgzf(paths["bgzf"], fh.read(), level=6, threads=16)
        t = time.perf_counter()
        want = host_rule(paths["plain"], args.ploidy)
        host_s = time.perf_counter() - t                           # a single run
        want_planes = planes_by_packbits(want[0])
        for encoding in ("plain", "bgzf"):
            m = measure(paths[encoding], args.ploidy, args.chunk_bytes, args.reps, want, want_planes)
            m["host_rule_s"], m["host_over_device"] = host_s, host_s / m["device_end_to_end_s"]
            res["multi_%s" % encoding] = m
            ok = ok and m["equal_to_host"]
            print("multi %s: %.0f MB file, %d data lines x %d slots; host rule %.2f s (one run, plain file); device %.3f s end "
                  "to end (%.1f x); k_gt_matrix %.4f s = %.2f x a device copy of the %.0f MB of text (%.4f s) = %.2f x "
                  "k_af_genotypes (%.4f s), %.0f GB/s of text; k_haplotype_planes %.4f s = %.2f x a device copy of the %.0f MB "
                  "of codes (%.4f s); equal: %s"
                  % (encoding, m["file_bytes"] / 1e6, m["data_lines"], m["slots"], host_s, m["device_end_to_end_s"],
                     m["host_over_device"], m["k_gt_matrix_s"], m["matrix_over_text_copy"], m["text_bytes"] / 1e6,
                     m["text_copy_s"], m["matrix_over_af_genotypes"], m["k_af_genotypes_s"],
                     m["matrix_text_bytes_per_s"] / 1e9, m["k_haplotype_planes_s"], m["planes_over_codes_copy"],
                     want[0].size / 1e6, m["codes_copy_s"], m["equal_to_host"]), flush=True)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
