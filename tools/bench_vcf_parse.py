#!/usr/bin/env python3
"""Secondary benchmark (not the headline): a VCF FILE to VariantArrays on one MI355X, host route against device route.
  python tools/bench_vcf_parse.py --sites 5e6 --multi-lines 2e4 --samples 2504
Two synthetic files are written to a temporary directory:
  sites   a sites-only VCF of --sites data lines (8 columns) on 22 chromosomes, 12 % of them indels
  multi   a multi-sample VCF of --multi-lines data lines, each with FORMAT GT and --samples phased genotype columns
          (2e4 lines x 2504 samples x 4 bytes: about 200 MB of text)
each as plain text, as Python gzip (gzip.open, level 6) and as BGZF (bgzf.write_bgzf, level 6).  For each of the six files,
from ONE run:
  (a) host     VariantArrays.from_vcf, the whole file, once (nothing is scaled from a prefix).
  (b) device   VariantArrays.from_vcf_on_device end to end, and the same loop with a clock around each stage: file read (for
               Python gzip this holds the host's inflate; for BGZF the member scan), upload, inflate (BGZF only, with the
               line cut), parse kernels (gki_vcf_parse_count + gki_vcf_parse_emit, both synchronous), copy back (device
               arrays to host arrays and names).  One warm-up pass, then --reps passes; the median is reported.
  (c) copy     a device-to-device copy of every piece's text bytes, in the same passes: the parse kernels' time is reported
               as a multiple of it.
Every device result is checked equal to the host's.  Prints one JSON object and a few summary lines."""
import argparse, gzip, json, mmap, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from graph_kmer_index_amd import _lib, bgzf, read_files, vcf_files
from graph_kmer_index_amd.unique_variant_kmers import VariantArrays

HEADER = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"


def site_columns(rng, n):
    """(chromosome 1..22, POS ascending inside a chromosome, REF, ALT) of n sites."""
    chrom = np.sort(rng.integers(1, 23, size=n))
    pos = np.empty(n, dtype=np.int64)
    for c in range(1, 23):
        sel = chrom == c
        pos[sel] = np.sort(rng.integers(1, 250_000_000, size=int(sel.sum())))
    kind = rng.random(n)
    base = np.array([b"A", b"C", b"G", b"T"])
    ref, alt = base[rng.integers(0, 4, size=n)].astype(object), base[rng.integers(0, 4, size=n)].astype(object)
    ref[kind < 0.06] = b"ACG"                                   # deletions
    alt[kind > 0.94] = b"TTGA"                                  # insertions
    return chrom, pos, ref, alt


def write_sites(path, rng, n, rows_per_write=500_000):
    chrom, pos, ref, alt = site_columns(rng, n)
    with open(path, "wb") as f:
        f.write(HEADER + b"\n")
        for a in range(0, n, rows_per_write):
            b = min(n, a + rows_per_write)
            f.write(b"".join([b"%d\t%d\t.\t%s\t%s\t.\tPASS\tAC=1\n" % row
                              for row in zip(chrom[a:b].tolist(), pos[a:b].tolist(), ref[a:b], alt[a:b])]))


def write_multi(path, rng, n, samples, rows_per_write=2_000):
    chrom, pos, ref, alt = site_columns(rng, n)
    with open(path, "wb") as f:
        f.write(HEADER + b"\tFORMAT" + b"".join(b"\tS%05d" % i for i in range(samples)) + b"\n")
        for a in range(0, n, rows_per_write):
            b = min(n, a + rows_per_write)
            gt = np.empty((b - a, samples, 4), dtype=np.uint8)
            gt[:, :, 0], gt[:, :, 2] = 9, ord("|")
            gt[:, :, 1] = ord("0") + (rng.random((b - a, samples)) < 0.1)
            gt[:, :, 3] = ord("0") + (rng.random((b - a, samples)) < 0.1)
            rows = gt.reshape(b - a, samples * 4)
            f.write(b"".join([b"%d\t%d\t.\t%s\t%s\t.\tPASS\tAC=1\tGT%s\n" % (c, p, r, t, rows[i].tobytes())
                              for i, (c, p, r, t) in enumerate(zip(chrom[a:b].tolist(), pos[a:b].tolist(), ref[a:b], alt[a:b]))]))


def same_variants(got, want):
    return bool(np.array_equal(got.positions, want.positions) and np.array_equal(got.is_snp, want.is_snp)
                and np.array_equal(got.line_numbers, want.line_numbers)
                and np.array_equal(got.chromosomes.astype(str), want.chromosomes.astype(str)))


def staged_route(path, chunk_bytes):
    """vcf_files.variant_arrays_from_file's steps with a clock around each stage, and the device copy of every piece."""
    lib = _lib.load()
    sync = lambda: _lib.check(lib.gki_device_synchronize())
    st = dict(file_read_s=0.0, upload_s=0.0, inflate_s=0.0, parse_count_s=0.0, parse_emit_s=0.0, copy_back_s=0.0,
              device_copy_s=0.0)
    joined, n_text = vcf_files.VariantPieces(), 0

    def parse(text, n):
        nonlocal n_text
        n_text += n
        with _lib.DeviceScope() as s:
            t = time.perf_counter()
            n_lines, n_variants, n_runs, n_names, bad, kind = vcf_files.vcf_count(text, n)
            st["parse_count_s"] += time.perf_counter() - t
            assert bad < 0
            t = time.perf_counter()
            arrays = vcf_files.vcf_emit(s, text, n, n_variants, n_runs, n_names)
            st["parse_emit_s"] += time.perf_counter() - t
            t = time.perf_counter()
            joined.add(*vcf_files.copy_back(*arrays), n_lines)
            st["copy_back_s"] += time.perf_counter() - t
            other = s.array(n, np.uint8); sync()
            t = time.perf_counter()
            _lib.check(lib.gki_memcpy_d2d(other.ptr, text.ptr, n)); sync()
            st["device_copy_s"] += time.perf_counter() - t

    t_all = time.perf_counter()
    if read_files.reads_file_route(path) == "bgzf-device":
        with _lib.DeviceScope() as run, open(path, "rb") as f:
            pieces, tail = read_files.iter_bgzf_pieces(f, chunk_bytes, path), None
            while True:
                t = time.perf_counter()
                item = next(pieces, None)
                st["file_read_s"] += time.perf_counter() - t
                if item is None:
                    break
                piece, members, base = item
                with _lib.DeviceScope() as s:
                    t = time.perf_counter()
                    d = s.keep(read_files.upload_piece(piece)); sync()
                    st["upload_s"] += time.perf_counter() - t
                    t = time.perf_counter()
                    text = s.keep(read_files.inflate_piece(d, members, base, tail, path))
                    cut, tail = read_files.cut_at_line_end(text); sync()
                    st["inflate_s"] += time.perf_counter() - t
                    d.free()
                    if tail is not None:
                        run.keep(tail)
                    if cut:
                        parse(text, cut)
            if tail is not None:
                parse(tail, tail.n)
    else:
        with read_files.open_reads_file(path) as f:
            pieces = read_files.iter_line_chunks(f, chunk_bytes)
            while True:
                t = time.perf_counter()
                piece = next(pieces, None)
                st["file_read_s"] += time.perf_counter() - t
                if piece is None:
                    break
                with _lib.DeviceScope() as s:
                    t = time.perf_counter()
                    d = s.keep(read_files.upload_piece(piece)); sync()
                    st["upload_s"] += time.perf_counter() - t
                    del piece
                    parse(d, d.n)
    t = time.perf_counter()
    va = joined.variant_arrays()
    st["join_s"] = time.perf_counter() - t
    st["s"] = time.perf_counter() - t_all - st["device_copy_s"]
    st["text_bytes"] = n_text
    return va, st


def measure(path, chunk_bytes, reps):
    lib = _lib.load()
    t = time.perf_counter()
    want = VariantArrays.from_vcf(path)
    row = {"file_bytes": os.path.getsize(path), "variants": len(want), "host_from_vcf_s": time.perf_counter() - t,
           "host_lines_scaled_from_prefix": False}
    runs, end_to_end, same = [], [], True
    for rep in range(reps + 1):                                    # the first pass warms the pool and the code up
        got, st = staged_route(path, chunk_bytes)
        same = same and same_variants(got, want)
        t = time.perf_counter()
        got = VariantArrays.from_vcf_on_device(path, chunk_bytes=chunk_bytes)
        _lib.check(lib.gki_device_synchronize())
        dt = time.perf_counter() - t
        same = same and same_variants(got, want)
        if rep:
            runs.append(st); end_to_end.append(dt)
    m = {key: statistics.median(r[key] for r in runs) for key in runs[0]}
    parse = m["parse_count_s"] + m["parse_emit_s"]
    e2e = statistics.median(end_to_end)
    m.update({"device_end_to_end_s": e2e, "device_end_to_end_all_s": end_to_end, "parse_kernels_s": parse,
              "parse_over_device_copy": parse / m["device_copy_s"], "parse_text_bytes_per_s": m["text_bytes"] / parse,
              "device_copy_bytes_per_s": 2 * m["text_bytes"] / m["device_copy_s"], "host_over_device": row["host_from_vcf_s"] / e2e,
              "equal_to_host": same})
    stages = ("file_read_s", "upload_s", "inflate_s", "parse_kernels_s", "copy_back_s", "join_s")
    m["binding_stage"] = max(stages, key=lambda k: m[k])
    row.update(m)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=float, default=5e6)
    ap.add_argument("--multi-lines", type=float, default=2e4)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--chunk-bytes", type=int, default=read_files.DEFAULT_CHUNK_BYTES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tmp", default=None, help="directory for the files (default: the system's temporary directory)")
    args = ap.parse_args()
    _lib.load(); _lib.require_device()
    rng = np.random.default_rng(2024)
    res = {"sites": int(args.sites), "multi_lines": int(args.multi_lines), "samples": args.samples,
           "chunk_bytes": args.chunk_bytes, "reps": args.reps}
    with tempfile.TemporaryDirectory(prefix="gki_bench_vcf_parse_", dir=args.tmp) as tmp:
        for name, write in (("sites", lambda p: write_sites(p, rng, int(args.sites))),
                            ("multi", lambda p: write_multi(p, rng, int(args.multi_lines), args.samples))):
            plain = os.path.join(tmp, name + ".vcf")
            t = time.perf_counter()
            write(plain)
            res[name + "_write_s"] = time.perf_counter() - t
            paths = {"plain": plain, "gzip": os.path.join(tmp, name + "_gzip.vcf.gz"), "bgzf": os.path.join(tmp, name + "_bgzf.vcf.gz")}
            with open(plain, "rb") as fh, mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) as text:
                t = time.perf_counter()
                with gzip.open(paths["gzip"], "wb", compresslevel=6) as out:
                    out.write(text)
                res[name + "_write_gzip_s"] = time.perf_counter() - t
                t = time.perf_counter()
                bgzf.write_bgzf(paths["bgzf"], text, level=6, threads=16)
                res[name + "_write_bgzf_s"] = time.perf_counter() - t
            assert read_files.reads_file_route(paths["bgzf"]) == "bgzf-device"
            assert read_files.reads_file_route(paths["gzip"]) == "gzip-host"
            for encoding in ("plain", "gzip", "bgzf"):
                res["%s_%s" % (name, encoding)] = measure(paths[encoding], args.chunk_bytes, args.reps)
                print("done %s %s" % (name, encoding), file=sys.stderr, flush=True)
            for p in paths.values():
                os.remove(p)
    print(json.dumps(res))
    ok = True
    for name in ("sites", "multi"):
        for encoding in ("plain", "gzip", "bgzf"):
            m = res["%s_%s" % (name, encoding)]
            ok = ok and m["equal_to_host"]
            print("%s %s: %.0f MB file, %d variants; host from_vcf %.2f s; device %.3f s (%.1f x): file read %.3f, upload %.3f, "
                  "inflate %.3f, parse kernels %.4f (count %.4f + emit %.4f = %.1f x a device copy of the %.0f MB of text, "
                  "%.4f s), copy back %.3f, join %.3f s; binds: %s; equal: %s"
                  % (name, encoding, m["file_bytes"] / 1e6, m["variants"], m["host_from_vcf_s"], m["device_end_to_end_s"],
                     m["host_over_device"], m["file_read_s"], m["upload_s"], m["inflate_s"], m["parse_kernels_s"],
                     m["parse_count_s"], m["parse_emit_s"], m["parse_over_device_copy"], m["text_bytes"] / 1e6,
                     m["device_copy_s"], m["copy_back_s"], m["join_s"], m["binding_stage"], m["equal_to_host"]))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
