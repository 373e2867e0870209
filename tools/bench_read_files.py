#!/usr/bin/env python3
"""Secondary benchmark (not the headline): a reads FILE to node counts on one MI355X.
  python tools/bench_read_files.py --bases 3e9 --sites 5e6 --reads 1e7
Index and reads as in tools/bench_reads.py / bench.py's read_mapping record: the boundary records of the synthetic SNP
graph, 150-base reads from gki_simulate_reads (seed 99, 1 % substitutions, 10 % random reads).  The reads are written to a
temporary directory as a FASTA and as a FASTQ file (fixed-width names, constant qualities), and from ONE run it reports
  (a) host_lines_then_map_reads   the route that existed before: readlines / strip per line / join, exactly as
                                  ReadKmers.from_fasta_file reads its file, then CollisionFreeKmerIndex.map_reads' packing
                                  and the fused probe.  Run once (it takes seconds on the host).
  (b) map_reads_file              the device route, end to end, and the same loop with a clock around each stage: file
                                  read (the file was just written: it comes from the page cache), upload, parse count,
                                  parse emit, probe.  One warm-up pass, then --reps passes; the median is reported.
  (c) device_copy_of_file_bytes   a device-to-device copy of every piece's bytes, in the same passes: the byte-bound
                                  floor of the parse kernels.
  (d) bgzf                        the same two files written once as BGZF (bgzf.write_bgzf, level 6): compressed size, the
                                  host route (Python's gzip, which reads BGZF as multi-member gzip: what a .gz file took
                                  before the device inflate) and the device route end to end, and the device route with a
                                  clock around each stage: file read with the member scan (and, beside it, the scan alone over
                                  the same pieces), upload, inflate (the whole read_files.inflate_piece call, and the inflate
                                  kernel's own device time from gki_bgzf_inflate_kernel_ms with GB/s of its output), line
                                  cut, parse, probe.
All routes' counts are checked equal.  Prints one JSON object and a few summary lines."""
import argparse, ctypes as C, json, mmap, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from graph_kmer_index_amd import _lib, DenseKmerFinder, CriticalGraphPaths, bgzf, read_files
from graph_kmer_index_amd.flat_kmers import DeviceFlatKmers
from graph_kmer_index_amd.collision_free_kmer_index import DeviceIndex, zeroed_counts
from graph_kmer_index_amd.graph import synthetic_snp_graph, synthetic_haplotype_sequence

READ_LEN = 150


def write_files(letters, n_reads, tmp, rows_per_write=1_000_000):
    """reads.fa: '>r' + ten digits, the read; reads.fq: '@r' + ten digits, the read, '+', 150 'I'.  Returns both paths."""
    fa, fq = os.path.join(tmp, "reads.fa"), os.path.join(tmp, "reads.fq")
    reads = letters.reshape(n_reads, READ_LEN)
    with open(fa, "wb") as f_fa, open(fq, "wb") as f_fq:
        for a in range(0, n_reads, rows_per_write):
            b = min(n_reads, a + rows_per_write)
            ids = np.arange(a, b, dtype=np.int64)
            digits = (ids[:, None] // 10 ** np.arange(9, -1, -1, dtype=np.int64)[None, :] % 10 + ord("0")).astype(np.uint8)
            rows = np.empty((b - a, 2 + 10 + 1 + READ_LEN + 1), dtype=np.uint8)
            rows[:, 0], rows[:, 1], rows[:, 2:12], rows[:, 12] = ord(">"), ord("r"), digits, 10
            rows[:, 13:13 + READ_LEN], rows[:, -1] = reads[a:b], 10
            f_fa.write(rows.tobytes())
            q = np.empty((b - a, rows.shape[1] + 2 + READ_LEN + 1), dtype=np.uint8)
            q[:, :rows.shape[1]] = rows
            q[:, 0] = ord("@")
            q[:, rows.shape[1]], q[:, rows.shape[1] + 1] = ord("+"), 10
            q[:, rows.shape[1] + 2:-1], q[:, -1] = ord("I"), 10
            f_fq.write(q.tobytes())
    return fa, fq


def host_lines_then_map_reads(idx, path, k, n_nodes, max_hits):
    """The route before this one, with a clock around its two halves."""
    t = time.perf_counter()
    with open(path) as f:                                                   # ReadKmers.from_fasta_file, read_kmers.py
        lines = [l.strip() for l in f.readlines() if not l.startswith(">")]
    enc = [r.encode("ascii") for r in lines]                                # CollisionFreeKmerIndex.map_reads' packing
    read_start = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum([len(e) for e in enc], out=read_start[1:])
    letters = np.frombuffer(b"".join(enc), dtype=np.uint8)
    t_host = time.perf_counter() - t
    t = time.perf_counter()
    counts, n_kmers, n_hits = idx.count_nodes_from_reads(letters, read_start, k, n_nodes, 3, max_hits)
    _lib.check(_lib.load().gki_device_synchronize())
    t_dev = time.perf_counter() - t
    out = counts.to_host(n_nodes)
    counts.free()
    return out, {"host_lines_s": t_host, "upload_and_probe_s": t_dev, "s": t_host + t_dev, "reads": len(lines),
                 "kmers": n_kmers, "hits": n_hits}


def staged_file_route(idx, path, k, n_nodes, max_hits, chunk_bytes):
    """read_files.count_nodes_from_file's steps on the pieces of `iter_line_chunks`, with a clock around each stage, and
    the device copy of every piece."""
    lib = _lib.load()
    sync = lambda: _lib.check(lib.gki_device_synchronize())
    st = dict(file_read_s=0.0, upload_s=0.0, parse_count_s=0.0, parse_emit_s=0.0, probe_s=0.0, device_copy_s=0.0)
    code, phase, n_reads, n_bytes = None, 0, 0, 0
    t_all = time.perf_counter()
    with _lib.DeviceScope() as run, read_files.open_reads_file(path) as f:
        counts = zeroed_counts(run, n_nodes)
        pieces = read_files.iter_line_chunks(f, chunk_bytes)
        while True:
            t = time.perf_counter()
            piece = next(pieces, None)
            st["file_read_s"] += time.perf_counter() - t
            if piece is None:
                break
            if code is None:
                code = read_files.FORMATS[read_files.detect_format(piece)]
            with _lib.DeviceScope() as s:
                t = time.perf_counter()
                d = s.keep(read_files.upload_piece(piece)); sync()
                st["upload_s"] += time.perf_counter() - t
                n_bytes += d.n
                t = time.perf_counter()
                lines, reads, n_letters, bad = read_files.parse_count(d, d.n, code, phase)
                st["parse_count_s"] += time.perf_counter() - t
                assert bad == 0
                t = time.perf_counter()
                letters, read_start = map(s.keep, read_files.parse_emit(d, d.n, code, phase, reads, n_letters)); sync()
                st["parse_emit_s"] += time.perf_counter() - t
                t = time.perf_counter()
                idx.count_nodes_from_reads(letters, read_start, k, n_nodes, 3, max_hits, counts); sync()
                st["probe_s"] += time.perf_counter() - t
                letters.free(); read_start.free()
                other = s.array(d.n, np.uint8); sync()
                t = time.perf_counter()
                _lib.check(lib.gki_memcpy_d2d(other.ptr, d.ptr, d.n)); sync()
                st["device_copy_s"] += time.perf_counter() - t
            n_reads += reads
            phase = (phase + lines) % 4
        st["s"] = time.perf_counter() - t_all - st["device_copy_s"]
        st["reads"], st["file_bytes"] = n_reads, n_bytes
        return counts.to_host(n_nodes), st


def staged_bgzf_route(idx, path, k, n_nodes, max_hits, chunk_bytes):
    """read_files.bgzf_text_pieces' steps and count_nodes_from_file's with a clock around each stage.  inflate_s is the
    whole `inflate_piece` call (inflate_on_device and the copy of the tail, less than one line, to its front), line_cut_s
    the whole `cut_at_line_end` call (the search for the last line end and the copy of what follows it, less than one
    line, into the next tail)."""
    lib = _lib.load()
    sync = lambda: _lib.check(lib.gki_device_synchronize())
    st = dict(file_read_s=0.0, member_scan_s=0.0, upload_s=0.0, inflate_s=0.0, inflate_kernel_s=0.0, line_cut_s=0.0, parse_s=0.0,
              probe_s=0.0)
    code, phase, n_reads, n_out, tail = None, 0, 0, 0, None
    kernel_ms = C.c_float(0)

    def parse_and_probe(d, n):
        nonlocal phase, n_reads
        with _lib.DeviceScope() as s:
            t = time.perf_counter()
            letters, read_start, reads, lines, bad = read_files.parse_piece(d, n, code, phase); sync()
            s.keep(letters), s.keep(read_start)
            st["parse_s"] += time.perf_counter() - t
            assert bad == 0
            t = time.perf_counter()
            idx.count_nodes_from_reads(letters, read_start, k, n_nodes, 3, max_hits, counts); sync()
            st["probe_s"] += time.perf_counter() - t
        n_reads += reads
        phase = (phase + lines) % 4

    t_all = time.perf_counter()
    with _lib.DeviceScope() as run, open(path, "rb") as f:
        counts = zeroed_counts(run, n_nodes)
        pieces = read_files.iter_bgzf_pieces(f, chunk_bytes, path)
        while True:
            t = time.perf_counter()
            item = next(pieces, None)
            st["file_read_s"] += time.perf_counter() - t
            if item is None:
                break
            piece, members, base = item
            t = time.perf_counter()
            assert len(bgzf.scan_all(piece)[0]) == len(members)                # the scan again, alone: its share of file_read_s
            st["member_scan_s"] += time.perf_counter() - t
            with _lib.DeviceScope() as s:
                t = time.perf_counter()
                d = s.keep(read_files.upload_piece(piece)); sync()
                st["upload_s"] += time.perf_counter() - t
                prefix = tail.n if tail is not None else 0
                t = time.perf_counter()
                text = s.keep(read_files.inflate_piece(d, members, base, tail, path)); sync()
                st["inflate_s"] += time.perf_counter() - t
                _lib.check(lib.gki_bgzf_inflate_kernel_ms(C.byref(kernel_ms)))
                st["inflate_kernel_s"] += kernel_ms.value * 1e-3
                d.free()
                n_out += text.n - prefix
                if code is None:
                    code = read_files.FORMATS[read_files.detect_format(text.to_host(1))]
                t = time.perf_counter()
                cut, tail = read_files.cut_at_line_end(text)
                st["line_cut_s"] += time.perf_counter() - t
                if tail is not None:
                    run.keep(tail)
                if cut:
                    parse_and_probe(text, cut)
        if tail is not None:
            parse_and_probe(tail, tail.n)
        st["s"] = time.perf_counter() - t_all - st["member_scan_s"]
        st["reads"], st["inflated_bytes"] = n_reads, n_out
        return counts.to_host(n_nodes), st


def median_of(runs):
    return {key: statistics.median(r[key] for r in runs) for key in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=3e9)
    ap.add_argument("--sites", type=float, default=5e6)
    ap.add_argument("--reads", type=float, default=1e7)
    ap.add_argument("--modulo", type=int, default=452930477)
    ap.add_argument("--max-hits", type=int, default=10)
    ap.add_argument("--chunk-bytes", type=int, default=read_files.DEFAULT_CHUNK_BYTES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tmp", default=None, help="directory for the two files (default: the system's temporary directory)")
    args = ap.parse_args()
    lib = _lib.load(); _lib.require_device()
    k, n_reads, mh = 31, int(args.reads), args.max_hits
    t0 = time.perf_counter()
    g = synthetic_snp_graph(int(args.bases), int(args.sites), k=k, seed=1234)
    cp = CriticalGraphPaths.from_graph(g, k)
    f = DenseKmerFinder(g, k, critical_graph_paths=cp, only_save_one_node_per_kmer=True, max_variant_nodes=5)
    flat = f.find_flat_on_device(); f.synchronize()
    n_int = f.interior_records()
    nb = flat.n - n_int
    bnd = DeviceFlatKmers(nb, flat.hashes.view(n_int, nb), flat.nodes.view(n_int, nb), flat.ref_offsets.view(n_int, nb),
                          flat.allele_frequencies.view(n_int, nb))
    idx = DeviceIndex.build(bnd, args.modulo)
    flat.free(); f = None
    idx.probe_table()
    n_nodes = len(g.node_size)
    hap = synthetic_haplotype_sequence(g)
    d_hap = _lib.DeviceArray.from_host(hap)
    d_letters = _lib.DeviceArray(n_reads * READ_LEN, np.uint8)
    _lib.check(lib.gki_simulate_reads(d_hap.ptr, len(hap), n_reads, READ_LEN, 99, 0.01, 0.1, 0, d_letters.ptr))
    letters = d_letters.to_host()
    d_hap.free(); d_letters.free(); hap = None
    res = {"graph_bases": int(args.bases), "snp_sites": int(args.sites), "index_records": int(nb), "modulo": args.modulo,
           "max_hits": mh, "k": k, "reads": n_reads, "read_length": READ_LEN, "chunk_bytes": args.chunk_bytes,
           "setup_s": time.perf_counter() - t0}
    with tempfile.TemporaryDirectory(prefix="gki_bench_read_files_", dir=args.tmp) as tmp:
        t = time.perf_counter()
        fa, fq = write_files(letters, n_reads, tmp)
        letters = None
        res["write_files_s"] = time.perf_counter() - t
        res["fasta_bytes"], res["fastq_bytes"] = os.path.getsize(fa), os.path.getsize(fq)

        want, base = host_lines_then_map_reads(idx, fa, k, n_nodes, mh)
        base["reads_per_s"] = n_reads / base["s"]
        res["host_lines_then_map_reads"] = base
        same = {}
        for name, path in (("fasta", fa), ("fastq", fq)):
            runs, end_to_end = [], []
            for rep in range(args.reps + 1):                               # the first pass warms the pool and the code up
                got, st = staged_file_route(idx, path, k, n_nodes, mh, args.chunk_bytes)
                same[name + "_staged"] = bool(np.array_equal(got, want))
                t = time.perf_counter()
                counts, reads, _, _ = read_files.count_nodes_from_file(idx, path, k, n_nodes, 3, mh, chunk_bytes=args.chunk_bytes)
                _lib.check(lib.gki_device_synchronize())
                dt = time.perf_counter() - t
                same[name] = bool(np.array_equal(counts.to_host(n_nodes), want)) and reads == n_reads
                counts.free()
                if rep:
                    runs.append(st); end_to_end.append(dt)
            m = median_of(runs)
            parse = m["parse_count_s"] + m["parse_emit_s"]
            m.update({"end_to_end_s": statistics.median(end_to_end), "end_to_end_all_s": end_to_end,
                      "reads_per_s": n_reads / statistics.median(end_to_end), "parse_s": parse,
                      "parse_over_device_copy": parse / m["device_copy_s"], "parse_over_probe": parse / m["probe_s"],
                      "parse_bytes_per_s": m["file_bytes"] / parse, "device_copy_bytes_per_s": 2 * m["file_bytes"] / m["device_copy_s"]})
            res["map_reads_file_" + name] = m
        for name, path in (("fasta", fa), ("fastq", fq)):
            packed = path + ".gz"
            t = time.perf_counter()
            with open(path, "rb") as fh, mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) as text:
                bgzf.write_bgzf(packed, text, level=6, threads=16)
            row = {"write_bgzf_s": time.perf_counter() - t, "compressed_bytes": os.path.getsize(packed)}
            assert read_files.reads_file_route(packed) == "bgzf-device"
            runs, host, device = [], [], []
            for rep in range(args.reps + 1):                               # the same order as above: warm-up, then reps
                for route, times in (("host", host), ("device", device)):
                    t = time.perf_counter()
                    counts, reads, _, _ = read_files.count_nodes_from_file(idx, packed, k, n_nodes, 3, mh,
                                                                           chunk_bytes=args.chunk_bytes, inflate=route)
                    _lib.check(lib.gki_device_synchronize())
                    dt = time.perf_counter() - t
                    same["bgzf_%s_%s" % (name, route)] = bool(np.array_equal(counts.to_host(n_nodes), want)) and reads == n_reads
                    counts.free()
                    if rep:
                        times.append(dt)
                got, st = staged_bgzf_route(idx, packed, k, n_nodes, mh, args.chunk_bytes)
                same["bgzf_%s_staged" % name] = bool(np.array_equal(got, want))
                if rep:
                    runs.append(st)
            m = median_of(runs)
            h, d = statistics.median(host), statistics.median(device)
            m.update(row)
            m.update({"host_gzip_end_to_end_s": h, "host_gzip_all_s": host, "host_gzip_reads_per_s": n_reads / h,
                      "device_end_to_end_s": d, "device_all_s": device, "device_reads_per_s": n_reads / d,
                      "device_over_host_speedup": h / d, "inflate_output_bytes_per_s": m["inflated_bytes"] / m["inflate_kernel_s"]})
            res["bgzf_" + name] = m
        res["counts_equal"] = same
    print(json.dumps(res))
    a = res["host_lines_then_map_reads"]
    print("(a) host lines + map_reads (FASTA): %.2f s = %.3g reads/s (host %.2f s, upload + probe %.2f s)"
          % (a["s"], a["reads_per_s"], a["host_lines_s"], a["upload_and_probe_s"]))
    for name in ("fasta", "fastq"):
        m = res["map_reads_file_" + name]
        print("(b) map_reads_file (%s): %.3f s = %.3g reads/s; file read %.3f, upload %.3f, parse count %.3f, parse emit %.3f, "
              "probe %.3f s" % (name.upper(), m["end_to_end_s"], m["reads_per_s"], m["file_read_s"], m["upload_s"],
                                m["parse_count_s"], m["parse_emit_s"], m["probe_s"]))
        print("(c) device copy of the %s bytes: %.4f s; parse = %.1f x the copy, %.2f x the probe"
              % (name.upper(), m["device_copy_s"], m["parse_over_device_copy"], m["parse_over_probe"]))
    for name in ("fasta", "fastq"):
        m = res["bgzf_" + name]
        print("(d) BGZF %s: %.0f MB compressed; host gzip %.3f s = %.3g reads/s; device %.3f s = %.3g reads/s (%.2f x); file read "
              "%.3f (member scan alone %.3f), upload %.3f, inflate call %.3f (kernel %.3f = %.2f GB/s out), line cut %.3f, "
              "parse %.3f, probe %.3f s"
              % (name.upper(), m["compressed_bytes"] / 1e6, m["host_gzip_end_to_end_s"], m["host_gzip_reads_per_s"],
                 m["device_end_to_end_s"], m["device_reads_per_s"], m["device_over_host_speedup"], m["file_read_s"], m["member_scan_s"],
                 m["upload_s"], m["inflate_s"], m["inflate_kernel_s"], m["inflate_output_bytes_per_s"] / 1e9, m["line_cut_s"], m["parse_s"], m["probe_s"]))
    print("counts equal: %s" % same)
    return 0 if all(same.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
