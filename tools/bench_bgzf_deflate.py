#!/usr/bin/env python3
"""Secondary benchmark (not the headline): text in HBM to a BGZF file, deflated on one MI355X.
  python tools/bench_bgzf_deflate.py --reads 1e7 --sites 5e6
Three texts in the shapes of the other tools' files:
  fasta, fastq   --reads reads of 150 bases from gki_simulate_reads (seed 99, 1 % substitutions, 10 % random reads) over a
                 seeded random haplotype, laid out as tools/bench_read_files.py writes them ('>r' / '@r' + ten digits,
                 constant qualities)
  vcf            the genotyped VCF of tools/bench_genotype.py's input lines (--sites lines at POS 600 i + 1), made by the
                 genotyper's own kernel from seeded calls (90 % 0/0, 7 % 0/1, 3 % 1/1; GQ 99 for four lines in five)
Per text, from ONE process, after a warm-up, --reps passes that alternate the routes, medians reported:
  deflate_kernel_ms     gki_bgzf_deflate's launches by events (deflate, scan of the sizes, pack) on the resident text
  deflate_call_s        the whole bgzf.deflate_on_device call on the resident text (allocation of the bound included)
  device_copy_ms        a device-to-device copy of the text: the byte-bound floor
  device_file_s         bgzf.write_bgzf_on_device from host bytes to a file: upload, deflate, download, write
  host_level1_file_s    bgzf.write_bgzf(level=1, threads=16) of the same bytes to a file
  host_level6_file_s    bgzf.write_bgzf(level=6, threads=16)
and the three files' sizes: the members hold the same input bytes (block_size 0xff00), so the sizes compare member for
member.  The device file is checked to inflate to the text (gzip on the host for the vcf, the inflate kernel for all).
For the vcf also genotyper.write_genotyped_vcf from a plain input file with compress "none" and "bgzf": the stage of the
genotype command that the option changes.  Prints one JSON object."""
import argparse, ctypes as C, gzip, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from graph_kmer_index_amd import _lib, bgzf
from graph_kmer_index_amd.genotyper import genotyped_lines_on_device, header_text, write_genotyped_vcf

READ_LEN = 150


def median(values):
    return round(statistics.median(values), 5)


def read_rows(letters, n_reads, fastq, rows_per_step=1_000_000):
    """The bytes tools/bench_read_files.py's write_files writes, in memory."""
    reads, out = letters.reshape(n_reads, READ_LEN), []
    for a in range(0, n_reads, rows_per_step):
        b = min(n_reads, a + rows_per_step)
        ids = np.arange(a, b, dtype=np.int64)
        digits = (ids[:, None] // 10 ** np.arange(9, -1, -1, dtype=np.int64)[None, :] % 10 + ord("0")).astype(np.uint8)
        rows = np.empty((b - a, 2 + 10 + 1 + READ_LEN + 1), dtype=np.uint8)
        rows[:, 0], rows[:, 1], rows[:, 2:12], rows[:, 12] = ord("@" if fastq else ">"), ord("r"), digits, 10
        rows[:, 13:13 + READ_LEN], rows[:, -1] = reads[a:b], 10
        if fastq:
            q = np.empty((b - a, rows.shape[1] + 2 + READ_LEN + 1), dtype=np.uint8)
            q[:, :rows.shape[1]] = rows
            q[:, rows.shape[1]], q[:, rows.shape[1] + 1] = ord("+"), 10
            q[:, rows.shape[1] + 2:-1], q[:, -1] = ord("I"), 10
            rows = q
        out.append(rows.tobytes())
    return b"".join(out)


def simulated_letters(lib, n_reads, hap_len):
    rng = np.random.default_rng(1234)
    with _lib.DeviceScope() as s:
        hap = s.on_device(rng.integers(0, 4, size=hap_len, dtype=np.uint8), np.uint8)
        letters = s.array(n_reads * READ_LEN, np.uint8)
        _lib.check(lib.gki_simulate_reads(hap.ptr, hap_len, n_reads, READ_LEN, 99, 0.01, 0.10, 0, letters.ptr))
        return letters.to_host()


def genotyped_text(n_sites):
    rng = np.random.default_rng(17)
    head = b"##fileformat=VCFv4.2\n##contig=<ID=1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
    text = head + b"".join(b"1\t%d\t.\tA\tC\t.\tPASS\t.\n" % (600 * i + 1) for i in range(n_sites))
    call = rng.choice(np.array([0, 1, 2], dtype=np.int8), size=n_sites, p=[0.90, 0.07, 0.03])
    gq = np.where(rng.random(n_sites) < 0.8, 99, rng.integers(0, 99, size=n_sites)).astype(np.uint8)
    with _lib.DeviceScope() as s:
        d_text = s.on_device(np.frombuffer(text, dtype=np.uint8), np.uint8)
        d_call, d_gq = s.on_device(call, np.int8), s.on_device(gq, np.uint8)
        out, n_out, _ = genotyped_lines_on_device(s, d_text, len(text), d_call, d_gq, 0, n_sites, 2, None)
        lines = out.to_host(n_out).tobytes()
    return text, call, gq, lines


def measure(lib, name, text, work, reps, threads):
    paths = {k: os.path.join(work, "%s.%s.gz" % (name, k)) for k in ("device", "level1", "level6")}
    rec = {"bytes": len(text), "members": -(-len(text) // 0xff00)}
    kernel, call, copy, files = [], [], [], {k: [] for k in paths}
    with _lib.DeviceScope() as s:
        d_text = s.on_device(np.frombuffer(text, dtype=np.uint8), np.uint8)
        twin = s.array(len(text), np.uint8)
        for rep in range(reps + 1):                          # the first is the warm-up
            t0 = time.perf_counter()
            out, n_out = bgzf.deflate_on_device(d_text)
            wall = time.perf_counter() - t0
            ms, cp = C.c_float(0), C.c_float(0)
            _lib.check(lib.gki_bgzf_deflate_kernel_ms(C.byref(ms)))
            _lib.check(lib.gki_measure_copy_ms(twin.ptr, d_text.ptr, len(text), C.byref(cp)))
            if rep == reps:                                  # back through the inflate kernel
                data = out.to_host(n_out)
                members, left = bgzf.scan_all(data)
                back = bgzf.inflate_on_device(data, members)
                assert left == 0 and back.checksum() == d_text.checksum()
                back.free()
                del data
            out.free()
            if rep:
                kernel.append(ms.value); call.append(wall); copy.append(cp.value)
    for rep in range(reps + 1):
        for key, run in (("device", lambda p: bgzf.write_bgzf_on_device(p, text)),
                         ("level1", lambda p: bgzf.write_bgzf(p, text, level=1, threads=threads)),
                         ("level6", lambda p: bgzf.write_bgzf(p, text, level=6, threads=threads))):
            t0 = time.perf_counter()
            run(paths[key])
            if rep:
                files[key].append(time.perf_counter() - t0)
    sizes = {k: os.path.getsize(p) for k, p in paths.items()}
    if len(text) < 1 << 29:
        assert gzip.decompress(open(paths["device"], "rb").read()) == text
    k_ms, c_ms = median(kernel), median(copy)
    rec.update({"deflate_kernel_ms": k_ms, "deflate_kernel_GBps_of_input": round(len(text) / k_ms / 1e6, 2),
                "deflate_call_s": median(call), "device_copy_ms": c_ms, "kernel_over_copy": round(k_ms / c_ms, 1),
                "device_file_s": median(files["device"]), "host_level1_file_s": median(files["level1"]),
                "host_level6_file_s": median(files["level6"]), "host_threads": threads,
                "device_file_bytes": sizes["device"], "level1_file_bytes": sizes["level1"], "level6_file_bytes": sizes["level6"],
                "device_ratio": round(sizes["device"] / len(text), 4), "level1_ratio": round(sizes["level1"] / len(text), 4),
                "level6_ratio": round(sizes["level6"] / len(text), 4),
                "device_over_level1_bytes": round(sizes["device"] / sizes["level1"], 4)})
    for p in paths.values():
        os.remove(p)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=1e7)
    ap.add_argument("--sites", type=float, default=5e6)
    ap.add_argument("--haplotype-bases", type=float, default=3e8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--texts", default="vcf,fasta,fastq")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    args = ap.parse_args()
    lib = _lib.load(); _lib.require_device()
    work = args.dir or tempfile.mkdtemp(prefix="bench_bgzf_deflate_")
    n_reads, n_sites, texts = int(args.reads), int(args.sites), args.texts.split(",")
    result = {"reads": n_reads, "sites": n_sites, "reps": args.reps, "block_size": 0xff00}
    if "vcf" in texts:
        text, call, gq, lines = genotyped_text(n_sites)
        plain = os.path.join(work, "in.vcf")
        open(plain, "wb").write(text)
        genotyped = header_text(plain) + lines
        result["vcf"] = measure(lib, "vcf", genotyped, work, args.reps, args.threads)
        print(json.dumps({"vcf": result["vcf"]}), flush=True)
        stage = {"none": [], "bgzf": []}
        for rep in range(args.reps + 1):
            for compress in ("none", "bgzf"):
                out = os.path.join(work, "out.vcf" + (".gz" if compress == "bgzf" else ""))
                t0 = time.perf_counter()
                write_genotyped_vcf(plain, out, call, gq, 2, compress=compress)
                if rep:
                    stage[compress].append(time.perf_counter() - t0)
        assert gzip.decompress(open(os.path.join(work, "out.vcf.gz"), "rb").read()) == open(os.path.join(work, "out.vcf"), "rb").read()
        result["write_genotyped_vcf"] = {"compress_none_s": median(stage["none"]), "compress_bgzf_s": median(stage["bgzf"]),
                                         "none_bytes": os.path.getsize(os.path.join(work, "out.vcf")),
                                         "bgzf_bytes": os.path.getsize(os.path.join(work, "out.vcf.gz"))}
        print(json.dumps({"write_genotyped_vcf": result["write_genotyped_vcf"]}), flush=True)
        del text, lines, genotyped
    if "fasta" in texts or "fastq" in texts:
        letters = simulated_letters(lib, n_reads, int(args.haplotype_bases))
        for name in ("fasta", "fastq"):
            if name in texts:
                text = read_rows(letters, n_reads, name == "fastq")
                result[name] = measure(lib, name, text, work, args.reps, args.threads)
                print(json.dumps({name: result[name]}), flush=True)
                del text
    print(json.dumps(result))


if __name__ == "__main__":
    main()
