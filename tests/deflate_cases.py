"""Named texts for the BGZF deflate (csrc/gki_deflate_core.h), seeded and built here: name -> (text,
block_size).  The same vectors go through the host program (test_deflate_core_cpu.py) and through the kernel
(test_gpu_bgzf_deflate.py), which must write the same bytes.  SEG is the core's segment and round size."""
import functools
import gzip
import struct
import zlib

import numpy as np

import spec_genotype

FULL = 0xff00
SEG = 256                                                  # GKI_DEF_SEG


def _rng(*key):
    return np.random.default_rng([20, 22] + list(key))


def random_bytes(n, seed=0):
    return _rng(1, n, seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def dna_wrapped(n, seed=0):
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[_rng(2, n, seed).integers(0, 4, size=n)]
    lines = [b">chr%d\n" % seed] + [letters[a:a + 60].tobytes() + b"\n" for a in range(0, n, 60)]
    return b"".join(lines)[:n]


def fastq(n, seed=0):
    rng = _rng(3, n, seed)
    out, size, i = [], 0, 0
    while size < n:
        bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=100)].tobytes()
        quals = (rng.integers(0, 12, size=100) + 58).astype(np.uint8).tobytes()
        rec = b"@read%d/1\n%s\n+\n%s\n" % (i, bases, quals)
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)[:n]


def genotyped_vcf(n, seed=0):
    """Lines as the genotyper writes them: spec_genotype.genotyped_vcf of site lines with seeded calls and qualities."""
    rng = _rng(4, n, seed)
    sites = n // 30 + 8
    pos = np.cumsum(rng.integers(1, 2000, size=sites))
    alleles = [b"A", b"C", b"G", b"T"]
    lines = [b"1\t%d\trs%d\t%s\t%s\t.\tPASS\tAF=0.%03d" % (pos[i], rng.integers(1, 10 ** 7), alleles[i % 4], alleles[(i + 1 + i // 4) % 4],
                                                          rng.integers(0, 1000)) for i in range(sites)]
    text = b"##fileformat=VCFv4.2\n##contig=<ID=1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" + b"\n".join(lines) + b"\n"
    call = rng.integers(-1, 3, size=sites).astype(np.int8)
    gq = rng.choice(np.array([0, 5, 9, 10, 42, 98, 99], dtype=np.uint8), size=sites)
    out = spec_genotype.genotyped_vcf(text, call, gq, 2, "NA12")
    assert len(out) >= n
    return out[:n]


def fibonacci_text(n=FULL):
    """Byte i occurs fib(i) times (the last one takes what is left), shuffled: an unconstrained Huffman code is deeper
    than 15 bits for it."""
    counts, a, b = [], 1, 1
    while sum(counts) + a <= n:
        counts.append(a)
        a, b = b, a + b
    counts.append(n - sum(counts))
    text = np.concatenate([np.full(c, i, dtype=np.uint8) for i, c in enumerate(counts)])
    _rng(5).shuffle(text)
    return text.tobytes()


@functools.lru_cache(maxsize=None)
def distinct_windows(n=FULL + 64):
    """n bytes over 64 letters in which every window of three bytes is distinct (the start of a de Bruijn sequence of order
    three, by the Lyndon-word construction): no match at all, yet a Huffman code saves a quarter."""
    k, order, a, seq = 64, 3, [0] * 4, []

    class Enough(Exception):
        pass

    def gen(t, p):
        if t > order:
            if order % p == 0:
                seq.extend(a[1:p + 1])
                if len(seq) >= n:
                    raise Enough
        else:
            a[t] = a[t - p]
            gen(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                gen(t + 1, t)
    try:
        gen(1, 1)
    except Enough:
        pass
    text = (np.array(seq[:n], dtype=np.uint8) + 48).tobytes()
    w = np.frombuffer(text, dtype=np.uint8).astype(np.uint32)
    assert len(text) == n and len(np.unique(w[:-2] << 16 | w[1:-1] << 8 | w[2:])) == n - 2
    return text


def repeated_windows(text, size=4):
    """{distance: windows} over the windows of `size` bytes that occurred before, each with its nearest earlier copy."""
    seen, out = {}, {}
    for p in range(len(text) - size + 1):
        w = text[p:p + size]
        if w in seen:
            out[p - seen[w]] = out.get(p - seen[w], 0) + 1
        seen[w] = p
    return out


def no_match_text():
    return distinct_windows()[:FULL]


def one_distance_text():
    """Distinct windows, then the first 300 bytes again: every repeat lies at distance 1500 exactly."""
    d = distinct_windows()[1000:]                          # away from the sequence's start of zeros, where a seam could repeat
    text = d[:1500] + d[:300]
    assert set(repeated_windows(text)) == {1500}, repeated_windows(text)
    return text


def far_repeat(distance):
    """Distinct windows whose only repeat is a run of 64 bytes `distance` behind itself."""
    d = distinct_windows()[1000:]
    text = d[:distance] + d[:64] + d[distance:distance + 32]
    assert set(repeated_windows(text)) == {distance}, repeated_windows(text)
    return text


def far_repeat_found(distance):
    """64 distinct bytes, zeros, and the 64 bytes again `distance` behind themselves.  The zeros all share one hash, so the
    most recent earlier position with the hash of a window of the 64 bytes IS its first copy (far_repeat's filler has
    long overwritten it): at 32 768 the match is taken, at 32 769 it must be refused."""
    head = distinct_windows()[1000:1064]
    return head + bytes(distance - 64) + head + b"end"


@functools.lru_cache(maxsize=None)
def vectors():
    v = {}
    for n in (0, 1, 2, 3, 4, 257, FULL):
        v["size_%d" % n] = (genotyped_vcf(n, seed=n), FULL)
    for n in (SEG - 1, SEG, SEG + 1, 2 * SEG - 1, 2 * SEG, 2 * SEG + 1, FULL - 1, FULL - SEG, FULL - SEG + 1):
        v["edge_%d" % n] = (fastq(n, seed=n), FULL)
    v["zeros"] = (bytes(FULL), FULL)
    v["ab"] = (b"ab" * (FULL // 2), FULL)
    v["random"] = (random_bytes(FULL), FULL)
    v["dist_32768"] = (far_repeat(32768), FULL)
    v["dist_32769"] = (far_repeat(32769), FULL)
    v["far_32768"] = (far_repeat_found(32768), FULL)
    v["far_32769"] = (far_repeat_found(32769), FULL)
    v["all_bytes"] = (bytes(range(256)) * 3 + dna_wrapped(3000, seed=9) + bytes(range(255, -1, -1)), FULL)
    v["fibonacci"] = (fibonacci_text(), FULL)
    v["no_match"] = (no_match_text(), FULL)
    v["one_distance"] = (one_distance_text(), FULL)
    v["dna"] = (dna_wrapped(FULL), FULL)
    v["fastq"] = (fastq(FULL), FULL)
    v["vcf"] = (genotyped_vcf(FULL), FULL)
    v["vcf_3_members"] = (genotyped_vcf(2 * FULL + 1234, seed=3), FULL)
    for m in (1, 63, 64, 65, 1025):
        for d in (-1, 0, 1):
            v["many_%d%+d" % (m, d)] = (genotyped_vcf(100 * m + d, seed=m), 100)
    return v


NAMES = sorted(vectors())


def members_of(data):
    """[(member bytes, payload, crc, isize)] of back-to-back BGZF members, by the package's own scan; nothing left over."""
    from graph_kmer_index_amd import bgzf
    found, left = bgzf.scan_all(data)
    assert left == 0
    out, at = [], 0
    for start, length, crc, isize, nxt in found:
        out.append((data[at:nxt], data[start:start + length], crc, isize))
        at = nxt
    return out


def check_members(name, data):
    """Everything a vector's compressed bytes must be, by zlib and gzip on the host."""
    from graph_kmer_index_amd import bgzf
    text, block_size = vectors()[name]
    members = members_of(data)
    assert len(members) == (len(text) + block_size - 1) // block_size, name
    at = 0
    for member, payload, crc, isize in members:
        want = text[at:at + block_size]
        assert member[:16] == bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0]), name
        assert struct.unpack_from("<H", member, 16)[0] == len(member) - 1, name
        assert zlib.decompress(payload, -15) == want, name
        assert (crc, isize) == (zlib.crc32(want), len(want)), name
        assert len(member) <= isize + 31, name
        at += len(want)
    assert at == len(text)
    assert gzip.decompress(data + bgzf.EOF_MEMBER) == text, name


def zlib_size(data, strategy, level=9):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return len(co.compress(data) + co.flush())


def write_vectors(path, names):
    """The file tests/deflate_core_main.cpp reads."""
    with open(path, "wb") as f:
        for name in names:
            text, block_size = vectors()[name]
            f.write(struct.pack("<II", len(text), block_size) + text)


def read_members(path, names):
    """{name: bytes} of the file tests/deflate_core_main.cpp writes."""
    data, out, at = open(path, "rb").read(), {}, 0
    for name in names:
        n, = struct.unpack_from("<I", data, at)
        out[name] = data[at + 4:at + 4 + n]
        at += 4 + n
    assert at == len(data)
    return out
