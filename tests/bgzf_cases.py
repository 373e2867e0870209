"""BGZF test vectors for tests/test_bgzf_host.py, test_inflate_core_cpu.py and test_gpu_bgzf.py: gzip members made with
zlib's raw deflate (zlib.compressobj(level, DEFLATED, -15, 9, strategy)), a few made by hand with a small bit writer for
the streams zlib never emits, and malformed ones with the status csrc/gki_inflate_core.h must give.  Ground truth is the
data that was compressed; test_bgzf_host.py also reads every good file back with Python's gzip.

A vector is a list of members (payload, crc32, isize, data, extra): `data` is what the payload inflates to (None for a
malformed one), `extra` further extra-field bytes in front of the 'BC' subfield."""
import random
import struct
import zlib

# csrc/gki_inflate_core.h
OK, INPUT_END, BLOCK_TYPE, STORED_LEN, CODE_LENGTHS, REPEAT_FIRST, LITLEN_SYMBOL, DIST_SYMBOL, DISTANCE = range(9)
OUTPUT_OVERFLOW, OUTPUT_SHORT, TRAILING_INPUT, CRC, INVALID_CODE = range(9, 14)

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(data) + co.flush()


def member(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, extra=b"", payload=None):
    payload = deflate(data, level, strategy) if payload is None else payload
    return (payload, zlib.crc32(data), len(data), data, extra)


def member_bytes(m):
    """The gzip member of BGZF: header with FEXTRA, `extra` then the 'BC' subfield holding the member's size - 1."""
    payload, crc, isize, _, extra = m
    xlen = len(extra) + 6
    total = 12 + xlen + len(payload) + 8
    assert total <= 65536
    return (struct.pack("<BBBBIBBH", 31, 139, 8, 4, 0, 0, 255, xlen) + extra + struct.pack("<BBHH", 66, 67, 2, total - 1)
            + payload + struct.pack("<II", crc, isize))


def file_bytes(members):
    return b"".join(member_bytes(m) for m in members)


def fasta_text(n_bytes, seed=1, width=60):
    rng = random.Random(seed)
    out, i = bytearray(), 0
    while len(out) < n_bytes:
        out += b">read_%d\n" % i
        out += bytes(rng.choices(b"ACGT", k=width)) + b"\n"
        i += 1
    return bytes(out[:n_bytes])


def fastq_text(n_records, seed=2, width=50):
    rng = random.Random(seed)
    out = bytearray()
    for i in range(n_records):
        seq = bytes(rng.choices(b"ACGTN", k=width))
        qual = bytes(rng.choices(b"IIIIIIFF:,#", k=width))
        out += b"@r%d\n" % i + seq + b"\n+\n" + qual + b"\n"
    return bytes(out)


def random_bytes(n, seed):
    return random.Random(seed).randbytes(n)


# ------------------------------------------------------------------ a bit writer, for the streams made by hand
class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, n):
        """n bits of a number, least significant first (header fields, extra bits)"""
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """a Huffman code of n bits, most significant first"""
        for i in range(n - 1, -1, -1):
            self.put(code >> i & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def position(self):
        """the number of bits written so far"""
        return len(self.out) * 8 + self.n

    def bytes(self):
        self.align()
        return bytes(self.out)


def fixed_litlen(w, sym):
    if sym < 144:
        w.code(0x30 + sym, 8)
    elif sym < 256:
        w.code(0x190 + sym - 144, 9)
    elif sym < 280:
        w.code(sym - 256, 7)
    else:
        w.code(0xC0 + sym - 280, 8)


def canonical(lengths):
    """symbol -> (code, bits) of the canonical Huffman code with these lengths (RFC 1951 3.2.2)"""
    code, out = 0, {}
    for bits in range(1, 16):
        for sym, n in enumerate(lengths):
            if n == bits:
                out[sym] = (code, bits)
                code += 1
        code <<= 1
    return out


CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# a complete code-length code in which the lengths 0..13 and the repeat codes 16, 17 all have a code
CL_PLAIN = [4] * 14 + [5, 5, 5, 5, 0]


def dynamic_header(w, final, n_litlen, n_dist, cl_lengths, ops):
    """BFINAL, BTYPE 2, the counts, the code-length code, then `ops`: (code-length symbol, extra value) in order"""
    w.put(final, 1)
    w.put(2, 2)
    w.put(n_litlen - 257, 5)
    w.put(n_dist - 1, 5)
    w.put(19 - 4, 4)
    for sym in CL_ORDER:
        w.put(cl_lengths[sym], 3)
    codes = canonical(cl_lengths)
    for sym, extra in ops:
        w.code(*codes[sym])
        if sym >= 16:
            w.put(extra, {16: 2, 17: 3, 18: 7}[sym])


def stored_then_far_match():
    """A stored block of 32 768 bytes, then a fixed block with one match of length 258 at distance exactly 32 768."""
    data = random_bytes(32768, 11)
    w = Bits()
    w.put(0, 1); w.put(0, 2); w.align()
    w.raw(struct.pack("<HH", 32768, 32768 ^ 0xFFFF) + data)
    w.put(1, 1); w.put(1, 2)
    fixed_litlen(w, 285)                      # length 258, no extra bits
    w.code(29, 5); w.put(32768 - 24577, 13)   # distance symbol 29: 24 577 + 13 extra bits
    fixed_litlen(w, 256)
    return member(data + data[:258], payload=w.bytes())


def one_distance_code():
    """A dynamic block whose distance tree has one code (of one bit: incomplete, and accepted as zlib accepts it):
    literal 'A', then length 3 at distance 1 five times, then end of block."""
    litlen = [0] * 258
    litlen[65], litlen[256], litlen[257] = 1, 2, 2
    w = Bits()
    dynamic_header(w, 1, 258, 1, CL_PLAIN, [(n, 0) for n in litlen] + [(1, 0)])
    ll = canonical(litlen)
    w.code(*ll[65])
    for _ in range(5):
        w.code(*ll[257])
        w.code(0, 1)
    w.code(*ll[256])
    return member(b"A" * 16, payload=w.bytes())


def _flushed():
    a, b, c = fasta_text(3000, 5), fasta_text(2000, 6), fasta_text(1000, 7)
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    payload = co.compress(a) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(b) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(c) + co.flush()
    return member(a + b + c, payload=payload)


EMPTY = (EOF_MEMBER[18:20], 0, 0, b"", b"")
assert member_bytes(EMPTY) == EOF_MEMBER

GOOD = {
    "stored": [member(fasta_text(5000, 3), level=0)],
    "fixed": [member(fasta_text(1000, 4), strategy=zlib.Z_FIXED)],
    "dynamic": [member(fasta_text(60000, 8), level=9)],
    "fastq": [member(fastq_text(300), level=6)],
    "run": [member(b"A" * 65536, level=6)],
    "far": [member(random_bytes(32000, 9) * 2, level=6)],
    "flushed": [_flushed()],
    "empty": [member(b">a\nAC", level=6), EMPTY, member(b"GT\n", level=6), EMPTY],
    "one_byte": [member(b"A", level=6)],
    "max_in": [member(random_bytes(0xff00, 10), level=6)],
    "extra_first": [member(fasta_text(500, 12), extra=struct.pack("<BBH", 88, 89, 3) + b"xyz")],
    "odd_starts": [member(fasta_text(n, 20 + n), level=1 + n % 9) for n in (1, 2, 3, 5, 7, 11, 13, 17, 19, 23)],
    "stored_then_far_match": [stored_then_far_match()],
    "one_distance_code": [one_distance_code()],
}


# ------------------------------------------------------------------ malformed: (member, expected status)
def _bad(payload, data_len, crc=0):
    return (payload, crc, data_len, None, b"")


def _malformed():
    out = {}
    # One flipped bit in a dynamic payload, made by hand so that its bytes do not depend on the zlib build: codes A 00,
    # C 01, G 10, T 110, end of block 111 and no distance code.  The low bit of the first literal's code is flipped, which
    # makes the 'A' a 'C': the stream is still well formed and of the right length, and only the CRC-32 tells.
    letters = b"ACGTACGGTTCA"
    litlen = [0] * 257
    litlen[65], litlen[67], litlen[71], litlen[84], litlen[256] = 2, 2, 2, 3, 3
    w = Bits()
    dynamic_header(w, 1, 257, 1, CL_PLAIN, [(n, 0) for n in litlen] + [(0, 0)])
    first_literal = w.position()
    codes = canonical(litlen)
    for c in letters:
        w.code(*codes[c])
    w.code(*codes[256])
    whole = w.bytes()
    assert zlib.decompress(whole, -15) == letters and codes[65] == (0, 2) and codes[67] == (1, 2)
    flipped = bytearray(whole)
    flipped[(first_literal + 1) >> 3] ^= 1 << ((first_literal + 1) & 7)
    assert zlib.decompress(bytes(flipped), -15) == b"C" + letters[1:]
    out["flipped_bit"] = ((bytes(flipped), zlib.crc32(letters), len(letters), None, b""), CRC)
    # the block of one_distance_code with the first distance bit 1: the set's only code is 0.  Two more bytes follow, as
    # the canonical-code walk looks at up to 15 bits before it knows that they are no code (fewer would be "input ended")
    litlen = [0] * 258
    litlen[65], litlen[256], litlen[257] = 1, 2, 2
    w = Bits()
    dynamic_header(w, 1, 258, 1, CL_PLAIN, [(n, 0) for n in litlen] + [(1, 0)])
    codes = canonical(litlen)
    w.code(*codes[65]); w.code(*codes[257]); w.code(1, 1); w.code(*codes[256]); w.put(0, 16)
    out["no_such_distance_code"] = (_bad(w.bytes(), 4), INVALID_CODE)
    text = fasta_text(60000, 8)
    good = deflate(text, 9)
    out["cut_payload"] = ((good[:len(good) // 2], zlib.crc32(text), len(text), None, b""), INPUT_END)
    w = Bits(); w.put(1, 1); w.put(0, 2); w.align(); w.raw(struct.pack("<HH", 4, 4) + b"ACGT")
    out["stored_len_mismatch"] = (_bad(w.bytes(), 4, zlib.crc32(b"ACGT")), STORED_LEN)
    w = Bits(); w.put(1, 1); w.put(3, 2)
    out["btype_3"] = (_bad(w.bytes(), 4), BLOCK_TYPE)
    w = Bits(); w.put(1, 1); w.put(1, 2); fixed_litlen(w, 65); fixed_litlen(w, 257); w.code(1, 5); fixed_litlen(w, 256)
    out["far_distance"] = (_bad(w.bytes(), 4), DISTANCE)              # length 3 at distance 2 behind one byte
    w = Bits(); w.put(1, 1); w.put(1, 2); fixed_litlen(w, 65); fixed_litlen(w, 286); fixed_litlen(w, 256)
    out["symbol_286"] = (_bad(w.bytes(), 4), LITLEN_SYMBOL)
    w = Bits(); w.put(1, 1); w.put(1, 2); fixed_litlen(w, 65); fixed_litlen(w, 257); w.code(30, 5); fixed_litlen(w, 256)
    out["distance_symbol_30"] = (_bad(w.bytes(), 4), DIST_SYMBOL)
    w = Bits(); dynamic_header(w, 1, 257, 1, [1, 1, 1] + [0] * 16, [])   # three codes of one bit
    out["oversubscribed"] = (_bad(w.bytes(), 4), CODE_LENGTHS)
    w = Bits(); dynamic_header(w, 1, 257, 1, CL_PLAIN, [(16, 0)])
    out["repeat_first"] = (_bad(w.bytes(), 4), REPEAT_FIRST)
    small = fasta_text(1000, 4)
    out["wrong_crc"] = ((deflate(small), zlib.crc32(small) ^ 1, len(small), None, b""), CRC)
    out["isize_too_small"] = ((deflate(small), zlib.crc32(small), len(small) - 1, None, b""), OUTPUT_OVERFLOW)
    out["isize_too_large"] = ((deflate(small), zlib.crc32(small), len(small) + 1, None, b""), OUTPUT_SHORT)
    out["trailing_bytes"] = ((deflate(small) + b"\0", zlib.crc32(small), len(small), None, b""), TRAILING_INPUT)
    return out


MALFORMED = _malformed()
GPU_MALFORMED = ("flipped_bit", "cut_payload", "wrong_crc", "far_distance", "isize_too_small")


def fuzz_cases(n=2000, seed=1234):
    """(payload, crc, isize) of n corruptions of the good vectors' members: one bit flipped, one byte replaced, or the
    payload cut."""
    rng = random.Random(seed)
    base = [m for name in sorted(GOOD) for m in GOOD[name] if len(m[0]) > 2]
    for i in range(n):
        payload, crc, isize, _, _ = base[i % len(base)]
        p = bytearray(payload)
        kind = rng.randrange(3)
        if kind == 0:
            at = rng.randrange(len(p) * 8)
            p[at >> 3] ^= 1 << (at & 7)
        elif kind == 1:
            p[rng.randrange(len(p))] = rng.randrange(256)
        else:
            del p[rng.randrange(len(p)):]
        yield bytes(p), crc, isize


def mixed_members(n, seed):
    """n members of mixed sizes from 0 to 65 280 bytes: mostly short FASTA text, every seventh empty, every 64th full."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        if i % 7 == 3:
            out.append(EMPTY)
        elif i % 64 == 5:
            out.append(member(fasta_text(0xff00, seed + i), level=1))
        else:
            out.append(member(fasta_text(rng.randrange(1, 400), seed + i), level=rng.choice((0, 1, 6, 9))))
    return out
