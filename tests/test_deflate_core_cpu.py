"""csrc/gki_deflate_core.h as a host program under AddressSanitizer and UndefinedBehaviorSanitizer: every vector of
tests/deflate_cases.py is compressed by tests/deflate_core_main.cpp, which drives the core's pieces in the kernel's order,
and the members must be what zlib and gzip read back as the text.  The program has its own main and is built here with
the system's C++ compiler, or with hipcc's host side; it is never loaded into Python.

Three comparisons with zlib on the same member keep a degenerate compressor out: the codes must work (random DNA below
zlib's fixed-code output), the matches must work (VCF lines below zlib's Huffman-only output), and long overlapping
matches must work (zeros below zlib's Huffman-only output)."""
import os
import shutil
import subprocess
import zlib

import pytest

import deflate_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "deflate_core_main.cpp")
HIPCC = "/opt/rocm/bin/hipcc"
SANITIZE = "-fsanitize=address,undefined"


def _compilers():
    for name in ("c++", "g++", "clang++"):
        path = shutil.which(name)
        if path:
            yield [path, "-O1", "-g", "-std=c++17", SANITIZE, "-fno-sanitize-recover=undefined"]
    if os.path.exists(HIPCC):
        yield [HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-Xarch_host", SANITIZE]


def build_program(tmp):
    """The program's path, built by the first compiler that builds and runs an empty main with the sanitizers; None when
    there is no such compiler.  The program itself failing to build is an AssertionError."""
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    for cmd in _compilers():
        built = subprocess.run(cmd + [probe, "-o", os.path.join(tmp, "probe")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        if built.returncode == 0 and subprocess.run([os.path.join(tmp, "probe")]).returncode == 0:
            break
    else:
        return None
    out = os.path.join(tmp, "deflate_core_main")
    built = subprocess.run(cmd + [MAIN, "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert built.returncode == 0, built.stdout.decode("utf-8", "replace")[-4000:]
    return out


def run_program(program, tmp, names):
    """{name: members} of the program; the sanitizers must stay silent."""
    vectors, members = os.path.join(tmp, "vectors.bin"), os.path.join(tmp, "members.bin")
    cases.write_vectors(vectors, names)
    r = subprocess.run([program, vectors, members], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode("utf-8", "replace")[-2000:]
    return cases.read_members(members, names)


@pytest.fixture(scope="module")
def compressed(tmp_path_factory):
    """Every vector compressed once, shared and read only; the second run is the determinism check's."""
    tmp = str(tmp_path_factory.mktemp("deflate_core"))
    program = build_program(tmp)
    if program is None:
        pytest.skip("no C++ compiler here that builds and runs a program with %s" % SANITIZE)
    return run_program(program, tmp, cases.NAMES), run_program(program, tmp, cases.NAMES)


@pytest.mark.parametrize("name", cases.NAMES)
def test_members_are_bgzf_that_zlib_and_gzip_read_back(compressed, name):
    cases.check_members(name, compressed[0][name])


def test_running_twice_gives_the_same_bytes(compressed):
    assert compressed[0] == compressed[1]


def test_no_bytes_give_no_member_and_random_bytes_are_stored(compressed):
    assert compressed[0]["size_0"] == b""
    assert len(compressed[0]["random"]) == cases.FULL + 31
    (_, payload, _, _), = cases.members_of(compressed[0]["random"])
    assert payload[0] == 1                                   # BFINAL, BTYPE 0


def _payload_size(data):
    (_, payload, _, _), = cases.members_of(data)
    return len(payload)


def test_the_codes_work_random_dna_is_below_zlibs_fixed_codes(compressed):
    ours, fixed = _payload_size(compressed[0]["dna"]), cases.zlib_size(cases.vectors()["dna"][0], zlib.Z_FIXED)
    print("dna: %d bytes, zlib Z_FIXED level 9 %d" % (ours, fixed))
    assert ours < fixed


def test_the_matches_work_vcf_lines_are_below_zlibs_huffman_only(compressed):
    ours, huffman = _payload_size(compressed[0]["vcf"]), cases.zlib_size(cases.vectors()["vcf"][0], zlib.Z_HUFFMAN_ONLY)
    print("vcf: %d bytes, zlib Z_HUFFMAN_ONLY %d" % (ours, huffman))
    assert ours < huffman


def test_long_overlapping_matches_work_zeros_are_below_zlibs_huffman_only(compressed):
    ours, huffman = _payload_size(compressed[0]["zeros"]), cases.zlib_size(cases.vectors()["zeros"][0], zlib.Z_HUFFMAN_ONLY)
    print("zeros: %d bytes, zlib Z_HUFFMAN_ONLY %d" % (ours, huffman))
    assert ours < huffman


def test_the_distance_limit_a_repeat_at_32768_is_taken_and_one_at_32769_is_not(compressed):
    """far_32768 and far_32769 differ in one zero byte of filler: the copy of 64 bytes costs a few bytes as a match and
    about 48 (64 letters of six bits) as literals."""
    near, far = len(compressed[0]["far_32768"]), len(compressed[0]["far_32769"])
    print("far repeat: %d bytes at 32768, %d at 32769" % (near, far))
    assert near + 16 < far


def test_the_fibonacci_text_states_no_length_above_15(compressed):
    """An unconstrained Huffman code for fib(i) counts is one bit deeper per symbol, 21 bits here; the matches the shuffled
    text still has take literals away, so how deep the member's own code is depends on the parse (14 when this was written)
    -- test_the_length_limit_acts_on_fibonacci_counts gives the construction the counts themselves."""
    text = cases.vectors()["fibonacci"][0]
    counts = sorted(text.count(bytes([b])) for b in set(text))
    assert len(counts) >= 20 and counts[:3] == [1, 1, 2]
    (_, payload, _, _), = cases.members_of(compressed[0]["fibonacci"])
    assert payload[0] & 7 == 5                               # BFINAL, BTYPE 2: the dynamic block was the smaller one
    assert 12 <= max(_literal_lengths(payload)) <= 15


def _code(program, max_bits, counts):
    r = subprocess.run([program, "code", str(max_bits)] + [str(c) for c in counts], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode("utf-8", "replace")[-2000:]
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.decode().split("\n")[:-1]]
    assert len(rows) == len(counts)
    return [a for a, _ in rows], [b for _, b in rows]


def _huffman_cost(counts):
    """The bits of an unconstrained Huffman code: the sum of the merged weights."""
    import heapq
    heap, cost = [c for c in counts if c], 0
    heapq.heapify(heap)
    while len(heap) > 1:
        a = heapq.heappop(heap) + heapq.heappop(heap)
        cost += a
        heapq.heappush(heap, a)
    return cost


def test_the_length_limit_acts_on_fibonacci_counts(tmp_path):
    program = build_program(str(tmp_path))
    if program is None:
        pytest.skip("no C++ compiler here that builds and runs a program with %s" % SANITIZE)
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    rng = __import__("numpy").random.default_rng(7)
    tried = [(15, fib[:30]), (15, fib[:16]), (15, [0, 5, 0, 0, 9]), (7, fib[:19]), (7, [1] * 19), (15, [1] * 286),
             (15, fib[:16] + [3] * 270), (15, [int(x) for x in rng.integers(0, 50, size=286)]), (7, [0, 1, 0, 1] + [0] * 15),
             (15, [int(x) for x in rng.integers(0, 60000, size=30)])]
    for max_bits, counts in tried:
        lengths, codes = _code(program, max_bits, counts)
        used = [s for s, c in enumerate(counts) if c]
        assert all((lengths[s] > 0) == (counts[s] > 0) for s in range(len(counts)))
        assert max(lengths) <= max_bits
        assert sum(2 ** (max_bits - lengths[s]) for s in used) == 2 ** max_bits          # complete: Kraft's sum is one
        for a in used:                                       # no symbol has a longer code than a rarer one
            for b in used:
                assert not (counts[a] > counts[b] and lengths[a] > lengths[b]), (max_bits, counts, a, b)
        # prefix-free, as the emitter writes them: the low bit first
        words = sorted(format(codes[s], "0%db" % lengths[s])[::-1] for s in used)
        assert all(not b.startswith(a) for a, b in zip(words, words[1:]))
        cost, best = sum(counts[s] * lengths[s] for s in used), _huffman_cost(counts)
        assert cost >= best
        if counts in (fib[:16], [1] * 19, [1] * 286) or len(used) == 2:
            assert cost == best, (max_bits, counts)          # the limit is not reached (fib[:16] is 15 deep): a Huffman code
    assert max(_code(program, 15, fib[:30])[0]) == 15 and max(_code(program, 7, fib[:19])[0]) == 7


def test_a_text_with_no_match_has_a_header_of_two_unused_distance_codes(compressed):
    (_, payload, _, _), = cases.members_of(compressed[0]["no_match"])
    assert payload[0] & 7 == 5
    assert payload[1] & 31 == 1                              # HDIST - 1: two codes, what zlib's own deflate writes
    assert _literal_lengths(payload)[257:] == []             # and no length symbol


def _literal_lengths(payload):
    """The literal/length code lengths a dynamic block's header states (RFC 1951, 3.2.7), read here bit by bit."""
    bits = int.from_bytes(payload[:700], "little")
    at = [3]

    def take(n):
        v = bits >> at[0] & ((1 << n) - 1)
        at[0] += n
        return v
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl = [0] * 19
    for k in range(hclen):
        cl[order[k]] = take(3)
    codes, code = {}, 0                                      # (length, code read first bit first) -> symbol
    for length in range(1, 8):
        for sym in range(19):
            if cl[sym] == length:
                codes[(length, code)] = sym
                code += 1
        code <<= 1
    lengths = []
    while len(lengths) < hlit + hdist:
        length, code = 0, 0
        while (length, code) not in codes or length == 0:
            code = code << 1 | take(1)
            length += 1
            assert length <= 7
        sym = codes[(length, code)]
        if sym < 16:
            lengths.append(sym)
        elif sym == 16:
            lengths += [lengths[-1]] * (3 + take(2))
        else:
            lengths += [0] * (3 + take(3) if sym == 17 else 11 + take(7))
    assert len(lengths) == hlit + hdist
    return lengths[:hlit]
