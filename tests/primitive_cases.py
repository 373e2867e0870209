"""Case builders and NumPy references for the device primitives every feature shares: the exclusive scans, the stable
compaction, the column checksum and the last-byte search (csrc/gki_runtime.hip, csrc/gki_inflate.hip).  No device here:
tests/test_primitive_cases_host.py checks this file on the CPU, tests/test_gpu_runtime_primitives.py runs the cases.

The constants are copied from the sources named beside them; SOURCE_LINES lists where each one stands, and the host test
reads those lines, so a retuned kernel shows which shape has to move."""
import functools

import numpy as np

SB = 256                     # csrc/gki_runtime.hip:274 threads per block of the scans
SI = 8                       # csrc/gki_runtime.hip:275 items per thread: the unit of load_items' two 16-byte loads
STILE = 2048                 # csrc/gki_runtime.hip:276 SB * SI items per block: one scan level per factor of STILE
GRID_BLOCKS = 256 * 8        # csrc/gki_common.h:69 stream_grid launches at most this many blocks ...
GRID_THREADS = GRID_BLOCKS * 256   # ... of 256 threads = 524 288: more items take a second grid-stride trip
FIRST_WINDOW = 1 << 20       # csrc/gki_inflate.hip:152 gki_last_byte_position searches the last MiB first
WINDOW_GROWTH = 4            # csrc/gki_inflate.hip:162 and then windows four times the last
PACK_BASES = 16              # csrc/gki_graph.hip:21 k_pack_2bit: bases per lane, one 16-byte load when aligned

# (file, line, what the line has to say)
SOURCE_LINES = (
    ("graph_kmer_index_amd/csrc/gki_runtime.hip", 274, r"constexpr int SB = %d;" % SB),
    ("graph_kmer_index_amd/csrc/gki_runtime.hip", 275, r"constexpr int SI = %d;" % SI),
    ("graph_kmer_index_amd/csrc/gki_runtime.hip", 276, r"constexpr int STILE = SB \* SI;"),
    ("graph_kmer_index_amd/csrc/gki_runtime.hip", 393, r"while \(n > STILE\)"),
    ("graph_kmer_index_amd/csrc/gki_runtime.hip", 395, r"total \+= 8 \* \(2 \* nb \+ 1\);"),
    ("graph_kmer_index_amd/csrc/gki_runtime.hip", 398, r"return total \+ 64;"),
    ("graph_kmer_index_amd/csrc/gki_common.h", 69, r"if \(g > 256 \* 8\) g = 256 \* 8;"),
    ("graph_kmer_index_amd/csrc/gki_inflate.hip", 152, r"window = 1 << 20;"),
    ("graph_kmer_index_amd/csrc/gki_inflate.hip", 162, r"window \*= %d;" % WINDOW_GROWTH),
    ("graph_kmer_index_amd/csrc/gki_graph.hip", 21, r"int64_t b = i \* %d;" % PACK_BASES),
)

U32_MAX = 0xFFFFFFFF
GUARD = 16                   # slots kept behind every input and output, which no primitive may read into a result or write


# ------------------------------------------------------------------ scans
def scan_tmp_bytes(n):
    """gki_scan_tmp_bytes (csrc/gki_runtime.hip:391-399) restated."""
    total = 0
    while n > STILE:
        n = -(-n // STILE)
        total += 8 * (2 * n + 1)
    return total + 64


def scan_levels(n):
    """Block-scan levels of an n-item scan: one, plus one per round of the loop above."""
    levels = 1
    while n > STILE:
        n = -(-n // STILE)
        levels += 1
    return levels


SCAN_NS = (0, 1, 7, 8, 9, 2047, 2048, 2049, 4095, 4096, 4097,
           STILE ** 2 - 1, STILE ** 2, STILE ** 2 + 1, STILE ** 2 + STILE + 1)
SCAN_ALIGN_NS = (2 * STILE + 1, STILE ** 2 + 1)
SCAN_IN_OFFSETS = (0, 1, 2, 3)       # elements of 4 bytes: only 0 is 16-byte aligned
SCAN_OUT_OFFSETS = (0, 1)            # int64 output at element 1 is 8 mod 16: the scalar stores
SCAN_KINDS = {0: (np.uint32, np.int64), 1: (np.int32, np.int64), 2: (np.uint32, np.uint32)}

# value patterns per kind; (name, the only n it runs at or None)
SCAN_VALUES = {
    0: (("random", None), ("zeros", None), ("all_ones", 2 * STILE + 1), ("last_only", None)),
    1: (("random", None), ("walk", None)),
    2: (("below_wrap", None), ("exactly_u32_max", None)),
}


def scan_cases():
    """(kind, n, values name) of every scan case."""
    out = []
    for kind, patterns in SCAN_VALUES.items():
        for n in SCAN_NS:
            for name, only_n in patterns:
                if only_n is not None and n != only_n:
                    continue
                if name == "exactly_u32_max" and n == 0:
                    continue
                out.append((kind, n, name))
    return out


_NAME_SEED = {"random": 1, "zeros": 2, "all_ones": 3, "last_only": 4, "walk": 5, "below_wrap": 6, "exactly_u32_max": 7}


def scan_values(kind, n, name, seed=0):
    """The n input items of a case, in the kind's input type."""
    rng = np.random.default_rng([kind, n, _NAME_SEED[name], seed])
    dtype = SCAN_KINDS[kind][0]
    if name == "zeros":
        return np.zeros(n, dtype)
    if name == "all_ones":
        return np.full(n, U32_MAX, dtype)
    if name == "last_only":
        v = np.zeros(n, dtype)
        if n:
            v[-1] = 0x89ABCDEF
        return v
    if name == "walk":                                   # +-1 steps: depths of the critical-path walk
        return (rng.integers(0, 2, size=n, dtype=np.int32) * 2 - 1).astype(dtype)
    if name == "random" and kind == 0:                   # full range: the running total passes 2^32 within a few items
        return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(dtype)
    if name == "random" and kind == 1:
        v = rng.integers(-(1 << 31), 1 << 31, size=n, dtype=np.int64).astype(dtype)
        if n >= 4:                                       # both extremes, next to each other and at the end
            v[n // 2], v[n // 2 + 1], v[-1] = np.iinfo(np.int32).min, np.iinfo(np.int32).max, np.iinfo(np.int32).min
        return v
    if name in ("below_wrap", "exactly_u32_max"):        # kind 2 accumulates modulo 2^32: the wrap is not pinned
        v = rng.integers(0, U32_MAX // max(n, 1) + 1, size=n, dtype=np.uint64)
        if name == "exactly_u32_max":
            at = int(rng.integers(0, n))
            v[at] += np.uint64(U32_MAX) - v.sum(dtype=np.uint64)
        assert int(v.sum(dtype=np.uint64)) <= U32_MAX and (n == 0 or int(v.max()) <= U32_MAX)
        return v.astype(dtype)
    raise KeyError((kind, name))


def scan_ref(kind, values):
    """out[i] = sum of values[:i] for i = 0..n, in int64, then in the kind's output type."""
    out = np.zeros(len(values) + 1, np.int64)
    np.cumsum(values, dtype=np.int64, out=out[1:])
    return out.astype(SCAN_KINDS[kind][1])


def in_guarded(values, offset, fill):
    """values at [offset, offset + n) of a buffer that is `fill` everywhere else, GUARD slots behind included."""
    buf = np.full(offset + len(values) + GUARD, fill, dtype=values.dtype)
    buf[offset:offset + len(values)] = values
    return buf


def scan_sentinel(kind):
    return np.array(0x5A5A5A5A5A5A5A5A if kind < 2 else 0xA5A5A5A5).astype(SCAN_KINDS[kind][1])


# the same scan behind gki_hash_reads(.., d_out NULL): out_start = scan of max(len - k + 1, 0)
def read_counts_ref(read_start, k):
    n = np.diff(np.asarray(read_start, np.int64)) - k + 1
    return np.maximum(n, 0)


def many_short_reads(n_reads, seed=0):
    """read_start of n_reads reads of 0..40 letters (built on the host only: count-only mode reads no letters)."""
    rng = np.random.default_rng([n_reads, seed])
    start = np.zeros(n_reads + 1, np.int64)
    np.cumsum(rng.integers(0, 41, size=n_reads), out=start[1:])
    return start


K_READS = 31
# name -> (read_start, accepted): refused where a read's k-mer count does not fit 32 bits
HUGE_READS = {
    "three_of_2^31": ([0, 1 << 31, 2 << 31, 3 << 31], True),
    "largest_accepted": ([0, (1 << 32) + K_READS - 2], True),                 # 2^32 - 1 k-mers
    "largest_accepted_after_others": ([0, 5, 40, 40 + (1 << 32) + K_READS - 2, 45 + (1 << 32) + K_READS - 2], True),
    "refused_2^32_k-mers": ([0, (1 << 32) + 30], False),                      # was counted as 0
    "refused_2^32+5_k-mers": ([0, (1 << 32) + 35], False),                    # was counted as 5
    "refused_among_others": ([0, 100, 100 + (1 << 33), 200 + (1 << 33)], False),
}


# ------------------------------------------------------------------ compaction
COMPACT_NS = (1, 2047, 2048, 2049, GRID_THREADS - 1, GRID_THREADS, GRID_THREADS + 1, STILE ** 2 + 1)
COMPACT_FLAGS = ("none", "all", "first", "last", "every_other", "random_1pct", "random_99pct")
SET_BYTES = np.array([1, 2, 255], np.uint8)          # every non-zero byte keeps its record
COLUMN_SENTINELS = (np.uint64(0xDEADBEEFDEADBEEF), np.uint32(0xDEADBEEF), np.uint64(0xFEEDFACEFEEDFACE), np.float32(-7.5))


def compact_flags(n, name):
    """uint8[n]: 0 or, where set, one of SET_BYTES by position."""
    rng = np.random.default_rng([n, COMPACT_FLAGS.index(name)])
    keep = np.zeros(n, bool)
    if name == "all":
        keep[:] = True
    elif name == "first":
        keep[0] = True
    elif name == "last":
        keep[-1] = True
    elif name == "every_other":
        keep[::2] = True
    elif name == "random_1pct":
        keep = rng.random(n) < 0.01
    elif name == "random_99pct":
        keep = rng.random(n) < 0.99
    elif name != "none":
        raise KeyError(name)
    return np.where(keep, SET_BYTES[np.arange(n) % 3], 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def flat_columns(n):
    """(hashes, nodes, ref_offsets, allele_frequencies) with every value distinct within its column and the columns
    unlike each other, so that a record moved, or a column taken for another, shows."""
    i = np.arange(n, dtype=np.uint64)
    hashes = i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)           # odd multiplier: a bijection mod 2^64
    nodes = (i * np.uint64(2654435761) + np.uint64(7)).astype(np.uint32)  # odd multiplier: distinct mod 2^32 for n <= 2^32
    refs = (np.uint64(1) << np.uint64(40)) + i * np.uint64(3)
    af = (i.astype(np.uint32) + np.uint32(0x3F000000)).view(np.float32)  # distinct bit patterns of finite floats
    return hashes, nodes, refs, af


def compact_ref(flags, columns):
    keep = flags != 0
    return tuple(c[keep] for c in columns)


# ------------------------------------------------------------------ checksum
CHECKSUM_NS = (0, 1, 63, 64, 65, 255, 256, 257, GRID_THREADS - 1, GRID_THREADS, GRID_THREADS + 1, 2 * GRID_THREADS + 1)
CHECKSUM_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
CHECKSUM_OFFSETS = (0, 1, 3)


def checksum_values(elem_bytes, n, seed=0):
    """n + 3 + GUARD random elements of the whole range (views of n elements start at 0, 1 and 3; what lies behind a view
    is garbage that must not count).  The extremes of the width are in every view."""
    dtype = CHECKSUM_DTYPES[elem_bytes]
    rng = np.random.default_rng([elem_bytes, n, seed])
    v = rng.integers(0, 1 << (8 * elem_bytes), size=n + 3 + GUARD, dtype=np.uint64, endpoint=False) \
        if elem_bytes < 8 else rng.integers(0, 1 << 64, size=n + 3 + GUARD, dtype=np.uint64, endpoint=False)
    v = v.astype(dtype)
    top = np.iinfo(dtype).max
    if n >= 8:
        v[3], v[4] = top, top // 2 + 1                   # all ones, and the top bit alone
    return v


def checksum_ref(a):
    """(sum mod 2^64, xor) of the zero-extended elements, as Python ints."""
    a = np.asarray(a)
    assert a.dtype in (np.uint8, np.uint16, np.uint32, np.uint64)
    if a.size == 0:
        return 0, 0
    return int(np.add.reduce(a, dtype=np.uint64)), int(np.bitwise_xor.reduce(a.astype(np.uint64)))


# ------------------------------------------------------------------ last byte
SEARCH_NS = (0, 1, FIRST_WINDOW - 1, FIRST_WINDOW, FIRST_WINDOW + 1, (1 + WINDOW_GROWTH) * FIRST_WINDOW + 3)
SEARCH_VALUES = (0, 10, 255)
_BACKGROUND = np.array([b for b in range(256) if b not in SEARCH_VALUES], np.uint8)


def search_background(n, seed=0):
    """n bytes that hold none of SEARCH_VALUES."""
    return _BACKGROUND[np.random.default_rng([n, seed]).integers(0, len(_BACKGROUND), size=n)]


def search_windows(n):
    """[begin, end) of the windows gki_last_byte_position looks at, last first."""
    out, end, window = [], n, FIRST_WINDOW
    while end > 0:
        begin = max(end - window, 0)
        out.append((begin, end))
        end, window = begin, window * WINDOW_GROWTH
    return out


def search_placements(n):
    """name -> positions that hold the byte, for a buffer of n bytes; every position is inside it."""
    out = {"absent": ()}
    if n == 0:
        return out
    out["at_0"] = (0,)
    out["at_n-1"] = (n - 1,)
    out["at_both_ends"] = (0, n - 1)
    seam = n - FIRST_WINDOW                               # the first byte of the first window
    for name, p in (("seam-1", seam - 1), ("seam", seam), ("seam+1", seam + 1)):
        if 0 <= p < n:
            out[name] = (p,)
    windows = search_windows(n)
    if len(windows) >= 2:                                 # several in the second window, none in the first
        b, e = windows[1]
        out["several_in_second_window"] = tuple(sorted({b, (b + e) // 2, e - 1}))
    if len(windows) >= 3:                                 # only in the third
        b, e = windows[2]
        out["several_in_third_window"] = tuple(sorted({b, e - 1}))
        out["third_and_second_window"] = (b, windows[1][0])
    return out


def search_ref(buf, value):
    at = np.flatnonzero(np.asarray(buf) == value)
    return int(at[-1]) if len(at) else -1


def long_last_line_fasta(n_short=300, long_letters=1_200_000, seed=0):
    """FASTA text: short reads, then one read of `long_letters` letters on a single line -- streamed in small pieces, the
    unfinished line carried on the device outgrows the first search window."""
    rng = np.random.default_rng([n_short, long_letters, seed])
    letters = np.frombuffer(b"ACGT", np.uint8)
    parts = []
    for i in range(n_short):
        parts.append(b">s%d\n" % i + letters[rng.integers(0, 4, size=int(rng.integers(1, 120)))].tobytes() + b"\n")
    parts.append(b">long\n" + letters[rng.integers(0, 4, size=long_letters)].tobytes() + b"\n")
    return b"".join(parts)


# ------------------------------------------------------------------ hash helpers past one grid
COMPLEMENT_NS = (GRID_THREADS + 1, 2 * GRID_THREADS + 1)
COMPLEMENT_KS = (1, 31)
HASH_K = 31
HASH_SEQUENCE_BASE = PACK_BASES * GRID_THREADS           # 8 388 608 bases: one full grid of k_pack_2bit lanes
HASH_SEQUENCE_NS = tuple(HASH_SEQUENCE_BASE + d for d in (0, 1, 15, 17)) + (HASH_K,)
HASH_VIEW_N = 100_003
HASH_VIEW_BYTE_OFFSETS = (1, 3, 8)


def random_hashes(n, seed=0):
    return np.random.default_rng([n, seed]).integers(0, 1 << 64, size=n, dtype=np.uint64, endpoint=False)


def random_codes(n, seed=0):
    return np.random.default_rng([n, seed, 4]).integers(0, 4, size=n, dtype=np.uint8)
