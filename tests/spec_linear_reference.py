"""NumPy restatement of the linear-reference path: SnpKmerFinder.find_kmers_on_linear_reference (snp_kmer_finder.py:298-312)
and the chunked `make -R` (command_line_interface.py:105-153), as the expectation of the GPU tests.  Test code only: the
product does not import it.  Everything here is written from the reference's observable behaviour; tests/
test_linear_reference_spec.py checks it against the reference itself and against tests/golden/linear_reference.npz.

Deliberate difference from the reference, as in the product: `ref_offsets` has one entry per record, the record's
position (the reference's column is longer than its hashes)."""
import numpy as np


def power_array(k):
    return np.power(4, np.arange(k - 1, -1, -1)).astype(np.uint64)


def letters_of(seq):
    if isinstance(seq, str):
        seq = seq.encode("ascii")
    if isinstance(seq, (bytes, bytearray)):
        seq = np.frombuffer(bytes(seq), dtype=np.uint8)
    return np.asarray(seq, dtype=np.uint8)


def codes_of(seq):
    """c/g/t -> 1/2/3 in either case, every other byte 0 (flat_kmers.py:134-145)."""
    lower = letters_of(seq) | np.uint8(0x20)
    codes = np.zeros(len(lower), dtype=np.uint64)
    codes[lower == ord("c")] = 1
    codes[lower == ord("g")] = 2
    codes[lower == ord("t")] = 3
    return codes


def window_hashes(seq, k):
    """Hash of every k-window: np.convolve with power_array(k) (read_kmers.py:68-70)."""
    return np.convolve(codes_of(seq), power_array(k), mode="valid").astype(np.uint64)


def window_hashes_by_shifts(seq, k):
    """The same hashes as sum_m code[i + m] << 2m: 31 passes over the array instead of a length-k dot product per window,
    for the large case."""
    codes = codes_of(seq)
    n = len(codes) - k + 1
    out = np.zeros(n, dtype=np.uint64)
    for m in range(k):
        out |= codes[m:m + n] << np.uint64(2 * m)
    return out


def reverse_complement_hashes(hashes, k):
    """kmer_hashing.py:24-28 digit by digit: rc = sum_j (3 - d_j) 4^(k-1-j)."""
    h = np.asarray(hashes, dtype=np.uint64)
    out = np.zeros(len(h), dtype=np.uint64)
    for j in range(k):
        digit = (h >> np.uint64(2 * j)) & np.uint64(3)
        out |= (np.uint64(3) - digit) << np.uint64(2 * (k - 1 - j))
    return out


def interval_records(seq, k, spacing, start, end, all_hashes=None):
    """(hashes, positions) of the inclusive interval [start, end]: the slice seq[start:end + k] clips it."""
    n = len(letters_of(seq))
    length = min(end + k, n) - start
    assert length >= k, "no whole k-mer in the interval"
    positions = start + np.arange(0, length - k + 1, spacing, dtype=np.int64)
    if all_hashes is None:
        hashes = window_hashes(letters_of(seq)[start:end + k], k)[::spacing]
    else:
        hashes = all_hashes[positions]
    return hashes, positions.astype(np.uint64)


def chunk_intervals(genome_size, spacing, threads):
    """command_line_interface.py:120-131."""
    n_jobs = threads * 10
    per = (genome_size // spacing) // n_jobs
    return [(per * i * spacing, per * (i + 1) * spacing) for i in range(n_jobs)]


def make_columns(seq, k, spacing, genome_size, threads, reverse_complement, all_hashes=None):
    """The four FlatKmers columns of `make -R -t threads`: chunk by chunk, each followed by its reverse complements."""
    hashes, offsets = [], []
    for start, end in chunk_intervals(genome_size, spacing, threads):
        h, p = interval_records(seq, k, spacing, start, end, all_hashes)
        hashes.append(h)
        offsets.append(p)
        if reverse_complement:
            hashes.append(reverse_complement_hashes(h, k))
            offsets.append(p)
    hashes = np.concatenate(hashes).astype(np.uint64)
    return dict(hashes=hashes, nodes=np.ones(len(hashes), dtype=np.uint32),
                ref_offsets=np.concatenate(offsets).astype(np.uint64),
                allele_frequencies=np.ones(len(hashes), dtype=np.float32))


def column_checksum(a):
    """(sum mod 2^64, xor) of a column's elements as unsigned integers of their own width (DeviceArray.checksum)."""
    u = np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]).astype(np.uint64)
    return int(np.add.reduce(u, dtype=np.uint64)), int(np.bitwise_xor.reduce(u))
