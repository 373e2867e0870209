"""The reads files of the read-file tests, as bytes: shared by tests/test_read_files_spec.py (CPU),
tests/golden/make_golden_read_files.py (the reference run) and tests/test_gpu_read_files.py (-m gpu).

GOLDEN_CASES   FASTA files the reference's ReadKmers.from_fasta_file can read (letters ACGTacgt, no line that is empty
               after the strip); their per-read hashes are recorded in tests/golden/read_files_reference.json.gz.
PARSE_CASES    small files for the parse itself, parsed under both formats (FASTQ rules are positional, so any bytes
               have a defined answer).
FASTQ_CASES    four-line records, each with the FASTA file that holds the same reads.
boundary_cases(T, S)   files laid out around the kernels' tile of T bytes and the scan's block of S items.
"""
import numpy as np

GOLDEN_KS = (5, 31)


def _dna(rng, n, lower=0.0):
    s = "".join("ACGT"[c] for c in rng.integers(0, 4, size=n))
    if lower:
        s = "".join(ch.lower() if rng.random() < lower else ch for ch in s)
    return s.encode("ascii")


def _fasta(reads, eol=b"\n", last_eol=True, header=lambda i: b">read%d" % i):
    out = b"".join(header(i) + eol + r + eol for i, r in enumerate(reads))
    return out if last_eol else out[:len(out) - len(eol)]


def _golden_cases():
    rng = np.random.default_rng(20240917)
    reads = [_dna(rng, int(n)) for n in rng.integers(35, 61, size=6)]
    cases = {
        "plain_lf": _fasta(reads),
        "crlf": _fasta(reads, eol=b"\r\n"),
        "no_final_newline": _fasta(reads, last_eol=False),
        "crlf_no_final_newline": _fasta(reads, eol=b"\r\n", last_eol=False),
        # blanks, tabs and the other bytes str.strip() removes, before and after the letters
        "blank_padded": b">a\n  " + reads[0] + b"\n>b\n" + reads[1] + b" \t \n>c\n\t" + reads[2] + b"\x0b\x0c\n>d\n\x1c\x1d"
                        + reads[3] + b"\x1e\x1f \n" + reads[4] + b"  ",
        "multi_line_records": b">chr1 three lines\n" + reads[0] + b"\n" + reads[1] + b"\n" + reads[2] + b"\n>chr2\n"
                              + reads[3] + b"\n" + reads[4] + b"\n",
        "consecutive_headers": b">x\n>y\n>z\n" + reads[0] + b"\n>u\n>v\n" + reads[1] + b"\n>w\n",
        "no_headers": b"".join(r + b"\n" for r in reads),
        "mixed_case": _fasta([_dna(rng, 40 + 3 * i, lower=0.5) for i in range(5)]),
        # lengths k, k - 1 and 1 at both k, between reads every k defines
        "short_reads": _fasta([_dna(rng, n) for n in (48, 31, 30, 52, 5, 4, 44, 1, 39, 63, 36, 57)]),
    }
    # the streaming case: longer than one tile of the parse kernels, about a hundred reads of 35..90 letters
    cases["stream"] = _fasta([_dna(rng, int(n), lower=0.1) for n in rng.integers(35, 91, size=100)])
    return cases


GOLDEN_CASES = _golden_cases()

PARSE_CASES = {
    "empty": b"",
    "one_letter": b"A",
    "one_newline": b"\n",
    "headers_only": b">a\n>b\n>c\n",
    "header_only_no_newline": b">a",
    "blank_lines": b">a\n\nACGT\n\n\n>b\n   \n\t\r\nAC\n\n",
    "whitespace_only": b" \t \n\x0b\x0c\n\x1c\x1d\x1e\x1f\n \n",
    "space_before_gt": b" >x\n>y\n  >z  \nACGT\n",
    "inner_blanks_kept": b">a\nAC GT\tA\n  A C  \n",
    "other_letters": b">a\nACGTNNNNacgtnRYKM*-\n>b\nnnnn\n",
    "crlf_blank": b">a\r\n\r\nACGT\r\n\r\n",
    "only_carriage_returns": b"\r\n\r\n\r\n",
    "control_bytes_not_stripped": b">a\n\x00AC\x08\n\x0eGT\x1b\n\x7fA\x21\n",
    "lengths_k_km1_1": b">a\nACGTA\n>b\nACGT\n>c\nA\n>d\n" + b"ACGT" * 7 + b"ACG\n>e\n" + b"ACGT" * 7 + b"AC\n",
}


def fastq_of(records, eol=b"\n", last_eol=True):
    """records: (name line, sequence line, plus line, quality line), raw, without terminators."""
    out = b"".join(eol.join(rec) + eol for rec in records)
    return out if last_eol else out[:len(out) - len(eol)]


def fasta_rewriting(records):
    """The same reads as a FASTA file: one header, then the raw sequence line."""
    return b"".join(b">" + rec[0][1:] + b"\n" + rec[1] + b"\n" for rec in records)


def _fastq_cases():
    rng = np.random.default_rng(77)

    def qual(n, first=None):
        q = bytes(rng.integers(33, 74, size=n).astype(np.uint8))
        return q if first is None or n == 0 else first + q[1:]

    def rec(i, n, first=None, plus=b"+", pad=(b"", b"")):
        seq = _dna(rng, n)
        return (b"@read%d extra words" % i, pad[0] + seq + pad[1], plus, qual(n, first))

    plain = [rec(i, int(n)) for i, n in enumerate(rng.integers(1, 70, size=10))]
    # quality lines that look like a FASTA header, a FASTQ name and a separator
    tricky = [rec(0, 40, b">"), rec(1, 41, b"@"), rec(2, 42, b"+"), rec(3, 36, b">", plus=b"+read3 again"),
              rec(4, 5, b"@"), rec(5, 4, b"+"), rec(6, 33, b"@", pad=(b" ", b"\t"))]
    cases = {
        "plain": (fastq_of(plain), plain),
        "tricky_quality": (fastq_of(tricky), tricky),
        "crlf": (fastq_of(plain, eol=b"\r\n"), plain),
        "no_final_newline": (fastq_of(plain, last_eol=False), plain),
        "empty_sequence": (fastq_of([plain[0], (b"@e", b"", b"+", b""), plain[1]]), [plain[0], (b"@e", b"", b"+", b""), plain[1]]),
    }
    # cut after a record's second line: the read is still there
    whole = fastq_of(plain[:3])
    third = plain[2]
    cut = fastq_of(plain[:2]) + third[0] + b"\n" + third[1] + b"\n"
    assert whole.startswith(cut)
    cases["cut_after_second_line"] = (cut, plain[:3])
    cases["cut_after_second_line_no_newline"] = (cut[:-1], plain[:3])
    return cases


FASTQ_CASES = _fastq_cases()            # name -> (FASTQ bytes, its records)
FORTY_LINES = FASTQ_CASES["plain"][0]   # ten records
assert FORTY_LINES.count(b"\n") == 40

# a record whose third line does not begin with "+": one bad line
_bad = [list(r) for r in FASTQ_CASES["plain"][1][:4]]
_bad[2][2] = b"-"
BAD_THIRD_LINE = fastq_of([tuple(r) for r in _bad])


def boundary_cases(T, S):
    """Files around the parse kernels' sizes.  T: bytes one workgroup scans; S: items one block of the scan covers."""
    cases = {}
    for name, at in (("newline_at_T_minus_1", T - 1), ("newline_at_T", T), ("newline_at_T_plus_1", T + 1)):
        # the first line end is byte `at` of the buffer (counted from 0); short lines follow
        cases[name] = b">" + b"h" * (at - 1) + b"\nACGTA\n>x\nAC\n"
        assert cases[name].index(b"\n") == at
    cases["line_of_2T_plus_3"] = b">a\n" + b"ACGT" * ((2 * T + 3) // 4) + b"ACG"[:(2 * T + 3) % 4] + b"\n>b\nACGTACGT\n"
    assert len(cases["line_of_2T_plus_3"].split(b"\n")[1]) == 2 * T + 3
    cases["long_line_no_final_newline"] = b">a\nAC\n" + b"  " + b"GATTACA" * ((T + 100) // 7) + b" \t"
    # a tile without any line end (the header runs over all of the second tile), then short lines
    cases["tile_without_newline"] = b">a\nACGT\n>" + b"h" * (2 * T) + b"\nAC\nGT\n\nA\n"
    cases["T_plus_3_newlines"] = b"\n" * (T + 3)
    cases["T_plus_3_newlines_then_read"] = b"\n" * (T + 3) + b"ACGTAC"
    for n in (S - 1, S, S + 1, 2 * S + 1):
        cases["%d_lines_of_A" % n] = b"A\n" * n
    cases["whitespace_line_over_a_tile"] = b">a\n" + b" " * (T + 5) + b"\nACGT\n" + b" " * (T + 7) + b"AC" + b"\t" * (T + 9) + b"\n"
    return cases
