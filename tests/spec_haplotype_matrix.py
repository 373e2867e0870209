"""The haplotype-matrix rules of include/gki.h ("VCF haplotype matrix") in plain Python over lines: what
gki_vcf_haplotype_matrix, gki_haplotype_planes and vcf_files' host layer produce together.  This is the oracle; the
reference has no VCF code.  tests/test_haplotype_matrix_spec.py checks it against spec_vcf_allele_frequencies wherever
the two read the same GTs."""
import numpy as np

from spec_vcf_allele_frequencies import DIGITS, MAX_ALLELE_DIGITS
from spec_vcf_parse import STRIP, lines_of

MAX_PLOIDY = 8
REF, ALT, OTHER, NONE = 0, 1, 2, 3                        # the slot codes
KIND_FORMAT, KIND_GT, KIND_SAMPLES, KIND_PLOIDY = 2, 3, 4, 5


class HmError(ValueError):
    """`line`: the data line at fault, numbered from 0 in the text; `kind`: 2 FORMAT does not begin with GT, 3 a GT outside
    the grammar, 4 not exactly S sample fields, 5 a GT of more than P alleles."""

    def __init__(self, line, kind):
        super().__init__("VCF data line %d: kind %d" % (line, kind))
        self.line, self.kind = line, kind


def is_data(raw):
    return raw[:1] != b"#" and bool(raw.strip(STRIP))


def samples_of(data, n_samples=None):
    """(S, sample names or None).  S: the caller's n_samples when given; else that of the last line beginning with #CHROM
    in front of the first data line, when it has 10 fields or more (S = fields - 9); else the first data line's field
    count - 9, at least 0; a text with neither has S = 0.  The names are that header line's fields 9 and up, as str, when
    it has 10 fields or more and they are S; None otherwise."""
    header = first = None
    for raw in lines_of(bytes(data)):
        if is_data(raw):
            first = raw.rstrip(b"\r").split(b"\t")
            break
        if raw.startswith(b"#CHROM"):
            header = raw.rstrip(b"\r").split(b"\t")
    names = [f.decode("utf-8") for f in header[9:]] if header is not None and len(header) >= 10 else None
    if n_samples is not None:
        s = int(n_samples)
    elif names is not None:
        s = len(names)
    else:
        s = max(len(first) - 9, 0) if first is not None else 0
    return s, names if names is not None and len(names) == s else None


def gt_alleles(sample):
    """The alleles of a sample field's GT in text order: None for '.', else the number; ValueError outside the grammar."""
    out = []
    for allele in sample.split(b":")[0].replace(b"|", b"/").split(b"/"):
        if allele == b".":
            out.append(None)
        elif 1 <= len(allele) <= MAX_ALLELE_DIGITS and all(c in DIGITS for c in allele):
            out.append(int(allele))
        else:
            raise ValueError(allele)
    return out


def code_of(allele):
    return NONE if allele is None else REF if allele == 0 else ALT if allele == 1 else OTHER


def line_row(fields, n_samples, ploidy):
    """(row list of S * P codes, phased) of one data line's fields, or the kind of its fault (an int)."""
    if len(fields) < 10:                                   # no sample field, and FORMAT is not looked at
        return KIND_SAMPLES if n_samples > 0 else ([], 1)
    kinds, row, phased = set(), [], 1
    if fields[8][:2] != b"GT" or fields[8][2:3] not in (b"", b":"):
        kinds.add(KIND_FORMAT)
    for sample in fields[9:]:
        try:
            alleles = gt_alleles(sample)
        except ValueError:
            kinds.add(KIND_GT)
            continue
        if len(alleles) > ploidy:
            kinds.add(KIND_PLOIDY)
        if b"/" in sample.split(b":")[0]:
            phased = 0
        row.extend(([code_of(a) for a in alleles] + [NONE] * ploidy)[:ploidy])
    if len(fields) - 9 != n_samples:
        kinds.add(KIND_SAMPLES)
    return min(kinds) if kinds else (row, phased)


def data_lines(data):
    return [raw.rstrip(b"\r").split(b"\t") for raw in lines_of(bytes(data)) if is_data(raw)]


def matrix_with_faults(text, ploidy=2, n_samples=None):
    """What the kernel leaves when lines are at fault: (codes uint8[V, S * P], phased uint8[V], S, names, faults), faults
    the list of (line, kind) in line order; a line at fault has a row of 3 and phased 0."""
    if not 1 <= ploidy <= MAX_PLOIDY:
        raise ValueError("ploidy")
    s, names = samples_of(text, n_samples)
    lines = data_lines(text)
    codes, phased, faults = np.full((len(lines), s * ploidy), NONE, dtype=np.uint8), np.zeros(len(lines), dtype=np.uint8), []
    for v, fields in enumerate(lines):
        out = line_row(fields, s, ploidy)
        if isinstance(out, int):
            faults.append((v, out))
        else:
            codes[v], phased[v] = out
    return codes, phased, s, names, faults


def haplotype_matrix(text, ploidy=2, n_samples=None):
    """(codes, phased, S, sample names); HmError for the lowest line at fault."""
    codes, phased, s, names, faults = matrix_with_faults(text, ploidy, n_samples)
    if faults:
        raise HmError(*faults[0])
    return codes, phased, s, names


def planes(codes):
    """(ref_bits, alt_bits) uint64[H, ceil(V / 64)] of codes uint8[V, H], bit by bit."""
    n_variants, n_slots = codes.shape
    out = [[[0] * ((n_variants + 63) // 64) for _ in range(n_slots)] for _ in range(2)]
    for v in range(n_variants):
        for h in range(n_slots):
            if codes[v, h] in (REF, ALT):
                out[int(codes[v, h])][h][v // 64] |= 1 << (v % 64)
    return tuple(np.array(p, dtype=np.uint64).reshape(n_slots, (n_variants + 63) // 64) for p in out)


def frequencies_of(codes, lines):
    """(ref_af, alt_af) the allele-frequency rule gives, from a matrix's rows: code 0, code 1 and codes <= 2 are n_ref,
    n_alt and n_called."""
    n_ref, n_alt = np.count_nonzero(codes == 0, axis=1), np.count_nonzero(codes == 1, axis=1)
    n_called = np.count_nonzero(codes <= 2, axis=1)
    counted = np.array([len(f) >= 10 for f in lines], dtype=bool) & (n_called > 0)
    safe = np.where(counted, n_called, 1).astype(np.float64)
    return np.where(counted, n_ref / safe, 1.0), np.where(counted, n_alt / safe, 1.0)


def planes_by_packbits(codes):
    """`planes` restated with NumPy: the same words from packbits, for matrices too large for the loop above."""
    n_variants, n_slots = codes.shape
    n_words = (n_variants + 63) // 64
    out = []
    for value in (0, 1):
        bits = np.zeros((n_slots, n_words * 64), dtype=np.uint8)
        bits[:, :n_variants] = (codes == value).T
        out.append(np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(n_slots, n_words))
    return tuple(out)
