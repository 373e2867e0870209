"""The allele-frequency rules of include/gki.h ("VCF allele frequencies") in plain Python over lines:
what gki_vcf_allele_frequencies and vcf_files' host layer produce together.  The value oracle is Python's float();
`device_value` restates the device's one-operation rule in NumPy doubles, and tests/test_vcf_allele_frequencies_spec.py
checks that the two agree wherever the device parses."""
import math

import numpy as np

from spec_vcf_parse import STRIP, lines_of

DIGITS = b"0123456789"
ROUTE_DEVICE, ROUTE_ABSENT, ROUTE_HOST = 0, 1, 2
MAX_MANTISSA_DIGITS, MAX_EXPONENT_DIGITS, MAX_POWER, MAX_ALLELE_DIGITS = 15, 3, 22, 9
POW10 = np.array([10.0 ** q for q in range(MAX_POWER + 1)], dtype=np.float64)   # each exact in a double


class AfError(ValueError):
    """`line`: the data line at fault, numbered from 0 in the text; `kind`: 'value' (not finite or outside [0, 1]),
    'text' (float() refuses it), 'format' (FORMAT does not begin with GT) or 'genotype' (a GT outside the grammar)."""

    def __init__(self, line, kind):
        super().__init__("VCF data line %d: %s" % (line, kind))
        self.line, self.kind = line, kind


def data_lines(data):
    """The data lines of the text as lists of fields, every '\\r' at a line's end dropped."""
    return [raw.rstrip(b"\r").split(b"\t") for raw in lines_of(bytes(data)) if raw[:1] != b"#" and raw.strip(STRIP)]


def _digits(text, at):
    end = at
    while end < len(text) and text[end] in DIGITS:
        end += 1
    return end


def device_value(text):
    """The device's rule on a value text: None when it is outside the grammar  D* [ . D* ] [ (e|E) [+|-] D+ ]  or its
    limits (route 2), else m / 10^-q or m * 10^q as one np.float64 operation."""
    a = _digits(text, 0)
    whole, fraction, p = text[:a], b"", a
    if text[p:p + 1] == b".":
        p = _digits(text, a + 1)
        fraction = text[a + 1:p]
    mantissa = whole + fraction
    if not 1 <= len(mantissa) <= MAX_MANTISSA_DIGITS:
        return None
    exponent = 0
    if text[p:p + 1] in (b"e", b"E"):
        p += 1
        sign = text[p:p + 1] if text[p:p + 1] in (b"+", b"-") else b""
        p += len(sign)
        end = _digits(text, p)
        if not 1 <= end - p <= MAX_EXPONENT_DIGITS:
            return None
        exponent = int(text[p:end]) * (-1 if sign == b"-" else 1)
        p = end
    q = exponent - len(fraction)
    if p != len(text) or abs(q) > MAX_POWER:
        return None
    m = np.float64(int(mantissa))                          # below 10^15: exact
    return m / POW10[-q] if q < 0 else m * POW10[q]


def info_value_text(fields):
    """The value text of the line's AF= entry, None when INFO or the entry is missing."""
    if len(fields) < 8:
        return None
    for entry in fields[7].split(b";"):
        if entry[:3] == b"AF=":
            return entry[3:].split(b",")[0]
    return None


def info_line(fields, line):
    text = info_value_text(fields)
    if text is None or text in (b"", b"."):
        return 1.0, 1.0, ROUTE_ABSENT
    route = ROUTE_HOST if device_value(text) is None else ROUTE_DEVICE
    try:
        value = float(text)
    except ValueError:
        raise AfError(line, "text") from None
    if not math.isfinite(value) or not 0.0 <= value <= 1.0:
        raise AfError(line, "value")
    return 1.0 - value, value, route


def genotype_line(fields, line):
    if len(fields) < 10:
        return 1.0, 1.0, ROUTE_ABSENT
    if fields[8][:2] != b"GT" or fields[8][2:3] not in (b"", b":"):
        raise AfError(line, "format")
    n_called = n_ref = n_alt = 0
    for sample in fields[9:]:
        alleles = sample.split(b":")[0].replace(b"|", b"/").split(b"/")
        for allele in alleles:
            if allele == b".":
                continue
            if not 1 <= len(allele) <= MAX_ALLELE_DIGITS or any(c not in DIGITS for c in allele):
                raise AfError(line, "genotype")
            n_called += 1
            n_ref += int(allele) == 0
            n_alt += int(allele) == 1
    if n_called == 0:
        return 1.0, 1.0, ROUTE_ABSENT
    return n_ref / n_called, n_alt / n_called, ROUTE_DEVICE


def allele_frequencies(data, source):
    """(ref_af float64, alt_af float64, route uint8) with one entry per data line of the text; AfError for the lowest
    line at fault.  source: 'info' or 'genotypes'."""
    rule = {"info": info_line, "genotypes": genotype_line}[source]
    out = [rule(fields, v) for v, fields in enumerate(data_lines(data))]
    return (np.array([o[0] for o in out], dtype=np.float64), np.array([o[1] for o in out], dtype=np.float64),
            np.array([o[2] for o in out], dtype=np.uint8))
