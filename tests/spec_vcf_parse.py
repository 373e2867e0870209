"""The VCF-file rules of include/gki.h ("VCF files") in plain Python and NumPy, producing what gki_vcf_parse_count and
gki_vcf_parse_emit produce.  The oracle behind it is VariantArrays.from_vcf (tests/test_vcf_parse_spec.py compares the two)."""
import numpy as np

STRIP = bytes([0x20]) + bytes(range(0x09, 0x0E)) + bytes(range(0x1C, 0x20))       # str.strip() of ASCII text
DIGITS = b"0123456789"
KIND1_TEXT = "VCF data line %d has fewer than two columns"                        # VariantArrays.from_vcf's message


def lines_of(data):
    """The lines of the buffer without their '\\n'; the last one may lack it."""
    if not data:
        return []
    lines = data.split(b"\n")
    return lines[:-1] if data.endswith(b"\n") else lines


def parse(data):
    """dict of the ABI's outputs: n_lines, positions int64, is_snp int8, chrom_run int32, run_name_start int64[runs + 1],
    run_names uint8, first_bad_variant, first_bad_kind.  The arrays cover every data line, the bad ones too (POS 0)."""
    positions, is_snp, chroms = [], [], []
    bad = (-1, 0)
    lines = lines_of(bytes(data))
    for raw in lines:
        if raw[:1] == b"#" or not raw.strip(STRIP):
            continue
        fields = raw.rstrip(b"\r").split(b"\t")
        pos, kind = 0, 0
        if len(fields) < 2:
            kind = 1
        elif not 1 <= len(fields[1]) <= 18 or any(c not in DIGITS for c in fields[1]):
            kind = 2
        else:
            pos = int(fields[1])
        if kind and bad[0] < 0:
            bad = (len(positions), kind)
        chroms.append(fields[0])
        positions.append(pos)
        is_snp.append(-1 if len(fields) < 5 else int(len(fields[3]) == 1 and len(fields[4]) == 1))
    run, names = [], []
    for v, c in enumerate(chroms):
        if v == 0 or c != chroms[v - 1]:
            names.append(c)
        run.append(len(names) - 1)
    return {"n_lines": len(lines), "positions": np.array(positions, dtype=np.int64), "is_snp": np.array(is_snp, dtype=np.int8),
            "chrom_run": np.array(run, dtype=np.int32),
            "run_name_start": np.cumsum([0] + [len(c) for c in names]).astype(np.int64),
            "run_names": np.frombuffer(b"".join(names), dtype=np.uint8), "first_bad_variant": bad[0],
            "first_bad_kind": bad[1]}


def run_name_list(out):
    """The runs' names as str, decoded as UTF-8."""
    s, names = out["run_name_start"], out["run_names"].tobytes()
    return [names[a:b].decode("utf-8") for a, b in zip(s[:-1], s[1:])]


def piece(data):
    """What graph_kmer_index_amd.vcf_files.parse_vcf_on_device returns for the buffer, with the bad line behind it:
    (positions, is_snp, chrom_run, run_names list[str], n_lines), (first_bad_variant, first_bad_kind)."""
    out = parse(data)
    return (out["positions"], out["is_snp"], out["chrom_run"], run_name_list(out), out["n_lines"]), \
        (out["first_bad_variant"], out["first_bad_kind"])
