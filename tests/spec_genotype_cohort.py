"""The rule of DESIGN.md 4.23 (include/gki.h, "genotyped cohort VCF text") as plain Python, on spec_genotype's lines_of and
sample_column: the text of a genotyped VCF with S sample columns, its header, the sample names' rule and the width identity
by which the device finds a byte's column.  No device and nothing of graph_kmer_index_amd: this is the oracle of
tests/test_gpu_genotype_cohort.py, itself checked in tests/test_genotype_cohort_spec.py."""
import spec_genotype as single

FAULTS = {1: "fewer than eight fields", 2: "a call outside -1 .. ploidy"}


def check_sample_names(names):
    """ValueError unless the names are non-empty, unique and free of tabs, spaces and line ends."""
    names = [str(n) for n in names]
    for n in names:
        if not n or any(c in n for c in "\t \n\r"):
            raise ValueError("sample name %r: a name is not empty and holds no tab, space or line end" % (n,))
    if len(set(names)) != len(names):
        raise ValueError("the sample names are not unique")
    return names


def is_wide(c, quality):
    return c >= 0 and min(int(quality), 99) >= 10


def column_width(c, quality, ploidy):
    """2P + 2 + w: the tab, P alleles and P - 1 slashes, ':', one digit or '.', and w = 1 for a second digit."""
    return 2 * ploidy + 2 + (1 if is_wide(c, quality) else 0)


def column_offsets(calls, gq, ploidy):
    """Where every column of one line begins behind "\\tGT:GQ", by the width identity: (2P + 2) s + the wide columns below s."""
    out, wide = [], 0
    for s in range(len(calls)):
        out.append((2 * ploidy + 2) * s + wide)
        wide += 1 if is_wide(int(calls[s]), gq[s]) else 0
    return out


def data_lines_text(text, call, gq, ploidy):
    """The genotyped data lines of `text` (one piece or the whole file) for call[S][V] and gq[S][V].  ValueError naming the
    lowest data line at fault and its kind, and when the text's data lines are not V."""
    n_samples = len(call)
    if n_samples < 1:
        raise ValueError("no sample")
    n_calls = len(call[0])
    out, v, fault = [], 0, None
    for line, is_data in single.lines_of(text):
        if not is_data:
            continue
        if v >= n_calls:
            raise ValueError("the text has more than %d data lines" % n_calls)
        fields = line.split(b"\t")
        kind = 1 if len(fields) < 8 else 2 if any(not -1 <= int(call[s][v]) <= ploidy for s in range(n_samples)) else 0
        if kind and fault is None:
            fault = (v, kind)
        if not kind:
            columns = [single.sample_column(int(call[s][v]), min(int(gq[s][v]), 99), ploidy) for s in range(n_samples)]
            out.append(b"\t".join(fields[:8]) + b"\tGT:GQ" + b"".join(b"\t" + c for c in columns) + b"\n")
        v += 1
    if fault is not None:
        raise ValueError("data line %d: %s" % (fault[0], FAULTS[fault[1]]))
    if v != n_calls:
        raise ValueError("the text has %d data lines, there are %d calls" % (v, n_calls))
    return b"".join(out)


def header_text(text, sample_names):
    """The single-sample header with the #CHROM line carrying all the names."""
    return single.header_text(text, "\t".join(check_sample_names(sample_names)))


def genotyped_vcf(text, call, gq, ploidy, sample_names):
    if len(sample_names) != len(call):
        raise ValueError("%d sample names for %d rows" % (len(sample_names), len(call)))
    return header_text(text, sample_names) + data_lines_text(text, call, gq, ploidy)
