"""tests/spec_genotype_cohort.py checked on the CPU: with one sample it is spec_genotype's text on that module's own kinds of
text, the width identity gives every column's true offset, faults are named by the lowest line, and names are validated."""
import numpy as np
import pytest

import spec_genotype as single
import spec_genotype_cohort as spec


def site(i, info=b".", more=b""):
    return b"1\t%d\trs%d\tA\tC\t.\tPASS\t%s%s" % (100 + i, i, info, more)


HEADER = b"##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"x\">\n" \
         b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\n"
TEXTS = {
    "a line end at the file's end": HEADER + b"\n".join(site(i) for i in range(5)) + b"\n",
    "none at the file's end": HEADER + b"\n".join(site(i) for i in range(5)),
    "nine and more fields": b"\n".join(site(i, b"X", b"\tGT:DP\t0/1:3\t1/1:4") for i in range(7)) + b"\n",
    "CRLF": HEADER.replace(b"\n", b"\r\n") + b"\r\n".join(site(i) for i in range(9)) + b"\r\n",
    "blank and comment lines between": b"\n \t\n" + site(0) + b"\n\n#x\n" + site(1) + b"\n   \n",
}


def n_data(text):
    return sum(1 for _, is_data in single.lines_of(text) if is_data)


@pytest.mark.parametrize("ploidy", [1, 2, 3, 8])
def test_one_sample_is_the_single_sample_text(ploidy):
    for what, text in TEXTS.items():
        n = n_data(text)
        rng = np.random.default_rng([n, ploidy])
        call = rng.integers(-1, ploidy + 1, size=n).astype(np.int8)
        gq = rng.choice(np.array([0, 9, 10, 99], dtype=np.uint8), size=n)
        assert spec.data_lines_text(text, [call], [gq], ploidy) == single.data_lines_text(text, call, gq, ploidy), what
        assert spec.genotyped_vcf(text, [call], [gq], ploidy, ["NA7"]) == single.genotyped_vcf(text, call, gq, ploidy, "NA7"), what


def test_two_samples_by_hand():
    text = site(0) + b"\n" + site(1, b"AF=1", b"\tGT\t0|1") + b"\n"
    got = spec.genotyped_vcf(HEADER + text, [[0, 2], [-1, 1]], [[5, 99], [50, 10]], 2, ["a", "b"])
    assert got == (b"##fileformat=VCFv4.2\n" + b"\n".join(single.FORMAT_LINES) + b"\n"
                   b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\n"
                   b"1\t100\trs0\tA\tC\t.\tPASS\t.\tGT:GQ\t0/0:5\t./.:.\n"
                   b"1\t101\trs1\tA\tC\t.\tPASS\tAF=1\tGT:GQ\t1/1:99\t0/1:10\n")
    # a quality above 99 is written as 99
    assert spec.data_lines_text(site(0), [[1]], [[200]], 1).endswith(b"\tGT:GQ\t1:99\n")


def columns_of(kind, n_samples, ploidy, seed):
    rng = np.random.default_rng([n_samples, ploidy, seed])
    if kind == "all narrow":
        return rng.integers(0, ploidy + 1, size=n_samples), rng.choice([0, 9], size=n_samples)
    if kind == "all wide":
        return rng.integers(0, ploidy + 1, size=n_samples), rng.choice([10, 99], size=n_samples)
    if kind == "no calls":                                 # narrow whatever the quality
        return np.full(n_samples, -1), rng.choice([0, 9, 10, 99], size=n_samples)
    return rng.integers(-1, ploidy + 1, size=n_samples), rng.choice([0, 9, 10, 99], size=n_samples)


@pytest.mark.parametrize("ploidy", [1, 2, 3, 8])
@pytest.mark.parametrize("kind", ["all narrow", "all wide", "mixed", "no calls"])
def test_the_width_identity_gives_every_columns_offset(ploidy, kind):
    for n_samples in (1, 2, 63, 64, 65, 129, 200):
        call, gq = columns_of(kind, n_samples, ploidy, 3)
        line = spec.data_lines_text(site(0), call.reshape(-1, 1), gq.reshape(-1, 1), ploidy)
        columns = line[line.index(b"\tGT:GQ") + 6:-1]
        offsets = spec.column_offsets(call, gq, ploidy)
        true, at = [], 0                                   # where the columns begin in the text itself
        for c in columns.split(b"\t")[1:]:
            true.append(at)
            at += 1 + len(c)
        assert offsets == true and at == len(columns)
        for s in range(n_samples):
            width = spec.column_width(int(call[s]), int(gq[s]), ploidy)
            assert columns[offsets[s]:offsets[s] + width] == b"\t" + single.sample_column(int(call[s]), int(gq[s]), ploidy)
        if kind == "all narrow" or kind == "no calls":
            assert len(columns) == (2 * ploidy + 2) * n_samples
        if kind == "all wide":
            assert len(columns) == (2 * ploidy + 3) * n_samples


def test_fault_order():
    lines = [site(i) for i in range(20)]
    lines[15] = b"1\t250\t.\tA\tC\t.\tPASS"                # seven fields
    lines[7] = b"1\t170"
    text = b"\n".join(lines) + b"\n"
    call, gq = np.zeros((3, 20), np.int8), np.zeros((3, 20), np.uint8)
    with pytest.raises(ValueError, match="data line 7: fewer than eight fields"):
        spec.data_lines_text(text, call, gq, 2)
    call[2][6], call[0][9] = 3, -2                         # any sample's column; the line is named, not the sample
    with pytest.raises(ValueError, match="data line 6: a call outside"):
        spec.data_lines_text(text, call, gq, 2)
    call[2][6], call[1][7] = 2, 5                          # both kinds on line 7: the fields come first
    with pytest.raises(ValueError, match="data line 7: fewer than eight fields"):
        spec.data_lines_text(text, call, gq, 2)
    text = b"\n".join(site(i) for i in range(20)) + b"\n"  # the text's data lines are not V
    for n in (19, 21):
        with pytest.raises(ValueError, match="data lines"):
            spec.data_lines_text(text, np.zeros((3, n), np.int8), np.zeros((3, n), np.uint8), 2)


def test_name_validation():
    assert spec.check_sample_names(["a", "NA12878", "x.y-z"]) == ["a", "NA12878", "x.y-z"]
    for bad in (["a", ""], ["a", "a"], ["a b"], ["a\tb"], ["a\n"], ["a\r"]):
        with pytest.raises(ValueError):
            spec.check_sample_names(bad)
        with pytest.raises(ValueError):
            spec.header_text(HEADER, bad)
    assert spec.header_text(HEADER, ["x", "y", "z"]).endswith(b"\tINFO\tFORMAT\tx\ty\tz\n")
    with pytest.raises(ValueError, match="sample names"):
        spec.genotyped_vcf(HEADER + site(0), [[0], [1]], [[0], [0]], 2, ["only"])
