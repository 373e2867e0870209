"""Named inputs of the graph build: (reference dict, VCF text) pairs for the spec and the device, and
the inputs that must be refused with the data line each of them is refused at.  Everything is generated here, seeded."""
import numpy as np

HEADER = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
BASES = b"ACGT"


def random_reference(n, seed, p_n=0.0, p_lower=0.0):
    rng = np.random.default_rng([seed, 1])
    letters = np.frombuffer(BASES, dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
    if p_n:
        letters[rng.random(n) < p_n] = ord("N")
    if p_lower:
        low = rng.random(n) < p_lower
        letters[low] |= 0x20
    return letters.tobytes()


def other_base(c, step=1):
    """A base that differs from letter `c` ignoring case (for N: any)."""
    i = BASES.find(bytes([c]).upper())
    return BASES[(i + step) % 4:(i + step) % 4 + 1] if i >= 0 else b"A"


def line(chrom, pos, ref, alt, tail=b"\t.\tPASS\t.\tGT\t0|1"):
    return b"%s\t%d\t.\t%s\t%s%s\n" % (chrom.encode(), pos, ref, alt, tail)


def vcf(lines, header=HEADER):
    return header + b"".join(lines)


def snp(chrom, ref, pos, step=1):
    """A SNP line at 1-based `pos` of `ref`."""
    return line(chrom, pos, ref[pos - 1:pos], other_base(ref[pos - 1], step))


def deletion(chrom, ref, pos, n):
    """Padded: REF = the base at pos and the n deleted bases behind it."""
    return line(chrom, pos, ref[pos - 1:pos + n], ref[pos - 1:pos])


def insertion(chrom, ref, pos, letters):
    return line(chrom, pos, ref[pos - 1:pos], ref[pos - 1:pos] + letters)


def mixed_lines(chrom, ref, n, seed, max_del=30, max_ins=20):
    """n random lines in POS order over `ref`: SNPs, padded deletions and insertions, MNPs and a few ALTs that are not
    plain.  Positions are drawn independently, so some sites overlap or repeat (status 3)."""
    rng = np.random.default_rng([seed, 2])
    out = []
    for pos in np.sort(rng.integers(2, len(ref) - max_del - 2, size=n)).tolist():
        kind = rng.random()
        if kind < 0.55:
            out.append(snp(chrom, ref, pos, int(rng.integers(1, 4))))
        elif kind < 0.72:
            out.append(deletion(chrom, ref, pos, int(rng.integers(1, max_del + 1))))
        elif kind < 0.89:
            ins = np.frombuffer(BASES, dtype=np.uint8)[rng.integers(0, 4, size=int(rng.integers(1, max_ins + 1)))].tobytes()
            out.append(insertion(chrom, ref, pos, ins.lower() if rng.random() < 0.2 else ins))
        elif kind < 0.94:
            m = int(rng.integers(2, 5))
            out.append(line(chrom, pos, ref[pos - 1:pos - 1 + m], b"".join(other_base(c, 2) for c in ref[pos - 1:pos - 1 + m])))
        else:
            out.append(line(chrom, pos, ref[pos - 1:pos], [b"<DEL>", b"A,C", b"*", b"."][int(rng.integers(0, 4))]))
    return out


def every_third_snp(chrom, ref, n, repeated=()):
    """n SNP lines at POS 2, 5, 8, ...; the lines numbered in `repeated` stand twice (the copy is dropped for overlap and
    counts among the n)."""
    out, i = [], 0
    while len(out) < n:
        out.append(snp(chrom, ref, 2 + 3 * i))
        if i in repeated and len(out) < n:
            out.append(snp(chrom, ref, 2 + 3 * i, 2))
        i += 1
    return out


def _good_cases():
    r = random_reference(60, 3)
    c = {}
    c["no_data_line"] = ({"1": r}, b"")
    c["headers_only"] = ({"1": r}, HEADER)
    c["one_snp"] = ({"1": r}, vcf([snp("1", r, 10)]))
    c["snp_at_pos_1"] = ({"1": r}, vcf([snp("1", r, 1), snp("1", r, 7)]))
    c["snp_on_last_base"] = ({"1": r}, vcf([snp("1", r, 60)]))
    c["adjacent_snps"] = ({"1": r}, vcf([snp("1", r, 10), snp("1", r, 11), snp("1", r, 12)]))
    c["insertion_and_snp_at_one_lo"] = ({"1": r}, vcf([insertion("1", r, 9, b"GG"), snp("1", r, 10)]))
    c["two_insertions_at_one_point"] = ({"1": r}, vcf([insertion("1", r, 9, b"GG"), insertion("1", r, 9, b"T")]))
    c["deletion_touching_next_snp"] = ({"1": r}, vcf([deletion("1", r, 9, 3), snp("1", r, 13)]))
    c["snp_inside_deletion"] = ({"1": r}, vcf([deletion("1", r, 9, 5), snp("1", r, 12), snp("1", r, 20)]))
    # the second line (a 6-base deletion from POS 12) is dropped; the third overlaps only that one and is dropped too
    c["overlap_of_dropped_only"] = ({"1": r}, vcf([deletion("1", r, 9, 5), deletion("1", r, 12, 6), snp("1", r, 17),
                                                   snp("1", r, 30)]))
    c["two_snps_at_one_pos"] = ({"1": r}, vcf([snp("1", r, 10, 1), snp("1", r, 10, 2)]))
    c["alts_not_plain"] = ({"1": r}, vcf([line("1", 5, r[4:5], b"C,G"), line("1", 8, r[7:8], b"<DEL>"),
                                          line("1", 9, r[8:9], b"*"), line("1", 11, r[10:11], b"."),
                                          line("1", 13, r[12:13], b"R"), line("1", 14, b"R", b"A"),
                                          line("1", 15, r[14:15], b""), snp("1", r, 20)]))
    c["lower_case_ref_and_alt"] = ({"1": r}, vcf([line("1", 10, r[9:10].lower(), other_base(r[9]).lower()),
                                                  line("1", 20, r[19:22].lower(), r[19:20]),
                                                  line("1", 30, r[29:30], r[29:30].lower() + b"acgt")]))
    low = random_reference(60, 4, p_lower=0.5)
    c["lower_case_reference"] = ({"1": low}, vcf([snp("1", low, 10), deletion("1", low.upper(), 20, 4),
                                                  insertion("1", low, 30, b"ac")]))
    with_n = r[:20] + b"NNNNnnnn" + r[28:]
    c["n_in_reference"] = ({"1": with_n}, vcf([snp("1", with_n, 10), line("1", 22, b"N", b"A"), deletion("1", with_n, 25, 5)]))
    c["mnp_shared_first_base"] = ({"1": r}, vcf([line("1", 10, r[9:12], r[9:10] + other_base(r[10]) + other_base(r[11]))]))
    c["ref_equals_alt"] = ({"1": r}, vcf([line("1", 10, r[9:10], r[9:10]), line("1", 20, r[19:22], r[19:22])]))
    a, b, d = random_reference(40, 5), random_reference(33, 6), random_reference(50, 7)
    c["two_chromosomes"] = ({"chrA": a, "chrB": b}, vcf([snp("chrA", a, 5), deletion("chrA", a, 20, 3), snp("chrB", b, 7),
                                                        insertion("chrB", b, 33, b"ACG")]))
    c["three_chromosomes_middle_empty"] = ({"chrA": a, "chrB": b, "chrC": d},
                                           vcf([snp("chrA", a, 5), snp("chrC", d, 2), snp("chrC", d, 50)]))
    c["three_chromosomes_first_and_last_empty"] = ({"chrA": a, "chrB": b, "chrC": d}, vcf([snp("chrB", b, 7)]))
    c["three_chromosomes_no_variants"] = ({"chrA": a, "chrB": b, "chrC": d}, HEADER)
    c["last_base_then_second_base"] = ({"chrA": a, "chrB": b}, vcf([snp("chrA", a, 40), snp("chrB", b, 2)]))
    big = random_reference(3 * 2049 + 10, 8)
    c["lines_2047"] = ({"1": big}, vcf(every_third_snp("1", big, 2047)))
    c["lines_2048"] = ({"1": big}, vcf(every_third_snp("1", big, 2048, repeated=(5, 900, 2000))))
    c["lines_2049"] = ({"1": big}, vcf(every_third_snp("1", big, 2049)))
    c["lines_2049_kept_2047"] = ({"1": big}, vcf(every_third_snp("1", big, 2049, repeated=(0, 1023))))
    rng = np.random.default_rng(9)
    long_alts = [np.frombuffer(BASES, dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes() for n in (1, 15, 16, 17, 4097)]
    c["alt_lengths"] = ({"1": r}, vcf([insertion("1", r, 5 + 7 * i, s) for i, s in enumerate(long_alts)]))
    far = random_reference(150000, 10)
    c["long_deletion_and_gap"] = ({"1": far}, vcf([snp("1", far, 3), deletion("1", far, 70010, 70000), snp("1", far, 149000)]))
    return c


RANDOM_CASES = ("mixed_random", "mixed_random_two_chromosomes")


def _random_cases():
    c = {}
    ref = random_reference(200003, 11, p_n=0.002, p_lower=0.05)
    c["mixed_random"] = ({"1": ref}, vcf(mixed_lines("1", ref, 400, 12)))
    a, b = random_reference(5003, 13), random_reference(4099, 14, p_lower=0.1)
    c["mixed_random_two_chromosomes"] = ({"a": a, "b": b}, vcf(mixed_lines("a", a, 150, 15) + mixed_lines("b", b, 120, 16)))
    return c


def _error_cases():
    """name -> (reference, text, data line at fault, kind as tests/spec_graph_build.py names it)"""
    r, b = random_reference(60, 3), random_reference(33, 6)
    ok = snp("1", r, 5)
    e = {}
    e["fewer_than_five_fields"] = ({"1": r}, vcf([ok, b"1\t9\t.\tA\n"]), 1, "fewer than five fields")
    e["ref_mismatch"] = ({"1": r}, vcf([ok, snp("1", r, 8), line("1", 10, other_base(r[9]), r[9:10])]), 2,
                         "REF differs from the reference")
    e["ref_mismatch_not_plain_alt"] = ({"1": r}, vcf([line("1", 10, other_base(r[9]), b"<DEL>")]), 0,
                                       "REF differs from the reference")
    e["ref_past_end"] = ({"1": r, "2": b}, vcf([ok, line("1", 59, r[58:60] + b[0:1], r[58:59])]), 1,
                         "REF past the chromosome's end")
    e["pos_zero"] = ({"1": r}, vcf([line("1", 0, b"A", b"C"), ok]), 0, "POS outside the chromosome")
    e["pos_beyond_end"] = ({"1": r, "2": b}, vcf([ok, line("1", 61, b[0:1], other_base(b[0]))]), 1,
                           "POS outside the chromosome")
    e["pos_not_plain_digits"] = ({"1": r}, vcf([ok, snp("1", r, 8), b"1\t+12\t.\tA\tC\n"]), 2, "POS is not plain digits")
    e["pos_decreasing"] = ({"1": r}, vcf([ok, snp("1", r, 20), snp("1", r, 19)]), 2, "POS decreasing")
    e["unknown_chromosome"] = ({"1": r}, vcf([ok, snp("3", r, 9)]), 1, "unknown chromosome")
    e["chromosome_in_two_runs"] = ({"1": r, "2": b}, vcf([ok, snp("2", b, 9), snp("1", r, 30)]), 2, "chromosome in two runs")
    e["runs_out_of_graph_order"] = ({"1": r, "2": b}, vcf([snp("2", b, 9), ok]), 1, "chromosome runs out of graph order")
    return e


GOOD_CASES = _good_cases()
GOOD_CASES.update(_random_cases())
ERROR_CASES = _error_cases()
