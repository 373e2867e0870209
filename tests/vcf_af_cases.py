"""Named inputs of the allele-frequency pass: VCF texts for the spec and the device, per source, and the
texts that must be refused with the data line each is refused at.  Everything is generated here, seeded.

W is what the genotype kernel takes per step (64 lanes x 16 bytes); offsets below are counted from a line's first byte,
which is where the kernel's lanes start."""
import numpy as np

HEADER = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
W = 1024
GT_FORMS = (b"0|1", b"1/1", b".", b"./.", b".|1", b"1", b"0/1/1", b"2|0", b"10|1", b"01|1", b"0|0", b"0/0:35:1,2", b"1|0:.",
            b".:7", b"0")
# every text the device must parse itself (route 0), 15 digits and q = +-22 among them; `5.` of the CPU list is above one
# and stands among the refused inputs
EDGE_TEXTS = (b"0", b"1", b"1.0", b".5", b"0.", b"1.", b"1e-05", b"1E-5", b"0.000199681", b"0.12345678901234", b"123456789012345e-15",
              b"1e-22", b"0.00000000000001e-8", b"0.0000000001e+10", b"1000000000000e-22", b"0e22", b"00000.50000",
              b"1.e-1", b"0.25E+0", b"1e-022")
# texts outside the device's limits that float() accepts as a value in [0, 1] (route 2): 16 and 17 digits, q = -23 and +23
# reached by a zero mantissa, an exponent of four digits, an underflow, a sign, blanks, an underscore
HOST_TEXTS = (b"0.123456789012345", b"0.12345678901234567", b"1e-23", b"0e23", b"1e-0005", b"1e-400", b"+0.5", b" 0.5",
              b"0.5 ", b"0_1e-2", b"-0", b"-0.0")


def gt_line(samples, ninth_tab_at=16, fmt=b"GT", pos=7):
    """A data line without its end whose ninth tab -- the one that opens the first sample -- is byte `ninth_tab_at` of the
    line when FORMAT is the two bytes of GT (14 at the least): QUAL, FILTER and INFO are empty and ID is as long as it
    takes."""
    head = b"1\t%d\t" % pos
    rest = b"\tA\tC\t\t\t\t" + fmt
    pad = ninth_tab_at - len(head) - len(rest) + len(fmt) - 2
    assert pad >= 0
    return head + b"x" * pad + rest + b"".join(b"\t" + s for s in samples)


def gt_line_of_length(n, ninth_tab_at=16):
    """A line of exactly n bytes: 0|1 samples, the last one with a subfield as long as it takes."""
    samples = [b"0|1"] * ((n - ninth_tab_at - 8) // 4)
    line = gt_line(samples + [b"1|1:"], ninth_tab_at)
    assert len(line) <= n
    return line + b"z" * (n - len(line))


def random_samples(n, seed):
    rng = np.random.default_rng([seed, 17])
    return [GT_FORMS[i] for i in rng.integers(0, len(GT_FORMS), size=n)]


def info_line(info, rest=b"", pos=5):
    return b"1\t%d\t.\tA\tC\t.\tPASS\t%s%s" % (pos, info, rest)


def text_of(lines, end=b"\n", header=HEADER, last_end=None):
    return header + b"".join(l + end for l in lines[:-1]) + lines[-1] + (end if last_end is None else last_end)


def _genotype_cases():
    c = {}
    for n in (1, 2, 63, 64, 65, 300):
        c["samples_%d" % n] = text_of([gt_line(random_samples(n, n)), gt_line(random_samples(n, n + 1000), 14)])
    c["every_gt_form"] = text_of([gt_line([g]) for g in GT_FORMS] + [gt_line(list(GT_FORMS))])
    c["line_lengths_around_w"] = text_of([gt_line_of_length(n) for n in (W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1)])
    # the ninth tab as the last byte of a lane's 16, the first of the next, and on both sides of a step's end
    c["ninth_tab_placements"] = text_of([gt_line(random_samples(5, at), at) for at in (15, 16, 31, 32, W - 1, W, W + 1)])
    # 4-byte samples from byte 15 on: the GT at bytes 15..17 straddles a lane's end, the one at 1023..1025 a step's
    c["gt_straddles_lane_and_step"] = text_of([gt_line([b"0|1", b"1|1"] * 150, 14), gt_line([b"1|0"] * 300, 14)])
    c["last_sample_lf"] = text_of([gt_line([b"0|1", b"1|1"])])
    c["last_sample_crlf"] = text_of([gt_line([b"0|1", b"1|1"]), gt_line([b"1|1", b"1"])], end=b"\r\n")
    c["last_line_unterminated"] = text_of([gt_line([b"0|0"]), gt_line([b"0|1", b"1"])], last_end=b"")
    c["last_line_unterminated_long"] = text_of([gt_line(random_samples(300, 5))], last_end=b"")
    c["all_missing"] = text_of([gt_line([b".", b"./.", b".|.:3"]), gt_line([b"0|1"])])
    c["sites_only"] = text_of([info_line(b"AF=0.5"), b"1\t9\t.\tA\tC", info_line(b".", b"\tGT")])
    c["bad_format_without_samples"] = text_of([info_line(b".", b"\tDP"), gt_line([b"0|1"])])
    # the kernel parses a GT from one 8-byte load: GTs that close on its last byte, just behind it and far behind it
    c["gt_around_eight_bytes"] = text_of([gt_line([b"1234567", b"12345678", b"123456789|0", b"0/1/1/0/1", b"10|10|10",
                                                   b"1|0:12345678", b"0000001|1", b"0/1/1/.", b"./././.", b"0|1/0|1", b"1"]),
                                          gt_line([b"0|1", b"0/1/1/0"]), gt_line([b"0|1", b"0/1/1/0/1"]),
                                          gt_line([b"0|1", b"0/1/1/0/1/1"])], last_end=b"")
    c["haploid_and_triploid"] = text_of([gt_line([b"1", b"0", b"1"]), gt_line([b"0/1/1", b"0/0/0", b"./1/2"])])
    rng = np.random.default_rng(23)
    mixed = []
    for i in range(60):
        kind = rng.random()
        if kind < 0.2:
            mixed.append(info_line(b"AF=0.25", pos=i + 1))
        elif kind < 0.3:
            mixed.append(gt_line([b"."] * int(rng.integers(1, 40)), int(rng.integers(16, 40)), pos=i + 1))
        else:
            mixed.append(gt_line(random_samples(int(rng.integers(1, 400)), 100 + i), int(rng.integers(16, 80)), pos=i + 1))
    mixed[10:10] = [b"#a comment line", b"", b" \t "]
    c["mixed_file"] = text_of(mixed)
    c["no_data_line"] = HEADER
    c["empty_text"] = b""
    return c


def _info_cases():
    c = {}
    c["af_placements"] = text_of([info_line(b"AF=0.25;DP=3"), info_line(b"DP=3;NS=2;AF=0.5"), info_line(b"AF=0.75"),
                                  info_line(b"XAF=0.1;AF=0.2"), info_line(b"MAF=0.1;AF_EUR=0.3;AF=0.4"),
                                  info_line(b"XAF=0.1"), info_line(b"AF_EUR=0.3;MAF=0.2"), info_line(b"DP=3;AF"),
                                  info_line(b"AF=0.1;AF=0.9")])
    c["af_lists_and_absent"] = text_of([info_line(b"AF=0.1,0.2"), info_line(b"AF=."), info_line(b"AF="), info_line(b"AF=;DP=1"),
                                        info_line(b"AF=.,0.5"), info_line(b"AF=,0.5"), info_line(b"."), info_line(b"")])
    c["no_info_field"] = text_of([b"1\t5\t.\tA\tC\t.\tPASS", b"1\t6\t.\tA\tC", info_line(b"AF=0.5")])
    c["info_is_last_lf"] = text_of([info_line(b"AF=0.125"), info_line(b"DP=1;AF=0.5")])
    c["info_is_last_crlf"] = text_of([info_line(b"AF=0.125"), info_line(b"DP=1;AF=0.5")], end=b"\r\n")
    c["info_is_last_unterminated"] = text_of([info_line(b"AF=0.125"), info_line(b"DP=1;AF=0.0625")], last_end=b"")
    c["info_before_samples"] = text_of([info_line(b"AF=0.3", b"\tGT\t0|1\t1|1"), info_line(b"DP=2", b"\tGT\t0|1;AF=0.9")])
    c["edge_texts"] = text_of([info_line(b"AF=" + t) for t in EDGE_TEXTS])
    c["host_texts"] = text_of([info_line(b"DP=1;AF=" + t + b";NS=3") for t in HOST_TEXTS])
    c["host_and_device_mixed"] = text_of([info_line(b"AF=" + t) for pair in zip(HOST_TEXTS, EDGE_TEXTS) for t in pair])
    rng = np.random.default_rng(29)
    c["random_values"] = text_of([info_line(b"NS=%d;AF=%s" % (i, random_value_text(rng)), pos=i + 1) for i in range(300)])
    c["no_data_line"] = HEADER
    c["empty_text"] = b""
    return c


def random_value_text(rng):
    """A text of the device's grammar, within its limits or just outside, whose value lies in [0, 1]."""
    n = int(rng.integers(1, 18))
    digits = b"".join(b"%d" % d for d in rng.integers(0, 10, size=n))
    shift = int(rng.integers(-6, 7))                       # value = 0.digits, written as (digits with a dot) e shift
    dot = int(rng.integers(0, n + 1))
    text = digits[:dot] + (b"." if dot < n or rng.random() < 0.3 else b"") + digits[dot:]
    exponent = -dot + min(shift, 0)
    if exponent or rng.random() < 0.2:
        text += (b"e" if rng.random() < 0.5 else b"E") + (b"%+d" if rng.random() < 0.5 else b"%d") % exponent
    return text


def _error_cases():
    """name -> (source, text, data line at fault, kind as the spec names it)"""
    ok_i, ok_g = info_line(b"AF=0.5"), gt_line([b"0|1", b"1|1"])
    e = {}
    e["af_above_one"] = ("info", text_of([ok_i, info_line(b"AF=1.5")]), 1, "value")
    e["af_above_one_by_an_ulp"] = ("info", text_of([info_line(b"AF=1.0000000000001")]), 0, "value")
    e["af_five_dot"] = ("info", text_of([ok_i, info_line(b"AF=5.")]), 1, "value")
    e["af_not_a_number"] = ("info", text_of([ok_i, ok_i, info_line(b"AF=abc")]), 2, "text")
    e["af_nan"] = ("info", text_of([ok_i, info_line(b"AF=nan")]), 1, "value")
    e["af_inf"] = ("info", text_of([info_line(b"AF=inf"), ok_i]), 0, "value")
    e["af_negative"] = ("info", text_of([ok_i, info_line(b"AF=-0.5")]), 1, "value")
    e["af_exponent_without_digits"] = ("info", text_of([ok_i, info_line(b"AF=1e")]), 1, "text")
    e["af_host_value_above_one"] = ("info", text_of([ok_i, info_line(b"AF=1.00000000000000001e1")]), 1, "value")
    e["lowest_of_several_info"] = ("info", text_of([ok_i, ok_i, info_line(b"AF=abc"), info_line(b"AF=1.5"), info_line(b"AF=7")]),
                                   2, "text")
    e["device_fault_before_host_fault"] = ("info", text_of([ok_i, info_line(b"AF=2"), info_line(b"AF=abc")]), 1, "value")
    e["format_without_gt"] = ("genotypes", text_of([ok_g, gt_line([b"0|1"], fmt=b"DP:GT")]), 1, "format")
    e["format_gtx"] = ("genotypes", text_of([gt_line([b"0|1"], fmt=b"GTX")]), 0, "format")
    e["format_g"] = ("genotypes", text_of([ok_g, ok_g, gt_line([b"0|1"], fmt=b"G")]), 2, "format")
    e["gt_empty_allele"] = ("genotypes", text_of([ok_g, gt_line([b"0|1", b"0|"])]), 1, "genotype")
    e["gt_letters"] = ("genotypes", text_of([gt_line([b"a|b"]), ok_g]), 0, "genotype")
    e["gt_empty"] = ("genotypes", text_of([ok_g, ok_g, ok_g, gt_line([b"0|1", b"", b"1|1"])]), 3, "genotype")
    e["gt_empty_before_subfield"] = ("genotypes", text_of([ok_g, gt_line([b":35"])]), 1, "genotype")
    e["gt_empty_last_sample"] = ("genotypes", text_of([ok_g, gt_line([b"0|1", b""])]), 1, "genotype")
    e["gt_ten_digits"] = ("genotypes", text_of([gt_line([b"0|1234567890"])]), 0, "genotype")
    e["gt_bad_beyond_first_step"] = ("genotypes", text_of([ok_g, gt_line([b"0|1"] * 400 + [b"0/x"] + [b"1|1"] * 30)]), 1,
                                     "genotype")
    e["gt_bad_on_a_window_s_last_byte"] = ("genotypes", text_of([ok_g, gt_line([b"0|1", b"0/1/1/x", b"1|1"])]), 1, "genotype")
    e["gt_bad_behind_a_window"] = ("genotypes", text_of([gt_line([b"0|1", b"0/1/1/0/x", b"1|1"]), ok_g]), 0, "genotype")
    e["gt_empty_allele_behind_a_window"] = ("genotypes", text_of([ok_g, ok_g, gt_line([b"0/1/1/0/"])]), 2, "genotype")
    e["lowest_of_several_genotypes"] = ("genotypes", text_of([ok_g, gt_line([b"0|1"] * 70 + [b"0|"]),
                                                              gt_line([b"0|1"], fmt=b"DP"), gt_line([b"x"])]), 1, "genotype")
    return e


GOOD_CASES = {"genotypes": _genotype_cases(), "info": _info_cases()}
ERROR_CASES = _error_cases()
