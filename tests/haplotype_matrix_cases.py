"""Named inputs of the haplotype matrix: VCF texts for the spec and the device with their ploidy and
n_samples argument, and the texts that must be refused with the data line and kind each is refused at.  Everything is
generated here, seeded, on top of vcf_af_cases' line builders.

A step of the kernel is W bytes (64 lanes x 16 bytes); offsets are counted from a line's first byte, which is where the
kernel's lanes start."""
import numpy as np

from vcf_af_cases import GT_FORMS, HEADER, W, gt_line, info_line, text_of

DIPLOID_FORMS = tuple(g for g in GT_FORMS if g.split(b":")[0].count(b"/") + g.split(b":")[0].count(b"|") <= 1)
THREE_BYTE_FORMS = (b"0|1", b"1/1", b".|1", b"2|0", b"0|0", b"./.", b"1|.")


def n_alleles(gt):
    return gt.split(b":")[0].replace(b"|", b"/").count(b"/") + 1


def header_of(n_samples):
    """A header whose #CHROM line names n_samples samples S0, S1, ..; without FORMAT when there is none."""
    if n_samples == 0:
        return HEADER
    return HEADER[:-1] + b"\tFORMAT" + b"".join(b"\tS%d" % i for i in range(n_samples)) + b"\n"


def pick(forms, n, seed):
    rng = np.random.default_rng([seed, 19])
    return [forms[i] for i in rng.integers(0, len(forms), size=n)]


def case(text, ploidy=2, n_samples=None):
    return {"text": text, "ploidy": ploidy, "n_samples": n_samples}


def _good_cases():
    c = {}
    c["samples_0"] = case(text_of([info_line(b"AF=0.5"), b"1\t9\t.\tA\tC", info_line(b".", b"\tDP")]))
    for n in (1, 2, 63, 64, 65, 300):                      # 300 samples: more than one step
        c["samples_%d" % n] = case(text_of([gt_line(pick(DIPLOID_FORMS, n, n)), gt_line(pick(DIPLOID_FORMS, n, n + 1000), 14)],
                                           header=header_of(n)))
    # 4-byte samples from the ninth tab on: over at = 14 .. 30 a GT starts at every byte of a lane's 16, and GTs straddle
    # a lane's end and a step's end at each of their bytes; the second line has GTs of every length
    for at in range(14, 31):
        c["ninth_tab_at_%d" % at] = case(text_of([gt_line(pick(THREE_BYTE_FORMS, 300, at), at),
                                                  gt_line(pick(DIPLOID_FORMS, 300, at + 100), at)], header=header_of(300)))
    c["ninth_tab_around_a_step"] = case(text_of([gt_line(pick(DIPLOID_FORMS, 5, at), at) for at in (W - 1, W, W + 1)],
                                                header=header_of(5)))
    for ploidy in (1, 2, 3):
        forms = [g for g in GT_FORMS if n_alleles(g) <= ploidy]
        lines = [gt_line(forms[i:] + forms[:i]) for i in range(len(forms))]
        c["every_gt_form_p%d" % ploidy] = case(text_of(lines, header=header_of(len(forms))), ploidy)
    long_gts = [b"10|11", b"0/1/1", b"123456789|0", b"0|1:" + b"9" * 40, b"0/1/1:35:1,2,3,4,5,6", b"12345678", b"1234567|1",
                b"0000001|1|0", b"./.|.", b"1"]
    c["gts_longer_than_a_window"] = case(text_of([gt_line(long_gts), gt_line(long_gts[::-1], 21)],
                                                 header=header_of(len(long_gts))), 3)
    octoploid = [b"0/1/2/3/4/5/6/7", b"1|1|1|1|0|0|0|0", b".", b"0|1", b"./././././././.", b"10/0/10/1/0/1/0/1:7"]
    c["ploidy_8"] = case(text_of([gt_line(octoploid), gt_line(octoploid[::-1], 30)], header=header_of(len(octoploid))), 8)
    c["gt_in_the_piece_s_last_bytes"] = case(text_of([gt_line([b"0|1", b"1|1"]), gt_line([b"0|0", b"1"])], last_end=b"",
                                                     header=header_of(2)))
    c["last_line_unterminated_long"] = case(text_of([gt_line(pick(DIPLOID_FORMS, 300, 5))], last_end=b"", header=header_of(300)))
    c["crlf"] = case(text_of([gt_line([b"0|1", b"1|1"]), gt_line([b"1/1", b"1"])], end=b"\r\n",
                             header=header_of(2).replace(b"\n", b"\r\n")))
    c["header_only"] = case(header_of(3))
    c["empty_text"] = case(b"")
    c["s_from_the_header"] = case(text_of([gt_line([b"0|1", b"1|0", b"."])], header=header_of(3)))
    c["s_from_the_last_chrom_line"] = case(text_of([gt_line([b"0|1", b"1|0"])], header=header_of(5) + header_of(2)))
    c["s_from_the_first_data_line"] = case(text_of([gt_line([b"0|1", b"1|0", b".", b"1/1"]), gt_line([b"1|1"] * 4)]))
    c["s_from_the_argument"] = case(text_of([gt_line([b"0|1", b"1|0"]), gt_line([b"1|1", b"0/0"])]), n_samples=2)
    c["s_from_the_argument_with_names"] = case(text_of([gt_line([b"0|1", b"1|0"])], header=header_of(2)), n_samples=2)
    c["s_0_from_the_argument"] = case(text_of([info_line(b"AF=0.5")], header=header_of(2)), n_samples=0)
    c["all_missing"] = case(text_of([gt_line([b".", b"./.", b".|.:3"]), gt_line([b"0|1", b".", b"."])], header=header_of(3)))
    c["haploid"] = case(text_of([gt_line([b"1", b"0", b".", b"2:5"]), gt_line([b"0"] * 4)], header=header_of(4)), 1)
    rng = np.random.default_rng(31)
    mixed = [gt_line(pick(DIPLOID_FORMS, 37, 200 + i), int(rng.integers(16, 80)), pos=i + 1) for i in range(200)]
    mixed[10:10] = [b"#a comment line", b"", b" \t ", b"#CHROM\tnot\tthe\theader\tany\tmore\t.\t.\t.\tX\tY"]
    c["mixed_file"] = case(text_of(mixed, header=header_of(37)))
    return c


def _error_cases():
    """name -> (case, data line at fault, kind)"""
    ok = gt_line([b"0|1", b"1|1"])
    h = header_of(2)
    e = {}
    e["format_without_gt"] = (case(text_of([ok, gt_line([b"0|1", b"1|1"], fmt=b"DP:GT")], header=h)), 1, 2)
    e["format_gtx"] = (case(text_of([gt_line([b"0|1", b"1|1"], fmt=b"GTX"), ok], header=h)), 0, 2)
    e["gt_letters"] = (case(text_of([ok, ok, gt_line([b"a|b", b"0|1"])], header=h)), 2, 3)
    e["gt_empty"] = (case(text_of([ok, gt_line([b"0|1", b""])], header=h)), 1, 3)
    e["gt_empty_allele_behind_a_window"] = (case(text_of([ok, gt_line([b"0/1/1/0/", b"0|1"])], header=h), 8), 1, 3)
    e["gt_bad_beyond_the_first_step"] = (case(text_of([gt_line([b"0|1"] * 300), gt_line([b"0|1"] * 290 + [b"0/x"] + [b"1|1"] * 9)],
                                                      header=header_of(300))), 1, 3)
    e["one_column_too_few"] = (case(text_of([ok, gt_line([b"0|1"])], header=h)), 1, 4)
    e["one_column_too_many"] = (case(text_of([ok, ok, gt_line([b"0|1", b"1|1", b"0|0"])], header=h)), 2, 4)
    e["many_columns_too_many"] = (case(text_of([ok, gt_line([b"0|1"] * 300)], header=h)), 1, 4)
    e["sites_only_line"] = (case(text_of([ok, info_line(b"AF=0.5"), ok], header=h)), 1, 4)
    e["format_without_samples"] = (case(text_of([ok, info_line(b".", b"\tGT")], header=h)), 1, 4)
    e["samples_where_none_are_expected"] = (case(text_of([info_line(b"."), ok]), n_samples=0), 1, 4)
    e["triploid_gt_in_a_diploid_file"] = (case(text_of([ok, gt_line([b"0|1", b"0/1/1"])], header=h)), 1, 5)
    e["diploid_gt_in_a_haploid_file"] = (case(text_of([gt_line([b"1", b"0|1"]), gt_line([b"1", b"0"])], header=h), 1), 0, 5)
    e["nine_alleles"] = (case(text_of([ok, gt_line([b"0|1", b"0/1/0/1/0/1/0/1/0"])], header=h), 8), 1, 5)
    e["lowest_of_two_lines"] = (case(text_of([ok, gt_line([b"0|1", b"0/1/1"]), gt_line([b"0|1", b"1|1"], fmt=b"DP"), ok],
                                             header=h)), 1, 5)
    e["lowest_of_two_lines_beyond_a_step"] = (case(text_of([gt_line([b"0|1"] * 300), gt_line([b"0|1"] * 299 + [b"0|"]),
                                                            gt_line([b"0|1"] * 300, fmt=b"DP"), gt_line([b"x"] * 300)],
                                                           header=header_of(300))), 1, 3)
    e["format_and_gt_on_one_line"] = (case(text_of([ok, gt_line([b"0|1", b"x"], fmt=b"DP")], header=h)), 1, 2)
    e["gt_and_ploidy_on_one_line"] = (case(text_of([gt_line([b"0/1/1", b"0|"]), ok], header=h)), 0, 3)
    e["columns_and_ploidy_on_one_line"] = (case(text_of([ok, gt_line([b"0|1", b"1|1", b"0/1/1"])], header=h)), 1, 4)
    e["gt_and_columns_on_one_line"] = (case(text_of([ok, gt_line([b"0|1", b"1|1", b"x"])], header=h)), 1, 3)
    return e


GOOD_CASES = _good_cases()
ERROR_CASES = _error_cases()
# the input of the C ABI's guard-byte check: good lines, lines at fault of every kind and the S + 1 columns line among them
GUARD_TEXT = text_of([gt_line([b"0|1", b"1/1"]), gt_line([b"0|1", b"1|1", b"0|0"]), gt_line(pick(DIPLOID_FORMS, 2, 3), 30),
                      info_line(b"AF=0.5"), gt_line([b"0|1", b"0/1/1"]), gt_line([b"x", b"0|1"]), gt_line([b"1|1", b"."])],
                     header=header_of(2), last_end=b"")
