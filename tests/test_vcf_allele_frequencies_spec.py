"""The allele-frequency rules (tests/spec_vcf_allele_frequencies.py) against hand-written expectations; a
census that tests/vcf_af_cases.py holds every route, every error kind and every boundary the device tests rely on; and
the fast-path claim itself: the device's one-operation rule, restated in NumPy doubles, equals float() bit for bit."""
import numpy as np
import pytest

import spec_vcf_allele_frequencies as spec
from vcf_af_cases import EDGE_TEXTS, ERROR_CASES, GOOD_CASES, HEADER, HOST_TEXTS, W, gt_line, info_line, random_value_text, text_of


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def test_info_by_hand():
    text = text_of([info_line(b"DP=3;AF=0.25;NS=2"), info_line(b"XAF=0.5;AF_EUR=0.1"), info_line(b"AF=0.1,0.7"),
                    info_line(b"AF=."), b"1\t9\t.\tA\tC\t.\tPASS", info_line(b"AF=0.12345678901234567"),
                    info_line(b"AF=1e-05", b"\tGT\t1|1")], end=b"\r\n")
    ref_af, alt_af, route = spec.allele_frequencies(text, "info")
    assert route.tolist() == [0, 1, 0, 1, 1, 2, 0]
    assert alt_af.tolist() == [0.25, 1.0, 0.1, 1.0, 1.0, 0.12345678901234567, 1e-05]
    assert ref_af.tolist() == [0.75, 1.0, 1.0 - 0.1, 1.0, 1.0, 1.0 - 0.12345678901234567, 1.0 - 1e-05]


def test_genotypes_by_hand():
    text = text_of([gt_line([b"0|1", b"1/1", b"./.", b".|1"]),        # called 5: one 0, four 1
                    gt_line([b"0/1/1", b"2|0", b"10|1", b"01|1:9:."]), # called 9: two 0, five 1 (10 is allele ten)
                    gt_line([b".", b"./."]), info_line(b"AF=0.5"), gt_line([b"1"]),
                    gt_line([b"0|0"], fmt=b"GT:DP")], last_end=b"")
    ref_af, alt_af, route = spec.allele_frequencies(text, "genotypes")
    assert route.tolist() == [0, 0, 1, 1, 0, 0]
    assert ref_af.tolist() == [1 / 5, 2 / 9, 1.0, 1.0, 0.0, 1.0]
    assert alt_af.tolist() == [4 / 5, 5 / 9, 1.0, 1.0, 1.0, 0.0]


def test_lines_are_numbered_as_the_vcf_parse_numbers_them():
    import spec_vcf_parse
    for cases in GOOD_CASES.values():
        for name, text in cases.items():
            assert len(spec.data_lines(text)) == len(spec_vcf_parse.parse(text)["positions"]), name


@pytest.mark.parametrize("name", sorted(ERROR_CASES))
def test_error_case_names_the_lowest_line(name):
    source, text, line, kind = ERROR_CASES[name]
    with pytest.raises(spec.AfError) as e:
        spec.allele_frequencies(text, source)
    assert (e.value.line, e.value.kind) == (line, kind)


def test_census_of_the_cases():
    routes = {source: np.concatenate([spec.allele_frequencies(t, source)[2] for t in cases.values()])
              for source, cases in GOOD_CASES.items()}
    assert set(routes["info"].tolist()) == {0, 1, 2} and set(routes["genotypes"].tolist()) == {0, 1}
    assert {(s, k) for s, _, _, k in ERROR_CASES.values()} == {("info", "value"), ("info", "text"), ("genotypes", "format"),
                                                               ("genotypes", "genotype")}
    # a device fault and a host fault in one text, either one the lower
    assert {"lowest_of_several_info", "device_fault_before_host_fault", "lowest_of_several_genotypes"} <= set(ERROR_CASES)
    lines = [l for t in GOOD_CASES["genotypes"].values() for l in t[len(HEADER):].split(b"\n") if l.count(b"\t") >= 9]

    def nth_tab(l, n):
        return [i for i, c in enumerate(l) if c == 9][n - 1]
    assert {15, 16, W - 1, W} <= {nth_tab(l, 9) for l in lines}
    assert {W - 1, W, W + 1} <= {len(l) for l in lines}
    assert {1, 2, 63, 64, 65, 300} <= {l.count(b"\t") - 8 for l in lines}
    # a GT over a lane's end and over a step's end: its first byte on one side, its last on the other
    starts = [(i + 1, l) for l in lines for i, c in enumerate(l) if c == 9 and l[:i].count(b"\t") >= 8]
    assert any(p % 16 == 15 and l[p:p + 3] in (b"0|1", b"1|1", b"1|0") for p, l in starts)
    assert any(p == W - 1 and l[p:p + 3] in (b"0|1", b"1|1", b"1|0") for p, l in starts)
    texts = list(GOOD_CASES["genotypes"].values())
    assert any(t.endswith(b"\r\n") for t in texts) and any(not t.endswith(b"\n") and t for t in texts)
    info_entries = b"".join(GOOD_CASES["info"].values())
    for needle in (b"\tAF=0.25;", b";AF=0.5\n", b"\tAF=0.75\n", b"XAF=", b"MAF=", b"AF_EUR=", b"AF=0.1,0.2", b"AF=.\n", b"AF=\n"):
        assert needle in info_entries, needle
    for t in EDGE_TEXTS + HOST_TEXTS:
        assert b"AF=" + t in info_entries


CPU_EDGE_TEXTS = (b"0", b"1", b"1.0", b".5", b"5.", b"1e-05", b"1E-5", b"0.000199681", b"123456789012345", b"0.12345678901234",
                  b"1234567890123456", b"0.123456789012345", b"1e22", b"1e-22", b"123456789012345e22", b"0.00000000000001e-8",
                  b"1e23", b"1e-23", b"0.1e-22", b"1.5e23")


def test_device_rule_on_the_edge_texts():
    device = {t: spec.device_value(t) for t in CPU_EDGE_TEXTS + EDGE_TEXTS}
    outside = {b"1234567890123456", b"0.123456789012345", b"1e23", b"1e-23", b"0.1e-22"}      # 16 digits, |q| = 23
    assert {t for t, v in device.items() if v is None} == outside
    for t, v in device.items():
        if v is not None:
            assert bits(v) == bits(float(t)), t
    for t in HOST_TEXTS + (b"nan", b"inf", b"-1", b"abc", b"", b".", b"e5", b"1e", b"1e+", b"1.2.3", b"1e0005", b"0x10"):
        assert spec.device_value(t) is None, t


def random_grammar_text(rng):
    """Any text of the device's grammar within its limits: 1 to 15 mantissa digits, the dot anywhere, |q| <= 22."""
    n = int(rng.integers(1, 16))
    digits = b"".join(b"%d" % d for d in rng.integers(0, 10, size=n))
    dot = int(rng.integers(0, n + 1))
    fraction = n - dot
    q = int(rng.integers(-22, 23))
    exponent = q + fraction
    text = digits[:dot] + (b"." if fraction or rng.random() < 0.3 else b"") + digits[dot:]
    if exponent or rng.random() < 0.3:
        text += (b"e", b"E")[int(rng.integers(0, 2))] + (b"%+d", b"%d", b"%03d")[int(rng.integers(0, 3))] % exponent
    return text


def test_device_rule_equals_float_on_random_texts():
    rng = np.random.default_rng(4017)
    texts = [random_grammar_text(rng) for _ in range(100000)] + [random_value_text(rng) for _ in range(20000)]
    parsed = 0
    for t in texts:
        v = spec.device_value(t)
        if v is not None:
            parsed += 1
            assert bits(v) == bits(float(t)), t
    assert parsed >= 100000
