"""The CPU restatement (tests/spec_unique_variant_kmers.py) against the reference's own UniqueVariantKmersFinder output
(tests/golden/uvk_reference.json.gz), and checks that the stored cases exercise every selection rule."""
import numpy as np
import pytest

import spec_unique_variant_kmers as spec
from uvk_golden import load_cases, case_graph, case_frequency, expected, chromosome_offsets

CASES = load_cases()


def _spec(case):
    g = case_graph(case)
    v = case["variants"]
    return spec.unique_variant_kmers(g, np.array(case["ref_nodes"]), np.array(case["var_nodes"]), v["positions"],
                                     v["lines"], case["k"], case["max_variant_nodes"], case_frequency(case),
                                     case["lowest"], case["chunk_size"], chromosome_offsets(case, g))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_spec_equals_reference(case):
    if case["name"] == "over_500_windows":
        with pytest.raises(NotImplementedError):          # the spec has no window ids; the GPU test pins this case
            _spec(case)
        return
    got = _spec(case)
    for a, b in zip(got, expected(case)):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def test_cases_bite():
    by = {c["name"]: c for c in CASES}
    for name in ("snp_del_repeats", "k15", "m3", "two_chromosomes"):
        lo, fi = expected(by[name + "_lowest"]), expected(by[name + "_first"])
        assert not all(len(a) == len(b) and np.array_equal(a, b) for a, b in zip(lo, fi)), name
    assert max(by["shared_nodes_chunk_None"]["index"]["counts"]) > 1
    outs = [expected(by["shared_nodes_chunk_%s" % c]) for c in ("None", "2", "5")]
    assert len(outs[0][0]) != len(outs[1][0]) or not np.array_equal(outs[0][0], outs[1][0])
    assert len(expected(by["over_500_windows"])[0]) > 500
    assert 2 in by["two_chromosomes_lowest"]["variants"]["chromosomes"]


def _per_start(case):
    """(shared, score) of every start of every variant with both nodes stored."""
    from oracle import oracle
    g = case_graph(case)
    freq = case_frequency(case)
    offs = chromosome_offsets(case, g)
    out = []
    for i, (pos, line) in enumerate(zip(case["variants"]["positions"], case["variants"]["lines"])):
        ref, alt = case["ref_nodes"][line], case["var_nodes"][line]
        if ref == 0 or alt == 0:
            continue
        row = []
        for d in spec.start_distances(case["k"]):
            node, off = spec.node_at_ref_offset(g, offs[i] + pos - d)
            rec = oracle.find_from_position(g, case["k"], node, off, False, case["max_variant_nodes"])
            kr = {int(h) for h, n in zip(rec["kmers"], rec["nodes"]) if n == ref}
            ka = {int(h) for h, n in zip(rec["kmers"], rec["nodes"]) if n == alt}
            row.append((bool(kr & ka), max([0] + [freq(h) for h, n in zip(rec["kmers"], rec["nodes"]) if n in (ref, alt)])))
        out.append(row)
    return out


def test_cases_hit_shared_hashes_and_hidden_zeros():
    case = {c["name"]: c for c in CASES}["snp_del_repeats_lowest"]
    rows = _per_start(case)
    assert any(s for row in rows for s, _ in row[:-1])                      # rule 5 rejects a start
    assert any(sc > 1 for row in rows for _, sc in row)                     # frequencies above 1 are probed
    hidden = 0
    for row in rows:
        valid = [sc for s, sc in row[:-1] if not s] + [row[-1][1]]
        for j, sc in enumerate(valid):
            if sc <= 1:
                hidden += sc == 1 and 0 in valid[j + 1:]
                break
    assert hidden > 0                                                       # a break hides a later zero
