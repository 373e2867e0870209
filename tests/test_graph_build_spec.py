"""The graph-build spec (tests/spec_graph_build.py) checked without a device: against the synthetic generators of
graph.py, which assemble the same bubble chain from arrays; by spelling paths through the graphs it builds; and a census
of the case list, so that the GPU tests compare on inputs that reach every rule."""
import numpy as np
import pytest

import spec_graph_build as spec
from graph_build_cases import ERROR_CASES, GOOD_CASES, HEADER, RANDOM_CASES
from graph_kmer_index_amd.graph import synthetic_indel_graph, synthetic_snp_graph

LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def files_of_generated(g):
    """A `synthetic_snp_graph` / `synthetic_indel_graph` with unsplit segments written out as what it was generated
    from: (reference letters, VCF text, ref_af, alt_af).  Nodes come as segment, ref allele, alt allele, segment ...;
    a deletion and an insertion at site s are padded with the base before it, POS = s (1-based: that base)."""
    ref_alleles = np.flatnonzero(g.is_ref == 0) - 1
    reference = LETTERS[g.seq[np.repeat(g.is_ref != 0, g.node_size)]].tobytes()
    lines, ref_af, alt_af = [], [], []
    for r in ref_alleles.tolist():
        a = r + 1
        s = int(g.node_to_ref_offset[r - 1]) + int(g.node_size[r - 1])          # 0-based site = end of the segment before
        ref = LETTERS[g.get_numeric_node_sequence(r)].tobytes()
        alt = LETTERS[g.get_numeric_node_sequence(a)].tobytes()
        if len(ref) == len(alt):
            pos = s + 1
        else:
            pad = reference[s - 1:s]
            ref, alt, pos = pad + ref, pad + alt, s
        lines.append(b"1\t%d\t.\t%s\t%s\t.\t.\t.\n" % (pos, ref, alt))
        ref_af.append(g.allele_freq[r]), alt_af.append(g.allele_freq[a])
    return reference, HEADER + b"".join(lines), np.array(ref_af), np.array(alt_af)


@pytest.mark.parametrize("generator", [synthetic_snp_graph, synthetic_indel_graph])
def test_spec_reproduces_the_generators(generator):
    g = generator(20000, 300, 31, 77, max_node_len=2 ** 31 - 1)
    reference, text, ref_af, alt_af = files_of_generated(g)
    b = spec.build({"1": reference}, text, allele_frequencies=(ref_af, alt_af))
    assert np.all(b.line_status == 0)
    assert np.array_equal(b.node_size[1:], g.node_size) and b.node_size[0] == 0 and b.exists[0] == 0
    assert np.array_equal(b.seq, g.seq)
    assert np.array_equal(b.edge_start[1:], g.edge_start) and b.edge_start[0] == 0
    assert np.array_equal(b.edges, g.edges + 1)
    assert np.array_equal(b.is_ref[1:], g.is_ref)
    assert np.array_equal(b.allele_freq[1:], g.allele_freq)
    assert np.array_equal(b.node_to_ref_offset[1:], g.node_to_ref_offset)
    alts = np.flatnonzero(g.is_ref == 0)
    assert np.array_equal(b.var_nodes, alts + 1) and np.array_equal(b.ref_nodes, alts)
    assert b.chromosome_start_nodes == [1] and b.first_node == 1


def sites_of_text(reference, text):
    """(global lo, ref allele, alt allele) of every data line, worked out from the text alone; None where REF or ALT is
    not letters."""
    names, c0, at = list(reference), {}, 0
    for n in names:
        c0[n] = at
        at += len(reference[n])
    out = []
    for raw in text.split(b"\n"):
        if not raw.strip() or raw.startswith(b"#"):
            continue
        f = raw.rstrip(b"\r").split(b"\t")
        ref, alt, pos = f[3], f[4], int(f[1])
        if not ref or not alt or ref.strip(b"ACGTNacgtn") or alt.strip(b"ACGTNacgtn"):
            out.append(None)
        elif len(ref) != len(alt) and ref[:1].upper() == alt[:1].upper():
            out.append((c0[f[0].decode()] + pos, ref[1:], alt[1:]))
        else:
            out.append((c0[f[0].decode()] + pos - 1, ref, alt))
    return out


def kept_of_sites(reference, sites):
    """The lines the overlap rule keeps, from `sites_of_text` alone: one prefix maximum over the lines that are plain and
    have a base before them."""
    starts, at = set(), 0
    for n in reference:
        starts.add(at)
        at += len(reference[n])
    kept, reach = [], 0
    for i, site in enumerate(sites):
        if site is None or site[0] in starts:
            continue
        if site[0] >= reach:
            kept.append(i)
        reach = max(reach, site[0] + len(site[1]))
    return kept


def walk(b, start, take_alt):
    """The codes along the path from `start`.  A node with two successors stands before a site, [ref, alt]: the t-th
    such node of the walk takes the alt allele where take_alt[t] holds."""
    out, n, t = [], start, 0
    while True:
        out.extend(b.seq[seq_start(b)[n]:seq_start(b)[n + 1]].tolist())
        succ = b.edges[b.edge_start[n]:b.edge_start[n + 1]].tolist()
        if not succ:
            assert t == len(take_alt)
            return out
        if len(succ) == 2:
            n, t = succ[1 if take_alt[t] else 0], t + 1
        else:
            n = succ[0]


def seq_start(b):
    if not hasattr(b, "_seq_start"):
        b._seq_start = np.concatenate([[0], np.cumsum(b.node_size, dtype=np.int64)])
    return b._seq_start


def codes(letters):
    return [spec.CODE.get(c, 0) for c in letters]


@pytest.mark.parametrize("name", sorted(GOOD_CASES))
def test_paths_spell_the_reference_with_the_kept_alleles(name):
    reference, text = GOOD_CASES[name]
    b = spec.build(reference, text)
    sites = sites_of_text(reference, text)
    assert len(sites) == len(b.line_status)
    kept = kept_of_sites(reference, sites)
    assert kept == [i for i in range(len(sites)) if b.line_status[i] == 0]
    rng = np.random.default_rng(len(text))
    choices = [np.zeros(len(kept), dtype=bool)] + [rng.random(len(kept)) < 0.5 for _ in range(20)]
    names, at = list(reference), 0
    assert len(b.chromosome_start_nodes) == len(names)
    for c, n in enumerate(names):
        c0, c1 = at, at + len(reference[n])
        at = c1
        mine = [(j, i) for j, i in enumerate(kept) if c0 <= sites[i][0] - 1 < c1]    # lo - 1: a base of the chromosome
        for choice in choices:
            want, p, take_alt = [], c0, []
            for j, i in mine:
                lo, ref, alt = sites[i]
                assert lo >= p, "kept sites overlap"
                want.extend(codes(reference[n][p - c0:lo - c0]))
                want.extend(codes(alt if choice[j] else ref))
                take_alt.append(bool(choice[j]))
                p = lo + len(ref)
            want.extend(codes(reference[n][p - c0:]))
            assert walk(b, b.chromosome_start_nodes[c], take_alt) == want, (name, n)


def test_census_of_the_case_list():
    statuses, kinds = set(), set()
    for name, (reference, text) in GOOD_CASES.items():
        status = spec.build(reference, text).line_status
        statuses.update(status.tolist())
        if name in RANDOM_CASES:
            assert 2 * int(np.sum(status == 0)) >= len(status) and int(np.sum(status == 3)) >= 1, name
    assert statuses == {0, 1, 2, 3}
    for name, (reference, text, line, kind) in ERROR_CASES.items():
        with pytest.raises(spec.BuildError) as e:
            spec.build(reference, text)
        assert (e.value.line, e.value.kind) == (line, kind), name
        kinds.add(kind)
    assert kinds == {"fewer than five fields", "REF differs from the reference", "REF past the chromosome's end",
                     "POS outside the chromosome", "POS is not plain digits", "POS decreasing", "unknown chromosome", "chromosome in two runs",
                     "chromosome runs out of graph order"}
    assert all(name in GOOD_CASES for name in RANDOM_CASES)


def test_line_count_cases_sit_on_both_sides_of_the_scan_tile():
    kept = {}
    for name in ("lines_2047", "lines_2048", "lines_2049", "lines_2049_kept_2047"):
        status = spec.build(*GOOD_CASES[name]).line_status
        kept[name] = (len(status), int(np.sum(status == 0)))
    assert kept == {"lines_2047": (2047, 2047), "lines_2048": (2048, 2045), "lines_2049": (2049, 2049),
                    "lines_2049_kept_2047": (2049, 2047)}
