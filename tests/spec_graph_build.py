"""The rules of DESIGN.md 4.15 (include/gki.h, "graph build") as plain Python loops over lines and nodes: reference
letters and VCF text in, the arrays of graph.py, variant-to-nodes and the status of every data line out.  No NumPy
tricks and no device: this is the oracle of tests/test_gpu_graph_build.py, itself checked against the synthetic
generators and by spelling paths (tests/test_graph_build_spec.py)."""
import numpy as np

KEPT, NOT_PLAIN, NO_BASE_BEFORE, OVERLAP = 0, 1, 2, 3
STRIP_BYTES = frozenset([0x20] + list(range(0x09, 0x0E)) + list(range(0x1C, 0x20)))      # str.strip() of ASCII text
PLAIN = frozenset(b"ACGTNacgtn")
CODE = {ord("c"): 1, ord("C"): 1, ord("g"): 2, ord("G"): 2, ord("t"): 3, ord("T"): 3}      # encode_letters


class BuildError(ValueError):
    """What the build raises; `line` is the data line at fault (from 0 in the file), `kind` names the rule."""

    def __init__(self, kind, line):
        super().__init__("%s at data line %d" % (kind, line))
        self.kind, self.line = kind, line


class SpecBuild:
    pass


def data_lines(text):
    """The data lines of DESIGN 4.14 as lists of fields: every '\\r' at a line's end dropped, lines that begin with '#'
    or hold nothing but strip bytes skipped, the rest split at tabs."""
    out = []
    for line in bytes(text).split(b"\n"):
        while line.endswith(b"\r"):
            line = line[:-1]
        if not line or line[0] == ord("#") or all(c in STRIP_BYTES for c in line):
            continue
        out.append(line.split(b"\t"))
    return out


def upper(c):
    return c - 32 if ord("a") <= c <= ord("z") else c


def is_plain(allele):
    return len(allele) > 0 and all(c in PLAIN for c in allele)


def build(reference, text, chromosomes=None, allele_frequencies=None):
    names = [n for n in reference] if chromosomes is None else list(chromosomes)
    letters, c0, c1 = [], [], []
    for n in names:
        c0.append(len(letters))
        letters.extend(bytes(reference[n]))
        c1.append(len(letters))
    lines = data_lines(text)

    # ---- lines -> sites
    status, lo, ref_allele, alt_allele, chrom_of = [], [], [], [], []
    seen, run_chrom, run_name, last_pos = set(), -1, None, 0
    for i, f in enumerate(lines):
        if len(f) < 5:
            raise BuildError("fewer than five fields", i)
        pos_text = f[1]
        if not (1 <= len(pos_text) <= 18 and all(ord("0") <= c <= ord("9") for c in pos_text)):
            raise BuildError("POS is not plain digits", i)
        pos = int(pos_text)
        name = f[0].decode("utf-8", "replace")
        if name != run_name:
            if name not in names:
                raise BuildError("unknown chromosome", i)
            if name in seen:
                raise BuildError("chromosome in two runs", i)
            if names.index(name) < run_chrom:
                raise BuildError("chromosome runs out of graph order", i)
            seen.add(name)
            run_name, run_chrom, last_pos = name, names.index(name), 0
        c = run_chrom
        if pos < 1 or pos > c1[c] - c0[c]:
            raise BuildError("POS outside the chromosome", i)
        if pos < last_pos:
            raise BuildError("POS decreasing", i)
        last_pos = pos
        ref, alt = f[3], f[4]
        if is_plain(ref):
            at = c0[c] + pos - 1
            if at + len(ref) > c1[c]:
                raise BuildError("REF past the chromosome's end", i)
            for j in range(len(ref)):
                if upper(ref[j]) != upper(letters[at + j]):
                    raise BuildError("REF differs from the reference", i)
        chrom_of.append(c)
        if not (is_plain(ref) and is_plain(alt)):
            status.append(NOT_PLAIN), lo.append(0), ref_allele.append(b""), alt_allele.append(b"")
            continue
        if len(ref) != len(alt) and upper(ref[0]) == upper(alt[0]):
            ref, alt, start = ref[1:], alt[1:], c0[c] + pos
        else:
            start = c0[c] + pos - 1
        lo.append(start), ref_allele.append(ref), alt_allele.append(alt)
        status.append(NO_BASE_BEFORE if start == c0[c] else KEPT)

    # ---- overlap: one prefix maximum over the well-formed lines
    reach = 0
    for i in range(len(lines)):
        if status[i] != KEPT:
            continue
        if lo[i] < reach:
            status[i] = OVERLAP
        reach = max(reach, lo[i] + len(ref_allele[i]))

    # ---- nodes, element by element; an element is (entry nodes, all nodes)
    node_size, node_seq, is_ref, af, ntro, successors = [0], [[]], [0], [1.0], [0], [[]]
    exists = [0]
    ref_nodes, var_nodes = [0] * len(lines), [0] * len(lines)
    chromosome_start_nodes = []

    def add(seq, linear, freq, offset):
        node_size.append(len(seq)), node_seq.append([CODE.get(c, 0) for c in seq]), is_ref.append(1 if linear else 0)
        af.append(freq), ntro.append(offset), successors.append([]), exists.append(1)
        return len(node_size) - 1

    for c in range(len(names)):
        elements, at = [], c0[c]
        for i in range(len(lines)):
            if status[i] != KEPT or chrom_of[i] != c:
                continue
            if lo[i] > at:
                g = add(letters[at:lo[i]], True, 1.0, at)
                elements.append([g])
            hi = lo[i] + len(ref_allele[i])
            ref_af, alt_af = (1.0, 1.0) if allele_frequencies is None else (float(allele_frequencies[0][i]),
                                                                           float(allele_frequencies[1][i]))
            r = add(letters[lo[i]:hi], True, ref_af, lo[i])
            a = add(alt_allele[i], False, alt_af, 0)
            ref_nodes[i], var_nodes[i] = r, a
            elements.append([r, a])
            at = hi
        if c1[c] > at:
            elements.append([add(letters[at:c1[c]], True, 1.0, at)])
        for e, nxt in zip(elements[:-1], elements[1:]):
            for n in e:
                successors[n] = list(nxt)
        chromosome_start_nodes.append(elements[0][0])

    n_nodes = len(node_size)
    predecessors = [[] for _ in range(n_nodes)]
    for n in range(n_nodes):                       # ascending source id
        for m in successors[n]:
            predecessors[m].append(n)

    def csr(lists):
        start, flat = [0], []
        for lst in lists:
            flat.extend(lst)
            start.append(len(flat))
        return np.array(start, dtype=np.int64), np.array(flat, dtype=np.int32)

    out = SpecBuild()
    out.node_size = np.array(node_size, dtype=np.int32)
    out.seq = np.array([c for s in node_seq for c in s], dtype=np.uint8)
    out.edge_start, out.edges = csr(successors)
    out.rev_start, out.rev_edges = csr(predecessors)
    out.is_ref = np.array(is_ref, dtype=np.uint8)
    out.allele_freq = np.array(af, dtype=np.float64)
    out.exists = np.array(exists, dtype=np.uint8)
    out.node_to_ref_offset = np.array(ntro + [0], dtype=np.int64)
    out.chromosome_start_nodes = chromosome_start_nodes
    out.first_node = 1
    out.ref_nodes = np.array(ref_nodes, dtype=np.uint32)
    out.var_nodes = np.array(var_nodes, dtype=np.uint32)
    out.line_status = np.array(status, dtype=np.uint8)
    return out
