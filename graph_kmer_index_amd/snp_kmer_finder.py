"""SnpKmerFinder on a linear reference (snp_kmer_finder.py:29-104, :298-318) and the chunked form of `make -R`
(command_line_interface.py:105-153), on the device through gki_linear_kmers.

The search over a SNP graph (snp_kmer_finder.py:117-290) is not ported: DenseKmerFinder covers graphs.  With
`reference=` the records are the k-mers at start_position, start_position + spacing, ... up to and including
end_position, clipped at the sequence's last whole k-mer like the reference's slice `reference[start:end + k]`.

One deliberate difference: the reference's `_ref_offsets` is `arange(start, start + len(slice), spacing)`, longer than
`_hashes` (FlatKmers never checks); here there is one offset per record, the record's position."""
import ctypes as C
import logging
import numpy as np

from . import _lib
from .flat_kmers import DeviceFlatKmers


class NoReferenceSequence(AssertionError):
    """An interval with no whole k-mer inside the sequence: where the reference's `assert len(reference_sequence) > 0`
    fails (snp_kmer_finder.py:302), or where fewer than k bases are left and its np.convolve returns nonsense."""


def reference_to_letters(reference):
    """str, bytes, a uint8 array, or anything whose full slice gives one of them -> uint8 array of ASCII letters."""
    if isinstance(reference, np.ndarray):
        if reference.dtype == np.uint8:
            return np.ascontiguousarray(reference)
        if reference.dtype.kind in "US":
            reference = "".join(str(x) for x in reference.tolist())
        else:
            raise TypeError("reference array must be uint8 letters, not %s" % reference.dtype)
    if isinstance(reference, str):
        reference = reference.encode("ascii", "replace")          # a non-ASCII letter is no c/g/t: code 0 either way
    if isinstance(reference, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(reference), dtype=np.uint8)
    return reference_to_letters(str(reference[:]))               # a FASTA record object (pyfaidx-like)


def read_fasta_records(file_name, names=None):
    """(names, bases): the records `names` of a FASTA file (None: every record, in file order), each as one uint8 array
    with line ends stripped, from ONE read of the file.  A record's name is the first word of its `>` line.  No .fai.
    A name ending in .gz (gzip or BGZF) is inflated by Python's gzip.  This is the host route; `fasta_files` has the
    device's."""
    from .text_files import open_reads_file
    with open_reads_file(file_name) as f:
        data = f.read()
    buf = np.frombuffer(data, dtype=np.uint8)
    gt = np.flatnonzero(buf == ord(">"))
    gt = gt[(gt == 0) | (buf[gt - 1] == 10)]                     # a `>` that begins a line
    found, bodies = [], {}
    for i, g in enumerate(gt.tolist()):
        eol = data.find(b"\n", g)
        eol = len(data) if eol < 0 else eol
        words = data[g + 1:eol].split()
        found.append(words[0].decode("ascii", "replace") if words else "")
        bodies.setdefault(found[-1], (min(eol + 1, len(data)), int(gt[i + 1]) if i + 1 < len(gt) else len(data)))
    names = found if names is None else list(names)
    out = []
    for name in names:
        if name not in bodies:
            raise KeyError("no record %r in %s (records: %s)" % (name, file_name, ", ".join(found)))
        body = buf[bodies[name][0]:bodies[name][1]]
        out.append(np.ascontiguousarray(body[(body != 10) & (body != 13)]))
    return names, out


def read_fasta_record(file_name, name):
    """The bases of record `name` (the first word of its `>` line) as one uint8 array, line ends stripped.  No .fai."""
    return read_fasta_records(file_name, [name])[1][0]


def chunk_intervals(genome_size, spacing, threads):
    """The intervals of `make -t N` (command_line_interface.py:120-131): 10 * N of them, each ending on the position the
    next one starts with."""
    n_jobs = int(threads) * 10
    per = (int(genome_size) // int(spacing)) // n_jobs
    return [(per * i * spacing, per * (i + 1) * spacing) for i in range(n_jobs)]


def segments_of_intervals(intervals, n_letters, k, spacing):
    """(first position, record count) of every inclusive interval [start, end], clipped at the sequence's last whole k-mer
    as the reference's slice clips it (snp_kmer_finder.py:301)."""
    first = np.zeros(len(intervals), dtype=np.int64)
    count = np.zeros(len(intervals), dtype=np.int64)
    for i, (start, end) in enumerate(intervals):
        length = min(int(end) + k, n_letters) - int(start)       # len(reference[start:end + k])
        if start < 0 or length < k:
            raise NoReferenceSequence(
                "no whole %d-mer between positions %d and %d: the sequence has %d letters (is the genome size, -G, larger "
                "than the sequence?)" % (k, start, int(end) + k, n_letters))
        first[i] = start
        count[i] = (length - k) // spacing + 1
    return first, count


def linear_kmers_on_device(letters, k, spacing, seg_first, seg_count, with_reverse_complement=False, hashes_only=False,
                           kernel_ms=None):
    """gki_linear_kmers on a DeviceArray of letters: a DeviceFlatKmers, or with hashes_only the hashes' DeviceArray.
    kernel_ms: a list that receives (pack ms, emit ms)."""
    lib = _lib.load()
    seg_first = np.ascontiguousarray(seg_first, dtype=np.int64)
    seg_count = np.ascontiguousarray(seg_count, dtype=np.int64)
    n_out = C.c_int64(0)
    args = (letters.ptr, letters.n, int(k), int(spacing), _lib.hptr(seg_first), _lib.hptr(seg_count), len(seg_first),
            int(bool(with_reverse_complement)))
    _lib.check(lib.gki_linear_kmers(*args, None, None, None, None, 0, C.byref(n_out), None))
    n = n_out.value
    ms = (C.c_float * 2)() if kernel_ms is not None else None
    with _lib.DeviceScope() as s:
        if hashes_only:
            out = s.array(n, np.uint64)
            cols = (out.ptr, None, None, None)
        else:
            out = s.keep(DeviceFlatKmers.allocate(n))
            cols = (out.hashes.ptr, out.nodes.ptr, out.ref_offsets.ptr, out.allele_frequencies.ptr)
        _lib.check(lib.gki_linear_kmers(*args, *cols, max(n, 1), C.byref(n_out), ms))
        assert n_out.value == n
        s.release(out)
    if kernel_ms is not None:
        kernel_ms[:] = [ms[0], ms[1]]
    return (out, n) if hashes_only else out


def make_linear_reference_flat_on_device(reference, k, spacing, genome_size, threads=1, include_reverse_complement=False,
                                         kernel_ms=None):
    """`make -R` (command_line_interface.py:105-153) as one device call: the reference's 10 * threads chunks in order, each
    followed by its own reverse complements when asked for."""
    if not isinstance(reference, _lib.DeviceArray):
        _lib.require_device()
        reference = reference_to_letters(reference)
        if reference.size == 0:
            raise NoReferenceSequence("the reference sequence is empty")
    with _lib.DeviceScope() as s:
        letters = s.on_device(reference, np.uint8)
        first, count = segments_of_intervals(chunk_intervals(genome_size, spacing, max(1, int(threads))), letters.n, k, spacing)
        return linear_kmers_on_device(letters, k, spacing, first, count, include_reverse_complement, kernel_ms=kernel_ms)


class SnpKmerFinder:
    """The reference's constructor (snp_kmer_finder.py:34-37).  Only the linear-reference mode is implemented."""

    def __init__(self, graph, k=15, spacing=None, include_reverse_complements=False, pruning=False,
                 max_kmers_same_position=100000, max_frequency=10000, max_variant_nodes=10000, only_add_variant_kmers=False,
                 whitelist=None, only_save_variant_nodes=False, start_position=None, end_position=None, only_store_nodes=None,
                 skip_kmers_with_nodes=None, only_save_one_node_per_kmer=False, reference=None, variant_to_nodes=None,
                 node_to_variants=None, haplotype_matrix=None):
        self.graph = graph
        self.reference = reference
        self.k = k
        self.spacing = k if spacing is None else spacing
        self._start_position = 0 if start_position is None else start_position
        self._end_position = end_position
        self._include_reverse_complements = include_reverse_complements      # unused on a linear reference, as in the reference
        self.pruning = pruning
        self._max_kmers_same_position = max_kmers_same_position
        self._max_frequency = max_frequency
        self._max_variant_nodes = max_variant_nodes
        self._only_add_variant_kmers = only_add_variant_kmers
        self._whitelist = whitelist
        self._only_save_variant_nodes = only_save_variant_nodes
        self._only_store_nodes = only_store_nodes
        self._skip_kmers_with_nodes = skip_kmers_with_nodes
        self._only_save_one_node_per_kmer = only_save_one_node_per_kmer
        self.variant_to_nodes = variant_to_nodes
        self.node_to_variants = node_to_variants
        self.haplotype_matrix = haplotype_matrix

    def find_kmers_on_device(self):
        """DeviceFlatKmers of the k-mers at start_position, start_position + spacing, ... <= end_position."""
        if self.reference is None:
            raise NotImplementedError("SnpKmerFinder over a graph is not implemented (use DenseKmerFinder); "
                                      "pass reference= for the k-mers of a linear reference")
        if self._end_position is None:
            # the reference adds k to None here (snp_kmer_finder.py:301)
            raise TypeError("SnpKmerFinder on a linear reference needs end_position")
        _lib.require_device()
        reference = self.reference
        if not isinstance(reference, _lib.DeviceArray):
            reference = reference_to_letters(reference)
            if reference.size == 0:
                raise NoReferenceSequence("No reference sequence between positions %d and %d: the sequence is empty"
                                          % (self._start_position, self._end_position + self.k))
        with _lib.DeviceScope() as s:
            letters = s.on_device(reference, np.uint8)
            first, count = segments_of_intervals([(self._start_position, self._end_position)], letters.n, self.k, self.spacing)
            return linear_kmers_on_device(letters, self.k, self.spacing, first, count)

    def find_kmers(self):
        if self.reference is not None:
            logging.warning("Will find kmers on linear reference and not graph")
        with _lib.DeviceScope() as s:
            return s.keep(self.find_kmers_on_device()).to_flat_kmers()
