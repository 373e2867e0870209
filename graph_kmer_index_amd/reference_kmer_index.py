"""ReferenceKmerIndex with the reference's attributes, file shapes and results (reference_kmer_index.py:24-149).
from_sequence / from_linear_reference hash the sequence on the device (gki_linear_kmers: spacing 1, one segment, hashes
only); from_flat_kmers is host NumPy with a stable sort."""
import logging
import numpy as np

from . import _lib


def fill_zeros_from_end(array):
    """reference_kmer_index.py:16-21."""
    array = array[::-1]
    prev = np.arange(len(array))
    prev[array == 0] = 0
    prev = np.maximum.accumulate(prev)
    return array[prev][::-1]


class ReferenceKmerIndex:
    properties = {"ref_position_to_index", "kmers", "ref_positions", "nodes"}

    def __init__(self, ref_position_to_index=None, kmers=None, ref_positions=None, nodes=None):
        self.ref_position_to_index = ref_position_to_index
        self.kmers = kmers
        self.ref_positions = ref_positions
        self.nodes = nodes

    def get_between(self, ref_start, ref_end):
        return self.kmers[
            self.ref_position_to_index[ref_start]:self.ref_position_to_index[min(len(self.ref_position_to_index) - 1, ref_end)]
        ]

    def get_between_except(self, ref_start, ref_end, except_position):
        assert self.ref_positions is None
        indexes = [i for i in np.arange(ref_start, ref_end) if i != except_position]
        return self.kmers[indexes]

    def get_all_between(self, ref_start, ref_end):
        if self.ref_positions is None:
            raise Exception("This index is missing reference positions and cannot be used to get all between. "
                            "Is it made from a linear reference? If so, use get_between() instead")
        start = self.ref_position_to_index[ref_start]
        end = self.ref_position_to_index[ref_end]
        return self.kmers[start:end], self.ref_positions[start:end], self.nodes[start:end]

    @classmethod
    def from_sequence(cls, genome_sequence, k, only_store_kmers=False):
        """reference_kmer_index.py:50-67: the hash of every k-window, uint32 for k <= 16 else uint64."""
        from .snp_kmer_finder import reference_to_letters
        _lib.require_device()
        host = reference_to_letters(genome_sequence)
        cls._check_length(len(host), k)
        return cls.from_device_letters(_lib.DeviceArray.from_host(host), k, only_store_kmers)

    @staticmethod
    def _check_length(n_letters, k):
        from .snp_kmer_finder import NoReferenceSequence
        if n_letters < k:
            raise NoReferenceSequence("the sequence has %d letters, fewer than k=%d" % (n_letters, k))

    @classmethod
    def from_device_letters(cls, letters, k, only_store_kmers=False):
        """The hashing step of `from_sequence`, from letters that are on the device already: a uint8 DeviceArray, which
        is taken over and freed here."""
        from .snp_kmer_finder import linear_kmers_on_device
        with _lib.DeviceScope() as s:
            s.keep(letters)
            n_letters = letters.n
            cls._check_length(n_letters, k)
            hashes, n = linear_kmers_on_device(letters, k, 1, [0], [n_letters - k + 1], hashes_only=True)
            s.keep(hashes)
            letters.free()                  # early: the letters are not needed while the hashes are copied
            kmers = hashes.to_host(n)
        ref_position_to_index = None
        if not only_store_kmers:
            ref_position_to_index = np.arange(0, n_letters, dtype=np.uint32)
        if k <= 16:
            kmers = kmers.astype(np.uint32)
        return cls(ref_position_to_index, kmers)

    @classmethod
    def from_linear_reference(cls, fasta_file_name, reference_name="ref", k=15, only_store_kmers=False, fasta_parse="auto"):
        """fasta_parse: 'device' the FASTA (plain, BGZF or gzip) is parsed on the device and hashed where it lies; 'host'
        `read_fasta_record` and an upload; 'auto' the faster of the two (`fasta_files.resolve_fasta_parse`)."""
        from .fasta_files import reference_from_file, resolve_fasta_parse
        from .snp_kmer_finder import read_fasta_record
        if resolve_fasta_parse(fasta_parse) == "host":
            return cls.from_sequence(read_fasta_record(fasta_file_name, reference_name), k, only_store_kmers)
        return cls.from_device_letters(reference_from_file(fasta_file_name, [reference_name]).letters, k, only_store_kmers)

    @classmethod
    def from_flat_kmers(cls, flat_kmers):
        """reference_kmer_index.py:76-114.  The reference's argsort is not stable, so the order of records that share a
        reference position is unspecified there; here they keep their input order."""
        ref_positions = np.asarray(flat_kmers._ref_offsets)
        sorting = np.argsort(ref_positions, kind="stable")
        ref_positions = ref_positions[sorting]
        kmers = np.asarray(flat_kmers._hashes)[sorting]
        if np.max(kmers) < 2 ** 32:
            logging.warning("Storing kmers as 32 bit uint since max hash is low enough")
            kmers = kmers.astype(np.uint32)
        nodes = np.asarray(flat_kmers._nodes)[sorting]
        assert len(kmers) < 4294967295, "Too many kmers to store (32 bit limit reached). There are %d kmers" % len(kmers)
        # np.where(np.ediff1d(ref_positions, to_begin=0)) of the reference, which NumPy 2 refuses for a uint64 column
        positions_of_new_ref_positions = np.flatnonzero(ref_positions[1:] != ref_positions[:-1]) + 1
        ref_position_to_index = np.zeros(int(ref_positions[-1]) + 1, dtype=np.uint32)
        ref_position_to_index[ref_positions[positions_of_new_ref_positions].astype(np.int64)] = positions_of_new_ref_positions
        ref_position_to_index = fill_zeros_from_end(ref_position_to_index)
        return cls(ref_position_to_index, kmers, ref_positions, nodes)

    def to_file(self, file_name):
        if self.ref_position_to_index is None:
            np.savez(file_name, kmers=self.kmers)
        elif self.ref_positions is None and self.nodes is None:
            np.savez(file_name, ref_position_to_index=self.ref_position_to_index, kmers=self.kmers)
        else:
            np.savez(file_name, ref_position_to_index=self.ref_position_to_index, kmers=self.kmers,
                     ref_positions=self.ref_positions, nodes=self.nodes)

    @classmethod
    def from_file(cls, file_name):
        try:
            data = np.load(file_name + ".npz")
        except FileNotFoundError:
            data = np.load(file_name)
        get = lambda key: data[key] if key in data else None
        return cls(get("ref_position_to_index"), data["kmers"], get("ref_positions"), get("nodes"))
