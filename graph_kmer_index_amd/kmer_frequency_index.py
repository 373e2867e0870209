"""KmerFrequencyIndex with the reference's surface (kmer_frequency_index.py:5-37): the distinct k-mers ascending
(`_kmers`, uint64) and how often each occurred (`_frequencies`, int64).  from_kmers runs on the device
(csrc/gki_count.hip: radix sort of the 64-bit keys and run lengths) and takes a NumPy array or a DeviceArray.

`get` mirrors the reference's, including its searchsorted(side="right"): the position it looks at lies AFTER a k-mer that
is present: a present k-mer is reported as a miss (0), and a k-mer at or above the largest key indexes past the array
(IndexError), as in the reference.  get_frequencies is this package's batched accessor and returns
the true counts, 0 when absent.
"""
import logging

import numpy as np

from . import _lib
from .kmer_counter import DeviceCounter, _bits_of, unique_counts


class KmerFrequencyIndex:
    def __init__(self, kmers, frequencies):
        self._kmers = kmers
        self._frequencies = frequencies
        self._device = None

    def get(self, kmer):
        index = np.searchsorted(self._kmers, kmer, side="right")
        if self._kmers[index] == kmer:
            return self._frequencies[index]

        logging.warning("No hit for kmer %d" % kmer)
        return 0

    def get_frequencies(self, kmers):
        """True counts of a batch of k-mers on the device (int64, 0 when absent)."""
        q = np.ascontiguousarray(kmers, dtype=np.uint64)
        if len(q) == 0:
            return np.zeros(0, np.int64)
        if self._device is None:
            _lib.require_device()
            keys = np.ascontiguousarray(self._kmers, dtype=np.uint64)
            self._device = DeviceCounter(_lib.DeviceArray.from_host(keys) if len(keys) else _lib.DeviceArray(0, np.uint64),
                                         _lib.DeviceArray.from_host(np.ascontiguousarray(self._frequencies, dtype=np.int64))
                                         if len(keys) else _lib.DeviceArray(0, np.int64), _bits_of(keys))
        d_q = _lib.DeviceArray.from_host(q)
        d_out = self._device.lookup_on_device(d_q)
        out = d_out.to_host()
        d_q.free()
        d_out.free()
        return out

    @classmethod
    def from_kmers(cls, kmers):
        unique, frequencies = unique_counts(kmers)
        return cls(unique, frequencies)

    def to_file(self, file_name):
        np.savez(file_name, kmers=self._kmers, frequencies=self._frequencies)

    @classmethod
    def from_file(cls, file_name):
        try:
            data = np.load(file_name)
        except FileNotFoundError:
            data = np.load(file_name + ".npz")

        return cls(data["kmers"], data["frequencies"])
