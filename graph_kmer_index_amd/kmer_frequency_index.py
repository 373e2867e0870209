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
from .kmer_counter import DeviceCounter, unique_counts


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
        if len(kmers) == 0:
            return np.zeros(0, np.int64)
        if self._device is None:
            _lib.require_device()
            self._device = DeviceCounter.from_host(self._kmers, self._frequencies)
        return self._device.lookup(kmers)

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
