"""KmerCounter with the reference's constructors and accessors (kmer_counter.py:9-83), on MI355X.

The reference counts with np.unique(kmers, return_counts=True) and stores the result in an `npstructures` hash table.
Here the unique keys and their counts come from the device (csrc/gki_count.hip, include/gki.h gki_unique_counts_*: a
key-only radix sort of the 64-bit hashes and run lengths) and are kept as two sorted arrays; batched lookups go through
a device counter with a prefix directory (gki_counter_*), scalar ones through the host arrays.  The `npstructures`
storage and the reference's pickled file are not reproduced: `modulo` is accepted and stored for interface parity only,
and to_file / from_file use this package's own .npz (`kmers`, `counts`, `modulo`).

What a consumer needs of a counter is get_frequency(kmer): the count of the k-mer among the (subsampled) input, 0 when
absent, with NO reverse complement added -- unlike CollisionFreeKmerIndex.get_frequency.
"""
import logging
import os

import numpy as np

from . import _lib

SORT_TILE = 4096          # keys per tile of the sort and of the run-length passes (CT of csrc/gki_count.hip)


def choose_modulo(n_elements):
    if n_elements < 1000000:
        return 2000003
    elif n_elements < 10000000:
        return 19999999
    else:
        return 200000003


def _bits_of(kmers):
    """2k for hashes of k-mers: the number of bits the largest key needs (at least 1)."""
    return max(1, int(kmers.max()).bit_length()) if len(kmers) else 1


def unique_counts_on_device(kmers, stride=1, key_bits=None):
    """np.unique(kmers[::stride], return_counts=True) on the device: (DeviceArray uint64 ascending, DeviceArray int64).
    kmers: a NumPy array of non-negative integers, or a DeviceArray of 8-byte keys, which is read in place and never
    written.  key_bits: the keys are below 2^key_bits (None: taken from a NumPy array's maximum, 64 for a DeviceArray);
    radix passes above it are skipped."""
    _lib.require_device()
    lib = _lib.load()
    stride = int(stride)
    if stride < 1:
        raise ValueError("stride must be at least 1 (got %d)" % stride)
    if isinstance(kmers, _lib.DeviceArray):
        if kmers.dtype.itemsize != 8 or kmers.dtype.kind not in "ui":
            raise TypeError("k-mers on the device must be uint64 or int64 (got %s)" % kmers.dtype)
        key_bits = 64 if key_bits is None else int(key_bits)
    else:
        kmers = np.asarray(kmers)
        if kmers.ndim != 1:
            raise ValueError("k-mers must be one-dimensional")
        if kmers.dtype.kind == "i" and len(kmers) and kmers.min() < 0:
            raise ValueError("k-mers must not be negative")
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        key_bits = _bits_of(kmers) if key_bits is None else int(key_bits)
    n_unique, plan = _lib._I64(0), _lib.C.c_void_p()
    ms, ms_emit = (_lib.C.c_float * 2)(), (_lib.C.c_float * 1)()
    with _lib.DeviceScope() as s:
        d_kmers = s.on_device(kmers, np.uint64)
        try:
            _lib.check(lib.gki_unique_counts_count(d_kmers.ptr, d_kmers.n, stride, key_bits, _lib.C.byref(n_unique),
                                                   _lib.C.byref(plan), ms))
            unique = s.array(n_unique.value, np.uint64)
            counts = s.array(n_unique.value, np.int64)
            _lib.check(lib.gki_unique_counts_emit(plan, unique.ptr, counts.ptr, ms_emit))
        finally:
            if plan.value:
                lib.gki_unique_counts_destroy(plan)
        s.release(unique), s.release(counts)
    unique_counts_on_device.last_kernel_ms = {"sort": float(ms[0]), "run_heads": float(ms[1]), "emit": float(ms_emit[0])}
    return unique, counts


def unique_counts(kmers, stride=1, key_bits=None):
    """np.unique(kmers[::stride], return_counts=True) through the device: (uint64 ascending, int64)."""
    with _lib.DeviceScope() as s:
        d_unique, d_counts = map(s.keep, unique_counts_on_device(kmers, stride, key_bits))
        return d_unique.to_host(), d_counts.to_host()


class DeviceCounter:
    """Sorted distinct keys and counts in HBM behind a gki_counter (prefix directory + bounded binary search)."""

    def __init__(self, d_kmers, d_counts, key_bits):
        self.kmers, self.counts, self.key_bits = d_kmers, d_counts, int(key_bits)
        handle = _lib.C.c_void_p()
        _lib.check(_lib.load().gki_counter_create(d_kmers.ptr, d_counts.ptr, d_kmers.n, self.key_bits, _lib.C.byref(handle)))
        self.handle = handle

    @classmethod
    def from_host(cls, kmers, counts):
        """The counter of sorted distinct host k-mers and their counts; both uploads are its own."""
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        with _lib.DeviceScope() as s:
            d_kmers, d_counts = s.on_device(kmers, np.uint64), s.on_device(counts, np.int64)
            out = cls(d_kmers, d_counts, _bits_of(kmers))
            s.release(d_kmers), s.release(d_counts)
        return out

    def lookup_on_device(self, d_queries):
        with _lib.DeviceScope() as s:
            out = s.array(d_queries.n, np.int64)
            _lib.check(_lib.load().gki_counter_lookup(self.handle, d_queries.ptr, d_queries.n, out.ptr))
            return s.release(out)

    def lookup(self, queries):
        """The counts of host k-mers as a NumPy array (int64, 0 when absent)."""
        q = np.ascontiguousarray(queries, dtype=np.uint64)
        if len(q) == 0:
            return np.zeros(0, np.int64)
        with _lib.DeviceScope() as s:
            return s.keep(self.lookup_on_device(s.on_device(q, np.uint64))).to_host()

    def free(self):
        if self.handle is not None and self.handle.value:
            _lib.load().gki_counter_destroy(self.handle)
            self.handle = None
            self.kmers.free()
            self.counts.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class KmerCounter:
    def __init__(self, kmers, counts, modulo=0):
        """kmers: the distinct k-mers ascending (uint64), counts: how often each occurred (int64)."""
        self._kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        self._counts = np.ascontiguousarray(counts, dtype=np.int64)
        if len(self._kmers) != len(self._counts):
            raise ValueError("%d k-mers, %d counts" % (len(self._kmers), len(self._counts)))
        self._modulo = int(modulo)
        self._device = None

    # ------------------------------------------------------------------ constructors (kmer_counter.py:23-70)
    @classmethod
    def from_flat_kmersv2(cls, flat, modulo, subsample_ratio=1):
        kmers = flat._hashes
        logging.info("Subsampling ratio: %d, k-mers before subsampling: %d" % (subsample_ratio, len(kmers)))
        return cls.from_kmers(kmers, modulo, subsample_ratio=subsample_ratio)

    @classmethod
    def from_kmers(cls, kmers, modulo, subsample_ratio=1, key_bits=None):
        """Counts of kmers[::subsample_ratio]; kmers may be a NumPy array or a DeviceArray."""
        unique_kmers, counts = unique_counts(kmers, subsample_ratio, key_bits)
        if modulo == 0:
            modulo = choose_modulo(len(unique_kmers))
            logging.info("Choosing suitable modulo for hashtable to be %d" % modulo)
        return cls(unique_kmers, counts, modulo)

    @classmethod
    def from_flat_kmers(cls, flat, modulo, chunk_size=50000000):
        """The reference counts chunk by chunk into a table of the unique k-mers (and leaves a debugging file behind);
        the result is the count of every k-mer, which one device call gives."""
        return cls.from_kmers(flat._hashes, modulo)

    # ------------------------------------------------------------------ accessors
    def _device_counter(self):
        if self._device is None:
            _lib.require_device()
            self._device = DeviceCounter.from_host(self._kmers, self._counts)
        return self._device

    def get_frequency(self, kmer):
        """The count of the k-mer, 0 when absent; no reverse complement (kmer_counter.py:72-74).  From host arrays."""
        kmer = int(kmer)
        if kmer < 0 or kmer >> 64:
            return 0
        i = int(np.searchsorted(self._kmers, np.uint64(kmer)))
        return int(self._counts[i]) if i < len(self._kmers) and int(self._kmers[i]) == kmer else 0

    def get_frequencies(self, kmers):
        """Batched get_frequency on the device: int64 counts, 0 when absent.  A DeviceArray gives a DeviceArray."""
        counter = self._device_counter()
        if isinstance(kmers, _lib.DeviceArray):
            return counter.lookup_on_device(kmers)
        return counter.lookup(kmers)

    def score_kmers(self, kmers):
        """A scorer for a set of k-mers, low is bad: minus the largest count among those present, 1 when none is
        (kmer_counter.py:76-83)."""
        hits = self.get_frequencies(np.array([int(k) for k in kmers], dtype=np.uint64))
        hits = hits[hits > 0]
        if len(hits) == 0:
            return 1
        return -np.max(hits)

    # ------------------------------------------------------------------ files (this package's own .npz)
    def to_file(self, file_name):
        np.savez(file_name, kmers=self._kmers, counts=self._counts, modulo=self._modulo)

    @classmethod
    def from_file(cls, file_name):
        name = str(file_name)
        path = name if os.path.exists(name) else name + ".npz"
        if not os.path.exists(path):
            raise FileNotFoundError("k-mer counter file not found: %s" % name)
        try:
            data = np.load(path)
            return cls(data["kmers"], data["counts"], int(data["modulo"]))
        except (KeyError, ValueError, TypeError, AttributeError, OSError) as e:
            raise ValueError("%s is not a KmerCounter written by graph_kmer_index_amd (count_kmers): %s; the reference's "
                             "pickled npstructures table is not read" % (path, e))
