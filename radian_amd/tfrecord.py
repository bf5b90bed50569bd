"""Labelled signal windows out of TFRecord shards (radian/data.py:9-31), read by the library's host parser (rd_tfrecord_*,
tfrecord.hip) -- no TensorFlow.  Both frame checksums are verified; a malformed record raises TFRecordError naming its index."""
import ctypes

import numpy as np

from . import _lib

WINDOW = 1024   # radian/data.py:11: 'signal' FixedLenFeature([1024])


class TFRecordError(ValueError):
    pass


def crc32c(data):
    """Castagnoli CRC of bytes (unmasked), the library's rd_crc32c"""
    b = bytes(data)
    buf = ctypes.create_string_buffer(b, len(b))
    return int(_lib.load().rd_crc32c(ctypes.cast(buf, ctypes.c_void_p), len(b)))


class Shard:
    """One shard's records in file order: signals float32 [n, 1024], input_len int32 [n] (signal_length), label_off int64 [n + 1]
    into labels uint8 (the first label_length values of each record's `label`), label_len int32 [n]."""

    def __init__(self, signals, input_len, labels, label_off, label_len):
        self.signals, self.input_len, self.labels, self.label_off, self.label_len = signals, input_len, labels, label_off, label_len

    def __len__(self):
        return len(self.input_len)

    def label(self, i):
        return self.labels[self.label_off[i]: self.label_off[i + 1]]


def _read(opener, arg, what):
    L = _lib.load()
    h = ctypes.c_void_p()
    rc = opener(arg, ctypes.byref(h))
    if rc != 0:
        msg = L.rd_last_error().decode("utf-8", "replace")
        if rc == -7:
            raise OSError(msg)
        raise TFRecordError(msg)
    try:
        n, nl = ctypes.c_int64(0), ctypes.c_int64(0)
        L.rd_tfrecord_count(h, ctypes.byref(n), ctypes.byref(nl))
        n, nl = n.value, nl.value
        sig = np.zeros((n, WINDOW), dtype=np.float32)
        ilen = np.zeros(n, dtype=np.int32)
        off = np.zeros(n + 1, dtype=np.int64)
        llen = np.zeros(n, dtype=np.int32)
        lab = np.zeros(max(nl, 1), dtype=np.uint8)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = L.rd_tfrecord_read(h, 0, n, p(sig), p(ilen), p(off), p(llen), p(lab), nl)
        if rc != 0:
            raise TFRecordError(f"{what}: " + L.rd_last_error().decode("utf-8", "replace"))
    finally:
        L.rd_tfrecord_close(h)
    return Shard(sig, ilen, lab[:nl], off, llen)


def read_shard(path):
    """every record of the shard at path"""
    return _read(_lib.load().rd_tfrecord_open, str(path).encode(), str(path))


def read_shard_bytes(data):
    """every record of a shard held in memory"""
    b = bytes(data)
    buf = ctypes.create_string_buffer(b, len(b))
    return _read(lambda a, o: _lib.load().rd_tfrecord_open_mem(ctypes.cast(buf, ctypes.c_void_p), len(b), o), None, "<buffer>")
