"""Host-side mirror of index4j's SuffixArray (suffixarray/SuffixArray.java, "SA") on the GPU: the text and its suffix array
of n + 1 entries (the empty suffix n first), sorted by prefix doubling in HBM (or by SA-IS on the host with build_device=-1),
and count / locate answered by HIP kernels that binary-search the resident array (csrc/fmx_sa_query.hip).  count keeps the
reference's quirk: it is one fewer than the occurrences when the largest suffix starts with the pattern."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .fmindex import as_chars, pack_patterns


class SuffixArray:
    def __init__(self, text, device=0, build_device=None):
        """text: str or uint16 array (a Java CharSequence).  device: where queries run (None: nowhere, e.g. to serialize);
        build_device: where construct() sorts the suffixes (default: `device`, or the host when that is None; -1 = host)."""
        self._text = as_chars(text)
        self._device = device
        self._build_device = build_device if build_device is not None else (-1 if device is None else int(device))
        self._h = None

    @classmethod
    def _from_handle(cls, h, device):
        self = cls.__new__(cls)
        self._h = h
        self._device = device
        self._build_device = -1
        self._text = None
        if device is not None:
            check(lib.fmx_to_device(h, int(device)), "fmx_to_device")
        return self

    def construct(self):
        """SA:89-91"""
        self.close()
        h = C.c_void_p()
        check(lib.fmx_sa_build(self._text.ctypes.data, len(self._text), int(self._build_device), C.byref(h)), "fmx_sa_build")
        self._h = h
        if self._device is not None and lib.fmx_device_of(h) != int(self._device):
            check(lib.fmx_to_device(h, int(self._device)), "fmx_to_device")
        return self

    def _handle(self):
        if not self._h:
            raise RuntimeError("SuffixArray: call construct() first")
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            lib.fmx_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def __len__(self):
        return lib.fmx_input_length(self._handle())

    # ---- batched ----
    def count_batch(self, patterns, offsets=None):
        """patterns: list of str / uint16 arrays, or (chars, offsets) already packed"""
        pat, off = (np.ascontiguousarray(patterns, dtype=np.uint16), np.ascontiguousarray(offsets, dtype=np.int32)) \
            if offsets is not None else pack_patterns(patterns)
        n = len(off) - 1
        counts = np.zeros(n, dtype=np.int32)
        check(lib.fmx_sa_count_batch(self._handle(), pat.ctypes.data, off.ctypes.data, n, counts.ctypes.data),
              "fmx_sa_count_batch")
        return counts

    def locate_batch(self, patterns, offsets=None, max_matches=16, fill=-1):
        """-> (locs [n, max_matches] int32, found, counts): locate(p, new int[max_matches]) per pattern; slots past
        found keep `fill`"""
        pat, off = (np.ascontiguousarray(patterns, dtype=np.uint16), np.ascontiguousarray(offsets, dtype=np.int32)) \
            if offsets is not None else pack_patterns(patterns)
        n = len(off) - 1
        locs = np.full((n, max_matches), fill, dtype=np.int32)
        found = np.zeros(n, dtype=np.int32)
        counts = np.zeros(n, dtype=np.int32)
        check(lib.fmx_sa_locate_batch(self._handle(), pat.ctypes.data, off.ctypes.data, n, int(max_matches),
                                      locs.ctypes.data, found.ctypes.data, counts.ctypes.data), "fmx_sa_locate_batch")
        return locs, found, counts

    def count_batch_dev(self, d_pat, d_off, n, d_counts, stream=None):
        """operands are torch tensors (or device pointers) in HBM; asynchronous on `stream` (a torch.cuda.Stream or pointer)"""
        check(lib.fmx_sa_count_batch_dev(self._handle(), _ptr(d_pat), _ptr(d_off), int(n), _ptr(d_counts), _stream(stream)),
              "fmx_sa_count_batch_dev")

    def locate_batch_dev(self, d_pat, d_off, n, max_matches, d_locs, d_found, d_counts=None, stream=None):
        check(lib.fmx_sa_locate_batch_dev(self._handle(), _ptr(d_pat), _ptr(d_off), int(n), int(max_matches), _ptr(d_locs),
                                          _ptr(d_found), _ptr(d_counts), _stream(stream)), "fmx_sa_locate_batch_dev")

    # ---- the reference's methods ----
    def count(self, pattern):  # SA:100-104
        return int(self.count_batch([pattern])[0])

    def locate(self, pattern, offsets):  # SA:116-129: fills offsets (a list / int32 array) in place
        m = len(offsets)
        locs, found, _ = self.locate_batch([pattern], max_matches=m)
        k = int(found[0])
        for i in range(k):
            offsets[i] = int(locs[0, i])
        return k

    def getSuffixArray(self):  # SA:164-166
        h = self._handle()
        rows = lib.fmx_sa_get(h, None, 0)
        out = np.zeros(rows, dtype=np.int32)
        check(0 if lib.fmx_sa_get(h, out.ctypes.data, rows) == rows else _lib.E_ARG, "fmx_sa_get")
        return out

    def write(self, framed=True):  # SA:172-184 (framed: as Serialization.writeToByteArray wraps it)
        buf, ln = C.c_void_p(), C.c_size_t()
        check(lib.fmx_sa_save(self._handle(), 1 if framed else 0, C.byref(buf), C.byref(ln)), "fmx_sa_save")
        try:
            return C.string_at(buf, ln.value)
        finally:
            lib.fmx_free_buffer(buf)

    @classmethod
    def read(cls, data, device=0):  # SA:186-199, raw or framed
        b = bytes(data)
        h = C.c_void_p()
        check(lib.fmx_sa_load(b, len(b), C.byref(h)), "fmx_sa_load")
        return cls._from_handle(h, device)

    def hashCode(self):  # SA:202-204
        v = C.c_int32()
        check(lib.fmx_sa_hash_code(self._handle(), C.byref(v)), "fmx_sa_hash_code")
        return v.value


def _ptr(x):
    if x is None:
        return None
    return x.data_ptr() if hasattr(x, "data_ptr") else int(x)


def _stream(s):
    if s is None:
        return None
    return s.cuda_stream if hasattr(s, "cuda_stream") else int(s)
