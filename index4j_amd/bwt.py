"""index4j's BurrowsWheelerTransform utility (encoding/BurrowsWheelerTransform.java, "BWT"): the transform of text + '\\0'
from its suffix array — sorted by prefix doubling in HBM with one gather kernel there (build_device >= 0), or on the host
(build_device = -1) — and the n / runs redundancy measure."""
import numpy as np

from . import _lib
from ._lib import check, lib
from .fmindex import as_chars, chars_to_str


def createBurrowsWheelerTransform(text, build_device=0):
    """BWT:43-113.  text: str or uint16 array (char[]).  Returns a str when given a str, else a uint16 array; n + 1 chars."""
    t = as_chars(text)
    out = np.zeros(len(t) + 1, dtype=np.uint16)
    rc = lib.fmx_bwt(t.ctypes.data, len(t), int(build_device), out.ctypes.data)
    if rc == _lib.E_ALPHABET:
        raise ValueError("Charset has more than 32767 different characters.")  # BWT:64-67
    check(rc, "fmx_bwt")
    return chars_to_str(out) if isinstance(text, str) else out


def computeRedundancyOfText(text):
    """BWT:116-135: n / (number of runs of equal symbols), as a double; the reference throws on an empty input"""
    a = as_chars(text) if isinstance(text, str) else np.asarray(text)
    if len(a) == 0:
        raise IndexError("Index 0 out of bounds for length 0")
    runs = 1 + int(np.count_nonzero(a[1:] != a[:-1]))
    return len(a) / float(runs)
