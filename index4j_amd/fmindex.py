"""Host-side mirror of index4j's public API for the backward-search path, over the C ABI.

``FmIndexBuilder`` mirrors fm/FmIndexBuilder.java:21-62 and ``FmIndex`` mirrors the query surface of
fm/FmIndex.java:443-941 (same method names, argument meaning and exceptions, with Java's
RuntimeException -> RuntimeError, IllegalArgumentException -> ValueError,
ArrayIndexOutOfBoundsException -> IndexError, IOException -> IOError).  Scalar calls are batches of
one; the ``*_batch`` methods are what a service would use.  All queries run on the GPU through
libfmx.so — there is no CPU query path.

In production the host language is Java (see INTEGRATION.md and bindings/java); this module is the
same binding written in Python for the test-suite and the benchmark.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib

_EXC = {0: RuntimeError, 1: ValueError, 2: IndexError}
NUMBER_MAX = 2 ** 63 - 1  # "no upper bound" of a ranged term (match_query_number_batch)
all_of = all  # (match_query's and grep's keyword `all` shadows the builtin there)


def as_chars(text):
    """str / array -> contiguous uint16 array of UTF-16 code units (a Java char[])."""
    if isinstance(text, str):
        return np.frombuffer(text.encode("utf-16-le"), dtype=np.uint16).copy()
    if isinstance(text, (bytes, bytearray)):
        raise TypeError("pass str or a uint16 array; use FmIndex.convertBytePatternToCharPattern for UTF-8 bytes")
    return np.ascontiguousarray(text, dtype=np.uint16)


def chars_to_str(arr):
    return np.ascontiguousarray(arr, dtype=np.uint16).tobytes().decode("utf-16-le", errors="surrogatepass")


def raise_for_status(status, aux=0):
    """Re-throw the reference's exception for a per-query status code (same type, same message)."""
    if status == _lib.ST_OK:
        return
    msg = lib.fmx_status_message(int(status)).decode()
    if "%d" in msg:
        msg = msg % aux
    raise _EXC[lib.fmx_status_kind(int(status))](msg)


def pack_patterns(patterns):
    """list of str / uint16 arrays -> (chars, offsets) in the layout fmx_count_batch takes."""
    arrs = [as_chars(p) for p in patterns]
    off = np.zeros(len(arrs) + 1, dtype=np.int32)
    if arrs:
        np.cumsum([len(a) for a in arrs], out=off[1:])
    chars = np.concatenate(arrs) if arrs else np.zeros(0, dtype=np.uint16)
    return np.ascontiguousarray(chars, dtype=np.uint16), off


CLASS_RANGES_MAX = 1024  # FMX_CLASS_RANGES_MAX
CLASS_ALTS_MAX = 64  # FMX_CLASS_ALTS_MAX
LINES_ALL = 2 ** 31 - 1  # the end of a window of lines that does not filter: lines=(0, LINES_ALL)
CLASS_RANGES_DEFAULT = 256  # max_ranges where the caller names none: two frontiers of 4 KiB per pattern


def pack_class_patterns(patterns):
    """list of class patterns -> (alt, pos_off, pat_off) in the layout fmx_count_class_batch takes.  A class pattern is a list
    of positions; a position is its alternatives: a str (every UTF-16 code unit of it is one) or an iterable of code units /
    one-unit strs.  ignore_case() and parse_classes() make such lists."""
    alts, pos_off, pat_off = [], [0], [0]
    total = 0
    for pattern in patterns:
        for position in pattern:
            a = as_chars(position) if isinstance(position, str) else as_chars([ord(x) if isinstance(x, str) else x for x in position])
            alts.append(a)
            total += len(a)
            pos_off.append(total)
        pat_off.append(len(pos_off) - 1)
    alt = np.concatenate(alts) if alts else np.zeros(0, dtype=np.uint16)
    return np.ascontiguousarray(alt, dtype=np.uint16), np.array(pos_off, dtype=np.int32), np.array(pat_off, dtype=np.int32)


def ignore_case(text):
    """str / uint16 array -> the class pattern that matches it in any case (grep -i): per code unit {c, lower(c), upper(c)},
    keeping only results that are one UTF-16 code unit ('ß' stays alone: its upper case is two)"""
    out = []
    for u in as_chars(text).tolist():
        ch = chr(u)
        units = [u]
        for other in (ch.lower(), ch.upper()):
            if len(other) == 1 and ord(other) < 0x10000 and ord(other) not in units:
                units.append(ord(other))
        out.append("".join(chr(v) for v in units))
    return out


_ignore_case = ignore_case  # (the methods below have a keyword of that name)


def parse_classes(expr):
    """"blk_[0-9a-f]x\\[" -> a class pattern: a character stands for itself, [...] for its members (a-z: the code units from a
    to z), a backslash takes the next character literally, inside brackets too.  ValueError for [^...], an unclosed bracket, an
    empty class, a range that runs backwards and a trailing backslash."""
    units = as_chars(expr).tolist()
    out, i, n = [], 0, len(units)
    BS, OPEN, CLOSE, DASH, NOT = ord("\\"), ord("["), ord("]"), ord("-"), ord("^")

    def take(at):  # (code unit, next index) of the possibly escaped character at `at`
        if units[at] == BS:
            if at + 1 >= n:
                raise ValueError("a backslash ends the expression")
            return units[at + 1], at + 2
        return units[at], at + 1

    while i < n:
        if units[i] != OPEN:
            u, i = take(i)
            out.append(chr(u))
            continue
        i += 1
        if i < n and units[i] == NOT:
            raise ValueError("negated classes ([^...]) are not supported")
        members = []
        while True:
            if i >= n:
                raise ValueError("unclosed bracket")
            if units[i] == CLOSE:
                i += 1
                break
            lo, i = take(i)
            if i + 1 < n and units[i] == DASH and units[i + 1] != CLOSE:
                hi, i = take(i + 1)
                if hi < lo:
                    raise ValueError("range runs backwards")
                members.extend(range(lo, hi + 1))
            else:
                members.append(lo)
        if not members:
            raise ValueError("empty class")
        out.append("".join(chr(v) for v in dict.fromkeys(members)))
    return out


class FmIndexBuilder:
    """fm/FmIndexBuilder.java: defaults sampleRate=32, enableExtraction=true (FMB:21-22)."""

    def __init__(self):
        self._sample_rate = 32
        self._enable_extraction = True
        self._build_device = None

    def setBuildDevice(self, device):
        """extension: run the suffix-array stage of the constructor on this GPU (same index, byte for byte)"""
        self._build_device = device
        return self

    def setSampleRate(self, sample_rate):  # FMB:34-37
        self._sample_rate = int(sample_rate)
        return self

    def setEnableExtraction(self, enable):  # FMB:46-49
        self._enable_extraction = bool(enable)
        return self

    def build(self, text, device=0):  # FMB:59-61
        return FmIndex(text, self._sample_rate, self._enable_extraction, device=device, build_device=self._build_device)


class NumberStats:
    """row i of a number_stats_where_batch answer: count, min, max (B), pct (B, P) as numpy arrays, sum as exact Python ints"""

    def __init__(self, out, i):
        self.count, self.min, self.max, self.pct = out["count"][i], out["min"][i], out["max"][i], out["pct"][i]
        self.sum = [(int(hi) << 64) | int(lo) for lo, hi in zip(out["sum_lo"][i], out["sum_hi"][i])]
        self.not_number, self.overflow = int(out["not_number"][i]), int(out["overflow"][i])
        self.occurrences, self.kept = int(out["occurrences"][i]), int(out["kept"][i])

    def mean(self):
        """sum / count per bucket as floats (nan where a bucket is empty): a convenience of the host"""
        return np.array([s / c if c else float("nan") for s, c in zip(self.sum, self.count.tolist())], dtype=np.float64)


class TopLines:
    """pattern i of a top_lines_where_batch answer: line, value, loc — the rows[i] ranked rows as numpy arrays (int32, int64, int32) —
    and lines (the lines that have a candidate), numbers, not_number, overflow, kept, occurrences as ints; text: the rows' lines
    as a list of str where the call asked for it, else None"""

    def __init__(self, out, i=0, text=None):
        r = int(out["rows"][i])
        self.line, self.value, self.loc = out["row_line"][i, :r].copy(), out["row_value"][i, :r].copy(), out["row_loc"][i, :r].copy()
        self.lines, self.numbers = int(out["lines"][i]), int(out["numbers"][i])
        self.not_number, self.overflow = int(out["not_number"][i]), int(out["overflow"][i])
        self.occurrences, self.kept = int(out["occurrences"][i]), int(out["kept"][i])
        self.text = text

    def __len__(self):
        return len(self.line)


class NumberStatsBy:
    """number pattern i of a number_stats_by_batch answer, by its key pattern by_of[i]: groups = [dict(value, lines, count, sum, min, max,
    pct, mean)] — sum an exact Python int, mean a float (nan for a group without numbers) — in the order of the values, or with
    top=k the k groups with the most lines, ties by value; the per-pattern counters as ints"""

    def __init__(self, out, top=None, i=0):
        k = int(out["by_of"][i])  # the key pattern number pattern i is grouped by
        k_lo, r_lo = int(out["val_off"][k]), int(out["row_off"][i])
        text_off, chars = out["text_off"], out["chars"]
        self.groups = []
        for g in range(int(out["row_off"][i + 1]) - r_lo):
            r, v = r_lo + g, k_lo + g
            c, total = int(out["count"][r]), (int(out["sum_hi"][r]) << 64) | int(out["sum_lo"][r])
            self.groups.append(dict(value=chars[text_off[v]:text_off[v + 1]].tobytes().decode("utf-16-le", "surrogatepass"), lines=int(out["lines"][v]),
                                    count=c, sum=total, min=int(out["min"][r]), max=int(out["max"][r]), pct=out["pct"][r].tolist(),
                                    mean=total / c if c else float("nan")))
        if top is not None:  # (a stable sort: equal line counts keep the order of the values)
            self.groups = sorted(self.groups, key=lambda grp: -grp["lines"])[:max(int(top), 0)]
        self.no_key, self.not_number, self.overflow = int(out["no_key"][i]), int(out["not_number"][i]), int(out["overflow"][i])
        self.occurrences, self.kept = int(out["occurrences"][i]), int(out["kept"][i])
        self.key_occurrences, self.key_kept = int(out["key_occurrences"][k]), int(out["key_kept"][k])

    def by_value(self):
        """{value: group}"""
        return {grp["value"]: grp for grp in self.groups}


def _group_strings(out, k):
    """the values of key pattern k's groups of a keyed answer"""
    text_off, chars = out["text_off"], out["chars"]
    return [chars[text_off[g]:text_off[g + 1]].tobytes().decode("utf-16-le", "surrogatepass") for g in range(int(out["val_off"][k]), int(out["val_off"][k + 1]))]


def _pair_values(out, j):
    """[((a, b), lines)] of pair j of a number_stats_by_pair_batch answer, in pair order"""
    a, b = _group_strings(out, int(out["pair_a"][j])), _group_strings(out, int(out["pair_b"][j]))
    lo, hi = int(out["pair_off"][j]), int(out["pair_off"][j + 1])
    return [((a[int(out["pair_group_a"][r])], b[int(out["pair_group_b"][r])]), int(out["pair_lines"][r])) for r in range(lo, hi)]


class NumberStatsByPair:
    """number pattern i of a number_stats_by_pair_batch answer, by its pair by_of[i]: groups = [dict(values=(a, b), lines, count, sum,
    min, max, pct, mean)] — sum an exact Python int, mean a float (nan for a pair without numbers) — in pair order (the value order of
    a, then of b), or with top=k the k pairs with the most lines, ties in pair order; the per-pattern counters as ints"""

    def __init__(self, out, top=None, i=0):
        j = int(out["by_of"][i])  # the pair number pattern i is grouped by
        r_lo = int(out["row_off"][i])
        self.groups = []
        for g, (values, lines) in enumerate(_pair_values(out, j) if int(out["row_off"][i + 1]) > r_lo else []):
            r = r_lo + g
            c, total = int(out["count"][r]), (int(out["sum_hi"][r]) << 64) | int(out["sum_lo"][r])
            self.groups.append(dict(values=values, lines=lines, count=c, sum=total, min=int(out["min"][r]), max=int(out["max"][r]),
                                    pct=out["pct"][r].tolist(), mean=total / c if c else float("nan")))
        if top is not None:  # (a stable sort: equal line counts keep the pair order)
            self.groups = sorted(self.groups, key=lambda grp: -grp["lines"])[:max(int(top), 0)]
        self.no_key, self.not_number, self.overflow = int(out["no_key"][i]), int(out["not_number"][i]), int(out["overflow"][i])
        self.occurrences, self.kept = int(out["occurrences"][i]), int(out["kept"][i])
        a, b = int(out["pair_a"][j]), int(out["pair_b"][j])
        self.key_occurrences = (int(out["key_occurrences"][a]), int(out["key_occurrences"][b]))
        self.key_kept = (int(out["key_kept"][a]), int(out["key_kept"][b]))

    def by_values(self):
        """{(a, b): group}"""
        return {grp["values"]: grp for grp in self.groups}


class NumberStatsByHistogram:
    """number pattern i of a number_stats_by_histogram_batch answer, by its key pattern by_of[i]: rows = [dict(value, lines, group, count
    (B), sum (B exact Python ints), min, max (B), pct (B, P))] — the key rows in descending order of lines, ties in value order; group
    the key's index among the pattern's groups —, other: the same shape without value, lines and group, over the keys that are no
    row; n_groups and the per-pattern counters as ints"""

    def __init__(self, out, i=0):
        k, B = int(out["by_of"][i]), int(out["buckets"])
        text_off, chars = out["text_off"], out["chars"]
        k_lo, k_hi, c_lo = int(out["key_row_off"][k]), int(out["key_row_off"][k + 1]), int(out["cell_off"][i])
        cells = int(out["cell_off"][i + 1]) - c_lo  # ((rows + 1) * B, or none at all where no key pattern has a kept hit)

        def cell_row(r):
            a, b = c_lo + r * B, c_lo + (r + 1) * B
            if cells == 0:
                P = out["pct"].shape[1]
                return dict(count=[0] * B, sum=[0] * B, min=[0] * B, max=[0] * B, pct=[[0] * P for _ in range(B)])
            return dict(count=out["count"][a:b].tolist(), sum=[(int(hi) << 64) | int(lo) for lo, hi in zip(out["sum_lo"][a:b], out["sum_hi"][a:b])],
                        min=out["min"][a:b].tolist(), max=out["max"][a:b].tolist(), pct=out["pct"][a:b].tolist())

        self.rows = [dict(value=chars[text_off[r]:text_off[r + 1]].tobytes().decode("utf-16-le", "surrogatepass"), lines=int(out["key_row_lines"][r]),
                          group=int(out["key_row_group"][r]), **cell_row(r - k_lo)) for r in range(k_lo, k_hi)]
        self.other = cell_row(k_hi - k_lo)
        self.n_groups = int(out["n_groups"][k])
        self.no_key, self.not_number, self.overflow = int(out["no_key"][i]), int(out["not_number"][i]), int(out["overflow"][i])
        self.occurrences, self.kept = int(out["occurrences"][i]), int(out["kept"][i])
        self.key_occurrences, self.key_kept = int(out["key_occurrences"][k]), int(out["key_kept"][k])

    def by_value(self):
        """{value: row}"""
        return {row["value"]: row for row in self.rows}


class FieldValuesHistogram:
    """pattern i of a field_values_histogram_where_batch answer: rows = [dict(value, count, group, hist)] — the top values in descending
    order of count, ties in value order; group the value's index among the pattern's distinct values, hist its B counters as a list —
    other (B ints: the kept hits whose value is no row), and n_values, kept, occurrences as ints"""

    def __init__(self, out, i=0):
        text_off, chars = out["text_off"], out["chars"]
        self.rows = [dict(value=chars[text_off[r]:text_off[r + 1]].tobytes().decode("utf-16-le", "surrogatepass"), count=int(out["row_count"][r]),
                          group=int(out["row_group"][r]), hist=out["hist"][r].tolist())
                     for r in range(int(out["row_off"][i]), int(out["row_off"][i + 1]))]
        self.other = out["other"][i].tolist()
        self.n_values, self.kept, self.occurrences = int(out["n_values"][i]), int(out["kept"][i]), int(out["occurrences"][i])

    def by_value(self):
        """{value: row}"""
        return {row["value"]: row for row in self.rows}


class DistinctValues:
    """pattern i of a distinct_values_histogram_where_batch answer: distinct (B ints: the different values among the kept hits of each
    bucket), first_seen (B ints: the values whose first kept hit lies in the bucket), and n_values, kept, occurrences as ints"""

    def __init__(self, out, i=0):
        self.distinct, self.first_seen = out["distinct"][i].tolist(), out["first_seen"][i].tolist()
        self.n_values, self.kept, self.occurrences = int(out["n_values"][i]), int(out["kept"][i]), int(out["occurrences"][i])


class FmIndex:
    """fm/FmIndex.java query surface.  `device=None` keeps the index on the host (build / save /
    load only); any query then fails loudly."""

    def __init__(self, text=None, sampleRate=32, enableExtract=True, device=0, _handle=None, build_device=None):
        self._h = None
        self.build_stats = None
        if _handle is not None:
            self._h = _handle
        else:
            a = as_chars(text)
            h = C.c_void_p()
            if build_device is None:
                check(lib.fmx_build(a.ctypes.data, len(a), int(sampleRate), int(bool(enableExtract)), C.byref(h)), "fmx_build")
            else:  # suffix array, BWT and samples computed in HBM (fmx_sa_gpu.hip); same index
                rounds, rows, secs = C.c_int32(0), C.c_int64(0), C.c_double(0)
                check(lib.fmx_build_on_device(a.ctypes.data, len(a), int(sampleRate), int(bool(enableExtract)),
                                              int(build_device), C.byref(h), C.byref(rounds), C.byref(rows),
                                              C.byref(secs)), "fmx_build_on_device")
                self.build_stats = {"doubling_rounds": rounds.value, "rows_sorted": rows.value,
                                    "device_stage_seconds": secs.value,
                                    # 0.0: the wavelet tree was encoded on the host (alphabet above 1,024 codes, or option)
                                    "wavelet_device_seconds": lib.fmx_build_wavelet_seconds(h)}
            self._h = h
        if device is not None:
            self.to_device(device)

    # ---- persistence (FM:948-1025 through SER:67-100) ----
    @classmethod
    def read(cls, data, device=0):
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        h = C.c_void_p()
        check(lib.fmx_load(buf.ctypes.data, len(buf), C.byref(h)), "fmx_load")
        return cls(device=device, _handle=h)

    def write(self, framed=True):
        buf, n = C.c_void_p(), C.c_size_t()
        check(lib.fmx_save(self._h, int(framed), C.byref(buf), C.byref(n)), "fmx_save")
        try:
            # (ctypes.string_at takes a C int: a sampleRate-1 index of 256 MiB serializes to more than 2 GiB)
            return bytes((C.c_ubyte * n.value).from_address(buf.value))
        finally:
            lib.fmx_free_buffer(buf)

    def serialized_key_order_is_modelled(self):
        """False: a JVM's HashMap would have made one of the character map's buckets a tree bin, whose iteration order write()
        does not model (fmx.h fmx_save_key_order_modelled): the stream is valid, its key order in that bucket unverified"""
        rc = lib.fmx_save_key_order_modelled(self._h)
        if rc < 0:
            check(rc, "fmx_save_key_order_modelled")
        return rc == 1

    @classmethod
    def attach_device_blob(cls, device_ptr, nbytes, device):
        """adopt a blob already in HBM (e.g. received through an RCCL broadcast)"""
        h = C.c_void_p()
        check(lib.fmx_attach_device_blob(C.c_void_p(device_ptr), nbytes, device, C.byref(h)), "fmx_attach_device_blob")
        return cls(device=None, _handle=h)

    def to_device(self, device=0):
        check(lib.fmx_to_device(self._h, int(device)), "fmx_to_device")
        return self

    def blob(self):
        p, n = C.c_void_p(), C.c_size_t()
        check(lib.fmx_blob(self._h, C.byref(p), C.byref(n)), "fmx_blob")
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value,))

    def device_blob(self):
        n = C.c_size_t()
        p = lib.fmx_device_blob(self._h, C.byref(n))
        return p, n.value

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h is not None:
            lib.fmx_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- convenience (FM:929-941, 1044-1046) ----
    def getInputLength(self):
        return lib.fmx_input_length(self._h)

    def getAlphabetLength(self):
        return lib.fmx_alphabet_length(self._h)

    def __str__(self):
        return "FMIndex-sampleRate:%d-extract:%s" % (
            lib.fmx_sample_rate(self._h),
            "true" if lib.fmx_extract_enabled(self._h) else "false",
        )

    toString = __str__

    @staticmethod
    def convertBytePatternToCharPattern(pattern, offset, length, destination):  # FM:239-298
        src = np.frombuffer(bytes(pattern), dtype=np.uint8)
        bad = C.c_int32(0)
        n = lib.fmx_convert_byte_pattern(src.ctypes.data, offset, length, destination.ctypes.data, C.byref(bad))
        if n < 0:
            raise RuntimeError("Found a character that exceeds (32767): it was %d" % bad.value)
        return n

    def window_cells_bytes(self):
        """bytes of the resident index's window directory (0: none) — fmx_window_cells_info"""
        nbytes = C.c_int64(0)
        check(lib.fmx_window_cells_info(self._h, C.byref(nbytes)), "fmx_window_cells_info")
        return nbytes.value

    def locate_rows_info(self):
        """(bytes, replay_rows) of the resident index's row table (0, 0: none) — fmx_locate_rows_info.  An index made resident
        while option "locate_rows" is 1 keeps what locate() returns for every BWT row (4 bytes per text character) and gathers
        its hits instead of walking to them; replay_rows = rows that are walked all the same"""
        nbytes, replay = C.c_int64(0), C.c_int64(0)
        check(lib.fmx_locate_rows_info(self._h, C.byref(nbytes), C.byref(replay)), "fmx_locate_rows_info")
        return nbytes.value, replay.value

    def suffix_table_info(self):
        """(characters, bytes) of the resident index's suffix table (0, 0: none) — fmx_suffix_table_info"""
        chars, nbytes = C.c_int32(0), C.c_int64(0)
        check(lib.fmx_suffix_table_info(self._h, C.byref(chars), C.byref(nbytes)), "fmx_suffix_table_info")
        return chars.value, nbytes.value

    # ---- batched queries ----
    def count_batch(self, chars, offsets, want_steps=False):
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        n = len(offsets) - 1
        counts = np.zeros(n, dtype=np.int32)
        steps = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        check(lib.fmx_count_batch(self._h, chars.ctypes.data, offsets.ctypes.data, n, counts.ctypes.data,
                                  steps.ctypes.data, status.ctypes.data), "fmx_count_batch")
        return (counts, status, steps) if want_steps else (counts, status)

    def locate_batch(self, chars, offsets, max_matches, loc_cap=None, want_steps=False, locs=None):
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        n = len(offsets) - 1
        if loc_cap is None:
            loc_cap = max_matches
        if locs is None:
            locs = np.zeros((n, max(loc_cap, 0)), dtype=np.int32)
        found = np.zeros(n, dtype=np.int32)
        steps = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        check(lib.fmx_locate_batch(self._h, chars.ctypes.data, offsets.ctypes.data, n, int(max_matches),
                                   locs.ctypes.data, int(loc_cap), found.ctypes.data, steps.ctypes.data,
                                   status.ctypes.data), "fmx_locate_batch")
        return (locs, found, status, steps) if want_steps else (locs, found, status)

    def locate_all_batch(self, chars, offsets, max_matches=-1, want_steps=False):
        """every hit of every pattern, packed (fmx_locate_all_batch; FM:487-552): the hits of pattern i are
        locs[hit_off[i]:hit_off[i + 1]], in the order locate() stores them.  Returns (locs, hit_off, status[, steps])."""
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        n = len(offsets) - 1
        hit_off = np.zeros(n + 1, dtype=np.int64)
        steps = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        buf = C.c_void_p()
        check(lib.fmx_locate_all_batch(self._h, chars.ctypes.data, offsets.ctypes.data, n, int(max_matches), hit_off.ctypes.data,
                                       C.byref(buf), steps.ctypes.data, status.ctypes.data), "fmx_locate_all_batch")
        total = int(hit_off[n])
        try:  # the library's buffer is copied into an array of NumPy's own and handed back
            locs = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_int32)), shape=(total,)).copy() if total else np.zeros(0, np.int32)
        finally:
            lib.fmx_free_buffer(buf)
        return (locs, hit_off, status, steps) if want_steps else (locs, hit_off, status)

    # ---- the lines that match (fmx.h "THE LINE TABLE", "THE LINES THAT MATCH") ----
    def build_line_table(self, boundary="\n"):
        """make the resident line table for `boundary` (fmx_line_table_build; a second call with the same boundary does nothing,
        another boundary replaces it); returns the number of lines.  Not beside queries on the same index."""
        b = boundary if isinstance(boundary, (int, np.integer)) else ord(boundary)
        n_lines = C.c_int64(0)
        check(lib.fmx_line_table_build(self._h, int(b), C.byref(n_lines)), "fmx_line_table_build")
        return n_lines.value

    def line_table_info(self):
        """(boundary, n_boundaries, bytes) of the resident line table; (-1, 0, 0): none — fmx_line_table_info"""
        b, k, nbytes = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        check(lib.fmx_line_table_info(self._h, C.byref(b), C.byref(k), C.byref(nbytes)), "fmx_line_table_info")
        return b.value, k.value, nbytes.value

    def line_bounds(self, lines):
        """(start, stop) of every line id, the boundary excluded: what extract_batch takes; -1, -1 for an id that is no line"""
        lines = np.ascontiguousarray(lines, dtype=np.int32)
        start = np.zeros(len(lines), dtype=np.int32)
        stop = np.zeros(len(lines), dtype=np.int32)
        check(lib.fmx_line_bounds_batch(self._h, lines.ctypes.data, len(lines), start.ctypes.data, stop.ctypes.data), "fmx_line_bounds_batch")
        return start, stop

    def match_lines_batch(self, chars, offsets, max_lines=0, want_counts=False):
        """the distinct lines of every pattern, packed and ascending (fmx_match_lines_batch): those of pattern i are
        lines[line_off[i]:line_off[i + 1]], at most max_lines of them for max_lines > 0.  Returns (lines, line_off, status
        [, line_count, occurrences]): line_count = all distinct lines of a pattern whatever the limit, occurrences = count()."""
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        n = len(offsets) - 1
        line_off = np.zeros(n + 1, dtype=np.int64)
        line_count = np.zeros(n, dtype=np.int32)
        occurrences = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        buf = C.c_void_p()
        check(lib.fmx_match_lines_batch(self._h, chars.ctypes.data, offsets.ctypes.data, n, int(max_lines), line_off.ctypes.data,
                                        C.byref(buf), line_count.ctypes.data, occurrences.ctypes.data, status.ctypes.data),
              "fmx_match_lines_batch")
        total = int(line_off[n])
        try:  # the library's buffer is copied into an array of NumPy's own and handed back
            lines = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_int32)), shape=(total,)).copy() if total else np.zeros(0, np.int32)
        finally:
            lib.fmx_free_buffer(buf)
        return (lines, line_off, status, line_count, occurrences) if want_counts else (lines, line_off, status)

    def match_query_batch(self, chars, offsets, query_off, term_kind, max_lines=0, want_counts=False):
        """the lines of every QUERY of several terms, packed and ascending (fmx_match_query_batch): the patterns (chars, offsets)
        are terms, query_off (q + 1 entries, from 0 to the number of terms) cuts them into queries, term_kind[t] is 0 ALL (the
        line must hold the term), 1 ANY (at least one of the query's ANY terms), 2 NONE (the line must not hold it); a query
        without an ALL or ANY term has no lines.  Those of query Q are lines[line_off[Q]:line_off[Q + 1]], at most max_lines of
        them for max_lines > 0.  Returns (lines, line_off, status[, line_count, occurrences]): status and occurrences per TERM,
        line_count per query (all its lines whatever the limit)."""
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        query_off = np.ascontiguousarray(query_off, dtype=np.int32)
        term_kind = np.ascontiguousarray(term_kind, dtype=np.uint8)
        n, q = len(offsets) - 1, len(query_off) - 1
        if len(term_kind) != n:
            raise ValueError("term_kind has %d entries for %d terms" % (len(term_kind), n))
        line_off = np.zeros(q + 1, dtype=np.int64)
        line_count = np.zeros(q, dtype=np.int32)
        occurrences = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        buf = C.c_void_p()
        check(lib.fmx_match_query_batch(self._h, chars.ctypes.data, offsets.ctypes.data, n, query_off.ctypes.data, term_kind.ctypes.data, q,
                                        int(max_lines), line_off.ctypes.data, C.byref(buf), line_count.ctypes.data, occurrences.ctypes.data,
                                        status.ctypes.data), "fmx_match_query_batch")
        total = int(line_off[q])
        try:  # the library's buffer is copied into an array of NumPy's own and handed back
            lines = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_int32)), shape=(total,)).copy() if total else np.zeros(0, np.int32)
        finally:
            lib.fmx_free_buffer(buf)
        return (lines, line_off, status, line_count, occurrences) if want_counts else (lines, line_off, status)

    # ---- patterns of character classes (fmx.h "PATTERNS OF CHARACTER CLASSES"; pack_class_patterns, ignore_case, parse_classes) ----
    @staticmethod
    def _class_arrays(alt, pos_off, pat_off):
        alt = np.ascontiguousarray(alt, dtype=np.uint16)
        pos_off = np.ascontiguousarray(pos_off, dtype=np.int32)
        pat_off = np.ascontiguousarray(pat_off, dtype=np.int32)
        return alt, pos_off, pat_off, len(pos_off) - 1, len(pat_off) - 1

    def count_class_batch(self, alt, pos_off, pat_off, max_ranges=CLASS_RANGES_DEFAULT):
        """count() of every class pattern: the sum over the literal strings it spells (fmx_count_class_batch).  (counts, status)"""
        alt, pos_off, pat_off, n_pos, n = self._class_arrays(alt, pos_off, pat_off)
        counts = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        check(lib.fmx_count_class_batch(self._h, alt.ctypes.data, pos_off.ctypes.data, n_pos, pat_off.ctypes.data, n, int(max_ranges),
                                        counts.ctypes.data, status.ctypes.data), "fmx_count_class_batch")
        return counts, status

    def locate_all_class_batch(self, alt, pos_off, pat_off, max_ranges=CLASS_RANGES_DEFAULT):
        """every hit of every class pattern, packed (fmx_locate_all_class_batch): those of pattern i are
        locs[hit_off[i]:hit_off[i + 1]], range after range (every literal's locate() list intact).  (locs, hit_off, status)"""
        alt, pos_off, pat_off, n_pos, n = self._class_arrays(alt, pos_off, pat_off)
        hit_off = np.zeros(n + 1, dtype=np.int64)
        status = np.zeros(n, dtype=np.int32)
        buf = C.c_void_p()
        check(lib.fmx_locate_all_class_batch(self._h, alt.ctypes.data, pos_off.ctypes.data, n_pos, pat_off.ctypes.data, n, int(max_ranges),
                                             hit_off.ctypes.data, C.byref(buf), status.ctypes.data), "fmx_locate_all_class_batch")
        total = int(hit_off[n])
        try:  # the library's buffer is copied into an array of NumPy's own and handed back
            locs = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_int32)), shape=(total,)).copy() if total else np.zeros(0, np.int32)
        finally:
            lib.fmx_free_buffer(buf)
        return locs, hit_off, status

    def match_query_class_batch(self, alt, pos_off, pat_off, query_off, term_kind, max_lines=0, want_counts=False,
                                max_ranges=CLASS_RANGES_DEFAULT):
        """match_query_batch with class patterns as terms (fmx_match_query_class_batch); same returns"""
        alt, pos_off, pat_off, n_pos, n = self._class_arrays(alt, pos_off, pat_off)
        query_off = np.ascontiguousarray(query_off, dtype=np.int32)
        term_kind = np.ascontiguousarray(term_kind, dtype=np.uint8)
        q = len(query_off) - 1
        if len(term_kind) != n:
            raise ValueError("term_kind has %d entries for %d terms" % (len(term_kind), n))
        line_off = np.zeros(q + 1, dtype=np.int64)
        line_count = np.zeros(q, dtype=np.int32)
        occurrences = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        buf = C.c_void_p()
        check(lib.fmx_match_query_class_batch(self._h, alt.ctypes.data, pos_off.ctypes.data, n_pos, pat_off.ctypes.data, n, int(max_ranges),
                                              query_off.ctypes.data, term_kind.ctypes.data, q, int(max_lines), line_off.ctypes.data,
                                              C.byref(buf), line_count.ctypes.data, occurrences.ctypes.data, status.ctypes.data),
              "fmx_match_query_class_batch")
        total = int(line_off[q])
        try:  # the library's buffer is copied into an array of NumPy's own and handed back
            lines = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_int32)), shape=(total,)).copy() if total else np.zeros(0, np.int32)
        finally:
            lib.fmx_free_buffer(buf)
        return (lines, line_off, status, line_count, occurrences) if want_counts else (lines, line_off, status)

    # ---- query terms on the number behind a pattern (fmx.h "THE LINES THAT MATCH A QUERY WITH TERMS ON NUMBERS") ----
    def _match_query_number_call(self, call, where, args, n, query_off, term_kind, num_lo, num_hi, frac_digits, max_lines, want_counts):
        query_off = np.ascontiguousarray(query_off, dtype=np.int32)
        term_kind = np.ascontiguousarray(term_kind, dtype=np.uint8)
        q = len(query_off) - 1
        if len(term_kind) != n:
            raise ValueError("term_kind has %d entries for %d terms" % (len(term_kind), n))
        lo = None if num_lo is None else np.ascontiguousarray(num_lo, dtype=np.int64)
        hi = None if num_hi is None else np.ascontiguousarray(num_hi, dtype=np.int64)
        for a in (lo, hi):
            if a is not None and len(a) != n:
                raise ValueError("num_lo / num_hi have %d entries for %d terms" % (len(a), n))
        line_off = np.zeros(q + 1, dtype=np.int64)
        line_count = np.zeros(q, dtype=np.int32)
        occurrences, kept, not_number, overflow, status = (np.zeros(n, dtype=np.int32) for _ in range(5))
        buf = C.c_void_p()
        check(call(self._h, *args, None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data, int(frac_digits),
                   query_off.ctypes.data, term_kind.ctypes.data, q, int(max_lines), line_off.ctypes.data, C.byref(buf), line_count.ctypes.data,
                   occurrences.ctypes.data, kept.ctypes.data, not_number.ctypes.data, overflow.ctypes.data, status.ctypes.data), where)
        total = int(line_off[q])
        try:  # the library's buffer is copied into an array of NumPy's own and handed back
            lines = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_int32)), shape=(total,)).copy() if total else np.zeros(0, np.int32)
        finally:
            lib.fmx_free_buffer(buf)
        return (lines, line_off, status, line_count, occurrences, kept, not_number, overflow) if want_counts else (lines, line_off, status)

    def match_query_number_batch(self, chars, offsets, query_off, term_kind, num_lo, num_hi, frac_digits=0, max_lines=0, want_counts=False):
        """match_query_batch with terms on the NUMBER behind a pattern (fmx_match_query_number_batch): term t is ranged iff
        num_lo[t] >= 0, and then holds on a line iff one of its hits there is followed by a number (number_stats' value, frac_digits
        as there) with num_lo[t] <= value <= num_hi[t]; 2^63 - 1 is "no upper bound", a negative num_lo[t] a plain string term.
        num_lo = num_hi = None: match_query_batch's answer.  Returns (lines, line_off, status[, line_count, occurrences, kept,
        not_number, overflow]): per TERM the hits in the whole text, those that pass, and those that did not parse, by reason."""
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        return self._match_query_number_call(lib.fmx_match_query_number_batch, "fmx_match_query_number_batch", (chars.ctypes.data, offsets.ctypes.data, len(offsets) - 1),
                                             len(offsets) - 1, query_off, term_kind, num_lo, num_hi, frac_digits, max_lines, want_counts)

    def match_query_number_class_batch(self, alt, pos_off, pat_off, query_off, term_kind, num_lo, num_hi, frac_digits=0, max_lines=0,
                                       want_counts=False, max_ranges=CLASS_RANGES_DEFAULT):
        """match_query_number_batch with class patterns as terms (fmx_match_query_number_class_batch); same returns"""
        alt, pos_off, pat_off, n_pos, n = self._class_arrays(alt, pos_off, pat_off)
        return self._match_query_number_call(lib.fmx_match_query_number_class_batch, "fmx_match_query_number_class_batch",
                                             (alt.ctypes.data, pos_off.ctypes.data, n_pos, pat_off.ctypes.data, n, int(max_ranges)), n, query_off,
                                             term_kind, num_lo, num_hi, frac_digits, max_lines, want_counts)

    # ---- the lines that hold a sequence of terms in order (fmx.h "THE LINES THAT HOLD A SEQUENCE OF TERMS IN ORDER") ----
    def _sequence_call(self, call, where, args, n, query_off, max_lines, want_counts, want_spans):
        query_off = np.ascontiguousarray(query_off, dtype=np.int32)
        q = len(query_off) - 1
        line_off = np.zeros(q + 1, dtype=np.int64)
        line_count = np.zeros(q, dtype=np.int32)
        occurrences = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        buf, spans_at = C.c_void_p(), C.c_void_p()
        check(call(self._h, *args, query_off.ctypes.data, q, int(max_lines), line_off.ctypes.data, C.byref(buf),
                   C.byref(spans_at) if want_spans else None, line_count.ctypes.data, occurrences.ctypes.data, status.ctypes.data), where)
        total = int(line_off[q])
        try:  # the library's buffer (the lines, the spans behind them) is copied into arrays of NumPy's own and handed back
            both = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_int32)), shape=(total * (3 if want_spans else 1),)).copy() if total \
                else np.zeros(0, np.int32)
        finally:
            lib.fmx_free_buffer(buf)
        out = (both[:total], line_off, status)
        if want_counts:
            out += (line_count, occurrences)
        if want_spans:
            out += (both[total:].reshape(total, 2),)
        return out

    def match_sequence_batch(self, chars, offsets, query_off, max_lines=0, want_counts=False, want_spans=False):
        """the lines of every SEQUENCE of terms, packed and ascending (fmx_match_sequence_batch; grep 'A.*B'): the patterns (chars,
        offsets) are terms, query_off (q + 1 entries, from 0 to the number of terms) cuts them into sequences; a line belongs to
        a sequence iff it holds occurrences of its terms in the order they stand in, inside the line, without overlap.  Those of
        sequence Q are lines[line_off[Q]:line_off[Q + 1]], at most max_lines of them for max_lines > 0.  Returns (lines, line_off,
        status[, line_count, occurrences][, spans]): status and occurrences per TERM, line_count per sequence (all its lines
        whatever the limit), spans[i] = (start, stop) for lines[i]: the leftmost start and from there the earliest end (what the
        non-greedy A.*?B matches), not the tightest window."""
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        return self._sequence_call(lib.fmx_match_sequence_batch, "fmx_match_sequence_batch", (chars.ctypes.data, offsets.ctypes.data, len(offsets) - 1),
                                   len(offsets) - 1, query_off, max_lines, want_counts, want_spans)

    def match_sequence_class_batch(self, alt, pos_off, pat_off, query_off, max_lines=0, want_counts=False, want_spans=False,
                                   max_ranges=CLASS_RANGES_DEFAULT):
        """match_sequence_batch with class patterns as terms (fmx_match_sequence_class_batch; a term's length is its number of
        positions); same returns"""
        alt, pos_off, pat_off, n_pos, n = self._class_arrays(alt, pos_off, pat_off)
        return self._sequence_call(lib.fmx_match_sequence_class_batch, "fmx_match_sequence_class_batch",
                                   (alt.ctypes.data, pos_off.ctypes.data, n_pos, pat_off.ctypes.data, n, int(max_ranges)), n, query_off, max_lines,
                                   want_counts, want_spans)

    # ---- the values that follow a pattern, with counts (fmx.h "THE VALUES THAT FOLLOW A PATTERN, WITH COUNTS") ----
    def _values_call(self, call, where, args, n, stop, max_len, n_terms=None):
        """n_terms: the `where` forms, which also fill kept (per pattern, in front of status) and term_status (behind it)"""
        stop = as_chars(stop)
        val_off = np.zeros(n + 1, dtype=np.int64)
        occurrences = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        buf, toff_at, chars_at = C.c_void_p(), C.c_void_p(), C.c_void_p()
        if n_terms is None:
            tail = (status.ctypes.data,)
        else:
            kept = np.zeros(n, dtype=np.int32)
            term_status = np.zeros(n_terms, dtype=np.int32)
            tail = (kept.ctypes.data, status.ctypes.data, term_status.ctypes.data)
        check(call(self._h, *args, stop.ctypes.data, len(stop), int(max_len), val_off.ctypes.data, C.byref(buf), C.byref(toff_at),
                   C.byref(chars_at), occurrences.ctypes.data, *tail), where)
        groups = int(val_off[n])
        try:  # the library's buffer (counts, offsets and code units in one block) is copied into arrays of NumPy's own
            if groups:
                counts = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_int32)), shape=(groups,)).copy()
                text_off = np.ctypeslib.as_array(C.cast(toff_at, C.POINTER(C.c_int64)), shape=(groups + 1,)).copy()
                units = int(text_off[groups])
                chars = np.ctypeslib.as_array(C.cast(chars_at, C.POINTER(C.c_uint16)), shape=(units,)).copy() if units else np.zeros(0, np.uint16)
            else:
                counts, text_off, chars = np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.uint16)
        finally:
            lib.fmx_free_buffer(buf)
        if n_terms is not None:
            return chars, text_off, counts, val_off, status, occurrences, kept, term_status
        return chars, text_off, counts, val_off, status, occurrences

    def field_values_batch(self, chars, offsets, stop, max_len):
        """the distinct VALUES that follow every pattern, with the number of hits that have each (fmx_field_values_batch; grep -o |
        sort | uniq -c): the value of a hit is the text behind the pattern up to, not including, the first code unit of `stop`
        (str or code units, at most 64), at most max_len (1 .. 64) units.  Returns (chars, text_off, counts, val_off, status,
        occurrences): the values of pattern i are the groups val_off[i] .. val_off[i + 1] - 1, ascending by code unit, a value in
        front of its extensions; group g is chars[text_off[g]:text_off[g + 1]] and counts[g] hits have it."""
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        n = len(offsets) - 1
        return self._values_call(lib.fmx_field_values_batch, "fmx_field_values_batch", (chars.ctypes.data, offsets.ctypes.data, n), n, stop, max_len)

    def field_values_class_batch(self, alt, pos_off, pat_off, stop, max_len, max_ranges=CLASS_RANGES_DEFAULT):
        """field_values_batch with class patterns (fmx_field_values_class_batch; a pattern's length is its number of positions): the
        values behind ALL spellings of a pattern make one answer; same returns"""
        alt, pos_off, pat_off, n_pos, n = self._class_arrays(alt, pos_off, pat_off)
        return self._values_call(lib.fmx_field_values_class_batch, "fmx_field_values_class_batch",
                                 (alt.ctypes.data, pos_off.ctypes.data, n_pos, pat_off.ctypes.data, n, int(max_ranges)), n, stop, max_len)

    # ---- ... only within the lines of a query (fmx.h "THE VALUES THAT FOLLOW A PATTERN, WHERE THE LINE MATCHES A QUERY") ----
    @staticmethod
    def _where_arrays(n, n_terms, query_off, term_kind, where_of, lines):
        query_off = np.ascontiguousarray(query_off, dtype=np.int32)
        term_kind = np.ascontiguousarray(term_kind, dtype=np.uint8)
        where_of = np.ascontiguousarray(where_of, dtype=np.int32)
        if len(term_kind) != n_terms:
            raise ValueError("term_kind has %d entries for %d terms" % (len(term_kind), n_terms))
        if len(where_of) != n:
            raise ValueError("where_of has %d entries for %d patterns" % (len(where_of), n))
        lo, hi = (0, LINES_ALL) if lines is None else (int(lines[0]), int(lines[1]))
        return query_off, term_kind, where_of, len(query_off) - 1, lo, hi

    def field_values_where_batch(self, chars, offsets, term_chars, term_offsets, query_off, term_kind, where_of, stop, max_len, lines=None):
        """field_values_batch over the hits that lie in the lines of a query and in a window of lines
        (fmx_field_values_where_batch; grep terminating | grep -o 'blk_[^ ]*' | sort | uniq -c).  The terms (term_chars,
        term_offsets) are cut into queries by query_off / term_kind exactly as in match_query_batch; a hit of pattern i counts iff
        its line — the line of its first character — is in lines = (lo, hi), lo <= line < hi (None: every line), and
        where_of[i] < 0 or the line matches query where_of[i].  Needs build_line_table() unless nothing filters.  Returns
        (chars, text_off, counts, val_off, status, occurrences, kept, term_status): as field_values_batch, occurrences still the
        pattern's count in the whole text, kept[i] the hits that passed (the counts of a pattern's values add up to it)."""
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        term_chars = np.ascontiguousarray(term_chars, dtype=np.uint16)
        term_offsets = np.ascontiguousarray(term_offsets, dtype=np.int32)
        n, n_terms = len(offsets) - 1, len(term_offsets) - 1
        query_off, term_kind, where_of, q, lo, hi = self._where_arrays(n, n_terms, query_off, term_kind, where_of, lines)
        return self._values_call(lib.fmx_field_values_where_batch, "fmx_field_values_where_batch",
                                 (chars.ctypes.data, offsets.ctypes.data, n, term_chars.ctypes.data, term_offsets.ctypes.data, n_terms,
                                  query_off.ctypes.data, term_kind.ctypes.data, q, where_of.ctypes.data, lo, hi), n, stop, max_len, n_terms)

    def field_values_where_class_batch(self, alt, pos_off, pat_off, term_alt, term_pos_off, term_pat_off, query_off, term_kind, where_of, stop,
                                       max_len, lines=None, max_ranges=CLASS_RANGES_DEFAULT):
        """field_values_where_batch with class patterns as value patterns and as terms (fmx_field_values_where_class_batch); same
        returns"""
        alt, pos_off, pat_off, n_pos, n = self._class_arrays(alt, pos_off, pat_off)
        term_alt, term_pos_off, term_pat_off, term_n_pos, n_terms = self._class_arrays(term_alt, term_pos_off, term_pat_off)
        query_off, term_kind, where_of, q, lo, hi = self._where_arrays(n, n_terms, query_off, term_kind, where_of, lines)
        return self._values_call(lib.fmx_field_values_where_class_batch, "fmx_field_values_where_class_batch",
                                 (alt.ctypes.data, pos_off.ctypes.data, n_pos, pat_off.ctypes.data, n, term_alt.ctypes.data,
                                  term_pos_off.ctypes.data, term_n_pos, term_pat_off.ctypes.data, n_terms, int(max_ranges), query_off.ctypes.data,
                                  term_kind.ctypes.data, q, where_of.ctypes.data, lo, hi), n, stop, max_len, n_terms)

    # ---- matching lines and hits per bucket of lines, the timeline (fmx.h "LINES AND HITS PER BUCKET OF LINES") ----
    @staticmethod
    def _edges(edges):
        edges = np.ascontiguousarray(edges, dtype=np.int32)
        if edges.ndim != 1:
            raise ValueError("edges is one array of line ids")
        return edges, max(len(edges) - 1, 0)

    def _line_histogram_call(self, call, where, args, n, query_off, term_kind, edges, want_counts):
        query_off = np.ascontiguousarray(query_off, dtype=np.int32)
        term_kind = np.ascontiguousarray(term_kind, dtype=np.uint8)
        edges, B = self._edges(edges)
        q = len(query_off) - 1
        if len(term_kind) != n:
            raise ValueError("term_kind has %d entries for %d terms" % (len(term_kind), n))
        hist = np.zeros((q, B), dtype=np.int32)
        line_count = np.zeros(q, dtype=np.int32)
        occurrences = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        check(call(self._h, *args, query_off.ctypes.data, term_kind.ctypes.data, q, edges.ctypes.data, len(edges), hist.ctypes.data,
                   line_count.ctypes.data, occurrences.ctypes.data, status.ctypes.data), where)
        return (hist, status, line_count, occurrences) if want_counts else hist

    def line_histogram_batch(self, chars, offsets, query_off, term_kind, edges, want_counts=False):
        """the matching lines of every QUERY per bucket of lines (fmx_line_histogram_batch; the timeline of a log search): the
        terms, query_off and term_kind are match_query_batch's; edges = B + 1 line ids that never decrease, bucket b is the
        lines edges[b] <= L < edges[b + 1], a line outside edges[0] .. edges[B] is counted nowhere.  Returns the (q, B) int32
        array — the lines themselves stay on the device —, with want_counts (hist, status, line_count, occurrences): status and
        occurrences per TERM, line_count per query."""
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        n = len(offsets) - 1
        return self._line_histogram_call(lib.fmx_line_histogram_batch, "fmx_line_histogram_batch", (chars.ctypes.data, offsets.ctypes.data, n), n,
                                         query_off, term_kind, edges, want_counts)

    def line_histogram_class_batch(self, alt, pos_off, pat_off, query_off, term_kind, edges, want_counts=False, max_ranges=CLASS_RANGES_DEFAULT):
        """line_histogram_batch with class patterns as terms (fmx_line_histogram_class_batch); same returns"""
        alt, pos_off, pat_off, n_pos, n = self._class_arrays(alt, pos_off, pat_off)
        return self._line_histogram_call(lib.fmx_line_histogram_class_batch, "fmx_line_histogram_class_batch",
                                         (alt.ctypes.data, pos_off.ctypes.data, n_pos, pat_off.ctypes.data, n, int(max_ranges)), n, query_off,
                                         term_kind, edges, want_counts)

    def _hit_histogram_call(self, call, where, args, n, n_terms, query_off, term_kind, where_of, edges, want_counts):
        query_off, term_kind, where_of, q, _, _ = self._where_arrays(n, n_terms, query_off, term_kind, where_of, None)
        edges, B = self._edges(edges)
        hist = np.zeros((n, B), dtype=np.int32)
        occurrences, kept, status = (np.zeros(n, dtype=np.int32) for _ in range(3))
        term_status = np.zeros(n_terms, dtype=np.int32)
        check(call(self._h, *args, query_off.ctypes.data, term_kind.ctypes.data, q, where_of.ctypes.data, edges.ctypes.data, len(edges),
                   hist.ctypes.data, occurrences.ctypes.data, kept.ctypes.data, status.ctypes.data, term_status.ctypes.data), where)
        return (hist, status, occurrences, kept, term_status) if want_counts else hist

    def hit_histogram_where_batch(self, chars, offsets, term_chars, term_offsets, query_off, term_kind, where_of, edges, want_counts=False):
        """the hits of every pattern per bucket of lines, only within the lines of a query (fmx_hit_histogram_where_batch):
        field_values_where_batch's patterns, terms, query_off, term_kind and where_of, no window and no values; edges as in
        line_histogram_batch.  A hit belongs to the line of its first character and counts as often as it occurs.  Returns the
        (n, B) int32 array, with want_counts (hist, status, occurrences, kept, term_status); row i adds up to kept[i] when the
        edges span every line.  Needs build_line_table()."""
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        term_chars = np.ascontiguousarray(term_chars, dtype=np.uint16)
        term_offsets = np.ascontiguousarray(term_offsets, dtype=np.int32)
        n, n_terms = len(offsets) - 1, len(term_offsets) - 1
        return self._hit_histogram_call(lib.fmx_hit_histogram_where_batch, "fmx_hit_histogram_where_batch",
                                        (chars.ctypes.data, offsets.ctypes.data, n, term_chars.ctypes.data, term_offsets.ctypes.data, n_terms), n,
                                        n_terms, query_off, term_kind, where_of, edges, want_counts)

    def hit_histogram_where_class_batch(self, alt, pos_off, pat_off, term_alt, term_pos_off, term_pat_off, query_off, term_kind, where_of, edges,
                                        want_counts=False, max_ranges=CLASS_RANGES_DEFAULT):
        """hit_histogram_where_batch with class patterns as value patterns and as terms (fmx_hit_histogram_where_class_batch); same
        returns"""
        alt, pos_off, pat_off, n_pos, n = self._class_arrays(alt, pos_off, pat_off)
        term_alt, term_pos_off, term_pat_off, term_n_pos, n_terms = self._class_arrays(term_alt, term_pos_off, term_pat_off)
        return self._hit_histogram_call(lib.fmx_hit_histogram_where_class_batch, "fmx_hit_histogram_where_class_batch",
                                        (alt.ctypes.data, pos_off.ctypes.data, n_pos, pat_off.ctypes.data, n, term_alt.ctypes.data,
                                         term_pos_off.ctypes.data, term_n_pos, term_pat_off.ctypes.data, n_terms, int(max_ranges)), n, n_terms,
                                        query_off, term_kind, where_of, edges, want_counts)

    # ---- statistics of the number behind a pattern, per bucket of lines (fmx.h "THE NUMBER BEHIND A PATTERN") ----
    def _number_stats_call(self, call, where, args, n, n_terms, query_off, term_kind, where_of, edges, permille, frac_digits):
        query_off, term_kind, where_of, q, _, _ = self._where_arrays(n, n_terms, query_off, term_kind, where_of, None)
        if edges is None:
            edges_ptr, n_edges, B = None, 0, 1
        else:
            edges, B = self._edges(edges)
            edges_ptr, n_edges = edges.ctypes.data, len(edges)
        permille = np.ascontiguousarray(permille, dtype=np.int32).reshape(-1)
        P = len(permille)
        count = np.zeros((n, B), dtype=np.int32)
        sum_lo, sum_hi = np.zeros((n, B), dtype=np.uint64), np.zeros((n, B), dtype=np.uint64)
        vmin, vmax = np.zeros((n, B), dtype=np.int64), np.zeros((n, B), dtype=np.int64)
        pct = np.zeros((n, B, P), dtype=np.int64)
        not_number, overflow, occurrences, kept, status = (np.zeros(n, dtype=np.int32) for _ in range(5))
        term_status = np.zeros(n_terms, dtype=np.int32)
        check(call(self._h, *args, query_off.ctypes.data, term_kind.ctypes.data, q, where_of.ctypes.data, edges_ptr, n_edges, int(frac_digits),
                   permille.ctypes.data, P, count.ctypes.data, sum_lo.ctypes.data, sum_hi.ctypes.data, vmin.ctypes.data, vmax.ctypes.data,
                   pct.ctypes.data, not_number.ctypes.data, overflow.ctypes.data, occurrences.ctypes.data, kept.ctypes.data, status.ctypes.data,
                   term_status.ctypes.data), where)
        return dict(count=count, sum_lo=sum_lo, sum_hi=sum_hi, min=vmin, max=vmax, pct=pct, not_number=not_number, overflow=overflow,
                    occurrences=occurrences, kept=kept, status=status, term_status=term_status)

    def number_stats_where_batch(self, chars, offsets, term_chars, term_offsets, query_off, term_kind, where_of, edges=None, permille=(500, 950),
                                 frac_digits=0):
        """statistics of the number behind every hit of every pattern per bucket of lines, only within the lines of a query
        (fmx_number_stats_where_batch): hit_histogram_where_batch's patterns, terms, query_off, term_kind, where_of and edges
        (edges=None: one bucket, every line).  The number is the run of digits behind the pattern, with frac_digits in [0, 9] a
        '.' and up to that many digits more, scaled by 10^frac_digits; permille: up to 16 nearest-rank percentiles in
        thousandths.  Returns a dict of arrays: count (n, B) int32; sum_lo, sum_hi (n, B) uint64, the exact sum sum_hi * 2^64 +
        sum_lo; min, max (n, B) int64; pct (n, B, P) int64; not_number, overflow, occurrences, kept, status (n); term_status."""
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        term_chars = np.ascontiguousarray(term_chars, dtype=np.uint16)
        term_offsets = np.ascontiguousarray(term_offsets, dtype=np.int32)
        n, n_terms = len(offsets) - 1, len(term_offsets) - 1
        return self._number_stats_call(lib.fmx_number_stats_where_batch, "fmx_number_stats_where_batch",
                                       (chars.ctypes.data, offsets.ctypes.data, n, term_chars.ctypes.data, term_offsets.ctypes.data, n_terms), n,
                                       n_terms, query_off, term_kind, where_of, edges, permille, frac_digits)

    def number_stats_where_class_batch(self, alt, pos_off, pat_off, term_alt, term_pos_off, term_pat_off, query_off, term_kind, where_of, edges=None,
                                       permille=(500, 950), frac_digits=0, max_ranges=CLASS_RANGES_DEFAULT):
        """number_stats_where_batch with class patterns as value patterns and as terms (fmx_number_stats_where_class_batch); same
        returns"""
        alt, pos_off, pat_off, n_pos, n = self._class_arrays(alt, pos_off, pat_off)
        term_alt, term_pos_off, term_pat_off, term_n_pos, n_terms = self._class_arrays(term_alt, term_pos_off, term_pat_off)
        return self._number_stats_call(lib.fmx_number_stats_where_class_batch, "fmx_number_stats_where_class_batch",
                                       (alt.ctypes.data, pos_off.ctypes.data, n_pos, pat_off.ctypes.data, n, term_alt.ctypes.data,
                                        term_pos_off.ctypes.data, term_n_pos, term_pat_off.ctypes.data, n_terms, int(max_ranges)), n, n_terms,
                                       query_off, term_kind, where_of, edges, permille, frac_digits)

    # ---- the lines ranked by the number behind a pattern (fmx.h "THE LINES RANKED BY THE NUMBER BEHIND A PATTERN") ----
    def _top_lines_call(self, call, where, args, n, n_terms, query_off, term_kind, where_of, descending, top, first, lines, frac_digits):
        query_off, term_kind, where_of, q, lo, hi = self._where_arrays(n, n_terms, query_off, term_kind, where_of, lines)
        descending = np.ascontiguousarray(descending, dtype=np.uint8).reshape(-1)
        if len(descending) != n:
            raise ValueError("descending has %d entries for %d patterns" % (len(descending), n))
        top = int(top)
        cells = max(top, 0)
        rows, n_lines, numbers, not_number, overflow, occurrences, kept, status = (np.zeros(n, dtype=np.int32) for _ in range(8))
        row_line, row_loc = np.zeros((n, cells), dtype=np.int32), np.zeros((n, cells), dtype=np.int32)
        row_value = np.zeros((n, cells), dtype=np.int64)
        term_status = np.zeros(n_terms, dtype=np.int32)
        check(call(self._h, *args, query_off.ctypes.data, term_kind.ctypes.data, q, where_of.ctypes.data, lo, hi, descending.ctypes.data,
                   int(frac_digits), int(first), top, rows.ctypes.data, row_line.ctypes.data, row_value.ctypes.data, row_loc.ctypes.data,
                   n_lines.ctypes.data, numbers.ctypes.data, not_number.ctypes.data, overflow.ctypes.data, occurrences.ctypes.data,
                   kept.ctypes.data, status.ctypes.data, term_status.ctypes.data), where)
        return dict(rows=rows, row_line=row_line, row_value=row_value, row_loc=row_loc, lines=n_lines, numbers=numbers, not_number=not_number,
                    overflow=overflow, occurrences=occurrences, kept=kept, status=status, term_status=term_status)

    def top_lines_where_batch(self, chars, offsets, term_chars, term_offsets, query_off, term_kind, where_of, descending, top=10, first=0,
                              lines=None, frac_digits=0):
        """the lines ranked by the number behind every pattern, only within the lines of a query and a window of lines
        (fmx_top_lines_where_batch; ... | sort -k latency -nr | head -10): number_stats_where_batch's patterns, terms, query_off,
        term_kind, where_of and frac_digits, field_values_where_batch's lines=(lo, hi).  descending[i] = 1: largest first, 0: smallest
        first.  The candidate of a line is its best parsing hit (equal values: the smallest position); the candidates are ranked by
        value, equal values by line id, and the ranks first .. first + top - 1 come down.  Returns a dict of arrays: rows (n);
        row_line, row_loc (n, top) int32 and row_value (n, top) int64, zero behind rows[i]; lines, numbers, not_number, overflow,
        occurrences, kept, status (n); term_status.  Needs build_line_table()."""
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        term_chars = np.ascontiguousarray(term_chars, dtype=np.uint16)
        term_offsets = np.ascontiguousarray(term_offsets, dtype=np.int32)
        n, n_terms = len(offsets) - 1, len(term_offsets) - 1
        return self._top_lines_call(lib.fmx_top_lines_where_batch, "fmx_top_lines_where_batch",
                                    (chars.ctypes.data, offsets.ctypes.data, n, term_chars.ctypes.data, term_offsets.ctypes.data, n_terms), n,
                                    n_terms, query_off, term_kind, where_of, descending, top, first, lines, frac_digits)

    def top_lines_where_class_batch(self, alt, pos_off, pat_off, term_alt, term_pos_off, term_pat_off, query_off, term_kind, where_of, descending,
                                    top=10, first=0, lines=None, frac_digits=0, max_ranges=CLASS_RANGES_DEFAULT):
        """top_lines_where_batch with class patterns as value patterns and as terms (fmx_top_lines_where_class_batch); same returns"""
        alt, pos_off, pat_off, n_pos, n = self._class_arrays(alt, pos_off, pat_off)
        term_alt, term_pos_off, term_pat_off, term_n_pos, n_terms = self._class_arrays(term_alt, term_pos_off, term_pat_off)
        return self._top_lines_call(lib.fmx_top_lines_where_class_batch, "fmx_top_lines_where_class_batch",
                                    (alt.ctypes.data, pos_off.ctypes.data, n_pos, pat_off.ctypes.data, n, term_alt.ctypes.data,
                                     term_pos_off.ctypes.data, term_n_pos, term_pat_off.ctypes.data, n_terms, int(max_ranges)), n, n_terms,
                                    query_off, term_kind, where_of, descending, top, first, lines, frac_digits)

    # ---- ... grouped by the value of a field of the same line (fmx.h "STATISTICS BY KEY") ----
    def number_stats_by_batch(self, key_chars, key_offsets, chars, offsets, by_of, term_chars, term_offsets, query_off, term_kind, key_where_of,
                              where_of, stop, max_len, lines=None, permille=(500, 950), frac_digits=0):
        """statistics of the number behind every hit of the n number patterns (chars, offsets), grouped by the value behind the key
        pattern by_of[i] of (key_chars, key_offsets) on the same line (fmx_number_stats_by_batch; stats count, sum(bytes=),
        p95(latency_ms=) by status=).  The key of a line is field_values' value (stop, max_len) of the key pattern's first kept hit
        on it; terms, query_off, term_kind and lines are field_values_where_batch's, key_where_of / where_of its where_of for the
        key and the number patterns.  Needs build_line_table().  Returns a dict of arrays: val_off (m + 1), lines (G, the lines
        that have each key), text_off (G + 1), chars — the groups as field_values_batch returns them; row_off (n + 1), count,
        sum_lo, sum_hi, min, max (R), pct (R, P) — row row_off[i] + g is number pattern i in group g of key by_of[i]; no_key,
        not_number, overflow, occurrences, kept, status (n); key_occurrences, key_kept, key_status (m); term_status."""
        key_chars = np.ascontiguousarray(key_chars, dtype=np.uint16)
        key_offsets = np.ascontiguousarray(key_offsets, dtype=np.int32)
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        term_chars = np.ascontiguousarray(term_chars, dtype=np.uint16)
        term_offsets = np.ascontiguousarray(term_offsets, dtype=np.int32)
        by_of = np.ascontiguousarray(by_of, dtype=np.int32)
        m, n, n_terms = len(key_offsets) - 1, len(offsets) - 1, len(term_offsets) - 1
        head = (key_chars.ctypes.data, key_offsets.ctypes.data, m, chars.ctypes.data, offsets.ctypes.data, n, by_of.ctypes.data, term_chars.ctypes.data,
                term_offsets.ctypes.data, n_terms)
        return self._number_stats_by_call(lib.fmx_number_stats_by_batch, "fmx_number_stats_by_batch", head, m, n, n_terms, by_of, query_off, term_kind,
                                          key_where_of, where_of, stop, max_len, lines, permille, frac_digits)

    def number_stats_by_class_batch(self, key_alt, key_pos_off, key_pat_off, alt, pos_off, pat_off, by_of, term_alt, term_pos_off, term_pat_off, query_off,
                                    term_kind, key_where_of, where_of, stop, max_len, lines=None, permille=(500, 950), frac_digits=0,
                                    max_ranges=CLASS_RANGES_DEFAULT):
        """number_stats_by_batch with class patterns as key patterns, as number patterns and as terms (fmx_number_stats_by_class_batch; a
        pattern's length is its number of positions): the keys and numbers behind ALL spellings of a pattern make one answer; same
        returns"""
        key_alt, key_pos_off, key_pat_off, key_n_pos, m = self._class_arrays(key_alt, key_pos_off, key_pat_off)
        alt, pos_off, pat_off, n_pos, n = self._class_arrays(alt, pos_off, pat_off)
        term_alt, term_pos_off, term_pat_off, term_n_pos, n_terms = self._class_arrays(term_alt, term_pos_off, term_pat_off)
        by_of = np.ascontiguousarray(by_of, dtype=np.int32)
        head = (key_alt.ctypes.data, key_pos_off.ctypes.data, key_n_pos, key_pat_off.ctypes.data, m, alt.ctypes.data, pos_off.ctypes.data, n_pos,
                pat_off.ctypes.data, n, by_of.ctypes.data, term_alt.ctypes.data, term_pos_off.ctypes.data, term_n_pos, term_pat_off.ctypes.data, n_terms,
                int(max_ranges))
        return self._number_stats_by_call(lib.fmx_number_stats_by_class_batch, "fmx_number_stats_by_class_batch", head, m, n, n_terms, by_of, query_off,
                                          term_kind, key_where_of, where_of, stop, max_len, lines, permille, frac_digits)

    def _number_stats_by_call(self, call, name, head, m, n, n_terms, by_of, query_off, term_kind, key_where_of, where_of, stop, max_len, lines, permille,
                              frac_digits):
        if len(by_of) != n:
            raise ValueError("by_of has %d entries for %d patterns" % (len(by_of), n))
        query_off, term_kind, where_of, q, lo, hi = self._where_arrays(n, n_terms, query_off, term_kind, where_of, lines)
        key_where_of = np.ascontiguousarray(key_where_of, dtype=np.int32)
        if len(key_where_of) != m:
            raise ValueError("key_where_of has %d entries for %d key patterns" % (len(key_where_of), m))
        stop = as_chars(stop)
        permille = np.ascontiguousarray(permille, dtype=np.int32).reshape(-1)
        P = len(permille)
        val_off, row_off = np.zeros(m + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
        no_key, not_number, overflow, occurrences, kept, status = (np.zeros(n, dtype=np.int32) for _ in range(6))
        key_occurrences, key_kept, key_status = (np.zeros(m, dtype=np.int32) for _ in range(3))
        term_status = np.zeros(n_terms, dtype=np.int32)
        ptr = [C.c_void_p() for _ in range(9)]  # lines (the allocation), text_off, chars, count, sum_lo, sum_hi, min, max, pct
        check(call(self._h, *head, query_off.ctypes.data, term_kind.ctypes.data, q, key_where_of.ctypes.data, where_of.ctypes.data, lo, hi,
                   stop.ctypes.data, len(stop), int(max_len), int(frac_digits), permille.ctypes.data, P, val_off.ctypes.data, C.byref(ptr[0]),
                   C.byref(ptr[1]), C.byref(ptr[2]), row_off.ctypes.data, *(C.byref(x) for x in ptr[3:]), no_key.ctypes.data, not_number.ctypes.data,
                   overflow.ctypes.data, occurrences.ctypes.data, kept.ctypes.data, status.ctypes.data, key_occurrences.ctypes.data,
                   key_kept.ctypes.data, key_status.ctypes.data, term_status.ctypes.data), name)
        G, R = int(val_off[m]), int(row_off[n])

        def take(at, ctype, dtype, count):  # (the library's buffer is copied into arrays of NumPy's own)
            if not at or count == 0:
                return np.zeros(count, dtype)
            return np.ctypeslib.as_array(C.cast(at, C.POINTER(ctype)), shape=(count,)).copy()

        try:
            group_lines = take(ptr[0], C.c_int32, np.int32, G)
            text_off = take(ptr[1], C.c_int64, np.int64, G + 1) if ptr[0] else np.zeros(1, np.int64)
            text = take(ptr[2], C.c_uint16, np.uint16, int(text_off[G]))
            count = take(ptr[3], C.c_int32, np.int32, R)
            sum_lo, sum_hi = take(ptr[4], C.c_uint64, np.uint64, R), take(ptr[5], C.c_uint64, np.uint64, R)
            vmin, vmax = take(ptr[6], C.c_int64, np.int64, R), take(ptr[7], C.c_int64, np.int64, R)
            pct = take(ptr[8], C.c_int64, np.int64, R * P).reshape(R, P)
        finally:
            lib.fmx_free_buffer(ptr[0])
        return dict(by_of=by_of.copy(), val_off=val_off, lines=group_lines, text_off=text_off, chars=text, row_off=row_off, count=count, sum_lo=sum_lo, sum_hi=sum_hi,
                    min=vmin, max=vmax, pct=pct, no_key=no_key, not_number=not_number, overflow=overflow, occurrences=occurrences, kept=kept,
                    status=status, key_occurrences=key_occurrences, key_kept=key_kept, key_status=key_status, term_status=term_status)

    # ---- ... grouped by the values of two fields of the same line (fmx.h "STATISTICS BY TWO KEYS") ----
    def number_stats_by_pair_batch(self, key_chars, key_offsets, chars, offsets, by_of, pair_a, pair_b, term_chars, term_offsets, query_off, term_kind,
                                   key_where_of, where_of, stop, max_len, lines=None, permille=(500, 950), frac_digits=0):
        """number_stats_by_batch grouped by PAIRS of key patterns (fmx_number_stats_by_pair_batch; stats p95(latency_ms=) by host=,
        status=): pair j is (pair_a[j], pair_b[j]), two key patterns of the call (they may be equal), and by_of[i] names the pair
        number pattern i is grouped by.  A line has a pair key where it has a key of both patterns; the pairs of j are the distinct
        (group of a, group of b) of its lines, ascending by a's value, then b's.  With no number pattern at all the call answers the
        pairs and their lines (count by a, b).  Returns number_stats_by_batch's dict — val_off, lines, text_off, chars are the single
        keys' groups, the rows run over the pairs of by_of[i] — and pair_a, pair_b, pair_off (c + 1), pair_group_a, pair_group_b,
        pair_lines (one entry per pair: the two groups' indexes among their key patterns' groups, the lines that have the pair)."""
        key_chars = np.ascontiguousarray(key_chars, dtype=np.uint16)
        key_offsets = np.ascontiguousarray(key_offsets, dtype=np.int32)
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        term_chars = np.ascontiguousarray(term_chars, dtype=np.uint16)
        term_offsets = np.ascontiguousarray(term_offsets, dtype=np.int32)
        by_of, pair_a, pair_b = (np.ascontiguousarray(x, dtype=np.int32).reshape(-1) for x in (by_of, pair_a, pair_b))
        m, n, n_terms = len(key_offsets) - 1, len(offsets) - 1, len(term_offsets) - 1
        head = (key_chars.ctypes.data, key_offsets.ctypes.data, m, chars.ctypes.data, offsets.ctypes.data, n, by_of.ctypes.data, len(pair_a),
                pair_a.ctypes.data, pair_b.ctypes.data, term_chars.ctypes.data, term_offsets.ctypes.data, n_terms)
        return self._number_stats_by_pair_call(lib.fmx_number_stats_by_pair_batch, "fmx_number_stats_by_pair_batch", head, m, n, n_terms, by_of, pair_a,
                                               pair_b, query_off, term_kind, key_where_of, where_of, stop, max_len, lines, permille, frac_digits)

    def number_stats_by_pair_class_batch(self, key_alt, key_pos_off, key_pat_off, alt, pos_off, pat_off, by_of, pair_a, pair_b, term_alt, term_pos_off,
                                         term_pat_off, query_off, term_kind, key_where_of, where_of, stop, max_len, lines=None, permille=(500, 950),
                                         frac_digits=0, max_ranges=CLASS_RANGES_DEFAULT):
        """number_stats_by_pair_batch with class patterns as key patterns, as number patterns and as terms
        (fmx_number_stats_by_pair_class_batch); same returns"""
        key_alt, key_pos_off, key_pat_off, key_n_pos, m = self._class_arrays(key_alt, key_pos_off, key_pat_off)
        alt, pos_off, pat_off, n_pos, n = self._class_arrays(alt, pos_off, pat_off)
        term_alt, term_pos_off, term_pat_off, term_n_pos, n_terms = self._class_arrays(term_alt, term_pos_off, term_pat_off)
        by_of, pair_a, pair_b = (np.ascontiguousarray(x, dtype=np.int32).reshape(-1) for x in (by_of, pair_a, pair_b))
        head = (key_alt.ctypes.data, key_pos_off.ctypes.data, key_n_pos, key_pat_off.ctypes.data, m, alt.ctypes.data, pos_off.ctypes.data, n_pos,
                pat_off.ctypes.data, n, by_of.ctypes.data, len(pair_a), pair_a.ctypes.data, pair_b.ctypes.data, term_alt.ctypes.data,
                term_pos_off.ctypes.data, term_n_pos, term_pat_off.ctypes.data, n_terms, int(max_ranges))
        return self._number_stats_by_pair_call(lib.fmx_number_stats_by_pair_class_batch, "fmx_number_stats_by_pair_class_batch", head, m, n, n_terms, by_of,
                                               pair_a, pair_b, query_off, term_kind, key_where_of, where_of, stop, max_len, lines, permille, frac_digits)

    def _number_stats_by_pair_call(self, call, name, head, m, n, n_terms, by_of, pair_a, pair_b, query_off, term_kind, key_where_of, where_of, stop,
                                   max_len, lines, permille, frac_digits):
        if len(by_of) != n:
            raise ValueError("by_of has %d entries for %d patterns" % (len(by_of), n))
        if len(pair_a) != len(pair_b):
            raise ValueError("pair_a has %d entries and pair_b %d" % (len(pair_a), len(pair_b)))
        c = len(pair_a)
        query_off, term_kind, where_of, q, lo, hi = self._where_arrays(n, n_terms, query_off, term_kind, where_of, lines)
        key_where_of = np.ascontiguousarray(key_where_of, dtype=np.int32)
        if len(key_where_of) != m:
            raise ValueError("key_where_of has %d entries for %d key patterns" % (len(key_where_of), m))
        stop = as_chars(stop)
        permille = np.ascontiguousarray(permille, dtype=np.int32).reshape(-1)
        P = len(permille)
        val_off, pair_off, row_off = np.zeros(m + 1, dtype=np.int64), np.zeros(c + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
        no_key, not_number, overflow, occurrences, kept, status = (np.zeros(n, dtype=np.int32) for _ in range(6))
        key_occurrences, key_kept, key_status = (np.zeros(m, dtype=np.int32) for _ in range(3))
        term_status = np.zeros(n_terms, dtype=np.int32)
        # lines (the allocation), text_off, chars, pair_group_a, pair_group_b, pair_lines, count, sum_lo, sum_hi, min, max, pct
        ptr = [C.c_void_p() for _ in range(12)]
        check(call(self._h, *head, query_off.ctypes.data, term_kind.ctypes.data, q, key_where_of.ctypes.data, where_of.ctypes.data, lo, hi,
                   stop.ctypes.data, len(stop), int(max_len), int(frac_digits), permille.ctypes.data, P, val_off.ctypes.data, C.byref(ptr[0]),
                   C.byref(ptr[1]), C.byref(ptr[2]), pair_off.ctypes.data, C.byref(ptr[3]), C.byref(ptr[4]), C.byref(ptr[5]), row_off.ctypes.data,
                   *(C.byref(x) for x in ptr[6:]), no_key.ctypes.data, not_number.ctypes.data, overflow.ctypes.data, occurrences.ctypes.data,
                   kept.ctypes.data, status.ctypes.data, key_occurrences.ctypes.data, key_kept.ctypes.data, key_status.ctypes.data,
                   term_status.ctypes.data), name)
        G, R, pairs = int(val_off[m]), int(row_off[n]), int(pair_off[c])

        def take(at, ctype, dtype, count):  # (the library's buffer is copied into arrays of NumPy's own)
            if not at or count == 0:
                return np.zeros(count, dtype)
            return np.ctypeslib.as_array(C.cast(at, C.POINTER(ctype)), shape=(count,)).copy()

        try:
            group_lines = take(ptr[0], C.c_int32, np.int32, G)
            text_off = take(ptr[1], C.c_int64, np.int64, G + 1) if ptr[0] else np.zeros(1, np.int64)
            text = take(ptr[2], C.c_uint16, np.uint16, int(text_off[G]))
            group_a, group_b, pair_lines = (take(ptr[k], C.c_int32, np.int32, pairs) for k in (3, 4, 5))
            count = take(ptr[6], C.c_int32, np.int32, R)
            sum_lo, sum_hi = take(ptr[7], C.c_uint64, np.uint64, R), take(ptr[8], C.c_uint64, np.uint64, R)
            vmin, vmax = take(ptr[9], C.c_int64, np.int64, R), take(ptr[10], C.c_int64, np.int64, R)
            pct = take(ptr[11], C.c_int64, np.int64, R * P).reshape(R, P)
        finally:
            lib.fmx_free_buffer(ptr[0])
        return dict(by_of=by_of.copy(), pair_a=pair_a.copy(), pair_b=pair_b.copy(), val_off=val_off, lines=group_lines, text_off=text_off, chars=text,
                    pair_off=pair_off, pair_group_a=group_a, pair_group_b=group_b, pair_lines=pair_lines, row_off=row_off, count=count, sum_lo=sum_lo,
                    sum_hi=sum_hi, min=vmin, max=vmax, pct=pct, no_key=no_key, not_number=not_number, overflow=overflow, occurrences=occurrences,
                    kept=kept, status=status, key_occurrences=key_occurrences, key_kept=key_kept, key_status=key_status, term_status=term_status)

    # ---- ... by the value of a field of the same line, per bucket of lines (fmx.h "STATISTICS BY KEY PER BUCKET") ----
    def number_stats_by_histogram_batch(self, key_chars, key_offsets, chars, offsets, by_of, term_chars, term_offsets, query_off, term_kind,
                                        key_where_of, where_of, stop, max_len, edges=None, top=10, permille=(500, 950), frac_digits=0):
        """statistics of the number behind every hit of the n number patterns, by the key of its line (number_stats_by_batch's patterns,
        by_of, terms, query_off, term_kind, key_where_of, where_of, stop, max_len) and per bucket of lines (hit_histogram_where_batch's
        edges; None: one bucket, every line — the device-side top-k of number_stats_by): timechart p95(latency_ms=) by status=
        (fmx_number_stats_by_histogram_batch).  With edges only the hits inside edges[0] .. edges[B] count.  Needs build_line_table().
        Returns a dict of arrays: n_groups (m), key_row_off (m + 1) — the key rows of key pattern k are its min(top, n_groups[k]) groups
        with the most lines, descending, ties in value order —, key_row_lines, key_row_group (R), text_off (R + 1), chars; cell_off
        (n + 1) — cell cell_off[i] + r * B + b is number pattern i, key row r of by_of[i] (the last row: every other key), bucket b —,
        count, sum_lo, sum_hi, min, max (cells), pct (cells, P); no_key, not_number, overflow, occurrences, kept, status (n);
        key_occurrences, key_kept, key_status (m); term_status; buckets (B).  Only the key rows and the cells come down."""
        key_chars = np.ascontiguousarray(key_chars, dtype=np.uint16)
        key_offsets = np.ascontiguousarray(key_offsets, dtype=np.int32)
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        term_chars = np.ascontiguousarray(term_chars, dtype=np.uint16)
        term_offsets = np.ascontiguousarray(term_offsets, dtype=np.int32)
        by_of = np.ascontiguousarray(by_of, dtype=np.int32)
        m, n, n_terms = len(key_offsets) - 1, len(offsets) - 1, len(term_offsets) - 1
        head = (key_chars.ctypes.data, key_offsets.ctypes.data, m, chars.ctypes.data, offsets.ctypes.data, n, by_of.ctypes.data, term_chars.ctypes.data,
                term_offsets.ctypes.data, n_terms)
        return self._number_stats_by_histogram_call(lib.fmx_number_stats_by_histogram_batch, "fmx_number_stats_by_histogram_batch", head, m, n, n_terms,
                                                    by_of, query_off, term_kind, key_where_of, where_of, stop, max_len, edges, top, permille,
                                                    frac_digits)

    def number_stats_by_histogram_class_batch(self, key_alt, key_pos_off, key_pat_off, alt, pos_off, pat_off, by_of, term_alt, term_pos_off,
                                              term_pat_off, query_off, term_kind, key_where_of, where_of, stop, max_len, edges=None, top=10,
                                              permille=(500, 950), frac_digits=0, max_ranges=CLASS_RANGES_DEFAULT):
        """number_stats_by_histogram_batch with class patterns as key patterns, as number patterns and as terms
        (fmx_number_stats_by_histogram_class_batch): the keys and numbers behind ALL spellings of a pattern make one answer; same returns"""
        key_alt, key_pos_off, key_pat_off, key_n_pos, m = self._class_arrays(key_alt, key_pos_off, key_pat_off)
        alt, pos_off, pat_off, n_pos, n = self._class_arrays(alt, pos_off, pat_off)
        term_alt, term_pos_off, term_pat_off, term_n_pos, n_terms = self._class_arrays(term_alt, term_pos_off, term_pat_off)
        by_of = np.ascontiguousarray(by_of, dtype=np.int32)
        head = (key_alt.ctypes.data, key_pos_off.ctypes.data, key_n_pos, key_pat_off.ctypes.data, m, alt.ctypes.data, pos_off.ctypes.data, n_pos,
                pat_off.ctypes.data, n, by_of.ctypes.data, term_alt.ctypes.data, term_pos_off.ctypes.data, term_n_pos, term_pat_off.ctypes.data, n_terms,
                int(max_ranges))
        return self._number_stats_by_histogram_call(lib.fmx_number_stats_by_histogram_class_batch, "fmx_number_stats_by_histogram_class_batch", head,
                                                    m, n, n_terms, by_of, query_off, term_kind, key_where_of, where_of, stop, max_len, edges, top,
                                                    permille, frac_digits)

    def _number_stats_by_histogram_call(self, call, name, head, m, n, n_terms, by_of, query_off, term_kind, key_where_of, where_of, stop, max_len,
                                        edges, top, permille, frac_digits):
        if len(by_of) != n:
            raise ValueError("by_of has %d entries for %d patterns" % (len(by_of), n))
        query_off, term_kind, where_of, q, _, _ = self._where_arrays(n, n_terms, query_off, term_kind, where_of, None)
        key_where_of = np.ascontiguousarray(key_where_of, dtype=np.int32)
        if len(key_where_of) != m:
            raise ValueError("key_where_of has %d entries for %d key patterns" % (len(key_where_of), m))
        if edges is None:
            edges_ptr, n_edges, B = None, 0, 1
        else:
            edges, B = self._edges(edges)
            edges_ptr, n_edges = edges.ctypes.data, len(edges)
        stop = as_chars(stop)
        permille = np.ascontiguousarray(permille, dtype=np.int32).reshape(-1)
        P = len(permille)
        n_groups = np.zeros(m, dtype=np.int32)
        key_row_off, cell_off = np.zeros(m + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
        no_key, not_number, overflow, occurrences, kept, status = (np.zeros(n, dtype=np.int32) for _ in range(6))
        key_occurrences, key_kept, key_status = (np.zeros(m, dtype=np.int32) for _ in range(3))
        term_status = np.zeros(n_terms, dtype=np.int32)
        ptr = [C.c_void_p() for _ in range(10)]  # key_row_lines (the allocation), key_row_group, text_off, chars, count, sum_lo, sum_hi, min, max, pct
        check(call(self._h, *head, query_off.ctypes.data, term_kind.ctypes.data, q, key_where_of.ctypes.data, where_of.ctypes.data, edges_ptr, n_edges,
                   int(top), stop.ctypes.data, len(stop), int(max_len), int(frac_digits), permille.ctypes.data, P, n_groups.ctypes.data,
                   key_row_off.ctypes.data, *(C.byref(x) for x in ptr[:4]), cell_off.ctypes.data, *(C.byref(x) for x in ptr[4:]), no_key.ctypes.data,
                   not_number.ctypes.data, overflow.ctypes.data, occurrences.ctypes.data, kept.ctypes.data, status.ctypes.data,
                   key_occurrences.ctypes.data, key_kept.ctypes.data, key_status.ctypes.data, term_status.ctypes.data), name)
        R, cells = int(key_row_off[m]), int(cell_off[n])

        def take(at, ctype, dtype, count):  # (the library's buffer is copied into arrays of NumPy's own)
            if not at or count == 0:
                return np.zeros(count, dtype)
            return np.ctypeslib.as_array(C.cast(at, C.POINTER(ctype)), shape=(count,)).copy()

        try:
            key_row_lines, key_row_group = take(ptr[0], C.c_int32, np.int32, R), take(ptr[1], C.c_int32, np.int32, R)
            text_off = take(ptr[2], C.c_int64, np.int64, R + 1) if ptr[0] else np.zeros(1, np.int64)
            text = take(ptr[3], C.c_uint16, np.uint16, int(text_off[R]))
            count = take(ptr[4], C.c_int32, np.int32, cells)
            sum_lo, sum_hi = take(ptr[5], C.c_uint64, np.uint64, cells), take(ptr[6], C.c_uint64, np.uint64, cells)
            vmin, vmax = take(ptr[7], C.c_int64, np.int64, cells), take(ptr[8], C.c_int64, np.int64, cells)
            pct = take(ptr[9], C.c_int64, np.int64, cells * P).reshape(cells, P)
        finally:
            lib.fmx_free_buffer(ptr[0])
        return dict(by_of=by_of.copy(), buckets=B, n_groups=n_groups, key_row_off=key_row_off, key_row_lines=key_row_lines, key_row_group=key_row_group,
                    text_off=text_off, chars=text, cell_off=cell_off, count=count, sum_lo=sum_lo, sum_hi=sum_hi, min=vmin, max=vmax, pct=pct,
                    no_key=no_key, not_number=not_number, overflow=overflow, occurrences=occurrences, kept=kept, status=status,
                    key_occurrences=key_occurrences, key_kept=key_kept, key_status=key_status, term_status=term_status)

    # ---- the top values of a field per bucket of lines, the stacked timeline (fmx.h "TOP VALUES PER BUCKET") ----
    def _field_values_histogram_call(self, call, name, head, n, n_terms, query_off, term_kind, where_of, edges, top, stop, max_len):
        query_off, term_kind, where_of, q, _, _ = self._where_arrays(n, n_terms, query_off, term_kind, where_of, None)
        if edges is None:
            edges_ptr, n_edges, B = None, 0, 1
        else:
            edges, B = self._edges(edges)
            edges_ptr, n_edges = edges.ctypes.data, len(edges)
        stop = as_chars(stop)
        n_values, occurrences, kept, status = (np.zeros(n, dtype=np.int32) for _ in range(4))
        row_off = np.zeros(n + 1, dtype=np.int64)
        other = np.zeros((n, B), dtype=np.int32)
        term_status = np.zeros(n_terms, dtype=np.int32)
        ptr = [C.c_void_p() for _ in range(5)]  # row_count (the allocation), row_group, text_off, chars, hist
        check(call(self._h, *head, query_off.ctypes.data, term_kind.ctypes.data, q, where_of.ctypes.data, edges_ptr, n_edges, int(top),
                   stop.ctypes.data, len(stop), int(max_len), n_values.ctypes.data, row_off.ctypes.data, *(C.byref(x) for x in ptr),
                   other.ctypes.data, occurrences.ctypes.data, kept.ctypes.data, status.ctypes.data, term_status.ctypes.data), name)
        R = int(row_off[n])

        def take(at, ctype, dtype, count):  # (the library's buffer is copied into arrays of NumPy's own)
            if not at or count == 0:
                return np.zeros(count, dtype)
            return np.ctypeslib.as_array(C.cast(at, C.POINTER(ctype)), shape=(count,)).copy()

        try:
            row_count, row_group = take(ptr[0], C.c_int32, np.int32, R), take(ptr[1], C.c_int32, np.int32, R)
            text_off = take(ptr[2], C.c_int64, np.int64, R + 1) if ptr[0] else np.zeros(1, np.int64)
            text = take(ptr[3], C.c_uint16, np.uint16, int(text_off[R]))
            hist = take(ptr[4], C.c_int32, np.int32, R * B).reshape(R, B)
        finally:
            lib.fmx_free_buffer(ptr[0])
        return dict(n_values=n_values, row_off=row_off, row_count=row_count, row_group=row_group, text_off=text_off, chars=text, hist=hist,
                    other=other, occurrences=occurrences, kept=kept, status=status, term_status=term_status)

    def field_values_histogram_where_batch(self, chars, offsets, term_chars, term_offsets, query_off, term_kind, where_of, edges=None, top=10,
                                           stop=" ", max_len=64):
        """the top values that follow every pattern, each with its hits per bucket of lines, and the rest as "other"
        (fmx_field_values_histogram_where_batch; count by status over time where line has ...): field_values_where_batch's patterns,
        terms, query_off, term_kind, where_of, stop and max_len, hit_histogram_where_batch's edges (None: one bucket, every line —
        the device-side top-k of field_values).  With edges only the hits inside edges[0] .. edges[B] count.  Returns a dict of
        arrays: n_values (n: the distinct values), row_off (n + 1) — the rows of pattern i are row_off[i] .. row_off[i + 1], its
        min(top, n_values[i]) values with the largest counts, descending, ties in value order —, row_count, row_group (R: the
        value's index among the pattern's values), text_off (R + 1), chars, hist (R, B), other (n, B), occurrences, kept, status (n),
        term_status.  Only the rows come down, however many values a pattern has."""
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        term_chars = np.ascontiguousarray(term_chars, dtype=np.uint16)
        term_offsets = np.ascontiguousarray(term_offsets, dtype=np.int32)
        n, n_terms = len(offsets) - 1, len(term_offsets) - 1
        head = (chars.ctypes.data, offsets.ctypes.data, n, term_chars.ctypes.data, term_offsets.ctypes.data, n_terms)
        return self._field_values_histogram_call(lib.fmx_field_values_histogram_where_batch, "fmx_field_values_histogram_where_batch", head, n,
                                                 n_terms, query_off, term_kind, where_of, edges, top, stop, max_len)

    def field_values_histogram_where_class_batch(self, alt, pos_off, pat_off, term_alt, term_pos_off, term_pat_off, query_off, term_kind, where_of,
                                                 edges=None, top=10, stop=" ", max_len=64, max_ranges=CLASS_RANGES_DEFAULT):
        """field_values_histogram_where_batch with class patterns as value patterns and as terms
        (fmx_field_values_histogram_where_class_batch): the values behind ALL spellings of a pattern make one answer; same returns"""
        alt, pos_off, pat_off, n_pos, n = self._class_arrays(alt, pos_off, pat_off)
        term_alt, term_pos_off, term_pat_off, term_n_pos, n_terms = self._class_arrays(term_alt, term_pos_off, term_pat_off)
        head = (alt.ctypes.data, pos_off.ctypes.data, n_pos, pat_off.ctypes.data, n, term_alt.ctypes.data, term_pos_off.ctypes.data, term_n_pos,
                term_pat_off.ctypes.data, n_terms, int(max_ranges))
        return self._field_values_histogram_call(lib.fmx_field_values_histogram_where_class_batch, "fmx_field_values_histogram_where_class_batch",
                                                 head, n, n_terms, query_off, term_kind, where_of, edges, top, stop, max_len)

    # ---- the distinct values of a field per bucket of lines, dc over time (fmx.h "DISTINCT VALUES PER BUCKET") ----
    def _distinct_values_histogram_call(self, call, name, head, n, n_terms, query_off, term_kind, where_of, edges, stop, max_len):
        query_off, term_kind, where_of, q, _, _ = self._where_arrays(n, n_terms, query_off, term_kind, where_of, None)
        if edges is None:
            edges_ptr, n_edges, B = None, 0, 1
        else:
            edges, B = self._edges(edges)
            edges_ptr, n_edges = edges.ctypes.data, len(edges)
        stop = as_chars(stop)
        n_values, occurrences, kept, status = (np.zeros(n, dtype=np.int32) for _ in range(4))
        distinct, first_seen = np.zeros((n, B), dtype=np.int32), np.zeros((n, B), dtype=np.int32)
        term_status = np.zeros(n_terms, dtype=np.int32)
        check(call(self._h, *head, query_off.ctypes.data, term_kind.ctypes.data, q, where_of.ctypes.data, edges_ptr, n_edges, stop.ctypes.data,
                   len(stop), int(max_len), distinct.ctypes.data, first_seen.ctypes.data, n_values.ctypes.data, occurrences.ctypes.data,
                   kept.ctypes.data, status.ctypes.data, term_status.ctypes.data), name)
        return dict(distinct=distinct, first_seen=first_seen, n_values=n_values, occurrences=occurrences, kept=kept, status=status,
                    term_status=term_status)

    def distinct_values_histogram_where_batch(self, chars, offsets, term_chars, term_offsets, query_off, term_kind, where_of, edges=None, stop=" ",
                                              max_len=64):
        """the number of different values that follow every pattern per bucket of lines, and the number of values seen for the first
        time in each bucket (fmx_distinct_values_histogram_where_batch; timechart dc(user=) where line has ...):
        field_values_histogram_where_batch's arguments without top.  With edges only the hits inside edges[0] .. edges[B] count;
        edges None: one bucket, every line.  Returns a dict of arrays: distinct (n, B), first_seen (n, B), n_values, occurrences, kept,
        status (n), term_status.  n * B pairs of ints come down, however many values a pattern has."""
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        term_chars = np.ascontiguousarray(term_chars, dtype=np.uint16)
        term_offsets = np.ascontiguousarray(term_offsets, dtype=np.int32)
        n, n_terms = len(offsets) - 1, len(term_offsets) - 1
        head = (chars.ctypes.data, offsets.ctypes.data, n, term_chars.ctypes.data, term_offsets.ctypes.data, n_terms)
        return self._distinct_values_histogram_call(lib.fmx_distinct_values_histogram_where_batch, "fmx_distinct_values_histogram_where_batch", head,
                                                    n, n_terms, query_off, term_kind, where_of, edges, stop, max_len)

    def distinct_values_histogram_where_class_batch(self, alt, pos_off, pat_off, term_alt, term_pos_off, term_pat_off, query_off, term_kind,
                                                    where_of, edges=None, stop=" ", max_len=64, max_ranges=CLASS_RANGES_DEFAULT):
        """distinct_values_histogram_where_batch with class patterns as value patterns and as terms
        (fmx_distinct_values_histogram_where_class_batch): the values behind ALL spellings of a pattern make one answer; same returns"""
        alt, pos_off, pat_off, n_pos, n = self._class_arrays(alt, pos_off, pat_off)
        term_alt, term_pos_off, term_pat_off, term_n_pos, n_terms = self._class_arrays(term_alt, term_pos_off, term_pat_off)
        head = (alt.ctypes.data, pos_off.ctypes.data, n_pos, pat_off.ctypes.data, n, term_alt.ctypes.data, term_pos_off.ctypes.data, term_n_pos,
                term_pat_off.ctypes.data, n_terms, int(max_ranges))
        return self._distinct_values_histogram_call(lib.fmx_distinct_values_histogram_where_class_batch,
                                                    "fmx_distinct_values_histogram_where_class_batch", head, n, n_terms, query_off, term_kind,
                                                    where_of, edges, stop, max_len)

    def extract_batch(self, starts, stops, dst_len, offset=0, dst=None, want_steps=False):
        starts = np.ascontiguousarray(starts, dtype=np.int32)
        stops = np.ascontiguousarray(stops, dtype=np.int32)
        n = len(starts)
        if dst is None:
            dst = np.zeros((n, dst_len), dtype=np.uint16)
        out_len = np.zeros(n, dtype=np.int32)
        steps = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        check(lib.fmx_extract_batch(self._h, starts.ctypes.data, stops.ctypes.data, n, dst.ctypes.data, int(dst_len),
                                    int(offset), out_len.ctypes.data, steps.ctypes.data, status.ctypes.data),
              "fmx_extract_batch")
        return (dst, out_len, status, steps) if want_steps else (dst, out_len, status)

    def _packed_text(self, call, where, *args):
        """(chars, text_off, status) of a host form that answers in one packed array of the library's making"""
        n = args[-1]
        text_off = np.zeros(n + 1, dtype=np.int64)
        status = np.zeros(n, dtype=np.int32)
        buf = C.c_void_p()
        check(call(self._h, *args, text_off.ctypes.data, C.byref(buf), status.ctypes.data), where)
        total = int(text_off[n])
        try:  # the library's buffer is copied into an array of NumPy's own and handed back
            chars = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_uint16)), shape=(total,)).copy() if total else np.zeros(0, np.uint16)
        finally:
            lib.fmx_free_buffer(buf)
        return chars, text_off, status

    def extract_packed_batch(self, starts, stops):
        """the text of every range [starts[i], stops[i]) in ONE packed array (fmx_extract_packed_batch; FM:564-608): range i is
        chars[text_off[i]:text_off[i + 1]], what extract(start, stop, destination, 0) leaves in destination[:stop - start]; a
        range with a status, or with stop <= start, is empty.  Returns (chars, text_off, status)."""
        starts = np.ascontiguousarray(starts, dtype=np.int32)
        stops = np.ascontiguousarray(stops, dtype=np.int32)
        if len(starts) != len(stops):
            raise ValueError("%d starts for %d stops" % (len(starts), len(stops)))
        return self._packed_text(lib.fmx_extract_packed_batch, "fmx_extract_packed_batch", starts.ctypes.data, stops.ctypes.data, len(starts))

    def line_text_batch(self, lines):
        """the text of every line id, the boundary excluded, in one packed array (fmx_line_text_batch; needs build_line_table):
        (chars, text_off, status), as extract_packed_batch; an id that is no line is empty and has status ST_POS_NEGATIVE"""
        lines = np.ascontiguousarray(lines, dtype=np.int32)
        return self._packed_text(lib.fmx_line_text_batch, "fmx_line_text_batch", lines.ctypes.data, len(lines))

    def extract_boundary_batch(self, froms, boundary, mode, dst_len, offset=0, dst=None, want_steps=False):
        froms = np.ascontiguousarray(froms, dtype=np.int32)
        n = len(froms)
        if dst is None:
            dst = np.zeros((n, dst_len), dtype=np.uint16)
        out_len = np.zeros(n, dtype=np.int32)
        steps = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        aux = np.zeros(n, dtype=np.int32)
        b = boundary if isinstance(boundary, (int, np.integer)) else ord(boundary)
        check(lib.fmx_extract_boundary_batch(self._h, froms.ctypes.data, n, int(b), int(mode), dst.ctypes.data,
                                             int(dst_len), int(offset), out_len.ctypes.data, steps.ctypes.data,
                                             status.ctypes.data, aux.ctypes.data), "fmx_extract_boundary_batch")
        return (dst, out_len, status, aux, steps) if want_steps else (dst, out_len, status, aux)

    # ---- locate -> extract pipelines (hits stay in HBM between the stages) ----
    def _pipeline(self, chars, offsets, max_matches, row_len, boundary, mode, fill):
        chars = np.ascontiguousarray(chars, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        n = len(offsets) - 1
        mm = int(max_matches)
        out = {
            "locs": np.full((n, mm), -1, dtype=np.int32), "found": np.zeros(n, dtype=np.int32),
            "dst": np.full((n, mm, row_len), fill, dtype=np.uint16), "out_len": np.full((n, mm), -1, dtype=np.int32),
            "steps": np.zeros(n, dtype=np.int32), "status": np.zeros(n, dtype=np.int32),
            "hit_status": np.zeros((n, mm), dtype=np.int32), "hit_aux": np.zeros((n, mm), dtype=np.int32),
        }
        o = out
        if mode < 0:
            check(lib.fmx_locate_extract_batch(self._h, chars.ctypes.data, offsets.ctypes.data, n, mm, int(row_len),
                                               o["locs"].ctypes.data, o["found"].ctypes.data, o["dst"].ctypes.data,
                                               o["out_len"].ctypes.data, o["steps"].ctypes.data, o["status"].ctypes.data,
                                               o["hit_status"].ctypes.data), "fmx_locate_extract_batch")
        else:
            b = boundary if isinstance(boundary, (int, np.integer)) else ord(boundary)
            check(lib.fmx_locate_lines_batch(self._h, chars.ctypes.data, offsets.ctypes.data, n, mm, int(b), int(mode),
                                             int(row_len), o["locs"].ctypes.data, o["found"].ctypes.data,
                                             o["dst"].ctypes.data, o["out_len"].ctypes.data, o["steps"].ctypes.data,
                                             o["status"].ctypes.data, o["hit_status"].ctypes.data,
                                             o["hit_aux"].ctypes.data), "fmx_locate_lines_batch")
        return out

    def locate_extract_batch(self, chars, offsets, max_matches, extract_len, fill=0):
        """locate, then extract(loc, min(getInputLength(), loc + extract_len), row, 0) per hit — the reference's
        locateAndExtractBenchmark (FmIndexThroughputBenchmark.java:231-249).  Returns a dict of arrays; slots
        k >= found[i] keep their initial values (locs/out_len -1, rows `fill`)."""
        return self._pipeline(chars, offsets, max_matches, extract_len, 0, -1, fill)

    def locate_lines_batch(self, chars, offsets, max_matches, boundary, dst_len, mode=0, fill=0):
        """locate, then extractUntilBoundary{,Left,Right}(loc, row, 0, boundary) per hit (FM:640-922)"""
        return self._pipeline(chars, offsets, max_matches, dst_len, boundary, mode, fill)

    # ---- scalar API, as in the reference ----
    def count(self, pattern, offset=0, length=None, ignore_case=False):  # FM:443-474
        p = as_chars(pattern)
        if length is None:
            length = len(p)
        if length <= 0 or offset < 0 or offset + length > len(p):
            raise IndexError("ArrayIndexOutOfBoundsException")  # pattern[i] out of range, FM:456-457
        sub = p[offset:offset + length]
        if ignore_case:  # (the count of every spelling, summed on the device)
            counts, status = self.count_class_batch(*pack_class_patterns([_ignore_case(sub)]))
            raise_for_status(status[0])
            return int(counts[0])
        counts, status = self.count_batch(sub, np.array([0, len(sub)], dtype=np.int32))
        raise_for_status(status[0])
        return int(counts[0])

    def locate(self, pattern, locations, offset=0, length=None, maxMatches=-1):  # FM:487-552
        """`locations` is the caller's int32 array (written in place); returns the number located."""
        p = as_chars(pattern)
        if length is None:
            length = len(p)
        if length <= 0 or offset < 0 or offset + length > len(p):
            raise IndexError("ArrayIndexOutOfBoundsException")
        sub = p[offset:offset + length]
        cap = len(locations)
        rows = np.ascontiguousarray(locations, dtype=np.int32).reshape(1, cap)
        locs, found, status = self.locate_batch(sub, np.array([0, len(sub)], dtype=np.int32), maxMatches, cap, locs=rows)
        locations[:] = locs[0]
        raise_for_status(status[0])
        return int(found[0])

    def locate_all(self, pattern, offset=0, length=None, maxMatches=-1, ignore_case=False):  # FM:487-552
        """all occurrences as an int32 array of the library's making: locate() without the caller's `locations`.  ignore_case:
        the occurrences of every spelling, one spelling after the other (no limit: maxMatches must be -1 or 0)"""
        p = as_chars(pattern)
        if length is None:
            length = len(p)
        if length <= 0 or offset < 0 or offset + length > len(p):
            raise IndexError("ArrayIndexOutOfBoundsException")
        sub = p[offset:offset + length]
        if ignore_case:
            if maxMatches > 0:
                raise ValueError("ignore_case locates every occurrence: maxMatches must be -1 or 0")
            locs, hit_off, status = self.locate_all_class_batch(*pack_class_patterns([_ignore_case(sub)]))
            raise_for_status(status[0])
            return locs
        locs, hit_off, status = self.locate_all_batch(sub, np.array([0, len(sub)], dtype=np.int32), maxMatches)
        raise_for_status(status[0])
        return locs

    def match_lines(self, pattern, max_lines=0, ignore_case=False):
        """the ids of the lines that hold `pattern`, each once, ascending (grep -n); at most max_lines of them for max_lines > 0"""
        p = as_chars(pattern)
        if len(p) == 0:
            raise IndexError("ArrayIndexOutOfBoundsException")
        if ignore_case:
            return self.match_query(all=[p], max_lines=max_lines, ignore_case=True)
        lines, line_off, status = self.match_lines_batch(p, np.array([0, len(p)], dtype=np.int32), max_lines)
        raise_for_status(status[0])
        return lines

    def match_query(self, all=(), any=(), none=(), max_lines=0, ignore_case=False, frac_digits=0):  # noqa: A002 (the words of the query)
        """the ids of the lines that hold every pattern of `all`, at least one of `any` (if given) and none of `none`, each once,
        ascending; at most max_lines of them for max_lines > 0.  Without `all` and `any` there are no lines (`none` filters).
        ignore_case: every term in any case (class patterns: match_query_class_batch).  A term may be a tuple (pattern, lo, hi): it
        holds on a line iff a hit of `pattern` there is followed by a number in [lo, hi] (None: open; number_stats' value with
        frac_digits) — match_query(all=["addStoredBlock", ("size ", None, 67108863)]); match_query_number_batch runs then."""
        terms, kinds, lo, hi = [], [], [], []
        for kind, group in enumerate((all, any, none)):  # (a lone str is one term, and so is a lone tuple (pattern, lo, hi))
            lone = isinstance(group, str) or (isinstance(group, tuple) and len(group) == 3 and
                                              all_of(b is None or isinstance(b, (int, np.integer)) for b in group[1:]))
            for p in ([group] if lone else group):
                ranged = isinstance(p, tuple)
                if ranged and len(p) != 3:
                    raise ValueError("a ranged term is (pattern, lo, hi)")
                terms.append(as_chars(p[0] if ranged else p))
                kinds.append(kind)
                lo.append(-1 if not ranged else 0 if p[1] is None else int(p[1]))
                hi.append(-1 if not ranged else NUMBER_MAX if p[2] is None else int(p[2]))
                if ranged and not (0 <= lo[-1] <= NUMBER_MAX and 0 <= hi[-1] <= NUMBER_MAX):
                    raise ValueError("the bounds of a ranged term lie in [0, 2^63 - 1]")
        if min((len(t) for t in terms), default=1) == 0:
            raise IndexError("ArrayIndexOutOfBoundsException")
        if max(lo, default=-1) >= 0:  # (some term is ranged)
            if ignore_case:
                packed = pack_class_patterns([_ignore_case(t) for t in terms])
                lines, line_off, status = self.match_query_number_class_batch(*packed, [0, len(terms)], np.array(kinds, np.uint8), lo, hi,
                                                                              frac_digits, max_lines)
            else:
                lines, line_off, status = self.match_query_number_batch(*pack_patterns(terms), [0, len(terms)], np.array(kinds, np.uint8), lo, hi,
                                                                        frac_digits, max_lines)
        elif ignore_case:
            packed = pack_class_patterns([_ignore_case(t) for t in terms])
            lines, line_off, status = self.match_query_class_batch(*packed, [0, len(terms)], np.array(kinds, np.uint8), max_lines)
        else:
            chars, offsets = pack_patterns(terms)
            lines, line_off, status = self.match_query_batch(chars, offsets, [0, len(terms)], np.array(kinds, np.uint8), max_lines)
        for st in status:
            raise_for_status(st)
        return lines

    def number_range_count(self, pattern, lo=None, hi=None, frac_digits=0, ignore_case=False):
        """(kept, not_number, overflow, occurrences) of `pattern`: its hits whose number (number_stats' value with frac_digits) lies in
        [lo, hi] (None: open), those that are followed by no number or by one above 2^63 - 1, and count()"""
        p = as_chars(pattern)
        if len(p) == 0:
            raise IndexError("ArrayIndexOutOfBoundsException")
        lo, hi = [0 if lo is None else int(lo)], [NUMBER_MAX if hi is None else int(hi)]
        if not (0 <= lo[0] <= NUMBER_MAX and 0 <= hi[0] <= NUMBER_MAX):
            raise ValueError("the bounds lie in [0, 2^63 - 1]")
        if ignore_case:
            out = self.match_query_number_class_batch(*pack_class_patterns([_ignore_case(p)]), [0, 1], [0], lo, hi, frac_digits, 1, True)
        else:
            out = self.match_query_number_batch(*pack_patterns([p]), [0, 1], [0], lo, hi, frac_digits, 1, True)
        raise_for_status(out[2][0])
        return int(out[5][0]), int(out[6][0]), int(out[7][0]), int(out[4][0])

    def match_sequence(self, terms, max_lines=0, ignore_case=False, want_spans=False):
        """the ids of the lines that hold the terms in this order, without overlap (grep 'A.*B.*C'), each once, ascending; at most
        max_lines of them for max_lines > 0.  No terms: no lines.  want_spans: (lines, spans), spans[i] = (start, stop) of the
        non-greedy match on lines[i].  ignore_case: every term in any case (class patterns: match_sequence_class_batch)."""
        terms = [as_chars(p) for p in ([terms] if isinstance(terms, str) else terms)]
        if min((len(t) for t in terms), default=1) == 0:
            raise IndexError("ArrayIndexOutOfBoundsException")
        if ignore_case:
            out = self.match_sequence_class_batch(*pack_class_patterns([_ignore_case(t) for t in terms]), [0, len(terms)], max_lines,
                                                  want_spans=want_spans)
        else:
            out = self.match_sequence_batch(*pack_patterns(terms), [0, len(terms)], max_lines, want_spans=want_spans)
        for st in out[2]:
            raise_for_status(st)
        return (out[0], out[3]) if want_spans else out[0]

    def _values_where(self, pattern, where, lines, stop, max_len, ignore_case, count_only=False):
        """one pattern through field_values_where_batch / field_values_where_class_batch: where = dict(all=, any=, none=) is ONE
        query (match_query's words; None: no query), lines = (lo, hi) a window of line ids (None: every line)"""
        p = as_chars(pattern)
        terms, kinds = [], []
        for kind, word in enumerate(("all", "any", "none")):
            group = (where or {}).get(word, ())
            for t in ([group] if isinstance(group, str) else group):  # (a lone str is one term)
                terms.append(as_chars(t))
                kinds.append(kind)
        if where is not None and set(where) - {"all", "any", "none"}:
            raise ValueError("where takes all=, any= and none=")
        if min((len(t) for t in terms + [p]), default=1) == 0:
            raise IndexError("ArrayIndexOutOfBoundsException")
        query_off, where_of = ([0, len(terms)], [0]) if where is not None else ([0], [-1])
        if ignore_case:
            out = self.field_values_where_class_batch(*pack_class_patterns([_ignore_case(p)]), *pack_class_patterns([_ignore_case(t) for t in terms]),
                                                      query_off, np.array(kinds, np.uint8), where_of, stop, max_len, lines)
        else:
            out = self.field_values_where_batch(*pack_patterns([p]), *pack_patterns(terms), query_off, np.array(kinds, np.uint8), where_of, stop,
                                                max_len, lines)
        for st in [out[4][0]] + out[7].tolist():
            if not (count_only and st == 1):  # (kept is filled on an index built without extraction too)
                raise_for_status(st)
        return out

    def count_where(self, pattern, where=None, lines=None, ignore_case=False):
        """the occurrences of `pattern` inside the lines that match where = dict(all=, any=, none=) (match_query's words) and lie in
        lines = (lo, hi): grep ... | grep -o pattern | wc -l.  A hit belongs to the line of its first character."""
        return int(self._values_where(pattern, where, lines, "", 1, ignore_case, count_only=True)[6][0])

    def field_values(self, pattern, stop=" \t\r\n", max_len=32, top=None, ignore_case=False, where=None, lines=None):
        """[(value, count)] of the distinct values that follow `pattern` (grep -o 'pattern[^stop]*' | sort | uniq -c): ascending by
        UTF-16 code unit, a value in front of its extensions; with top=k the k entries with the largest counts, ties by value
        (sorted on the host over the groups).  ignore_case: the pattern in any case, one answer for all spellings.
        where=dict(all=, any=, none=) and lines=(lo, hi): only the hits in the lines that match that query (match_query's words)
        and lie in that window of line ids — count by value WHERE the line holds ...; needs build_line_table()."""
        p = as_chars(pattern)
        if len(p) == 0:
            raise IndexError("ArrayIndexOutOfBoundsException")
        if where is not None or lines is not None:
            out = self._values_where(p, where, lines, stop, max_len, ignore_case)[:6]
        elif ignore_case:
            out = self.field_values_class_batch(*pack_class_patterns([_ignore_case(p)]), stop, max_len)
        else:
            out = self.field_values_batch(*pack_patterns([p]), stop, max_len)
        chars, text_off, counts, _, status, _ = out
        raise_for_status(status[0])
        values = [chars[a:b].tobytes().decode("utf-16-le", "surrogatepass") for a, b in zip(text_off[:-1], text_off[1:])]
        pairs = list(zip(values, counts.tolist()))
        if top is not None:  # (a stable sort: equal counts keep the order of the values)
            pairs = sorted(pairs, key=lambda vc: -vc[1])[:max(int(top), 0)]
        return pairs

    def line_histogram(self, edges, all=(), any=(), none=(), ignore_case=False):  # noqa: A002 (the words of the query)
        """the lines of match_query(all, any, none) per bucket of lines: B = len(edges) - 1 ints, bucket b the lines edges[b] <= L <
        edges[b + 1] (the timeline; an edge from a timestamp: match_lines("081109 2035", max_lines=1) is the first line of that
        minute).  Only the B counters come down."""
        terms, kinds = [], []
        for kind, group in enumerate((all, any, none)):  # (a lone str is one term)
            for p in ([group] if isinstance(group, str) else group):
                terms.append(as_chars(p))
                kinds.append(kind)
        if min((len(t) for t in terms), default=1) == 0:
            raise IndexError("ArrayIndexOutOfBoundsException")
        if ignore_case:
            out = self.line_histogram_class_batch(*pack_class_patterns([_ignore_case(t) for t in terms]), [0, len(terms)], np.array(kinds, np.uint8),
                                                  edges, want_counts=True)
        else:
            out = self.line_histogram_batch(*pack_patterns(terms), [0, len(terms)], np.array(kinds, np.uint8), edges, want_counts=True)
        for st in out[1]:
            raise_for_status(st)
        return out[0][0]

    def hit_histogram(self, pattern, edges, where=None, ignore_case=False):
        """the occurrences of `pattern` per bucket of lines (edges as in line_histogram), with where=dict(all=, any=, none=) only
        those in the lines that match that query: B = len(edges) - 1 ints.  A hit belongs to the line of its first character; two
        on one line are two."""
        p = as_chars(pattern)
        terms, kinds = [], []
        for kind, word in enumerate(("all", "any", "none")):
            group = (where or {}).get(word, ())
            for t in ([group] if isinstance(group, str) else group):  # (a lone str is one term)
                terms.append(as_chars(t))
                kinds.append(kind)
        if where is not None and set(where) - {"all", "any", "none"}:
            raise ValueError("where takes all=, any= and none=")
        if min((len(t) for t in terms + [p]), default=1) == 0:
            raise IndexError("ArrayIndexOutOfBoundsException")
        query_off, where_of = ([0, len(terms)], [0]) if where is not None else ([0], [-1])
        if ignore_case:
            out = self.hit_histogram_where_class_batch(*pack_class_patterns([_ignore_case(p)]), *pack_class_patterns([_ignore_case(t) for t in terms]),
                                                       query_off, np.array(kinds, np.uint8), where_of, edges, want_counts=True)
        else:
            out = self.hit_histogram_where_batch(*pack_patterns([p]), *pack_patterns(terms), query_off, np.array(kinds, np.uint8), where_of, edges,
                                                 want_counts=True)
        for st in [out[1][0]] + out[4].tolist():
            raise_for_status(st)
        return out[0][0]

    def number_stats(self, pattern, edges=None, where=None, permille=(500, 950), frac_digits=0, ignore_case=False):
        """sum, min, max and percentiles of the number behind `pattern` per bucket of lines (edges as in hit_histogram; None: one
        bucket, every line), with where=dict(all=, any=, none=) only over the hits in the lines that match that query: stats
        sum(size) p95(size) by minute where line has addStoredBlock.  "size 67108864" is 67108864; with frac_digits=3 "251.73" is
        251730.  Returns a NumberStats: count, sum (Python ints, exact), min, max (B), pct (B, P), mean(), and not_number,
        overflow, occurrences, kept as ints.  Only the rows come down."""
        p = as_chars(pattern)
        terms, kinds = [], []
        for kind, word in enumerate(("all", "any", "none")):
            group = (where or {}).get(word, ())
            for t in ([group] if isinstance(group, str) else group):  # (a lone str is one term)
                terms.append(as_chars(t))
                kinds.append(kind)
        if where is not None and set(where) - {"all", "any", "none"}:
            raise ValueError("where takes all=, any= and none=")
        if min((len(t) for t in terms + [p]), default=1) == 0:
            raise IndexError("ArrayIndexOutOfBoundsException")
        query_off, where_of = ([0, len(terms)], [0]) if where is not None else ([0], [-1])
        if ignore_case:
            out = self.number_stats_where_class_batch(*pack_class_patterns([_ignore_case(p)]), *pack_class_patterns([_ignore_case(t) for t in terms]),
                                                      query_off, np.array(kinds, np.uint8), where_of, edges, permille, frac_digits)
        else:
            out = self.number_stats_where_batch(*pack_patterns([p]), *pack_patterns(terms), query_off, np.array(kinds, np.uint8), where_of, edges,
                                                permille, frac_digits)
        for st in [out["status"][0]] + out["term_status"].tolist():
            raise_for_status(st)
        return NumberStats(out, 0)

    def top_lines_by_number(self, pattern, top=10, largest=True, first=0, where=None, lines=None, frac_digits=0, ignore_case=False, text=False):
        """the `top` lines ranked by the number behind `pattern`, from rank `first` on: ... | sort -k latency -nr | head -10 — the ten
        slowest requests, the largest blocks, with largest=False the smallest.  A line counts with its best number (two ids on one
        line: the larger, or with largest=False the smaller; equal numbers: the first); equal numbers of two lines rank by line id.
        where=dict(all=, any=, none=) and lines=(lo, hi) keep only the hits in the lines that match, as in field_values; frac_digits
        as in number_stats.  Returns a TopLines: line, value, loc (arrays, best first) and lines, numbers, not_number, overflow,
        kept, occurrences as ints; with text=True also text, the rows' lines as str (line_text_batch).  Needs build_line_table().
        Only the rows come down."""
        p = as_chars(pattern)
        terms, kinds = [], []
        for kind, word in enumerate(("all", "any", "none")):
            group = (where or {}).get(word, ())
            for t in ([group] if isinstance(group, str) else group):  # (a lone str is one term)
                terms.append(as_chars(t))
                kinds.append(kind)
        if where is not None and set(where) - {"all", "any", "none"}:
            raise ValueError("where takes all=, any= and none=")
        if min((len(t) for t in terms + [p]), default=1) == 0:
            raise IndexError("ArrayIndexOutOfBoundsException")
        query_off, where_of = ([0, len(terms)], [0]) if where is not None else ([0], [-1])
        if ignore_case:
            out = self.top_lines_where_class_batch(*pack_class_patterns([_ignore_case(p)]), *pack_class_patterns([_ignore_case(t) for t in terms]),
                                                   query_off, np.array(kinds, np.uint8), where_of, [1 if largest else 0], top, first, lines,
                                                   frac_digits)
        else:
            out = self.top_lines_where_batch(*pack_patterns([p]), *pack_patterns(terms), query_off, np.array(kinds, np.uint8), where_of,
                                             [1 if largest else 0], top, first, lines, frac_digits)
        for st in [out["status"][0]] + out["term_status"].tolist():
            raise_for_status(st)
        res = TopLines(out, 0)
        if text:
            res.text = self.line_text(res.line)
        return res

    def number_stats_by(self, pattern, by, stop=" \t\r\n", max_len=32, where=None, lines=None, permille=(500, 950), frac_digits=0, top=None,
                        ignore_case=False):
        """statistics of the number behind `pattern` grouped by the value behind `by` on the same line: stats count, sum(bytes=),
        p95(latency_ms=) by status=.  The key of a line is field_values' value (stop, max_len) of the first hit of `by` on it;
        where=dict(all=, any=, none=) and lines=(lo, hi) filter the hits of both patterns as in field_values.  Returns a
        NumberStatsBy: groups = [dict(value, lines, count, sum (a Python int, exact), min, max, pct, mean)] in field_values' order —
        with top=k the k groups with the most lines, ties by value, sorted on the host — and no_key, not_number, overflow,
        occurrences, kept, key_occurrences, key_kept as ints.  ignore_case: both patterns and the filter's terms in any case, one
        answer for all spellings (the values keep the text's case).  Needs build_line_table().  Only the groups and rows come down."""
        p, k = as_chars(pattern), as_chars(by)
        terms, kinds = [], []
        for kind, word in enumerate(("all", "any", "none")):
            group = (where or {}).get(word, ())
            for t in ([group] if isinstance(group, str) else group):  # (a lone str is one term)
                terms.append(as_chars(t))
                kinds.append(kind)
        if where is not None and set(where) - {"all", "any", "none"}:
            raise ValueError("where takes all=, any= and none=")
        if min((len(t) for t in terms + [p, k]), default=1) == 0:
            raise IndexError("ArrayIndexOutOfBoundsException")
        query_off, where_of = ([0, len(terms)], [0]) if where is not None else ([0], [-1])
        if ignore_case:
            out = self.number_stats_by_class_batch(*pack_class_patterns([_ignore_case(k)]), *pack_class_patterns([_ignore_case(p)]), [0],
                                                   *pack_class_patterns([_ignore_case(t) for t in terms]), query_off, np.array(kinds, np.uint8),
                                                   where_of, where_of, stop, max_len, lines, permille, frac_digits)
        else:
            out = self.number_stats_by_batch(*pack_patterns([k]), *pack_patterns([p]), [0], *pack_patterns(terms), query_off, np.array(kinds, np.uint8),
                                             where_of, where_of, stop, max_len, lines, permille, frac_digits)
        for st in [out["status"][0], out["key_status"][0]] + out["term_status"].tolist():
            raise_for_status(st)
        return NumberStatsBy(out, top)

    def _by_pair(self, pattern, by_a, by_b, stop, max_len, where, lines, permille, frac_digits, ignore_case):
        """one call of number_stats_by_pair_batch for the pair (by_a, by_b): one number pattern, or none at all (pattern is None)"""
        numbers = [] if pattern is None else [as_chars(pattern)]
        keys = [as_chars(by_a), as_chars(by_b)]
        terms, kinds = [], []
        for kind, word in enumerate(("all", "any", "none")):
            group = (where or {}).get(word, ())
            for t in ([group] if isinstance(group, str) else group):  # (a lone str is one term)
                terms.append(as_chars(t))
                kinds.append(kind)
        if where is not None and set(where) - {"all", "any", "none"}:
            raise ValueError("where takes all=, any= and none=")
        if min((len(t) for t in terms + numbers + keys), default=1) == 0:
            raise IndexError("ArrayIndexOutOfBoundsException")
        query_off, w = ([0, len(terms)], 0) if where is not None else ([0], -1)
        by_of, key_where, num_where = [0] * len(numbers), [w, w], [w] * len(numbers)
        if ignore_case:
            out = self.number_stats_by_pair_class_batch(*pack_class_patterns([_ignore_case(k) for k in keys]),
                                                        *pack_class_patterns([_ignore_case(p) for p in numbers]), by_of, [0], [1],
                                                        *pack_class_patterns([_ignore_case(t) for t in terms]), query_off, np.array(kinds, np.uint8),
                                                        key_where, num_where, stop, max_len, lines, permille, frac_digits)
        else:
            out = self.number_stats_by_pair_batch(*pack_patterns(keys), *pack_patterns(numbers), by_of, [0], [1], *pack_patterns(terms), query_off,
                                                  np.array(kinds, np.uint8), key_where, num_where, stop, max_len, lines, permille, frac_digits)
        for st in out["status"].tolist() + out["key_status"].tolist() + out["term_status"].tolist():
            raise_for_status(st)
        return out

    def number_stats_by_pair(self, pattern, by_a, by_b, stop=" \t\r\n", max_len=32, where=None, lines=None, permille=(500, 950), frac_digits=0, top=None,
                             ignore_case=False):
        """statistics of the number behind `pattern` grouped by the values behind `by_a` and `by_b` on the same line: stats count,
        p95(latency_ms=) by host=, status=.  The key of a line for each of the two is number_stats_by's; a line counts where it has
        both.  where, lines, permille, frac_digits and ignore_case as there.  Returns a NumberStatsByPair: groups = [dict(values=(a, b),
        lines, count, sum (a Python int, exact), min, max, pct, mean)] in pair order — ascending by a's value, then b's; with top=k
        the k pairs with the most lines, ties in pair order, sorted on the host — and no_key (the kept hits on a line without both
        keys), not_number, overflow, occurrences, kept, key_occurrences, key_kept.  Needs build_line_table().  Only the groups, the
        pairs and the rows come down."""
        return NumberStatsByPair(self._by_pair(pattern, by_a, by_b, stop, max_len, where, lines, permille, frac_digits, ignore_case), top)

    def field_value_pairs(self, by_a, by_b, stop=" \t\r\n", max_len=32, where=None, lines=None, top=None, ignore_case=False):
        """[(a, b, lines)] of the distinct pairs of values behind `by_a` and `by_b` on the same line, each with the lines that have
        it: the pivot table count by host=, status=.  Ascending by a's value, then b's; with top=k the k pairs with the most lines,
        ties in that order (sorted on the host).  The key of a line, where, lines and ignore_case as in number_stats_by_pair, whose
        call without a number pattern this is.  Needs build_line_table()."""
        out = self._by_pair(None, by_a, by_b, stop, max_len, where, lines, (), 0, ignore_case)
        rows = [(a, b, count) for (a, b), count in _pair_values(out, 0)]
        if top is not None:  # (a stable sort: equal line counts keep the pair order)
            rows = sorted(rows, key=lambda r: -r[2])[:max(int(top), 0)]
        return rows

    def number_stats_by_histogram(self, pattern, by, edges=None, top=10, stop=" \t\r\n", max_len=32, where=None, permille=(500, 950), frac_digits=0,
                                  ignore_case=False):
        """statistics of the number behind `pattern` by the value behind `by` on the same line, per bucket of lines: timechart
        p95(latency_ms=) by status= — the `top` keys with the most lines, each with its statistics per bucket, and the rest as
        "other".  The key of a line as in number_stats_by; edges as in hit_histogram (None: one bucket, every line — the top-k of
        number_stats_by, ranked on the device); where=dict(all=, any=, none=) filters the hits of both patterns as in field_values.
        Returns a NumberStatsByHistogram: rows = [dict(value, lines, group, count (B), sum (B Python ints), min, max, pct (B, P))] in
        descending order of lines, ties in value order, other in the same shape, and n_groups, no_key, not_number, overflow, kept,
        occurrences.  Needs build_line_table().  Only the rows come down, however many distinct keys there are."""
        p, k = as_chars(pattern), as_chars(by)
        terms, kinds = [], []
        for kind, word in enumerate(("all", "any", "none")):
            group = (where or {}).get(word, ())
            for t in ([group] if isinstance(group, str) else group):  # (a lone str is one term)
                terms.append(as_chars(t))
                kinds.append(kind)
        if where is not None and set(where) - {"all", "any", "none"}:
            raise ValueError("where takes all=, any= and none=")
        if min((len(t) for t in terms + [p, k]), default=1) == 0:
            raise IndexError("ArrayIndexOutOfBoundsException")
        query_off, where_of = ([0, len(terms)], [0]) if where is not None else ([0], [-1])
        if ignore_case:
            out = self.number_stats_by_histogram_class_batch(*pack_class_patterns([_ignore_case(k)]), *pack_class_patterns([_ignore_case(p)]), [0],
                                                             *pack_class_patterns([_ignore_case(t) for t in terms]), query_off,
                                                             np.array(kinds, np.uint8), where_of, where_of, stop, max_len, edges, top, permille,
                                                             frac_digits)
        else:
            out = self.number_stats_by_histogram_batch(*pack_patterns([k]), *pack_patterns([p]), [0], *pack_patterns(terms), query_off,
                                                       np.array(kinds, np.uint8), where_of, where_of, stop, max_len, edges, top, permille, frac_digits)
        for st in [out["status"][0], out["key_status"][0]] + out["term_status"].tolist():
            raise_for_status(st)
        return NumberStatsByHistogram(out, 0)

    def field_values_histogram(self, pattern, edges=None, top=10, where=None, stop=" ", max_len=64, ignore_case=False):
        """the `top` most frequent values that follow `pattern`, each with its occurrences per bucket of lines, and the rest as
        "other": count by status over time where line has user=svc3, the stacked timeline.  edges as in hit_histogram (None: one
        bucket, every line — the top-k of field_values, ranked on the device); where=dict(all=, any=, none=) as in field_values.
        Returns a FieldValuesHistogram: rows = [dict(value, count, group, hist)] in descending order of count, ties in value order,
        other (B ints), n_values, kept, occurrences.  Only the rows come down, however many distinct values there are."""
        p = as_chars(pattern)
        terms, kinds = [], []
        for kind, word in enumerate(("all", "any", "none")):
            group = (where or {}).get(word, ())
            for t in ([group] if isinstance(group, str) else group):  # (a lone str is one term)
                terms.append(as_chars(t))
                kinds.append(kind)
        if where is not None and set(where) - {"all", "any", "none"}:
            raise ValueError("where takes all=, any= and none=")
        if min((len(t) for t in terms + [p]), default=1) == 0:
            raise IndexError("ArrayIndexOutOfBoundsException")
        query_off, where_of = ([0, len(terms)], [0]) if where is not None else ([0], [-1])
        if ignore_case:
            out = self.field_values_histogram_where_class_batch(*pack_class_patterns([_ignore_case(p)]),
                                                                *pack_class_patterns([_ignore_case(t) for t in terms]), query_off,
                                                                np.array(kinds, np.uint8), where_of, edges, top, stop, max_len)
        else:
            out = self.field_values_histogram_where_batch(*pack_patterns([p]), *pack_patterns(terms), query_off, np.array(kinds, np.uint8), where_of,
                                                          edges, top, stop, max_len)
        for st in [out["status"][0]] + out["term_status"].tolist():
            raise_for_status(st)
        return FieldValuesHistogram(out, 0)

    def distinct_values(self, pattern, edges=None, where=None, stop=" ", max_len=64, ignore_case=False):
        """how many different values follow `pattern` per bucket of lines, and how many of them are seen for the first time there:
        timechart dc(user=) where line has ..., new block ids per minute.  edges as in hit_histogram (None: one bucket, every line);
        where=dict(all=, any=, none=) as in field_values.  Returns a DistinctValues: distinct and first_seen (B ints each), n_values,
        kept, occurrences.  Two ints per bucket come down, however many distinct values there are."""
        p = as_chars(pattern)
        terms, kinds = [], []
        for kind, word in enumerate(("all", "any", "none")):
            group = (where or {}).get(word, ())
            for t in ([group] if isinstance(group, str) else group):  # (a lone str is one term)
                terms.append(as_chars(t))
                kinds.append(kind)
        if where is not None and set(where) - {"all", "any", "none"}:
            raise ValueError("where takes all=, any= and none=")
        if min((len(t) for t in terms + [p]), default=1) == 0:
            raise IndexError("ArrayIndexOutOfBoundsException")
        query_off, where_of = ([0, len(terms)], [0]) if where is not None else ([0], [-1])
        if ignore_case:
            out = self.distinct_values_histogram_where_class_batch(*pack_class_patterns([_ignore_case(p)]),
                                                                   *pack_class_patterns([_ignore_case(t) for t in terms]), query_off,
                                                                   np.array(kinds, np.uint8), where_of, edges, stop, max_len)
        else:
            out = self.distinct_values_histogram_where_batch(*pack_patterns([p]), *pack_patterns(terms), query_off, np.array(kinds, np.uint8),
                                                             where_of, edges, stop, max_len)
        for st in [out["status"][0]] + out["term_status"].tolist():
            raise_for_status(st)
        return DistinctValues(out, 0)

    def line_text(self, lines):
        """the lines with these ids as a list of str (the boundary excluded); raises for an id that is no line"""
        chars, text_off, status = self.line_text_batch(lines)
        for st in status:
            raise_for_status(st)
        return [chars[a:b].tobytes().decode("utf-16-le", "surrogatepass") for a, b in zip(text_off[:-1], text_off[1:])]

    def grep(self, pattern=None, all=(), any=(), none=(), max_lines=0, ignore_case=False, sequence=None, frac_digits=0):  # noqa: A002 (the words of the query)
        """[(line id, line)] of the lines that hold `pattern` — or, without one, that match the query of all / any / none
        (match_query; a term may be (pattern, lo, hi), frac_digits as there), or that hold the terms of `sequence` in order
        (match_sequence; not together with the others: ValueError) — ascending, at most max_lines of them for max_lines > 0:
        match_lines / match_query / match_sequence, then line_text_batch"""
        if sequence is not None:
            if pattern is not None or all or any or none:
                raise ValueError("a sequence, or a pattern, or a query: one of them")
            ids = self.match_sequence(sequence, max_lines, ignore_case=ignore_case)
        elif pattern is not None:
            if all or any or none:
                raise ValueError("a pattern or a query, not both")
            ids = self.match_lines(pattern, max_lines, ignore_case=ignore_case)
        else:
            ids = self.match_query(all, any, none, max_lines, ignore_case=ignore_case, frac_digits=frac_digits)
        return list(zip(ids.tolist(), self.line_text(ids)))

    def extract(self, start, stop, destination, offset=0):  # FM:564-608
        dst = np.ascontiguousarray(destination, dtype=np.uint16).reshape(1, len(destination))
        dst, out_len, status = self.extract_batch([start], [stop], len(destination), offset, dst=dst)
        destination[:] = dst[0]
        raise_for_status(status[0])
        return int(out_len[0])

    def _boundary(self, mode, frm, destination, offset, boundary):
        dst = np.ascontiguousarray(destination, dtype=np.uint16).reshape(1, len(destination))
        dst, out_len, status, aux = self.extract_boundary_batch([frm], boundary, mode, len(destination), offset, dst=dst)
        destination[:] = dst[0]
        raise_for_status(status[0], int(aux[0]))
        return int(out_len[0])

    def extractUntilBoundary(self, frm, destination, offset, boundary):  # FM:640-759
        return self._boundary(0, frm, destination, offset, boundary)

    def extractUntilBoundaryLeft(self, frm, destination, offset, boundary):  # FM:772-831
        return self._boundary(1, frm, destination, offset, boundary)

    def extractUntilBoundaryRight(self, frm, destination, offset, boundary):  # FM:844-922
        return self._boundary(2, frm, destination, offset, boundary)


def synth_log(n, seed=42):
    """deterministic synthetic ASCII log text of exactly n chars"""
    out = np.zeros(n, dtype=np.uint16)
    check(lib.fmx_synth_log(seed, n, out.ctypes.data), "fmx_synth_log")
    return out


def synth_log_multichar(n, symbols=1100, seed=42):
    """the same log with runs of multi-byte characters at word boundaries, `symbols` distinct characters: the shape of the
    reference's fixture HDFS_2k_multichar.log and of the > 1,000-symbol data set its numbers are quoted on"""
    out = np.zeros(n, dtype=np.uint16)
    check(lib.fmx_synth_log_multichar(seed, n, symbols, out.ctypes.data), "fmx_synth_log_multichar")
    return out


def synth_patterns(text, m, count, seed=43):
    """`count` substrings of length m at SplitMix64(seed) % (n - m); returns (chars, offsets, positions)"""
    text = np.ascontiguousarray(text, dtype=np.uint16)
    pat = np.zeros(count * m, dtype=np.uint16)
    off = np.zeros(count + 1, dtype=np.int32)
    pos = np.zeros(count, dtype=np.int32)
    check(lib.fmx_synth_patterns(seed, text.ctypes.data, len(text), m, count, pat.ctypes.data, off.ctypes.data,
                                 pos.ctypes.data), "fmx_synth_patterns")
    return pat, off, pos
