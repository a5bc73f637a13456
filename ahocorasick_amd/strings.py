"""Host-side mirror of the reference's public API (package com.roklenarcic.util.strings) over libacgpu.so.

Same class names, constructor arguments, listener contract and error behaviour as the reference, so the parity
tests read like the reference's own tests:

  StringSet.match(haystack, SetMatchListener)                  S/StringSet.java:3-5
  StringMap.match(haystack, MapMatchListener)                  S/StringMap.java:5-9
  SetMatchListener.match(haystack, start, end) -> bool         S/SetMatchListener.java:6
  MapMatchListener.match(haystack, start, end, value) -> bool  S/MapMatchListener.java:6
  AhoCorasickSet(keywords, caseSensitive)                      S/AhoCorasickSet.java:16
  AhoCorasickMap(keywords, values, caseSensitive)              S/AhoCorasickMap.java:20
  LongestMatchSet / LongestMatchMap                            S/LongestMatchSet.java:15, S/LongestMatchMap.java
  WholeWordMatchSet / WholeWordMatchMap (+ wordCharacters[, toggleFlags])   S/WholeWordMatchMap.java:21-53

The matching itself always runs on the GPU through the C ABI (include/acgpu.h); the listener loop runs here, and
stops at the first listener call that returns False -- which is observationally what the reference does
(S/AhoCorasickSet.java:223-225).  The Thresholder constructor argument of the reference is accepted and ignored
(results-neutral node-representation knob).  StringMap.match also takes a Readable (an object with read(n), or an
iterable of chunks) with a value-only ReadableMatchListener, S/StringMap.java:6-8: match_readable over acgpu_stream_*.

Every native call goes through one body per call shape: _records_call (records into a buffer that grows until they fit),
_rewrite_call (a rewritten text, retried by the caller's rule), _fill_shard (the acgpu_shard of a device call).  StringSet and
StringMap are _Matcher with the two listener loops and the replacement rule of their flavour.
"""
import ctypes
import itertools
import os

import numpy as np

from . import _native as N
from ._native import Utf8Error
from .unicode_tables import (default_word_chars, java_lower_table, word_chars_from_list, word_chars_with_toggles)


class IllegalArgumentException(ValueError):
    """java.lang.IllegalArgumentException of the WholeWord constructors (S/WholeWordMatchMap.java:263-267)."""


def utf16(s):
    """str -> UTF-16 code units exactly as a Java String holds them (surrogate pairs for supplementary chars)."""
    if isinstance(s, str):
        return np.frombuffer(s.encode("utf-16-le", "surrogatepass"), dtype=np.uint16).copy()
    return np.ascontiguousarray(s, dtype=np.uint16)


def _utf8_bytes(data):
    """bytes / bytearray / memoryview / uint8 array -> a contiguous uint8 array over the same memory where that is possible"""
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    return np.frombuffer(data, dtype=np.uint8)


def utf8_unit_offsets(data):
    """The mapping rule of acgpu_match_utf8 (include/acgpu.h) restated on the host, for WELL-FORMED UTF-8: an int64 array with
    one entry per UTF-16 unit the text decodes to; entry u is the byte offset of the first byte of the code point that holds
    unit u (both units of a surrogate pair name the same 4-byte sequence).  A record (start, end) in units is
    (off[start], off[end - 1] + the length of the sequence at off[end - 1]) in bytes.  For tests and tools, not the hot path."""
    b = _utf8_bytes(data)
    leads = np.flatnonzero((b & 0xC0) != 0x80)
    return np.repeat(leads, 1 + (b[leads] >= 0xF0)).astype(np.int64)


def utf8_line_offsets(data):
    """The offsets of the lines of a UTF-8 buffer for the offsets= form of the batch entries: every line with its "\\n", a last
    line without one if the buffer does not end in "\\n" -- bytes.splitlines(keepends=True) of a text whose only line break is
    "\\n" -- as a uint64 array of (lines + 1) entries.  A log file goes in as it is:
    contains_batch_utf8(buf, offsets=utf8_line_offsets(buf))."""
    b = _utf8_bytes(data)
    ends = np.flatnonzero(b == 0x0A).astype(np.uint64) + np.uint64(1)
    tail = [b.size] if b.size and (not ends.size or int(ends[-1]) != b.size) else []
    return np.concatenate([np.zeros(1, np.uint64), ends, np.array(tail, np.uint64)])


def _utf8_entry(name, errors):
    """(the native entry, the stats type it fills) for errors="strict" | "replace" -- the lossy entries scan every maximal
    ill-formed subpart as one U+FFFD, as bytes.decode("utf-8", "replace") does; anything else is refused before a native call"""
    if _check_errors(errors) == "replace":
        name += "_lossy"
    return getattr(N.lib(), name), N.UTF8_STATS[name]


def _check_errors(errors):
    """errors= of a method that reaches its native entry later (a generator's first next(), a stream's first feed): the same
    ValueError, now"""
    if errors not in ("strict", "replace"):
        raise ValueError("errors must be 'strict' or 'replace', not %r" % (errors,))
    return errors


def _pack_utf8(data, offsets):
    """-> (uint8 buffer, uint64 offsets): a sequence of bytes-like haystacks joined once, or with `offsets` ONE buffer used in place"""
    if offsets is not None:
        off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        if off.size < 1:
            raise ValueError("offsets needs at least one entry")
        buf = _utf8_bytes(data)
        if int(off[-1]) > buf.size:
            raise ValueError("offsets reach past the end of the buffer")
        return buf, off
    parts = [_utf8_bytes(h) for h in data]
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        off[1:] = np.cumsum([p.size for p in parts], dtype=np.uint64)
    buf = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return np.ascontiguousarray(buf, dtype=np.uint8), off


def _to_str(units):
    """UTF-16 code units -> str (lone surrogates pass through, as in a Java String)"""
    return np.ascontiguousarray(units, dtype=np.uint16).tobytes().decode("utf-16-le", "surrogatepass")


def _pack(keywords):
    parts = [utf16(k) if k is not None else np.zeros(0, np.uint16) for k in keywords]
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    units = np.concatenate(parts) if parts else np.zeros(0, np.uint16)
    if units.size == 0:
        units = np.zeros(1, np.uint16)
    return np.ascontiguousarray(units, dtype=np.uint16), off


def _vp(a):
    """array -> void* (None -> NULL); the pointer object keeps a reference to the array (numpy: ndarray.ctypes.data_as)"""
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _readable(a):
    """the text of a native call: never an empty array, whose pointer the library would refuse even for n = 0"""
    return a if a.size else np.zeros(1, a.dtype)


def _kind(with_ids):
    return N.REC_MAP if with_ids else N.REC_SET


def _stats_dict(st):
    """a stats struct of integers (N.CountStats, N.ReplaceStats, N.SummaryStats, N.CursorStats) -> dict"""
    return {f: int(getattr(st, f)) for f, _ in st._fields_}


def _profile_dict(prof):
    """N.Profile -> dict"""
    return dict(scan_ms=prof.scan_ms, finalize_ms=prof.finalize_ms, total_ms=prof.total_ms,
                scan_units=prof.scan_units, n_matches=prof.n_matches, scan_kernel=prof.scan_kernel.decode())


def _fill_shard(sh, d_hay, n_units, own=None, text_begin=True, text_end=True, chain_entry=None, d_result=None):
    """The acgpu_shard of a device call, filled in place.  own: (begin, end), None: the whole of d_hay; chain_entry None: the
    chain enters where the owned range begins."""
    sh.d_hay = d_hay
    sh.n_units = n_units
    sh.own_begin, sh.own_end = (0, n_units) if own is None else own
    sh.text_begin = 1 if text_begin else 0
    sh.text_end = 1 if text_end else 0
    sh.chain_entry = sh.own_begin if chain_entry is None else chain_entry
    sh.chain_exit = -1
    sh.d_result = d_result
    return sh


def _raise_for(rc, entry, stats=()):
    """The error mapping of every call with a return code: ACGPU_E_ENCODING with a stats struct that names the place ->
    Utf8Error, anything else but OK -> AcgpuError whose `where` is the entry that was called."""
    if rc == N.E_ENCODING:
        for st in stats:
            if hasattr(st, "first_bad"):
                raise Utf8Error(st.first_bad, haystack=getattr(st, "bad_haystack", None))
    N.check(rc, entry.__name__)


def _new_records(cap, cols):
    return np.empty((cap, cols), dtype=np.int32)


def _records_call(entry, head, kind, cols, cap, tail=(), stats=None, alloc=_new_records):
    """The records call: entry(*head, kind, out, cap, &n_out, *tail[, &stats]) into a (cap, cols) int32 buffer from alloc ->
    the rows that were written.  ACGPU_E_OVERFLOW consumed nothing and reports the capacity that is needed in n_out: the same
    call again with exactly that, as often as the entry asks.  stats: the UTF-8 stats struct of an entry that has one."""
    extra = tail if stats is None else tail + (ctypes.byref(stats),)
    while True:
        out = alloc(cap, cols)
        n_out = ctypes.c_uint64(0)
        rc = entry(*head, kind, _vp(out), cap, ctypes.byref(n_out), *extra)
        if rc != N.E_OVERFLOW:
            break
        cap = int(n_out.value)
    _raise_for(rc, entry, (stats,))
    return out[:n_out.value]


def _retry_once(attempt, asked, cap):
    """the rule of Automaton's rewrite calls: the first call reports the size, the second has it; a second overflow is an error"""
    return attempt == 0


def _retry_while_more(attempt, asked, cap):
    """the rule of a stream's rewrite feeds: again as long as the entry asks for more room than it was given"""
    return asked > cap


def _rewrite_call(entry, head, dtype, n, cap, stats, retry, mid=()):
    """The rewrite call: entry(*head, out, cap, *mid, &n_out, *&stats) into a buffer of cap elements of dtype -> the elements
    that were written.  cap None: the text's size n and a quarter.  ACGPU_E_OVERFLOW committed nothing and reports the size that is
    needed in n_out; retry(attempt, that size, cap) says whether the call is made again with it, otherwise it is an error."""
    if cap is None:
        cap = n + n // 4 + 64
    tail = [ctypes.byref(s) for s in stats]
    attempt = 0
    while True:
        out = np.empty(max(cap, 1), dtype=dtype)
        n_out = ctypes.c_uint64(0)
        rc = entry(*head, _vp(out), cap, *mid, ctypes.byref(n_out), *tail)
        if rc != N.E_OVERFLOW or not retry(attempt, int(n_out.value), cap):
            break
        cap, attempt = int(n_out.value), attempt + 1
    _raise_for(rc, entry, stats)
    return out[:n_out.value]


def configured_devices():
    """The device list of match(String, ...): the environment variable ACGPU_DEVICES ("0,1,2,3"), this mirror's counterpart of
    the Java facade's system property -Dacgpu.devices=....  None: the current device alone."""
    v = os.environ.get("ACGPU_DEVICES", "").strip()
    return [int(x) for x in v.split(",") if x.strip() != ""] if v else None


class Automaton:
    """Owns one acgpu_automaton handle."""

    def __init__(self, mode, keywords, case_sensitive, word_chars=None, lower=None):
        L = N.lib()
        units, off = _pack(keywords)
        self.keywords = keywords
        lower_t = None
        if not case_sensitive:
            lower_t = np.ascontiguousarray(java_lower_table() if lower is None else lower, dtype=np.uint16)
        wc = None if word_chars is None else np.ascontiguousarray(word_chars, dtype=np.uint8)
        h = ctypes.c_void_p()
        bad = ctypes.c_int64(-1)
        rc = L.acgpu_build(mode, _vp(units), _vp(off), len(off) - 1, 1 if case_sensitive else 0, _vp(lower_t), _vp(wc),
                           ctypes.byref(h), ctypes.byref(bad))
        if rc == N.E_NONWORD:
            kw = keywords[bad.value]
            raise IllegalArgumentException("%s contains non-word characters." % (kw if isinstance(kw, str) else bad.value))
        N.check(rc, "acgpu_build")
        self._h = h
        self.mode = mode
        self.word_chars = wc

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                N.lib().acgpu_free(h)
            except Exception:
                pass
            self._h = None

    @property
    def handle(self):
        return self._h

    def info(self):
        i = N.Info()
        N.check(N.lib().acgpu_get_info(self._h, ctypes.byref(i)), "acgpu_get_info")
        return {f: getattr(i, f) for f, _ in N.Info._fields_}

    def match_host(self, hay_units, with_ids, cap=None, devices=None):
        """acgpu_match_u16 -- or, with a device list (argument, or ACGPU_DEVICES), acgpu_match_u16_multi: haystack in host
        memory -> (n, 2|3) int32 array in reference call order."""
        hay = np.ascontiguousarray(hay_units, dtype=np.uint16)
        n = int(hay.size)
        kind = _kind(with_ids)
        head = (self._h, _vp(_readable(hay)), n)
        if devices is None:
            devices = configured_devices()
        if devices:
            entry, head = N.lib().acgpu_match_u16_multi, head + ((ctypes.c_int * len(devices))(*devices), len(devices))
        else:
            entry = N.lib().acgpu_match_u16
        return _records_call(entry, head, kind, kind // 4, max(4096, n // 64) if cap is None else cap)

    def match_utf8(self, data, with_ids, cap=None, stats=None, errors="strict"):
        """acgpu_match_utf8: a UTF-8 haystack (bytes, bytearray, memoryview or uint8 array) in host memory -> (n, 2|3) int32 array
        in reference call order with BYTE offsets into `data`, end exclusive.  Ill-formed input raises Utf8Error (.start as
        UnicodeDecodeError.start).  stats: an N.Utf8Stats to fill in, if wanted.  errors="replace": acgpu_match_utf8_lossy --
        the records of data.decode("utf-8", "replace"), a replaced subpart's U+FFFD mapped to its bytes; nothing is raised, and
        stats is an N.Utf8LossyStats."""
        entry, stats_type = _utf8_entry("acgpu_match_utf8", errors)
        buf = _utf8_bytes(data)
        n = int(buf.size)
        kind = _kind(with_ids)
        return _records_call(entry, (self._h, _vp(_readable(buf)), n), kind, kind // 4, max(4096, n // 64) if cap is None else cap,
                             stats=stats if stats is not None else stats_type())

    def match_batch(self, haystacks, with_ids, cap=None):
        """acgpu_match_batch_u16: many short haystacks (str or uint16 arrays) in one call -> (n, 3|4) int32 array of
        (haystack index, start, end[, keyword index]) records, haystack by haystack in reference call order."""
        units, off = _pack(haystacks)
        kind = _kind(with_ids)
        return _records_call(N.lib().acgpu_match_batch_u16, (self._h, _vp(units), _vp(off), len(off) - 1), kind, kind // 4 + 1,
                             max(4096, int(off[-1]) // 16) if cap is None else cap)

    def match_batch_utf8(self, data, with_ids, cap=None, stats=None, offsets=None, errors="strict"):
        """acgpu_match_batch_utf8: many short UTF-8 haystacks in one call -> (n, 3|4) int32 array of (haystack index, start,
        end[, keyword index]) records, haystack by haystack in reference call order, start and end in BYTES relative to the
        haystack.  data: a sequence of bytes-like objects, joined once on the host; with offsets= (n + 1 ascending byte
        offsets) ONE buffer, used in place.  An ill-formed haystack raises Utf8Error (.haystack, and .start inside it).
        stats: an N.Utf8BatchStats to fill in, if wanted.  errors="replace": acgpu_match_batch_utf8_lossy -- every haystack as
        its own .decode("utf-8", "replace"); nothing is raised, and stats is an N.Utf8LossyStats."""
        entry, stats_type = _utf8_entry("acgpu_match_batch_utf8", errors)
        buf, off = _pack_utf8(data, offsets)
        kind = _kind(with_ids)
        return _records_call(entry, (self._h, _vp(_readable(buf)), _vp(off), len(off) - 1), kind, kind // 4 + 1,
                             max(4096, int(off[-1] - off[0]) // 16) if cap is None else cap,
                             stats=stats if stats is not None else stats_type())

    def summary_batch_utf8(self, data, stats=None, offsets=None, errors="strict"):
        """acgpu_summary_batch_utf8: many short UTF-8 haystacks decided in one call -> (array of N.SUMMARY_DTYPE with one entry
        per haystack: n_matches and the first record in listener order in BYTES relative to the haystack, -1s where there is
        none; stats dict).  data and offsets as for match_batch_utf8; an ill-formed haystack raises Utf8Error.
        errors="replace": acgpu_summary_batch_utf8_lossy, as for match_batch_utf8."""
        entry, stats_type = _utf8_entry("acgpu_summary_batch_utf8", errors)
        buf, off = _pack_utf8(data, offsets)
        n = len(off) - 1
        out = np.zeros(n, dtype=N.SUMMARY_DTYPE)
        st = N.SummaryStats()
        ust = stats if stats is not None else stats_type()
        _raise_for(entry(self._h, _vp(_readable(buf)), _vp(off), n, _vp(out) if n else None, ctypes.byref(st), ctypes.byref(ust)),
                   entry, (ust,))
        return out, _stats_dict(st)

    def match_device(self, d_hay_ptr, n_units, with_ids, d_out_ptr, cap, own=None, text_begin=True, text_end=True,
                     chain_entry=None, stream=0, profile=False, d_result=None):
        """acgpu_match_device on raw device pointers.  Returns (n_out, rc, profile_dict|None, chain_exit)."""
        sh = _fill_shard(N.Shard(), d_hay_ptr, n_units, own, text_begin, text_end, chain_entry, d_result)
        prof = N.Profile() if profile else None
        n_out = ctypes.c_uint64(0)
        rc = N.lib().acgpu_match_device(self._h, ctypes.byref(sh), N.REC_MAP if with_ids else N.REC_SET, d_out_ptr, cap, ctypes.byref(n_out),
                                        ctypes.c_void_p(stream), ctypes.byref(prof) if profile else None)
        return int(n_out.value), rc, _profile_dict(prof) if profile else None, int(sh.chain_exit)

    def count_host(self, hay_units):
        """acgpu_count_u16: haystack in host memory -> (uint64 array with one count per keyword given to the constructor,
        stats dict).  No record leaves the device."""
        hay = np.ascontiguousarray(hay_units, dtype=np.uint16)
        counts = np.zeros(max(len(self.keywords), 1), dtype=np.uint64)
        st = N.CountStats()
        N.check(N.lib().acgpu_count_u16(self._h, _vp(_readable(hay)), int(hay.size), _vp(counts), len(self.keywords), ctypes.byref(st)),
                "acgpu_count_u16")
        return counts[:len(self.keywords)], _stats_dict(st)

    def count_device(self, d_hay_ptr, n_units, d_counts_ptr, own=None, text_begin=True, text_end=True, chain_entry=None, stream=0):
        """acgpu_count_device on raw device pointers: ADDS this shard's counts to the uint64 device array d_counts_ptr (one
        word per keyword given to the constructor, zeroed by the caller).  Returns (rc, stats dict, chain_exit)."""
        sh = _fill_shard(N.Shard(), d_hay_ptr, n_units, own, text_begin, text_end, chain_entry)
        st = N.CountStats()
        rc = N.lib().acgpu_count_device(self._h, ctypes.byref(sh), d_counts_ptr, len(self.keywords), ctypes.c_void_p(stream),
                                        ctypes.byref(st))
        return rc, _stats_dict(st), int(sh.chain_exit)

    def _replacements(self, replacements):
        """one str or uint16 array per keyword, or a single str that stands for every keyword -> (units, offsets, n_repl)"""
        if isinstance(replacements, str):
            replacements = [replacements]
        elif len(replacements) != len(self.keywords):
            raise ValueError("%d replacements for %d keywords" % (len(replacements), len(self.keywords)))
        units, off = _pack(replacements)
        return units, off, len(off) - 1

    def replace_host(self, hay_units, replacements, cap=None):
        """acgpu_replace_u16: haystack in host memory -> (the rewritten text as a uint16 array, stats dict).  `replacements`: a
        list with one str or uint16 array per keyword given to the constructor, or a single str for all of them.  A result
        larger than the first buffer (the text's size and a quarter) is fetched by one more call with the size the first reports."""
        hay = np.ascontiguousarray(hay_units, dtype=np.uint16)
        n = int(hay.size)
        units, off, n_repl = self._replacements(replacements)
        st = N.ReplaceStats()
        out = _rewrite_call(N.lib().acgpu_replace_u16, (self._h, _vp(_readable(hay)), n, _vp(units), _vp(off), n_repl), np.uint16, n, cap,
                            (st,), _retry_once)
        return out, _stats_dict(st)

    def _replacements_utf8(self, replacements):
        """as _replacements, in bytes: a str is encoded as UTF-8; bytes, bytearray and uint8 arrays are taken as they are (and
        not validated) -> (bytes, offsets, n_repl)"""
        if isinstance(replacements, (str, bytes, bytearray)):
            replacements = [replacements]
        elif len(replacements) != len(self.keywords):
            raise ValueError("%d replacements for %d keywords" % (len(replacements), len(self.keywords)))
        parts = [_utf8_bytes(r.encode("utf-8") if isinstance(r, str) else r) for r in replacements]
        off = np.zeros(len(parts) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([p.size for p in parts], dtype=np.uint64)
        blob = np.concatenate(parts + [np.zeros(1, np.uint8)])  # (never an empty array: its pointer is read as "no table")
        return np.ascontiguousarray(blob, dtype=np.uint8), off, len(parts)

    def replace_utf8(self, data, replacements, cap=None, stats=None, errors="strict"):
        """acgpu_replace_utf8: a UTF-8 haystack (bytes, bytearray, memoryview or uint8 array) in host memory -> (the rewritten
        bytes as a uint8 array, stats dict); outside the matches a byte-for-byte copy.  `replacements`: a list with one str
        (encoded as UTF-8), bytes, bytearray or uint8 array per keyword given to the constructor, or a single one for all of
        them.  Ill-formed input raises Utf8Error.  The one retry of replace_host; stats: an N.Utf8Stats to fill in, if wanted.
        errors="replace": acgpu_replace_utf8_lossy -- the matches are those of match_utf8(errors="replace"), outside them the
        result is still a copy of `data`, ill-formed bytes included; nothing is raised, and stats is an N.Utf8LossyStats."""
        entry, stats_type = _utf8_entry("acgpu_replace_utf8", errors)
        buf = _utf8_bytes(data)
        n = int(buf.size)
        r_bytes, off, n_repl = self._replacements_utf8(replacements)
        st = N.ReplaceStats()
        out = _rewrite_call(entry, (self._h, _vp(_readable(buf)), n, _vp(r_bytes), _vp(off), n_repl), np.uint8, n, cap,
                            (st, stats if stats is not None else stats_type()), _retry_once)
        return out, _stats_dict(st)

    def replace_batch_utf8(self, data, replacements, cap=None, stats=None, offsets=None, errors="strict"):
        """acgpu_replace_batch_utf8: many short UTF-8 haystacks rewritten in one call -> (uint8 array, out_offsets, stats dict):
        the result of haystack i is out[out_offsets[i]:out_offsets[i + 1]], byte for byte what replace_utf8 returns for it.
        data and offsets as for match_batch_utf8, `replacements` as for replace_utf8, the one retry of replace_batch.  An
        ill-formed haystack raises Utf8Error (.haystack, and .start inside it); stats: an N.Utf8BatchStats to fill in, if wanted.
        errors="replace": acgpu_replace_batch_utf8_lossy -- every haystack as replace_utf8(errors="replace") rewrites it alone;
        nothing is raised, and stats is an N.Utf8LossyStats."""
        entry, stats_type = _utf8_entry("acgpu_replace_batch_utf8", errors)
        buf, off = _pack_utf8(data, offsets)
        r_bytes, r_off, n_repl = self._replacements_utf8(replacements)
        st = N.ReplaceStats()
        out_off = np.zeros(len(off), dtype=np.uint64)
        out = _rewrite_call(entry, (self._h, _vp(_readable(buf)), _vp(off), len(off) - 1, _vp(r_bytes), _vp(r_off), n_repl), np.uint8,
                            int(off[-1] - off[0]), cap, (st, stats if stats is not None else stats_type()), _retry_once, mid=(_vp(out_off),))
        return out, out_off, _stats_dict(st)

    def replace_batch(self, haystacks, replacements, cap=None):
        """acgpu_replace_batch_u16: many short haystacks (str or uint16 arrays) rewritten in one call -> (units, out_offsets,
        stats dict): the result of haystack i is units[out_offsets[i]:out_offsets[i + 1]].  `replacements` as for replace_host,
        and the same one retry with the size the first call reports."""
        units, off = _pack(haystacks)
        r_units, r_off, n_repl = self._replacements(replacements)
        st = N.ReplaceStats()
        out_off = np.zeros(len(off), dtype=np.uint64)
        out = _rewrite_call(N.lib().acgpu_replace_batch_u16, (self._h, _vp(units), _vp(off), len(off) - 1, _vp(r_units), _vp(r_off), n_repl),
                            np.uint16, int(off[-1]), cap, (st,), _retry_once, mid=(_vp(out_off),))
        return out, out_off, _stats_dict(st)

    def summary_batch(self, haystacks):
        """acgpu_summary_batch_u16: many short haystacks (str or uint16 arrays) decided in one call -> (array of N.SUMMARY_DTYPE
        with one entry per haystack: n_matches and the first record in listener order, -1s where there is none; stats dict).
        No record leaves the device and there is no capacity to guess."""
        units, off = _pack(haystacks)
        n = len(off) - 1
        out = np.zeros(n, dtype=N.SUMMARY_DTYPE)
        st = N.SummaryStats()
        N.check(N.lib().acgpu_summary_batch_u16(self._h, _vp(units), _vp(off), n, _vp(out) if n else None, ctypes.byref(st)),
                "acgpu_summary_batch_u16")
        return out, _stats_dict(st)

    def replace_device(self, d_hay_ptr, n_units, replacements, d_out_ptr, cap, stream=0):
        """acgpu_replace_device on raw device pointers: the whole text d_hay_ptr[0 .. n_units) rewritten into d_out_ptr (cap
        units, 16-byte aligned).  Returns (n_out, rc, stats dict); rc == E_OVERFLOW: n_out is the capacity to call again with."""
        sh = _fill_shard(N.Shard(), d_hay_ptr, n_units)
        units, off, n_repl = self._replacements(replacements)
        st = N.ReplaceStats()
        n_out = ctypes.c_uint64(0)
        rc = N.lib().acgpu_replace_device(self._h, ctypes.byref(sh), _vp(units), _vp(off), n_repl, d_out_ptr, cap, ctypes.byref(n_out),
                                          ctypes.c_void_p(stream), ctypes.byref(st))
        return int(n_out.value), rc, _stats_dict(st)

    def match_device_begin(self, d_hay_ptr, n_units, with_ids, d_out_ptr, cap, own=None, text_begin=True, text_end=True,
                           stream=0, profile=False, d_result=None, chain_entry=None):
        """acgpu_match_device_begin: enqueue without waiting (AhoCorasick, WholeWord with fold-consistent tables, the LongestMatch
        walk pipeline; the other families run inside the call).  Returns (ticket, rc); the ticket keeps the acgpu_shard alive
        (the library writes chain_exit into it when the ticket is collected)."""
        sh = _fill_shard(N.Shard(), d_hay_ptr, n_units, own, text_begin, text_end, chain_entry, d_result)
        tk = ctypes.c_void_p()
        rc = N.lib().acgpu_match_device_begin(self._h, ctypes.byref(sh), N.REC_MAP if with_ids else N.REC_SET, d_out_ptr, cap,
                                              ctypes.c_void_p(stream), 1 if profile else 0, ctypes.byref(tk))
        return Ticket(tk, sh), rc

    def match_device_end(self, ticket, profile=False):
        """acgpu_match_device_end: waits for that call only.  Returns (n_out, rc, profile_dict|None); ticket.chain_exit holds
        the shard's chain exit afterwards."""
        prof = N.Profile() if profile else None
        n_out = ctypes.c_uint64(0)
        rc = N.lib().acgpu_match_device_end(self._h, ticket.handle, ctypes.byref(n_out), ctypes.byref(prof) if profile else None)
        return int(n_out.value), rc, _profile_dict(prof) if profile else None

    def match_device_abandon(self, ticket):
        """acgpu_match_device_abandon: give the ticket up (waits for its kernels, never redoes the call)."""
        return N.lib().acgpu_match_device_abandon(self._h, ticket.handle)

    def pages(self, hay_units, with_ids, page_records=1 << 20):
        """acgpu_cursor_*: the records of match_host(hay_units) as a generator of (n, 2|3) int32 pages of at most page_records
        records, scanned only as far as the pages taken so far require.  Closing the generator closes the cursor."""
        with Cursor(self, hay_units, with_ids) as cur:
            while True:
                page = cur.next(page_records)
                if not len(page):
                    return
                yield page


class Comm:
    """acgpu_comm: the devices of a single-process multi-GPU job, one stream per device, and the transport of the gather
    (RCCL ncclCommInitAll / peer copies).  match_device_allgather: every device scans its shard into its slot of its gather
    buffer, one all-gather leaves every device with every shard's records."""

    def __init__(self, devices, transport=N.TRANSPORT_AUTO):
        self.devices = list(devices)
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        h = ctypes.c_void_p()
        N.check(N.lib().acgpu_comm_open(arr, len(self.devices), transport, ctypes.byref(h)), "acgpu_comm_open")
        self._h = h

    @property
    def transport(self):
        return N.lib().acgpu_comm_transport(self._h)

    def stream(self, i):
        return N.lib().acgpu_comm_stream(self._h, i) or 0

    def match_device_allgather(self, automaton, shards, with_ids, gather_ptrs, gcap, profile=False):
        """shards: list of dicts(d_hay, n_units, own=(b, e), text_begin, text_end[, chain_entry]) -- shard i on devices[i];
        gather_ptrs: device pointers, buffer i on devices[i].  Returns (rc, counts list, chain exits list, profiles | None)."""
        k = len(self.devices)
        arr = (N.Shard * k)()
        for i, sd in enumerate(shards):
            _fill_shard(arr[i], sd["d_hay"], sd["n_units"], sd.get("own"), sd.get("text_begin", i == 0), sd.get("text_end", i == k - 1),
                        sd.get("chain_entry"))
        ptrs = (ctypes.c_void_p * k)(*gather_ptrs)
        counts = (ctypes.c_uint64 * k)()
        profs = (N.Profile * k)() if profile else None
        rc = N.lib().acgpu_match_device_allgather(automaton.handle, self._h, arr, _kind(with_ids), ptrs, gcap, counts, profs)
        pd = [_profile_dict(p) for p in profs] if profile else None
        return rc, [int(c) for c in counts], [int(arr[i].chain_exit) for i in range(k)], pd

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            N.lib().acgpu_comm_close(h)

    __del__ = close


class Ticket:
    """One acgpu_match_device_begin call in flight: the native ticket and the acgpu_shard it was begun with."""

    def __init__(self, handle, shard):
        self.handle = handle
        self.shard = shard

    @property
    def chain_exit(self):
        return int(self.shard.chain_exit)


class Stream:
    """acgpu_stream: the haystack arrives in chunks (match(Readable, ...)); feed() returns the records that have become
    decidable as an (n, 2|3) int64 array with GLOBAL positions (units since the first feed)."""

    def __init__(self, automaton, with_ids=True, pipelined=False):
        """pipelined: acgpu_stream_set_pipelined -- a feed returns the records of the PREVIOUS feed's chunk (the final feed both),
        host copy, transfer and scan of neighbouring chunks overlap."""
        self._auto = automaton  # keeps the handle alive
        self._kind = _kind(with_ids)
        self._errors = None  # the policy of a stream of bytes: its first byte feed's, every later one's
        h = ctypes.c_void_p()
        N.check(N.lib().acgpu_stream_open(automaton.handle, ctypes.byref(h)), "acgpu_stream_open")
        self._h = h
        if pipelined:
            N.check(N.lib().acgpu_stream_set_pipelined(h, 1), "acgpu_stream_set_pipelined")

    def reserve(self, n_units):
        """acgpu_stream_reserve: a uint16 numpy view of the staging memory the next chunk may be written into; feed that view."""
        p = ctypes.c_void_p()
        N.check(N.lib().acgpu_stream_reserve(self._h, int(n_units), ctypes.byref(p)), "acgpu_stream_reserve")
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint16)), shape=(int(n_units),))

    def _utf8_policy(self, name, errors):
        """_utf8_entry for a feed of bytes: the first byte feed fixes the stream's policy, and a feed with the other one is
        refused here as the library would refuse it (ACGPU_E_INVALID), without a native call."""
        entry, stats_type = _utf8_entry(name, errors)
        if self._errors is None:
            self._errors = errors
        elif self._errors != errors:
            raise ValueError("errors=%r on a stream that is fed with errors=%r" % (errors, self._errors))
        return entry, stats_type

    def _record_buffer(self, cap, cols):
        """one record buffer per stream: a fresh one per feed costs more than the feed"""
        out = getattr(self, "_out", None)
        if out is None or out.shape != (cap, cols):
            out = self._out = _new_records(cap, cols)
        return out

    def _feed(self, entry, src, final, cap, stats=None):
        """The body of feed and feed_utf8: the records call into the stream's own buffer (an overflow consumed nothing: the same
        feed again), the records as int64 with GLOBAL positions.  stats: the entry's last argument, where it has one."""
        n = int(src.size)
        base = ctypes.c_int64(0)
        r = _records_call(entry, (self._h, _vp(_readable(src)), n, 1 if final else 0), self._kind, self._kind // 4,
                          max(4096, n // 64) if cap is None else cap, (ctypes.byref(base),), stats, self._record_buffer).astype(np.int64)
        r[:, :2] += base.value
        return r

    def feed(self, units, final=False, cap=None):
        # (a view of the reserved staging memory stays where it is)
        return self._feed(N.lib().acgpu_stream_feed, np.ascontiguousarray(units, dtype=np.uint16), final, cap)

    def feed_utf8(self, data, final=False, cap=None, stats=None, errors="strict"):
        """acgpu_stream_feed_utf8: the next bytes of a UTF-8 text (bytes-like or a uint8 array; a chunk may end inside a
        sequence) -> the records that have become decidable as an (n, 2|3) int64 array with GLOBAL BYTE offsets (bytes since the
        first feed), end exclusive.  Ill-formed input raises Utf8Error (.start: the global offset) and finishes the stream.
        A stream is fed either units or bytes.  stats: an N.Utf8StreamStats to fill in, if wanted.
        errors="replace": acgpu_stream_feed_utf8_lossy -- the records of match_utf8(errors="replace") on everything fed, whatever
        the chunking; nothing is raised, and stats is an N.Utf8LossyStreamStats.  The first feed fixes the stream's policy."""
        entry, stats_type = self._utf8_policy("acgpu_stream_feed_utf8", errors)
        return self._feed(entry, _utf8_bytes(data), final, cap, stats if stats is not None else stats_type())

    def _replace_feed(self, entry, src, table, final, cap, stats):
        """The body of replace_feed and replace_feed_utf8: the rewrite call, made again while it asks for more room (nothing was
        committed), the result as an array of src's type.  table: (replacements, offsets, n).  stats: the entry's last arguments."""
        n = int(src.size)
        r, off, n_repl = table
        return _rewrite_call(entry, (self._h, _vp(_readable(src)), n, 1 if final else 0, _vp(r), _vp(off), n_repl), src.dtype, n, cap, stats,
                             _retry_while_more)

    def replace_feed(self, units, replacements, final=False, cap=None, stats=None):
        """acgpu_stream_replace_u16: the next units of a text that is REWRITTEN as it arrives -> the units of the result that have
        become decidable, a uint16 array (the concatenation over all feeds: the whole text with every match replaced).
        `replacements` as for Automaton.replace_host, the same at every feed.  A stream is fed through one entry only.
        stats: an N.ReplaceStats to fill in, if wanted (this feed alone)."""
        return self._replace_feed(N.lib().acgpu_stream_replace_u16, utf16(units), self._auto._replacements(replacements), final, cap,
                                  [stats if stats is not None else N.ReplaceStats()])

    def replace_feed_utf8(self, data, replacements, final=False, stats=None, cap=None, replace_stats=None, errors="strict"):
        """acgpu_stream_replace_utf8: the next bytes of a UTF-8 text that is rewritten as it arrives (a chunk may end inside a
        sequence) -> the bytes of the result that have become decidable.  `replacements` as for Automaton.replace_utf8, the same
        at every feed.  Ill-formed input raises Utf8Error (.start: the global offset) and finishes the stream; what had been
        withheld is not delivered.  stats: an N.Utf8StreamStats, replace_stats: an N.ReplaceStats to fill in, if wanted.
        errors="replace": acgpu_stream_replace_utf8_lossy -- replace_utf8(errors="replace") of everything fed, whatever the
        chunking; nothing is raised, and stats is an N.Utf8LossyStreamStats.  The first feed fixes the stream's policy."""
        entry, stats_type = self._utf8_policy("acgpu_stream_replace_utf8", errors)
        return self._replace_feed(entry, _utf8_bytes(data), self._auto._replacements_utf8(replacements), final, cap,
                                  [stats if stats is not None else stats_type(),
                                   replace_stats if replace_stats is not None else N.ReplaceStats()]).tobytes()

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            N.lib().acgpu_stream_close(h)

    __del__ = close


def _replace_stream(auto, chunks, feed, replacements, empty):
    """The rewritten text of a stream of chunks, one piece of it per feed; closing the generator closes the stream, and no chunk is
    read before the result of the one before it has been taken.  The stream is opened, and the families that replace refuses are
    refused, at the first next()."""
    st = Stream(auto)
    try:
        for chunk in chunks:
            yield feed(st, chunk, replacements)
        yield feed(st, empty, replacements, final=True)
    finally:
        st.close()


def _str_feed():
    """Stream.replace_feed as a feed of _replace_stream that yields str: a feed's output may end between the two units of a
    surrogate pair (the position it ends at is one of the TEXT's, any unit), and two str that hold half a pair each do not
    join to the pair -- the high surrogate waits for the next feed's output."""
    held = [np.zeros(0, np.uint16)]

    def feed(st, chunk, r, final=False):
        out = np.concatenate([held[0], st.replace_feed(utf16(chunk), r, final=final)])
        cut = out.size - 1 if not final and out.size and 0xD800 <= int(out[-1]) < 0xDC00 else out.size
        held[0] = out[cut:]
        return _to_str(out[:cut])
    return feed


def _byte_chunks(readable, chunk_bytes):
    """A binary file object (read(n) -> bytes, b"" at the end) or any iterable of bytes-like chunks."""
    if hasattr(readable, "read"):
        while True:
            c = readable.read(chunk_bytes)
            if not c:
                return
            yield c
    else:
        yield from readable


def _utf8_stream_pages(auto, readable, chunk_bytes, with_ids, errors="strict"):
    """The records of a UTF-8 text that is read chunk by chunk, as one int64 array of global byte offsets per feed; closing the
    generator closes the stream, and no chunk is read before the records of the one before it have been taken."""
    st = Stream(auto, with_ids=with_ids)
    try:
        for chunk in _byte_chunks(readable, chunk_bytes):
            yield st.feed_utf8(chunk, errors=errors)
        yield st.feed_utf8(b"", final=True, errors=errors)
    finally:
        st.close()


class Cursor:
    """acgpu_cursor: one match(String) call handed out in pages (include/acgpu.h).  next(cap) returns the next 1 .. cap records
    as an (n, 2|3) int32 array with haystack positions -- an empty one when every record has been handed out."""

    def __init__(self, automaton, hay_units, with_ids=True):
        self._auto = automaton  # keeps the handle alive
        hay = np.ascontiguousarray(hay_units, dtype=np.uint16)
        self._src = _readable(hay)  # the library reads it until close
        self._kind = _kind(with_ids)
        self._out = None
        h = ctypes.c_void_p()
        N.check(N.lib().acgpu_cursor_open(automaton.handle, _vp(self._src), int(hay.size), self._kind, ctypes.byref(h)),
                "acgpu_cursor_open")
        self._h = h

    def next(self, cap):
        cap = int(cap)
        cols = self._kind // 4
        if self._out is None or self._out.shape[0] < cap:
            self._out = _new_records(cap, cols)
        n_out = ctypes.c_uint64(0)
        N.check(N.lib().acgpu_cursor_next(self._h, _vp(self._out), cap, ctypes.byref(n_out)), "acgpu_cursor_next")
        return self._out[:n_out.value].copy()

    def stats(self):
        st = N.CursorStats()
        N.check(N.lib().acgpu_cursor_get_stats(self._h, ctypes.byref(st)), "acgpu_cursor_get_stats")
        return _stats_dict(st)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            N.lib().acgpu_cursor_close(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    __del__ = close


# match(String, listener) pages through a cursor from this many units on (shorter texts: the one call, whose fixed cost is lower)
CURSOR_MIN_UNITS = 1 << 22


def _listener_records(auto, hay, with_ids):
    """The records of match(String, listener), as lists of rows: pages of a cursor for long haystacks on the current device,
    the single call otherwise (and with a device list)."""
    if hay.size >= CURSOR_MIN_UNITS and configured_devices() is None:
        pages = auto.pages(hay, with_ids)
        try:
            for p in pages:
                yield p.tolist()
        finally:
            pages.close()
    else:
        yield auto.match_host(hay, with_ids=with_ids).tolist()


class ReadableMatchListener:
    """S/ReadableMatchListener.java:3-9"""

    def match(self, value):
        raise NotImplementedError


def _chunks(readable, chunk_chars):
    """A Java Readable hands out characters until it returns -1; here: an object with read(n) -> str ('' at the end),
    or any iterable of str / uint16 arrays."""
    if hasattr(readable, "read"):
        while True:
            c = readable.read(chunk_chars)
            if not c:
                return
            yield c
    else:
        yield from readable


# ---- listener plumbing -----------------------------------------------------------------------------------

class SetMatchListener:
    """S/SetMatchListener.java:3-8"""

    def match(self, haystack, start_position, end_position):
        raise NotImplementedError


class MapMatchListener:
    """S/MapMatchListener.java:3-8"""

    def match(self, haystack, start_position, end_position, value):
        raise NotImplementedError


def _listener_fn(listener):
    return listener.match if hasattr(listener, "match") else listener


def _checked(haystacks):
    haystacks = list(haystacks)
    if any(h is None for h in haystacks):
        raise TypeError("haystack is None")
    return haystacks


def _not_none(haystack):
    if haystack is None:
        raise TypeError("haystack is None")  # the reference throws NullPointerException at haystack.length()
    return haystack


def _split_batch(units, out_off):
    """the result of Automaton.replace_batch -> one str per haystack"""
    o = out_off.tolist()
    return [_to_str(units[o[i]:o[i + 1]]) for i in range(len(o) - 1)]


def _split_batch_utf8(out, out_off):
    """the result of Automaton.replace_batch_utf8 -> one bytes object per haystack"""
    o = out_off.tolist()
    return [out[o[i]:o[i + 1]].tobytes() for i in range(len(o) - 1)]


_NO_HAYSTACK = object()  # _emit without a haystack argument for the listener: a text that is read as it goes has no one object


class _Matcher:
    """What StringSet and StringMap share: every public method that both have, written once.  A flavour contributes
      _WITH_IDS              whether its records carry the keyword index (and its listener gets a value),
      _replacement(r)        a replacement argument as Automaton takes it,
      _emit(fn, rows[, h])   rows to the listener until it returns False -> whether every row was delivered,
      _emit_batch(fn, hs, rows)   the same per haystack: a False ends THAT haystack's rows,
    and its public replace* methods, whose replacement parameter is named and defaulted differently (S/StringMap has values to
    fall back on); their bodies are the _replace* methods here.

    The *_batch decisions are not in the reference: what a listener that decides about each text of a list would hold, from ONE
    device call that returns 24 bytes per haystack and no record (Automaton.summary_batch).  An empty list gives empty results
    without a device."""
    _MODE = None

    def match(self, haystack, listener):
        """match(String, listener): the listener is called for every match in reference order -- (haystack, start, end) for a
        set, (haystack, start, end, value) for a map -- until it returns False."""
        fn = _listener_fn(listener)
        pages = _listener_records(self._auto, utf16(_not_none(haystack)), self._WITH_IDS)
        try:
            for page in pages:
                if not self._emit(fn, page, haystack):
                    return
        finally:
            pages.close()  # (a long haystack's cursor: closed at the first False, the rest is never scanned)

    def count(self, haystack):
        """Not in the reference: how often every keyword of the constructor's list is reported for `haystack` -- what a listener
        doing counts[index_of(keyword)] += 1; return True would hold (a duplicate keyword: its last occurrence in the list
        counts, for ShortestMatch its first) -- as a uint64 array, computed on the device without a record being handed out.
        For a map: how often the listener of match(String, ...) would be called with each value, aligned with the constructor's
        keyword / value lists (a duplicate keyword: the value that won)."""
        return self._auto.count_host(utf16(_not_none(haystack)))[0]

    def _replacement_utf8(self, r):
        """a replacement argument of the byte forms: bytes are taken as they are, anything else under the rules of _replacement"""
        return r if isinstance(r, (bytes, bytearray)) else self._replacement(r)

    def _replace(self, haystack, r):
        return _to_str(self._auto.replace_host(utf16(_not_none(haystack)), self._replacement(r))[0])

    def _replace_batch(self, haystacks, r):
        return _split_batch(*self._auto.replace_batch(_checked(haystacks), self._replacement(r))[:2])

    def _replace_utf8(self, data, r, errors):
        _check_errors(errors)
        return self._auto.replace_utf8(_not_none(data), self._replacement_utf8(r), errors=errors)[0].tobytes()

    def _replace_batch_utf8(self, datas, r, offsets, errors):
        _check_errors(errors)
        r = self._replacement_utf8(r)
        return _split_batch_utf8(*self._auto.replace_batch_utf8(datas if offsets is not None else _checked(datas), r, offsets=offsets,
                                                                errors=errors)[:2])

    def _replace_readable(self, readable, r, chunk_chars):
        return _replace_stream(self._auto, _chunks(readable, chunk_chars), _str_feed(), self._replacement(r), "")

    def _replace_utf8_readable(self, readable, r, chunk_bytes, errors):
        _check_errors(errors)
        feed = lambda st, chunk, r, final=False: st.replace_feed_utf8(chunk, r, final=final, errors=errors)
        return _replace_stream(self._auto, _byte_chunks(readable, chunk_bytes), feed, self._replacement_utf8(r), b"")

    def find_all(self, haystack):
        """Convenience (not in the reference): the (n,2) int32 array of (start, end) records; for a map the (n,3) array of
        (start, end, keyword_index) records."""
        return self._auto.match_host(utf16(haystack), with_ids=self._WITH_IDS)

    def find_all_utf8(self, data, errors="strict"):
        """Not in the reference: the (n,2) int32 array of (start, end) records of a UTF-8 haystack (bytes, bytearray, memoryview
        or uint8 array) -- for a map the (n,3) array of (start, end, keyword_index) records -- in BYTE offsets into `data`:
        decoded, scanned and mapped back on the device.  Utf8Error if ill-formed."""
        return self._auto.match_utf8(data, with_ids=self._WITH_IDS, errors=errors)

    def match_utf8(self, data, listener, errors="strict"):
        """Not in the reference: match(data.decode("utf-8"), listener) with the listener receiving `data` itself and byte
        offsets into it (a map's listener the value as well); a listener call that returns False stops the loop."""
        fn = _listener_fn(listener)
        self._emit(fn, self._auto.match_utf8(_not_none(data), with_ids=self._WITH_IDS, errors=errors).tolist(), data)

    def match_utf8_readable(self, readable, listener, chunk_bytes=1 << 22, errors="strict"):
        """Not in the reference: match_utf8 for a text that is read as it goes -- a binary file object (read(n)) or an iterable
        of bytes-like chunks, cut anywhere, inside a sequence too.  The listener gets (start, end) -- for a map (start, end,
        value) -- in GLOBAL byte offsets (there is no one haystack object to hand over); a call that returns False stops the
        feeding AND the reading.  Utf8Error (.start: the global offset) if the text is ill-formed -- unless errors="replace":
        the records of match_utf8(errors="replace") on the whole text, whatever the chunking."""
        _check_errors(errors)
        fn = _listener_fn(listener)
        pages = _utf8_stream_pages(self._auto, readable, chunk_bytes, self._WITH_IDS, errors)
        try:
            for page in pages:
                if not self._emit(fn, page.tolist()):
                    return
        finally:
            pages.close()

    def find_all_utf8_readable(self, readable, chunk_bytes=1 << 22, errors="strict"):
        """Not in the reference: the (n,2) int64 array of (start, end) records -- for a map the (n,3) array of (start, end,
        keyword_index) records -- of a UTF-8 text read chunk by chunk, in GLOBAL byte offsets: find_all_utf8 of the whole
        text, which may be longer than 2^31 bytes (errors: as find_all_utf8)."""
        _check_errors(errors)
        pages = list(_utf8_stream_pages(self._auto, readable, chunk_bytes, self._WITH_IDS, errors))
        return np.concatenate(pages) if pages else np.zeros((0, 3 if self._WITH_IDS else 2), np.int64)

    def match_batch(self, haystacks, listener):
        """Not in the reference: match(haystack, listener) for every haystack of a list in ONE device call (short inputs: a
        call has tens of microseconds of fixed cost).  A listener call that returns False ends THAT haystack's matches."""
        self._emit_batch(_listener_fn(listener), haystacks, self._auto.match_batch(haystacks, with_ids=self._WITH_IDS).tolist())

    def find_all_batch_utf8(self, datas, offsets=None, errors="strict"):
        """Not in the reference: the (n,3) int32 array of (haystack index, start, end) records -- for a map the (n,4) array of
        (haystack index, start, end, keyword index) records -- of many UTF-8 haystacks (a sequence of bytes-like objects, or
        with offsets= one buffer in place) from ONE device call, start and end in BYTES relative to the haystack.  Utf8Error
        (.haystack, .start) if one of them is ill-formed."""
        return self._auto.match_batch_utf8(datas if offsets is not None else _checked(datas), with_ids=self._WITH_IDS, offsets=offsets,
                                           errors=errors)

    def match_batch_utf8(self, datas, listener, errors="strict"):
        """Not in the reference: match_utf8(data, listener) for every haystack of a list in ONE device call: the listener
        gets the haystack's own bytes and byte offsets into them (a map's listener the value as well).  A listener call that
        returns False ends THAT haystack's matches."""
        datas = _checked(datas)
        self._emit_batch(_listener_fn(listener), datas, self._auto.match_batch_utf8(datas, with_ids=self._WITH_IDS, errors=errors).tolist())

    @property
    def automaton(self):
        return self._auto

    def _summary(self, haystacks):
        haystacks = _checked(haystacks)
        if not haystacks:
            return np.zeros(0, dtype=N.SUMMARY_DTYPE)
        return self._auto.summary_batch(haystacks)[0]

    def contains_batch(self, haystacks):
        """[does match(h, listener) call the listener at all for h in haystacks] as a bool array"""
        return self._summary(haystacks)["n_matches"] > 0

    def count_matches_batch(self, haystacks):
        """[how often match(h, listener) calls a listener that always returns True for h in haystacks] as a uint64 array"""
        return self._summary(haystacks)["n_matches"].copy()

    def first_batch(self, haystacks):
        """[the arguments of the first listener call of match(h, listener), without the haystack, or None for h in haystacks]:
        (start, end) for a set, (start, end, value) for a map"""
        return self._first_rows(self._summary(haystacks))

    def _first_rows(self, s):
        vals = getattr(self, "_values", None)
        rows = zip(s["n_matches"].tolist(), s["start"].tolist(), s["end"].tolist(), s["keyword_id"].tolist())
        if vals is None:
            return [(b, e) if n else None for n, b, e, _ in rows]
        return [(b, e, vals[k]) if n else None for n, b, e, k in rows]

    def _summary_utf8(self, datas, offsets, errors="strict"):
        if offsets is None:
            datas = _checked(datas)
        elif datas is None:
            raise TypeError("haystack is None")
        return self._auto.summary_batch_utf8(datas, offsets=offsets, errors=errors)[0]

    def contains_batch_utf8(self, datas, offsets=None, errors="strict"):
        """contains_batch for UTF-8 haystacks: a sequence of bytes-like objects, or with offsets= one buffer in place (a log
        file: offsets=utf8_line_offsets(buf)).  Utf8Error (.haystack, .start) if one of them is ill-formed -- unless
        errors="replace": then every haystack is scanned as its .decode("utf-8", "replace"), offsets still those of its bytes."""
        return self._summary_utf8(datas, offsets, errors)["n_matches"] > 0

    def count_matches_batch_utf8(self, datas, offsets=None, errors="strict"):
        """count_matches_batch for UTF-8 haystacks (see contains_batch_utf8)"""
        return self._summary_utf8(datas, offsets, errors)["n_matches"].copy()

    def first_batch_utf8(self, datas, offsets=None, errors="strict"):
        """first_batch for UTF-8 haystacks (see contains_batch_utf8): start and end in BYTES relative to the haystack"""
        return self._first_rows(self._summary_utf8(datas, offsets, errors))


class StringSet(_Matcher):
    """S/StringSet.java:3-5"""
    _WITH_IDS = False

    def _init(self, keywords, case_sensitive, word_chars=None):
        self._keywords = list(keywords)
        self._auto = Automaton(self._MODE, self._keywords, bool(case_sensitive), word_chars=word_chars)

    def _emit(self, fn, rows, haystack=_NO_HAYSTACK):
        if haystack is _NO_HAYSTACK:
            for s, e in rows:
                if not fn(s, e):
                    return False
        else:
            for s, e in rows:
                if not fn(haystack, s, e):
                    return False
        return True

    def _emit_batch(self, fn, haystacks, rows):
        skip = -1
        for h, s, e in rows:
            if h != skip and not fn(haystacks[h], s, e):
                skip = h

    def _replacement(self, r):
        return str(r)

    def replace(self, haystack, replacement):
        """Not in the reference: `haystack` with every match replaced by the str `replacement` (the empty one deletes the
        matches), rewritten on the device.  The non-overlapping families only: AhoCorasickSet raises the library's error."""
        return self._replace(haystack, replacement)

    def replace_batch(self, haystacks, replacement):
        """Not in the reference: [replace(h, replacement) for h in haystacks] in ONE device call (short inputs: a call has tens
        of microseconds of fixed cost) -> a list of str."""
        return self._replace_batch(haystacks, replacement)

    def replace_utf8(self, data, replacement, errors="strict"):
        """Not in the reference: the UTF-8 haystack `data` (bytes, bytearray, memoryview or uint8 array) with every match
        replaced by `replacement` (a str, encoded as UTF-8, or bytes taken as they are; empty deletes the matches) -> bytes,
        rewritten on the device without a decode or an encode on the host.  Utf8Error if `data` is ill-formed -- unless
        errors="replace": then the matches are those of find_all_utf8(data, errors="replace"), and every byte outside them,
        ill-formed ones included, is copied as it is."""
        return self._replace_utf8(data, replacement, errors)

    def replace_batch_utf8(self, datas, replacement, offsets=None, errors="strict"):
        """Not in the reference: [replace_utf8(d, replacement) for d in datas] in ONE device call -> a list of bytes, one per
        haystack.  datas: a sequence of bytes-like objects, or with offsets= ONE buffer used in place -- a log file line by line:
        replace_batch_utf8(buf, "***", offsets=utf8_line_offsets(buf)).  Utf8Error (.haystack, .start) if one is ill-formed --
        unless errors="replace" (see replace_utf8)."""
        return self._replace_batch_utf8(datas, replacement, offsets, errors)

    def replace_readable(self, readable, replacement, chunk_chars=1 << 22):
        """Not in the reference: replace() for a text that is read as it goes -- an object with read(n) -> str, or an iterable of
        str / uint16 arrays, cut anywhere, inside a keyword too -> a generator of str whose concatenation is replace() of the
        whole text; a feed yields what no later chunk can change.  Closing the generator closes the stream."""
        return self._replace_readable(readable, replacement, chunk_chars)

    def replace_utf8_readable(self, readable, replacement, chunk_bytes=1 << 22, errors="strict"):
        """Not in the reference: replace_utf8() for a text that is read as it goes -- a binary file object or an iterable of
        bytes-like chunks, cut anywhere, inside a sequence too (see match_utf8_readable) -> a generator of bytes whose
        concatenation is replace_utf8() of the whole text.  Utf8Error (.start: the global offset) if the text is ill-formed --
        unless errors="replace": then nothing is raised, and the concatenation is replace_utf8(errors="replace") of the whole."""
        return self._replace_utf8_readable(readable, replacement, chunk_bytes, errors)


class StringMap(_Matcher):
    """S/StringMap.java:5-9 (String overload only)"""
    _WITH_IDS = True

    def _init(self, keywords, values, case_sensitive, word_chars=None):
        # the reference consumes keywords and values pairwise and stops at the shorter one (S/AhoCorasickMap.java:32)
        pairs = list(zip(keywords, values))
        self._keywords = [k for k, _ in pairs]
        self._values = [v for _, v in pairs]
        self._auto = Automaton(self._MODE, self._keywords, bool(case_sensitive), word_chars=word_chars)

    def _emit(self, fn, rows, haystack=_NO_HAYSTACK):
        vals = self._values
        if haystack is _NO_HAYSTACK:
            for s, e, k in rows:
                if not fn(s, e, vals[k]):
                    return False
        else:
            for s, e, k in rows:
                if not fn(haystack, s, e, vals[k]):
                    return False
        return True

    def _emit_batch(self, fn, haystacks, rows):
        vals = self._values
        skip = -1
        for h, s, e, k in rows:
            if h != skip and not fn(haystacks[h], s, e, vals[k]):
                skip = h

    def _replacement(self, replacements):
        if replacements is None:
            if not all(isinstance(v, str) for v in self._values):
                raise TypeError("replace() without replacements needs str values")
            return self._values
        return replacements if isinstance(replacements, str) else list(replacements)[:len(self._keywords)]

    def match(self, haystack, listener):
        """match(String, MapMatchListener<T>) -- or, when `haystack` has read() / is an iterable of chunks,
        match(Readable, ReadableMatchListener<T>) (S/StringMap.java:6-8)."""
        if haystack is not None and not isinstance(haystack, (str, np.ndarray)):
            return self.match_readable(haystack, listener)
        return _Matcher.match(self, haystack, listener)

    def match_readable(self, readable, listener, chunk_chars=1 << 22):
        """S/AhoCorasickMap.java:208-275, S/LongestMatchMap.java:203-286, S/WholeWordMatchMap.java:55-153: the listener
        receives only the value; returning False stops the scan (and the reading)."""
        fn = _listener_fn(listener)
        vals = self._values
        st = Stream(self._auto, with_ids=True)
        try:
            feeds = itertools.chain(((chunk, False) for chunk in _chunks(readable, chunk_chars)), [("", True)])
            for chunk, final in feeds:  # (the value-only listener of this flavour's one Readable form: its loop is here)
                for k in st.feed(utf16(chunk), final=final)[:, 2].tolist():
                    if not fn(vals[k]):
                        return
        finally:
            st.close()

    def replace(self, haystack, replacements=None):
        """Not in the reference: `haystack` with every match replaced, rewritten on the device -- by its value (replacements is
        None: the values must all be str), by the entry of a list aligned with the constructor's keywords, or by one str for
        every keyword.  The non-overlapping families only: AhoCorasickMap raises the library's error."""
        return self._replace(haystack, replacements)

    def replace_batch(self, haystacks, replacements=None):
        """Not in the reference: [replace(h, replacements) for h in haystacks] in ONE device call (see
        StringSet.replace_batch) -> a list of str."""
        return self._replace_batch(haystacks, replacements)

    def replace_utf8(self, data, replacements=None, errors="strict"):
        """Not in the reference: the UTF-8 haystack `data` with every match replaced -> bytes (see StringSet.replace_utf8);
        `replacements` under the rules of replace(), a str encoded as UTF-8, bytes taken as they are."""
        return self._replace_utf8(data, replacements, errors)

    def replace_batch_utf8(self, datas, replacements=None, offsets=None, errors="strict"):
        """Not in the reference: [replace_utf8(d, replacements) for d in datas] in ONE device call -> a list of bytes (see
        StringSet.replace_batch_utf8); `replacements` under the rules of replace_utf8()."""
        return self._replace_batch_utf8(datas, replacements, offsets, errors)

    def replace_readable(self, readable, replacements=None, chunk_chars=1 << 22):
        """Not in the reference: replace() for a text that is read as it goes -> a generator of str (see
        StringSet.replace_readable); `replacements` under the rules of replace()."""
        return self._replace_readable(readable, replacements, chunk_chars)

    def replace_utf8_readable(self, readable, replacements=None, chunk_bytes=1 << 22, errors="strict"):
        """Not in the reference: replace_utf8() for a text that is read as it goes -> a generator of bytes (see
        StringSet.replace_utf8_readable); `replacements` under the rules of replace_utf8()."""
        return self._replace_utf8_readable(readable, replacements, chunk_bytes, errors)


def _word_chars(word_characters, toggle_flags):
    if word_characters is None:
        return default_word_chars()
    if toggle_flags is None:
        return word_chars_from_list(word_characters)
    return word_chars_with_toggles(word_characters, toggle_flags)


class AhoCorasickSet(StringSet):
    """S/AhoCorasickSet.java:11-20: every occurrence of every keyword."""
    _MODE = N.MODE_ALL

    def __init__(self, keywords, case_sensitive, threshold_strategy=None):
        self._init(keywords, case_sensitive)


class AhoCorasickMap(StringMap):
    """S/AhoCorasickMap.java:14-24"""
    _MODE = N.MODE_ALL

    def __init__(self, keywords, values, case_sensitive, threshold_strategy=None):
        self._init(keywords, values, case_sensitive)


class LongestMatchSet(StringSet):
    """S/LongestMatchSet.java:11-19: leftmost-longest, non-overlapping."""
    _MODE = N.MODE_LONGEST

    def __init__(self, keywords, case_sensitive, threshold_strategy=None):
        self._init(keywords, case_sensitive)


class LongestMatchMap(StringMap):
    """S/LongestMatchMap.java"""
    _MODE = N.MODE_LONGEST

    def __init__(self, keywords, values, case_sensitive, threshold_strategy=None):
        self._init(keywords, values, case_sensitive)


class ShortestMatchSet(StringSet):
    """S/ShortestMatchSet.java:8-20: reports a match as soon as any keyword ends, then restarts after it (the
    reference's "leftmost shortest" matcher; non-overlapping)."""
    _MODE = N.MODE_SHORTEST

    def __init__(self, keywords, case_sensitive, threshold_strategy=None):
        self._init(keywords, case_sensitive)


class ShortestMatchMap(StringMap):
    """S/ShortestMatchMap.java:16-24; of equal keywords the FIRST one's value is kept (:47-49)."""
    _MODE = N.MODE_SHORTEST

    def __init__(self, keywords, values, case_sensitive, threshold_strategy=None):
        self._init(keywords, values, case_sensitive)


class WholeWordMatchSet(StringSet):
    """S/WholeWordMatchSet.java: keywords that span a whole maximal run of word characters."""
    _MODE = N.MODE_WHOLEWORD

    def __init__(self, keywords, case_sensitive, word_characters=None, toggle_flags=None, threshold_strategy=None):
        self._init(keywords, case_sensitive, word_chars=_word_chars(word_characters, toggle_flags))

    def get_word_chars(self):
        return self._auto.word_chars


class WholeWordMatchMap(StringMap):
    """S/WholeWordMatchMap.java:21-53"""
    _MODE = N.MODE_WHOLEWORD

    def __init__(self, keywords, values, case_sensitive, word_characters=None, toggle_flags=None,
                 threshold_strategy=None):
        self._init(keywords, values, case_sensitive, word_chars=_word_chars(word_characters, toggle_flags))

    def get_word_chars(self):
        return self._auto.word_chars


class WholeWordLongestMatchSet(StringSet):
    """S/WholeWordLongestMatchSet.java:7-45: whole-word matches of keywords that may contain non-word characters
    ("as if"); of the keywords starting at a word the longest whole-word one wins, and the scan continues after the
    text it looked at."""
    _MODE = N.MODE_WWLONGEST

    def __init__(self, keywords, case_sensitive, word_characters=None, toggle_flags=None, threshold_strategy=None):
        self._init(keywords, case_sensitive, word_chars=_word_chars(word_characters, toggle_flags))

    def get_word_chars(self):
        return self._auto.word_chars


class WholeWordLongestMatchMap(StringMap):
    """S/WholeWordLongestMatchMap.java:22-54"""
    _MODE = N.MODE_WWLONGEST

    def __init__(self, keywords, values, case_sensitive, word_characters=None, toggle_flags=None,
                 threshold_strategy=None):
        self._init(keywords, values, case_sensitive, word_chars=_word_chars(word_characters, toggle_flags))

    def get_word_chars(self):
        return self._auto.word_chars
