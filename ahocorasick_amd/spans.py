"""Which parts of a text a dictionary covers: the records of a match call merged into covered runs on the device (include/acgpu.h:
acgpu_spans_u16, acgpu_spans_batch_u16, acgpu_spans_device, acgpu_spans_utf8, acgpu_spans_utf8_lossy, acgpu_spans_batch_utf8,
acgpu_spans_batch_utf8_lossy) -- what redaction, highlighting and PII tagging
ask, for all five families, AhoCorasick's overlapping records included.

A span is a maximal run of positions that some record covers: overlapping, nested and touching records fall into one span, so
(1, 5) and (5, 8) give (1, 8), and two consecutive spans have an uncovered position between them.  No record reaches the host.

    for start, end in spans(AhoCorasickSet(names, False), text):
        text = text[:start] + "#" * (end - start) + text[end:]
"""
import ctypes

import numpy as np

from . import _native as N
from .strings import Automaton, _fill_shard, _not_none, _pack, _pack_utf8, _raise_for, _readable, _stats_dict, _utf8_bytes, _utf8_entry, _vp, utf16

__all__ = ["spans", "spans_batch", "spans_batch_utf8", "spans_utf8", "spans_device"]


def _automaton(matcher):
    """an Automaton, or the one behind a StringSet / StringMap"""
    return matcher if isinstance(matcher, Automaton) else matcher.automaton


def _spans_call(entry, head, n, stats, tail=(), cols=2):
    """entry(*head, out, cap, &n_out, &stats, *tail) -> the (n_out, cols) int32 array.  The first capacity is a guess from the text's
    size; ACGPU_E_OVERFLOW reports the spans the text has, and the same call with exactly that capacity succeeds (include/acgpu.h):
    ONE retry, a second overflow is an error."""
    st = stats if stats is not None else N.SpansStats()
    cap = max(4096, n // 4)
    for attempt in range(2):
        out = np.empty((cap, cols), dtype=np.int32)
        n_out = ctypes.c_uint64(0)
        rc = entry(*head, _vp(out), cap, ctypes.byref(n_out), ctypes.byref(st), *tail)
        if rc != N.E_OVERFLOW:
            break
        cap = int(n_out.value)
    _raise_for(rc, entry, [t._obj for t in tail])
    return out[:int(n_out.value)]


def spans(matcher, haystack, stats=None):
    """The spans of a haystack (str or uint16 array) -> (n, 2) int32 array of (start, end) in units, ascending: the merge of the
    records matcher.find_all returns for a set.  matcher: an Automaton or any StringSet / StringMap, all five families.  stats:
    an N.SpansStats to fill in, if wanted."""
    hay = utf16(_not_none(haystack))
    return _spans_call(N.lib().acgpu_spans_u16, (_automaton(matcher).handle, _vp(_readable(hay)), int(hay.size)), int(hay.size), stats)


def spans_batch(matcher, haystacks, stats=None):
    """The spans of many short haystacks (str or uint16 arrays) in ONE device call -> (n, 3) int32 array of (haystack, start, end),
    ordered by haystack and ascending within it, start and end relative to the haystack: the rows of haystack i are spans(matcher,
    haystacks[i]).  Spans never reach across two haystacks: "xab", "abx" with keyword ab gives two."""
    units, off = _pack([_not_none(h) for h in haystacks])
    return _spans_call(N.lib().acgpu_spans_batch_u16, (_automaton(matcher).handle, _vp(units), _vp(off), len(off) - 1), int(off[-1]), stats, cols=3)


def spans_utf8(matcher, data, errors="strict", stats=None):
    """spans for a UTF-8 haystack (bytes, bytearray, memoryview or uint8 array) -> (n, 2) int32 array in BYTE offsets into `data`:
    the merge of the records find_all_utf8 returns.  Ill-formed input raises Utf8Error exactly as find_all_utf8 does -- unless
    errors="replace": the text as its .decode("utf-8", "replace")."""
    entry, stats_type = _utf8_entry("acgpu_spans_utf8", errors)
    buf = _utf8_bytes(_not_none(data))
    return _spans_call(entry, (_automaton(matcher).handle, _vp(_readable(buf)), int(buf.size)), int(buf.size), stats,
                       tail=(ctypes.byref(stats_type()),))


def spans_batch_utf8(matcher, datas, offsets=None, errors="strict", stats=None):
    """The spans of many short UTF-8 haystacks in ONE device call -> (n, 3) int32 array of (haystack, start, end), start and end in
    BYTES relative to the haystack: the rows of haystack i are spans_utf8(matcher, datas[i]).  datas: a sequence of bytes-like
    objects, or with offsets= ONE buffer used in place (utf8_line_offsets: a log file line by line).  Spans never reach across two
    haystacks.  An ill-formed haystack raises Utf8Error (.haystack, and .start inside it) as find_all_batch_utf8 does -- unless
    errors="replace": every haystack as its .decode("utf-8", "replace")."""
    entry, stats_type = _utf8_entry("acgpu_spans_batch_utf8", errors)
    buf, off = _pack_utf8(datas if offsets is not None else [_not_none(h) for h in datas], offsets)
    return _spans_call(entry, (_automaton(matcher).handle, _vp(_readable(buf)), _vp(off), len(off) - 1), int(off[-1] - off[0]), stats,
                       tail=(ctypes.byref(stats_type()),), cols=3)


def spans_device(matcher, d_hay, n_units, d_out, cap, stream=0):
    """acgpu_spans_device on raw device pointers: the spans of the whole text d_hay[0 .. n_units) written to d_out (cap spans of two
    int32, 16-byte aligned).  Returns (n_out, rc, stats dict); rc == E_OVERFLOW: n_out is the capacity to call again with."""
    sh = _fill_shard(N.Shard(), d_hay, n_units)
    st = N.SpansStats()
    n_out = ctypes.c_uint64(0)
    rc = N.lib().acgpu_spans_device(_automaton(matcher).handle, ctypes.byref(sh), d_out, cap, ctypes.byref(n_out), ctypes.c_void_p(stream),
                                    ctypes.byref(st))
    return int(n_out.value), rc, _stats_dict(st)
