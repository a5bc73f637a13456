"""Mask, highlight or redact every covered run of a text on the device (include/acgpu.h: acgpu_cover_u16, acgpu_cover_batch_u16, acgpu_cover_device,
acgpu_cover_utf8, acgpu_cover_utf8_lossy, acgpu_cover_batch_utf8, acgpu_cover_batch_utf8_lossy): every span of the text -- the spans of ahocorasick_amd.spans, for all five families,
AhoCorasick's overlapping records included -- becomes open + body + close, everything else is copied.

    mask(AhoCorasickSet(names, False), text)                    # "call **** or ***" -- the length is preserved
    highlight(AhoCorasickSet(names, False), text, "<b>", "</b>")
    redact(AhoCorasickSet(names, False), text, "[name]")
    mask_batch(AhoCorasickSet(names, False), lines)             # many short texts: ONE device call, a list of str
    mask_batch_utf8(AhoCorasickSet(names, False), log, offsets=utf8_line_offsets(log))  # ... of bytes, the buffer used in place

Not replace: overlapping, nested and TOUCHING matches are one span, so two matches that touch give ONE replacement, not two.
No span and no record reaches the host.
"""
import ctypes

import numpy as np

from . import _native as N
from .spans import _automaton
from .strings import _fill_shard, _not_none, _pack, _pack_utf8, _raise_for, _readable, _stats_dict, _to_str, _utf8_bytes, _utf8_entry, _vp, utf16

__all__ = ["cover", "cover_utf8", "cover_device", "mask", "mask_utf8", "highlight", "highlight_utf8", "redact", "redact_utf8",
           "cover_batch", "cover_batch_units", "mask_batch", "highlight_batch", "redact_batch",
           "cover_batch_utf8", "cover_batch_bytes", "mask_batch_utf8", "highlight_batch_utf8", "redact_batch_utf8"]

BODIES = {"keep": 0, "fill": 1, "drop": 2}  # ACGPU_COVER_KEEP, _FILL, _DROP


def _body(body):
    if body not in BODIES:
        raise ValueError("body must be 'keep', 'fill' or 'drop', not %r" % (body,))
    return BODIES[body]


def _units(what, s):
    if s is None:
        raise TypeError("%s is None" % what)
    return utf16(s)


def _bytes(what, s):
    if s is None:
        raise TypeError("%s is None" % what)
    return _utf8_bytes(s.encode("utf-8") if isinstance(s, str) else s)


def _spec(open_, close, body, fill):
    """(N.CoverSpec, the arrays its pointers point into)"""
    spec = N.CoverSpec(open_.ctypes.data if open_.size else None, int(open_.size), close.ctypes.data if close.size else None, int(close.size),
                       body, fill)
    return spec, (open_, close)


def _fill_unit(fill):
    f = _units("fill", fill)
    if f.size != 1:
        raise ValueError("fill must be one UTF-16 unit, not %r" % (fill,))
    return int(f[0])


def _fill_byte(fill):
    f = _bytes("fill", fill)
    if f.size != 1 or int(f[0]) >= 0x80:
        raise ValueError("fill must be one ASCII byte, not %r" % (fill,))
    return int(f[0])


def _cover_call(entry, head, spec, dtype, n, stats, tail=(), mid=(), cap=None):
    """entry(*head, &spec, out, cap, *mid, &n_out, &stats, *tail) -> the elements written.  The first capacity is the text's size and a
    quarter plus one open and one close; ACGPU_E_OVERFLOW reports the result's size, and the same call with exactly that capacity
    succeeds (include/acgpu.h): ONE retry, a second overflow is an error."""
    st = stats if stats is not None else N.CoverStats()
    if cap is None:
        cap = n + n // 4 + int(spec.open_len) + int(spec.close_len)
    for attempt in range(2):
        out = np.empty(max(cap, 1), dtype=dtype)
        n_out = ctypes.c_uint64(0)
        rc = entry(*head, ctypes.byref(spec), _vp(out), cap, *mid, ctypes.byref(n_out), ctypes.byref(st), *tail)
        if rc != N.E_OVERFLOW:
            break
        cap = int(n_out.value)
    _raise_for(rc, entry, [t._obj for t in tail])
    return out[:int(n_out.value)]


def cover(matcher, haystack, open="", close="", body="keep", fill="*", stats=None):
    """The haystack (str or uint16 array) with every span rewritten as open + body + close -> str.  body: "keep" (the covered
    text), "fill" (fill once per covered UTF-16 unit) or "drop" (nothing).  matcher: an Automaton or any StringSet / StringMap,
    all five families.  stats: an N.CoverStats to fill in, if wanted."""
    hay = utf16(_not_none(haystack))
    spec, keep = _spec(_units("open", open), _units("close", close), _body(body), _fill_unit(fill))
    out = _cover_call(N.lib().acgpu_cover_u16, (_automaton(matcher).handle, _vp(_readable(hay)), int(hay.size)), spec, np.uint16, int(hay.size), stats)
    return _to_str(out)


def cover_utf8(matcher, data, open=b"", close=b"", body="keep", fill=b"*", errors="strict", stats=None):
    """cover for a UTF-8 haystack (bytes, bytearray, memoryview or uint8 array) -> bytes; the spans are those of spans_utf8, in
    bytes.  open, close: bytes-like, taken as they are, or str, encoded as UTF-8.  fill: one ASCII byte, written once per covered
    BYTE, so the result stays well-formed and byte offsets into `data` hold on it.  Ill-formed input raises Utf8Error as
    find_all_utf8 does -- unless errors="replace": stray bytes outside the spans are copied, inside a "fill" span filled."""
    entry, stats_type = _utf8_entry("acgpu_cover_utf8", errors)
    buf = _utf8_bytes(_not_none(data))
    spec, keep = _spec(_bytes("open", open), _bytes("close", close), _body(body), _fill_byte(fill))
    out = _cover_call(entry, (_automaton(matcher).handle, _vp(_readable(buf)), int(buf.size)), spec, np.uint8, int(buf.size), stats,
                      tail=(ctypes.byref(stats_type()),))
    return out.tobytes()


def cover_device(matcher, d_hay, n_units, d_out, cap, open="", close="", body="keep", fill="*", stream=0):
    """acgpu_cover_device on raw device pointers: the whole text d_hay[0 .. n_units) (16-byte aligned) rewritten into d_out (cap
    units, at any unit address).  Returns (n_out, rc, stats dict); rc == E_OVERFLOW: n_out is the capacity to call again with."""
    sh = _fill_shard(N.Shard(), d_hay, n_units)
    spec, keep = _spec(_units("open", open), _units("close", close), _body(body), _fill_unit(fill))
    st = N.CoverStats()
    n_out = ctypes.c_uint64(0)
    rc = N.lib().acgpu_cover_device(_automaton(matcher).handle, ctypes.byref(sh), ctypes.byref(spec), d_out, cap, ctypes.byref(n_out),
                                    ctypes.c_void_p(stream), ctypes.byref(st))
    return int(n_out.value), rc, _stats_dict(st)


def cover_batch_units(matcher, haystacks, open="", close="", body="keep", fill="*", cap=None):
    """acgpu_cover_batch_u16: many short haystacks (str or uint16 arrays) rewritten in ONE device call -> (units, out_offsets, stats
    dict): the result of haystack i is units[out_offsets[i]:out_offsets[i + 1]], unit for unit what cover returns for it alone.
    cap None: the first capacity of cover, over the batch's units; one retry with the size the first call reports."""
    units, off = _pack([_not_none(h) for h in haystacks])
    spec, keep = _spec(_units("open", open), _units("close", close), _body(body), _fill_unit(fill))
    st = N.CoverStats()
    out_off = np.zeros(len(off), dtype=np.uint64)
    out = _cover_call(N.lib().acgpu_cover_batch_u16, (_automaton(matcher).handle, _vp(units), _vp(off), len(off) - 1), spec, np.uint16, int(off[-1]),
                      st, mid=(_vp(out_off),), cap=cap)
    return out, out_off, _stats_dict(st)


def cover_batch(matcher, haystacks, open="", close="", body="keep", fill="*"):
    """[cover(matcher, h, open, close, body, fill) for h in haystacks] in ONE device call (short inputs: a call has tens of
    microseconds of fixed cost) -> a list of str.  A span never reaches across two haystacks: "xab", "abx" with keyword ab is
    rewritten twice, where the joined text "xababx" has one span."""
    units, out_off, _ = cover_batch_units(matcher, haystacks, open, close, body, fill)
    whole = _to_str(units)  # (a unit is two bytes of UTF-16: unit offsets cut the str only where no surrogate pair is split)
    if len(whole) == units.size:
        return [whole[int(out_off[i]):int(out_off[i + 1])] for i in range(len(out_off) - 1)]
    return [_to_str(units[int(out_off[i]):int(out_off[i + 1])]) for i in range(len(out_off) - 1)]


def mask_batch(matcher, haystacks, fill="*"):
    """mask for many short haystacks in one device call: every result has its haystack's length"""
    return cover_batch(matcher, haystacks, body="fill", fill=fill)


def highlight_batch(matcher, haystacks, open, close):
    return cover_batch(matcher, haystacks, open=open, close=close, body="keep")


def redact_batch(matcher, haystacks, replacement):
    return cover_batch(matcher, haystacks, open=replacement, body="drop")


def cover_batch_bytes(matcher, datas, open=b"", close=b"", body="keep", fill=b"*", offsets=None, errors="strict", cap=None):
    """acgpu_cover_batch_utf8: many short UTF-8 haystacks rewritten in ONE device call -> (uint8 array, out_offsets, stats dict): the
    result of haystack i is out[out_offsets[i]:out_offsets[i + 1]], byte for byte what cover_utf8 returns for it alone.  datas: a
    sequence of bytes-like objects, or with offsets= ONE buffer used in place (utf8_line_offsets: a log file line by line).  open,
    close, fill as for cover_utf8.  An ill-formed haystack raises Utf8Error (.haystack, and .start inside it) -- unless
    errors="replace" (acgpu_cover_batch_utf8_lossy).  cap None: the first capacity of cover_utf8, over the batch's bytes; one retry
    with the size the first call reports."""
    entry, stats_type = _utf8_entry("acgpu_cover_batch_utf8", errors)
    buf, off = _pack_utf8(datas if offsets is not None else [_not_none(h) for h in datas], offsets)
    spec, keep = _spec(_bytes("open", open), _bytes("close", close), _body(body), _fill_byte(fill))
    st = N.CoverStats()
    out_off = np.zeros(len(off), dtype=np.uint64)
    out = _cover_call(entry, (_automaton(matcher).handle, _vp(_readable(buf)), _vp(off), len(off) - 1), spec, np.uint8, int(off[-1] - off[0]), st,
                      tail=(ctypes.byref(stats_type()),), mid=(_vp(out_off),), cap=cap)
    return out, out_off, _stats_dict(st)


def cover_batch_utf8(matcher, datas, open=b"", close=b"", body="keep", fill=b"*", offsets=None, errors="strict"):
    """[cover_utf8(matcher, d, open, close, body, fill, errors) for d in datas] in ONE device call -> a list of bytes.  A span never
    reaches across two haystacks: b"xab", b"abx" with keyword ab is rewritten twice."""
    out, out_off, _ = cover_batch_bytes(matcher, datas, open, close, body, fill, offsets, errors)
    whole = out.tobytes()
    return [whole[int(out_off[i]):int(out_off[i + 1])] for i in range(len(out_off) - 1)]


def mask_batch_utf8(matcher, datas, fill=b"*", offsets=None, errors="strict"):
    """mask_utf8 for many short haystacks in one device call: every result has its haystack's length and byte offsets"""
    return cover_batch_utf8(matcher, datas, body="fill", fill=fill, offsets=offsets, errors=errors)


def highlight_batch_utf8(matcher, datas, open, close, offsets=None, errors="strict"):
    return cover_batch_utf8(matcher, datas, open=open, close=close, body="keep", offsets=offsets, errors=errors)


def redact_batch_utf8(matcher, datas, replacement, offsets=None, errors="strict"):
    return cover_batch_utf8(matcher, datas, open=replacement, body="drop", offsets=offsets, errors=errors)


def mask(matcher, haystack, fill="*"):
    """every covered UTF-16 unit replaced by fill: the length is preserved"""
    return cover(matcher, haystack, body="fill", fill=fill)


def mask_utf8(matcher, data, fill=b"*", errors="strict"):
    """every covered byte replaced by the ASCII byte fill: the length and every byte offset are preserved"""
    return cover_utf8(matcher, data, body="fill", fill=fill, errors=errors)


def highlight(matcher, haystack, open, close):
    """every span wrapped in open and close"""
    return cover(matcher, haystack, open=open, close=close, body="keep")


def highlight_utf8(matcher, data, open, close, errors="strict"):
    return cover_utf8(matcher, data, open=open, close=close, body="keep", errors=errors)


def redact(matcher, haystack, replacement):
    """every span replaced by replacement -- touching matches are one span and give one replacement"""
    return cover(matcher, haystack, open=replacement, body="drop")


def redact_utf8(matcher, data, replacement, errors="strict"):
    return cover_utf8(matcher, data, open=replacement, body="drop", errors=errors)
