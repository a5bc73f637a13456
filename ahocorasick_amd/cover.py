"""Mask, highlight or redact every covered run of a text on the device (include/acgpu.h: acgpu_cover_u16, acgpu_cover_batch_u16, acgpu_cover_device,
acgpu_cover_utf8, acgpu_cover_utf8_lossy, acgpu_cover_batch_utf8, acgpu_cover_batch_utf8_lossy, acgpu_stream_cover_u16, acgpu_stream_cover_utf8,
acgpu_stream_cover_utf8_lossy): every span of the text -- the spans of ahocorasick_amd.spans, for all five families,
AhoCorasick's overlapping records included -- becomes open + body + close, everything else is copied.

    mask(AhoCorasickSet(names, False), text)                    # "call **** or ***" -- the length is preserved
    highlight(AhoCorasickSet(names, False), text, "<b>", "</b>")
    redact(AhoCorasickSet(names, False), text, "[name]")
    mask_batch(AhoCorasickSet(names, False), lines)             # many short texts: ONE device call, a list of str
    mask_batch_utf8(AhoCorasickSet(names, False), log, offsets=utf8_line_offsets(log))  # ... of bytes, the buffer used in place
    for piece in mask_utf8_readable(AhoCorasickSet(names, False), open("app.log", "rb")):  # a text of any length, chunk by chunk
        sink.write(piece)

Not replace: overlapping, nested and TOUCHING matches are one span, so two matches that touch give ONE replacement, not two.
No span and no record reaches the host.
"""
import ctypes

import numpy as np

from . import _native as N
from .spans import _automaton
from .strings import (_byte_chunks, _check_errors, _chunks, _fill_shard, _not_none, _pack, _pack_utf8, _raise_for, _readable, _retry_while_more,
                      _rewrite_call, _stats_dict, _to_str, _utf8_bytes, _utf8_entry, _vp, utf16)

__all__ = ["cover", "cover_utf8", "cover_device", "mask", "mask_utf8", "highlight", "highlight_utf8", "redact", "redact_utf8",
           "cover_batch", "cover_batch_units", "mask_batch", "highlight_batch", "redact_batch",
           "cover_batch_utf8", "cover_batch_bytes", "mask_batch_utf8", "highlight_batch_utf8", "redact_batch_utf8",
           "CoverStream", "cover_readable", "cover_utf8_readable", "mask_readable", "mask_utf8_readable", "highlight_readable",
           "highlight_utf8_readable", "redact_readable", "redact_utf8_readable"]

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


class CoverStream:
    """acgpu_stream_cover_u16 / _utf8 / _utf8_lossy: cover for a text that arrives in chunks of any size -- a log of 40 GB, a socket.
    The concatenation of what the feeds return is cover (cover_utf8) of everything fed, whatever the chunking; a feed returns what
    no later chunk can change, and withholds at most a keyword's length however long a span is: a span that is still open at a
    feed's end gets its open and the body so far now, and its close from the feed that sees it end.  open, close, fill: str, or for
    a stream of bytes bytes-like as well (cover_utf8's rules).  A stream is fed either units (feed) or bytes (feed_utf8)."""

    def __init__(self, matcher, open="", close="", body="keep", fill="*"):
        self._auto = _automaton(matcher)  # keeps the handle alive
        self._args = (_not_none(open), _not_none(close), _body(body), _not_none(fill))
        self._spec = {}  # per element size: (N.CoverSpec, the arrays it points into)
        self._errors = None
        h = ctypes.c_void_p()
        N.check(N.lib().acgpu_stream_open(self._auto.handle, ctypes.byref(h)), "acgpu_stream_open")
        self._h = h

    def _spec_for(self, esz):
        if esz not in self._spec:
            o, c, body, fill = self._args
            if esz == 2:
                self._spec[esz] = _spec(_units("open", o), _units("close", c), body, _fill_unit(fill))
            else:
                self._spec[esz] = _spec(_bytes("open", o), _bytes("close", c), body, _fill_byte(fill))
        return self._spec[esz][0]

    def _feed(self, entry, src, final, cap, stats):
        """the rewrite call, made again while it asks for more room (an overflow committed nothing) -> an array of src's type"""
        if self._h is None:
            raise ValueError("the stream is closed")
        spec = self._spec_for(src.dtype.itemsize)
        n = int(src.size)
        if cap is None:
            cap = n + n // 4 + 64 + int(spec.open_len) + int(spec.close_len)
        return _rewrite_call(entry, (self._h, _vp(_readable(src)), n, 1 if final else 0, ctypes.byref(spec)), src.dtype, n, cap, stats,
                             _retry_while_more)

    def feed(self, units, final=False, cap=None, stats=None):
        """the next units (str or uint16 array) -> the units of the result that have become decidable, a uint16 array.
        stats: an N.CoverStats to fill in, if wanted (this feed alone; n_spans: the spans whose open it delivered)."""
        return self._feed(N.lib().acgpu_stream_cover_u16, utf16(_not_none(units)), final, cap, [stats if stats is not None else N.CoverStats()])

    def feed_utf8(self, data, final=False, errors="strict", stats=None, cap=None, cover_stats=None):
        """the next bytes of a UTF-8 text (a chunk may end inside a sequence) -> the bytes of the result that have become decidable.
        Ill-formed input raises Utf8Error (.start: the GLOBAL offset) and finishes the stream; what had been withheld is not
        delivered -- unless errors="replace": nothing is raised, and the concatenation is cover_utf8(errors="replace") of everything
        fed.  The first feed fixes the stream's policy.  stats: an N.Utf8StreamStats (errors="replace": N.Utf8LossyStreamStats),
        cover_stats: an N.CoverStats to fill in, if wanted."""
        entry, stats_type = _utf8_entry("acgpu_stream_cover_utf8", errors)
        if self._errors is None:
            self._errors = errors
        elif self._errors != errors:
            raise ValueError("errors=%r on a stream that is fed with errors=%r" % (errors, self._errors))
        return self._feed(entry, _utf8_bytes(_not_none(data)), final, cap,
                          [stats if stats is not None else stats_type(), cover_stats if cover_stats is not None else N.CoverStats()]).tobytes()

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            N.lib().acgpu_stream_close(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    __del__ = close


def cover_readable(matcher, readable, open="", close="", body="keep", fill="*", chunk_chars=1 << 22):
    """cover for a text that is read as it goes -- an object with read(n) -> str, or an iterable of str / uint16 arrays, cut
    anywhere, inside a keyword or a span too -> a generator of str whose concatenation is cover() of the whole text.  A piece never
    ends between the two units of a surrogate pair: a trailing high surrogate waits for the next piece.  Closing the generator
    closes the stream; the stream is opened at the first next()."""
    st = CoverStream(matcher, open, close, body, fill)
    held = np.zeros(0, np.uint16)
    try:
        for final, chunk in _with_final(_chunks(readable, chunk_chars), ""):
            out = np.concatenate([held, st.feed(chunk, final=final)])
            cut = out.size - 1 if not final and out.size and 0xD800 <= int(out[-1]) < 0xDC00 else out.size
            held = out[cut:]
            yield _to_str(out[:cut])
    finally:
        st.close()


def cover_utf8_readable(matcher, readable, open=b"", close=b"", body="keep", fill=b"*", chunk_bytes=1 << 22, errors="strict"):
    """cover_utf8 for a text that is read as it goes -- a binary file object or an iterable of bytes-like chunks, cut anywhere,
    inside a sequence too -> a generator of bytes whose concatenation is cover_utf8() of the whole text.  Utf8Error (.start: the
    global offset) if the text is ill-formed -- unless errors="replace".  Closing the generator closes the stream."""
    _check_errors(errors)
    st = CoverStream(matcher, open, close, body, fill)
    try:
        for final, chunk in _with_final(_byte_chunks(readable, chunk_bytes), b""):
            yield st.feed_utf8(chunk, final=final, errors=errors)
    finally:
        st.close()


def _with_final(chunks, empty):
    """(False, chunk) for every chunk, then (True, empty): the feed that ends the text"""
    for chunk in chunks:
        yield False, chunk
    yield True, empty


def mask_readable(matcher, readable, fill="*", chunk_chars=1 << 22):
    return cover_readable(matcher, readable, body="fill", fill=fill, chunk_chars=chunk_chars)


def mask_utf8_readable(matcher, readable, fill=b"*", chunk_bytes=1 << 22, errors="strict"):
    """mask_utf8 of a file of any length, bytes in, bytes out: every piece has its chunk's byte offsets, shifted by what is withheld"""
    return cover_utf8_readable(matcher, readable, body="fill", fill=fill, chunk_bytes=chunk_bytes, errors=errors)


def highlight_readable(matcher, readable, open, close, chunk_chars=1 << 22):
    return cover_readable(matcher, readable, open=open, close=close, body="keep", chunk_chars=chunk_chars)


def highlight_utf8_readable(matcher, readable, open, close, chunk_bytes=1 << 22, errors="strict"):
    return cover_utf8_readable(matcher, readable, open=open, close=close, body="keep", chunk_bytes=chunk_bytes, errors=errors)


def redact_readable(matcher, readable, replacement, chunk_chars=1 << 22):
    return cover_readable(matcher, readable, open=replacement, body="drop", chunk_chars=chunk_chars)


def redact_utf8_readable(matcher, readable, replacement, chunk_bytes=1 << 22, errors="strict"):
    return cover_utf8_readable(matcher, readable, open=replacement, body="drop", chunk_bytes=chunk_bytes, errors=errors)
