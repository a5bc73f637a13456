"""CPU-side checks of stream cover (include/acgpu.h: acgpu_stream_cover_u16, acgpu_stream_cover_utf8, acgpu_stream_cover_utf8_lossy):
the symbols and their bindings, and everything the entries decide before a device is touched -- the argument checks, the refusals,
which kind of feed a stream takes, the empty feeds and the feed after the last -- and the wrappers' argument handling."""
import ctypes
import importlib

import numpy as np
import pytest

import ahocorasick_amd
from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, Stream, utf16
from tests.helpers import WORD

C = importlib.import_module("ahocorasick_amd.cover")  # (the package's name `cover` is the function)

vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
CANARY8 = (7, 7, 7, 7)            # acgpu_utf8_stream_stats / acgpu_utf8_lossy_stream_stats
CANARY_C = (9, 9, 9, 9, 9, 9, 9)  # acgpu_cover_stats
FILL = 0x5A
MODES = [N.MODE_ALL, N.MODE_LONGEST, N.MODE_WHOLEWORD, N.MODE_SHORTEST, N.MODE_WWLONGEST]
ENTRIES = ("acgpu_stream_cover_u16", "acgpu_stream_cover_utf8", "acgpu_stream_cover_utf8_lossy")


def automaton(mode, kws=("ab", "b")):
    return Automaton(mode, list(kws), True, word_chars=WORD if mode in (N.MODE_WHOLEWORD, N.MODE_WWLONGEST) else None)


def open_stream(a):
    h = ctypes.c_void_p()
    assert N.lib().acgpu_stream_open(a.handle, ctypes.byref(h)) == N.OK
    return h


def spec_of(esz, open_=b"<", close=b">", body=N.COVER_KEEP, fill=ord("*")):
    """-> (N.CoverSpec, what it points into)"""
    dt = np.uint16 if esz == 2 else np.uint8
    o, c = np.frombuffer(open_, np.uint8).astype(dt), np.frombuffer(close, np.uint8).astype(dt)
    return N.CoverSpec(o.ctypes.data if o.size else None, o.size, c.ctypes.data if c.size else None, c.size, body, fill), (o, c)


def cov16(h, units, n, final, out, cap, n_out=True, spec="default", stats=True):
    """-> (rc, n_out, cover stats)"""
    sp, keep = spec_of(2)
    sp = sp if isinstance(spec, str) else spec
    st, m = N.CoverStats(*CANARY_C), ctypes.c_uint64(99)
    rc = N.lib().acgpu_stream_cover_u16(h, vp(units), n, final, ctypes.byref(sp) if sp is not None else None, vp(out), cap,
                                        ctypes.byref(m) if n_out else None, ctypes.byref(st) if stats else None)
    return rc, m.value, st


def cov8(h, data, n, final, out, cap, n_out=True, spec="default", stats=True, lossy=False):
    """-> (rc, n_out, cover stats, utf8 stream stats)"""
    sp, keep = spec_of(1)
    sp = sp if isinstance(spec, str) else spec
    ust = (N.Utf8LossyStreamStats if lossy else N.Utf8StreamStats)(*CANARY8)
    st, m = N.CoverStats(*CANARY_C), ctypes.c_uint64(99)
    entry = N.lib().acgpu_stream_cover_utf8_lossy if lossy else N.lib().acgpu_stream_cover_utf8
    rc = entry(h, vp(data), n, final, ctypes.byref(sp) if sp is not None else None, vp(out), cap, ctypes.byref(m) if n_out else None,
               ctypes.byref(ust) if stats else None, ctypes.byref(st) if stats else None)
    return rc, m.value, st, ust


def feed16(h, units, n, final=0):
    m, b = ctypes.c_uint64(99), ctypes.c_int64(-99)
    return N.lib().acgpu_stream_feed(h, vp(units), n, final, N.REC_SET, None, 0, ctypes.byref(m), ctypes.byref(b))


def feed8(h, data, n, final=0, lossy=False):
    m, b = ctypes.c_uint64(99), ctypes.c_int64(-99)
    entry = N.lib().acgpu_stream_feed_utf8_lossy if lossy else N.lib().acgpu_stream_feed_utf8
    return entry(h, vp(data), n, final, N.REC_SET, None, 0, ctypes.byref(m), ctypes.byref(b), None)


def rep16(h, final=0):
    r, off, m = np.full(1, ord("#"), np.uint16), np.arange(2, dtype=np.uint64), ctypes.c_uint64(99)
    return N.lib().acgpu_stream_replace_u16(h, None, 0, final, vp(r), vp(off), 1, None, 0, ctypes.byref(m), None)


def rep8(h, final=0, lossy=False):
    r, off, m = np.full(1, ord("#"), np.uint8), np.arange(2, dtype=np.uint64), ctypes.c_uint64(99)
    entry = N.lib().acgpu_stream_replace_utf8_lossy if lossy else N.lib().acgpu_stream_replace_utf8
    return entry(h, None, 0, final, vp(r), vp(off), 1, None, 0, ctypes.byref(m), None, None)


def fields(st):
    return tuple(int(getattr(st, f)) for f, _ in st._fields_)


def untouched_c(st):
    return fields(st) == CANARY_C


def untouched8(st):
    return fields(st) == CANARY8


def zero_c(st):
    return fields(st) == (0,) * 7


def test_the_library_exports_the_three_entries_and_python_binds_them():
    N.lib()  # (first: it loads torch's HIP runtime in front of the library, see _native.lib)
    L = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert name in N.SYMBOLS and hasattr(L, name)
        assert getattr(N.lib(), name).restype is ctypes.c_int
    assert [len(getattr(N.lib(), name).argtypes) for name in ENTRIES] == [9, 10, 10]
    assert N.UTF8_STATS["acgpu_stream_cover_utf8"] is N.Utf8StreamStats
    assert N.UTF8_STATS["acgpu_stream_cover_utf8_lossy"] is N.Utf8LossyStreamStats
    assert N.lib().acgpu_abi_version() == N.ABI_VERSION == 5
    header = open(N.LIB_PATH.rsplit("/ahocorasick_amd/", 1)[0] + "/include/acgpu.h").read()
    for name in ENTRIES:
        assert "int %s(" % name in header
    for name in ("CoverStream", "cover_readable", "cover_utf8_readable", "mask_readable", "mask_utf8_readable", "highlight_readable",
                 "highlight_utf8_readable", "redact_readable", "redact_utf8_readable"):
        assert name in C.__all__ and name in ahocorasick_amd.__all__ and getattr(ahocorasick_amd, name) is getattr(C, name)
    # nothing was added to Stream: the binding classes are pinned (tests/golden/python_surface.json)
    assert not any("cover" in name for name in dir(Stream))


def bad_specs(esz):
    keep = []

    def sp(**kw):
        s, k = spec_of(esz, **kw)
        keep.append(k)
        return s
    none_open, none_close, long_open = sp(), sp(), sp()
    none_open.open = None     # a length, and no pointer
    none_close.close = None
    long_open.open_len = 1 << 31
    return keep, [None, sp(body=3), none_open, none_close, long_open, sp(body=N.COVER_FILL, fill=0x10000 if esz == 2 else 0x80)]


def test_argument_checks_come_before_any_device():
    a = automaton(N.MODE_ALL)
    units = utf16("zabzab")
    data = np.frombuffer(b"zabzab", np.uint8).copy()
    out16, out8 = np.full(16, FILL, np.uint16), np.full(16, FILL, np.uint8)
    h = open_stream(a)
    try:
        keep, specs = bad_specs(2)
        calls = [cov16(None, units, 6, 0, out16, 16), cov16(h, units, 6, 0, out16, 16, n_out=False),
                 cov16(h, None, 6, 0, out16, 16),       # units to read, and no buffer
                 cov16(h, units, 6, 1, None, 16),       # a capacity, and no array
                 cov16(h, units, 1 << 31, 0, out16, 16), cov16(h, units, 1 << 40, 1, out16, 16)]  # (nothing is read before the check)
        calls += [cov16(h, units, 6, 0, out16, 16, spec=s) for s in specs]
        for i, (rc, n, st) in enumerate(calls):
            assert rc == N.E_INVALID and untouched_c(st), (i, rc)
        # (a FILL unit that a unit holds and a byte does not is fine for units)
        keep8, specs8 = bad_specs(1)
        for lossy in (False, True):
            calls = [cov8(None, data, 6, 0, out8, 16, lossy=lossy), cov8(h, data, 6, 0, out8, 16, n_out=False, lossy=lossy),
                     cov8(h, None, 6, 0, out8, 16, lossy=lossy), cov8(h, data, 6, 1, None, 16, lossy=lossy),
                     cov8(h, data, 1 << 31, 0, out8, 16, lossy=lossy), cov8(h, data, 1 << 40, 1, out8, 16, lossy=lossy)]
            calls += [cov8(h, data, 6, 0, out8, 16, spec=s, lossy=lossy) for s in specs8]
            for i, (rc, n, st, ust) in enumerate(calls):
                assert rc == N.E_INVALID and untouched_c(st) and untouched8(ust), (lossy, i, rc)
        assert (out16 == FILL).all() and (out8 == FILL).all()
        # none of these has decided what the stream is: it still takes a match feed (an empty one: no device)
        assert feed16(h, None, 0) == N.OK
    finally:
        N.lib().acgpu_stream_close(h)


def test_a_fill_only_counts_with_the_fill_body():
    a = automaton(N.MODE_LONGEST)
    h = open_stream(a)
    try:
        sp, keep = spec_of(1, body=N.COVER_KEEP, fill=0xFF)
        rc, n, st, ust = cov8(h, None, 0, 0, None, 0, spec=sp)
        assert (rc, n) == (N.OK, 0) and zero_c(st)
    finally:
        N.lib().acgpu_stream_close(h)


def test_a_pipelined_stream_is_unsupported():
    a = automaton(N.MODE_LONGEST)
    units, data = utf16("ab"), np.frombuffer(b"ab", np.uint8).copy()
    h = open_stream(a)
    try:
        assert N.lib().acgpu_stream_set_pipelined(h, 1) == N.OK
        for args in ((None, 0, 0), (units, 2, 0), (units, 2, 1)):
            rc, n, st = cov16(h, args[0], args[1], args[2], None, 0)
            assert rc == N.E_UNSUPPORTED and untouched_c(st)
        for lossy in (False, True):
            for args in ((None, 0, 0), (data, 2, 0), (data, 2, 1)):
                rc, n, st, ust = cov8(h, args[0], args[1], args[2], None, 0, lossy=lossy)
                assert rc == N.E_UNSUPPORTED and untouched_c(st) and untouched8(ust)
        # a bad spec is refused first, as the entries without a stream refuse it
        assert cov16(h, None, 0, 0, None, 0, spec=None)[0] == N.E_INVALID
    finally:
        N.lib().acgpu_stream_close(h)
    # ... and a cover stream cannot be switched to the pipelined form
    h = open_stream(a)
    try:
        assert cov16(h, None, 0, 0, None, 0)[0] == N.OK
        assert N.lib().acgpu_stream_set_pipelined(h, 1) == N.E_INVALID
    finally:
        N.lib().acgpu_stream_close(h)


COVER_KINDS = {"cover units": lambda h, final=0: cov16(h, None, 0, final, None, 0)[0],
               "cover bytes": lambda h, final=0: cov8(h, None, 0, final, None, 0)[0],
               "cover bytes lossy": lambda h, final=0: cov8(h, None, 0, final, None, 0, lossy=True)[0]}
OTHER_KINDS = {"match units": lambda h, final=0: feed16(h, None, 0, final),
               "match bytes": lambda h, final=0: feed8(h, None, 0, final),
               "match bytes lossy": lambda h, final=0: feed8(h, None, 0, final, lossy=True),
               "replace units": lambda h, final=0: rep16(h, final),
               "replace bytes": lambda h, final=0: rep8(h, final),
               "replace bytes lossy": lambda h, final=0: rep8(h, final, lossy=True)}
KINDS = dict(COVER_KINDS, **OTHER_KINDS)


# (every pair with a cover entry in it: the others are tests/test_stream_replace_cpu.py's)
PAIRS = [(f, l) for f in sorted(KINDS) for l in sorted(KINDS) if f in COVER_KINDS or l in COVER_KINDS]


@pytest.mark.parametrize("first,later", PAIRS)
def test_the_first_feed_decides_the_kind_in_both_directions(first, later):
    a = automaton(N.MODE_LONGEST)
    h = open_stream(a)
    try:
        assert KINDS[first](h) == N.OK  # a feed of length 0 decides it, no device
        want = N.OK if later == first else N.E_INVALID
        assert KINDS[later](h) == want
        assert KINDS[later](h, 1) == want
        if later != first:  # the stream is still what it was, and open
            assert KINDS[first](h, 1) == N.OK
    finally:
        N.lib().acgpu_stream_close(h)


def test_a_refused_cover_feed_of_another_kind_leaves_everything_untouched():
    a = automaton(N.MODE_ALL)
    out16, out8 = np.full(8, FILL, np.uint16), np.full(8, FILL, np.uint8)
    h = open_stream(a)
    try:
        assert feed16(h, None, 0) == N.OK
        rc, n, st = cov16(h, utf16("ab"), 2, 1, out16, 8)
        assert rc == N.E_INVALID and untouched_c(st)
        for lossy in (False, True):
            rc, n, st, ust = cov8(h, np.frombuffer(b"ab", np.uint8).copy(), 2, 1, out8, 8, lossy=lossy)
            assert rc == N.E_INVALID and untouched_c(st) and untouched8(ust)
        assert (out16 == FILL).all() and (out8 == FILL).all()
    finally:
        N.lib().acgpu_stream_close(h)


@pytest.mark.parametrize("mode", MODES)
def test_empty_feeds_need_no_device_and_nothing_follows_the_final_one(mode):
    a = automaton(mode)
    units, data = utf16("ab"), np.frombuffer(b"ab", np.uint8).copy()
    h = open_stream(a)
    try:
        for body in (N.COVER_KEEP, N.COVER_FILL, N.COVER_DROP):
            sp, keep = spec_of(2, body=body)
            rc, n, st = cov16(h, None, 0, 0, None, 0, spec=sp)
            assert (rc, n) == (N.OK, 0) and zero_c(st)
        assert cov16(h, None, 0, 0, None, 0, stats=False)[:2] == (N.OK, 0)
        rc, n, st = cov16(h, None, 0, 1, None, 0)  # the end of a stream that holds nothing and is not inside a span
        assert (rc, n) == (N.OK, 0) and zero_c(st)
        for args in ((None, 0, 0), (None, 0, 1), (units, 2, 0)):  # the stream is finished
            rc, n, st = cov16(h, args[0], args[1], args[2], None, 0)
            assert rc == N.E_INVALID and untouched_c(st)
    finally:
        N.lib().acgpu_stream_close(h)
    for lossy in (False, True):
        preset = (0, 0, 1, 0) if lossy else (0, -1, 1, 0)
        h = open_stream(a)
        try:
            rc, n, st, ust = cov8(h, None, 0, 0, None, 0, lossy=lossy)
            assert (rc, n) == (N.OK, 0) and zero_c(st) and fields(ust) == preset
            assert cov8(h, None, 0, 0, None, 0, stats=False, lossy=lossy)[:2] == (N.OK, 0)
            rc, n, st, ust = cov8(h, None, 0, 1, None, 0, lossy=lossy)
            assert (rc, n) == (N.OK, 0) and zero_c(st) and fields(ust) == preset
            for args in ((None, 0, 0), (None, 0, 1), (data, 2, 0)):
                rc, n, st, ust = cov8(h, args[0], args[1], args[2], None, 0, lossy=lossy)
                assert rc == N.E_INVALID and untouched_c(st) and untouched8(ust)
        finally:
            N.lib().acgpu_stream_close(h)


def test_a_detached_stream_is_invalid():
    a = automaton(N.MODE_LONGEST)
    h = open_stream(a)
    try:
        N.lib().acgpu_free(a.handle)
        a._h = None
        rc, n, st = cov16(h, None, 0, 0, None, 0)
        assert rc == N.E_INVALID and untouched_c(st)
        rc, n, st, ust = cov8(h, None, 0, 0, None, 0)
        assert rc == N.E_INVALID and untouched_c(st) and untouched8(ust)
    finally:
        N.lib().acgpu_stream_close(h)


def test_the_wrapper_checks_its_arguments_and_passes_empty_feeds():
    a = automaton(N.MODE_ALL)
    with pytest.raises(ValueError):
        C.CoverStream(a, body="mask")
    with pytest.raises(TypeError):
        C.CoverStream(a, open=None)
    with C.CoverStream(a, "<", ">", "fill", "*") as s:
        got = s.feed(np.zeros(0, np.uint16))
        assert got.shape == (0,) and got.dtype == np.uint16
        st = N.CoverStats(*CANARY_C)
        assert s.feed("", final=True, stats=st).size == 0 and zero_c(st)
        with pytest.raises(N.AcgpuError) as e:
            s.feed("")
        assert e.value.code == N.E_INVALID
    with pytest.raises(ValueError):  # closed by the context manager
        s.feed("")
    s.close()  # (twice is fine)
    with C.CoverStream(a, b"<", b">") as s:
        assert s.feed_utf8(b"") == b"" and s.feed_utf8(bytearray(), final=True) == b""
    with C.CoverStream(a) as s:
        assert s.feed_utf8(b"", errors="replace") == b""
        with pytest.raises(ValueError):  # the first byte feed fixed the policy
            s.feed_utf8(b"", errors="strict")
        with pytest.raises(ValueError):
            s.feed_utf8(b"", errors="ignore")
        with pytest.raises(N.AcgpuError) as e:  # a stream of bytes takes no units
            s.feed("")
        assert e.value.code == N.E_INVALID
    with C.CoverStream(a, fill="**") as s:  # the fill is looked at when the first feed says what an element is
        with pytest.raises(ValueError):
            s.feed("")
    with C.CoverStream(a, fill="é") as s:
        assert s.feed("").size == 0  # one unit
    with C.CoverStream(a, fill="é") as s:
        with pytest.raises(ValueError):  # ... and no ASCII byte
            s.feed_utf8(b"")


def test_the_generators_pass_an_empty_text_and_close_their_stream():
    a = automaton(N.MODE_ALL)
    assert list(C.cover_readable(a, [], "<", ">")) == [""]
    assert list(C.mask_readable(a, iter(["", ""]))) == ["", "", ""]
    assert list(C.redact_utf8_readable(a, [b""], b"#")) == [b"", b""]
    assert list(C.highlight_utf8_readable(a, [], b"<", b">", errors="replace")) == [b""]
    with pytest.raises(ValueError):
        next(C.mask_utf8_readable(a, [b""], errors="ignore"))
    g = C.highlight_readable(a, [""], "<", ">")
    assert next(g) == ""
    g.close()
    assert list(g) == []
