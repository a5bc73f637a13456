"""CPU-side checks of stream replace (include/acgpu.h: acgpu_stream_replace_u16, acgpu_stream_replace_utf8): the symbols and their
bindings, and everything the entries decide before a device is touched -- the argument checks, the refusals, which of the four
kinds of feed a stream takes, the empty feeds and the feed after the last."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, LongestMatchMap, LongestMatchSet, Stream, utf16
from tests.helpers import WORD

vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
CANARY8 = (7, 7, 7, 7)      # acgpu_utf8_stream_stats
CANARY_R = (9, 9, 9, 9)     # acgpu_replace_stats
FILL = 0x5A
REPLACE_MODES = [N.MODE_LONGEST, N.MODE_WHOLEWORD, N.MODE_SHORTEST, N.MODE_WWLONGEST]


def automaton(mode, kws=("ab", "b")):
    return Automaton(mode, list(kws), True, word_chars=WORD if mode in (N.MODE_WHOLEWORD, N.MODE_WWLONGEST) else None)


def open_stream(a):
    h = ctypes.c_void_p()
    assert N.lib().acgpu_stream_open(a.handle, ctypes.byref(h)) == N.OK
    return h


def table(n_repl, esz, off=None):
    """n_repl replacements "#" -> (elements, offsets)"""
    units = np.full(max(n_repl, 1), ord("#"), np.uint16 if esz == 2 else np.uint8)
    return units, np.arange(n_repl + 1, dtype=np.uint64) if off is None else np.asarray(off, np.uint64)


def rep16(h, units, n, final, out, cap, n_out=True, tab=None, n_repl=1, stats=True):
    """-> (rc, n_out, replace stats)"""
    r_units, r_off = tab if tab is not None else table(n_repl, 2)
    st, m = N.ReplaceStats(*CANARY_R), ctypes.c_uint64(99)
    rc = N.lib().acgpu_stream_replace_u16(h, vp(units), n, final, vp(r_units), vp(r_off), n_repl, vp(out), cap,
                                          ctypes.byref(m) if n_out else None, ctypes.byref(st) if stats else None)
    return rc, m.value, st


def rep8(h, data, n, final, out, cap, n_out=True, tab=None, n_repl=1, stats=True):
    """-> (rc, n_out, replace stats, utf8 stream stats)"""
    r_bytes, r_off = tab if tab is not None else table(n_repl, 1)
    st, ust, m = N.ReplaceStats(*CANARY_R), N.Utf8StreamStats(*CANARY8), ctypes.c_uint64(99)
    rc = N.lib().acgpu_stream_replace_utf8(h, vp(data), n, final, vp(r_bytes), vp(r_off), n_repl, vp(out), cap,
                                           ctypes.byref(m) if n_out else None, ctypes.byref(ust) if stats else None,
                                           ctypes.byref(st) if stats else None)
    return rc, m.value, st, ust


def feed16(h, units, n, final=0):
    m, b = ctypes.c_uint64(99), ctypes.c_int64(-99)
    return N.lib().acgpu_stream_feed(h, vp(units), n, final, N.REC_MAP, None, 0, ctypes.byref(m), ctypes.byref(b))


def feed8(h, data, n, final=0):
    m, b = ctypes.c_uint64(99), ctypes.c_int64(-99)
    return N.lib().acgpu_stream_feed_utf8(h, vp(data), n, final, N.REC_MAP, None, 0, ctypes.byref(m), ctypes.byref(b), None)


def untouched_r(st):
    return (st.n_records, st.units_out, st.pieces, st.rescans) == CANARY_R


def untouched8(st):
    return (st.n_units, st.first_bad, st.ascii, st.held) == CANARY8


def zero_r(st):
    return (st.n_records, st.units_out, st.pieces, st.rescans) == (0, 0, 0, 0)


def test_the_library_exports_both_entries_and_python_binds_them():
    N.lib()  # (first: it loads torch's HIP runtime in front of the library, see _native.lib)
    L = ctypes.CDLL(N.LIB_PATH)
    for name in ("acgpu_stream_replace_u16", "acgpu_stream_replace_utf8"):
        assert name in N.SYMBOLS and hasattr(L, name)
        assert getattr(N.lib(), name).restype is ctypes.c_int
    assert len(N.lib().acgpu_stream_replace_u16.argtypes) == 11 and len(N.lib().acgpu_stream_replace_utf8.argtypes) == 12
    assert N.lib().acgpu_abi_version() == N.ABI_VERSION == 5
    assert hasattr(Stream, "replace_feed") and hasattr(Stream, "replace_feed_utf8")
    for cls in (LongestMatchSet, LongestMatchMap):
        assert hasattr(cls, "replace_readable") and hasattr(cls, "replace_utf8_readable")


def test_argument_checks_come_before_any_device():
    a = automaton(N.MODE_LONGEST)
    units = utf16("zabzab")
    data = np.frombuffer(b"zabzab", np.uint8).copy()
    out16, out8 = np.full(16, FILL, np.uint16), np.full(16, FILL, np.uint8)
    bad_tables = [dict(n_repl=3),                                        # neither 1 nor the number of keywords
                  dict(n_repl=2, tab=(table(2, 2)[0], None)),            # entries, and no offsets
                  dict(n_repl=2, tab=table(2, 2, off=[0, 2, 1])),        # descending offsets
                  dict(n_repl=1, tab=(None, np.array([0, 4], np.uint64)))]  # units to read, and no array
    h = open_stream(a)
    try:
        calls = [rep16(None, units, 6, 0, out16, 16), rep16(h, units, 6, 0, out16, 16, n_out=False),
                 rep16(h, None, 6, 0, out16, 16),       # units to read, and no buffer
                 rep16(h, units, 6, 1, None, 16),       # a capacity, and no array
                 rep16(h, units, 1 << 31, 0, out16, 16), rep16(h, units, 1 << 40, 1, out16, 16)]  # (nothing is read before the check)
        calls += [rep16(h, units, 6, 0, out16, 16, **t) for t in bad_tables]
        for i, (rc, n, st) in enumerate(calls):
            assert rc == N.E_INVALID and untouched_r(st), (i, rc)
        bad_tables[1]["tab"] = (table(2, 1)[0], None)
        bad_tables[2]["tab"] = table(2, 1, off=[0, 2, 1])
        calls = [rep8(None, data, 6, 0, out8, 16), rep8(h, data, 6, 0, out8, 16, n_out=False), rep8(h, None, 6, 0, out8, 16),
                 rep8(h, data, 6, 1, None, 16), rep8(h, data, 1 << 31, 0, out8, 16), rep8(h, data, 1 << 40, 1, out8, 16)]
        calls += [rep8(h, data, 6, 0, out8, 16, **t) for t in bad_tables]
        for i, (rc, n, st, ust) in enumerate(calls):
            assert rc == N.E_INVALID and untouched_r(st) and untouched8(ust), (i, rc)
        assert (out16 == FILL).all() and (out8 == FILL).all()
        # none of these has decided what the stream is: it still takes a match feed (an empty one: no device)
        assert feed16(h, None, 0) == N.OK
    finally:
        N.lib().acgpu_stream_close(h)


def test_all_matches_mode_is_unsupported():
    a = automaton(N.MODE_ALL)
    units, data = utf16("zab"), np.frombuffer(b"zab", np.uint8).copy()
    out16, out8 = np.full(8, FILL, np.uint16), np.full(8, FILL, np.uint8)
    h = open_stream(a)
    try:
        for args in ((None, 0, 0), (units, 3, 0), (units, 3, 1)):
            rc, n, st = rep16(h, args[0], args[1], args[2], out16, 8)
            assert rc == N.E_UNSUPPORTED and untouched_r(st)
        for args in ((None, 0, 0), (data, 3, 0), (data, 3, 1)):
            rc, n, st, ust = rep8(h, args[0], args[1], args[2], out8, 8)
            assert rc == N.E_UNSUPPORTED and untouched_r(st) and untouched8(ust)
        assert (out16 == FILL).all() and (out8 == FILL).all()
    finally:
        N.lib().acgpu_stream_close(h)
    s = Stream(a)
    try:
        with pytest.raises(N.AcgpuError) as e:
            s.replace_feed(units, "#")
        assert e.value.code == N.E_UNSUPPORTED
        with pytest.raises(N.AcgpuError) as e:
            s.replace_feed_utf8(b"zab", "#")
        assert e.value.code == N.E_UNSUPPORTED
    finally:
        s.close()


def test_a_dictionary_with_an_unpaired_surrogate_is_unsupported_for_bytes_only():
    lone = np.concatenate([utf16("a"), utf16("😀")[:1]])
    a = Automaton(N.MODE_LONGEST, [lone, "b"], True)
    data = np.frombuffer(b"zab", np.uint8).copy()
    out8 = np.full(8, FILL, np.uint8)
    h = open_stream(a)
    try:
        for args in ((None, 0, 0), (data, 3, 1)):
            rc, n, st, ust = rep8(h, args[0], args[1], args[2], out8, 8)
            assert rc == N.E_UNSUPPORTED and untouched_r(st) and untouched8(ust)
        assert (out8 == FILL).all()
        # the refusal has not decided what the stream is, and units are not refused: an empty feed passes (no device)
        rc, n, st = rep16(h, None, 0, 0, None, 0)
        assert (rc, n) == (N.OK, 0) and zero_r(st)
    finally:
        N.lib().acgpu_stream_close(h)


def test_a_pipelined_stream_is_unsupported():
    a = automaton(N.MODE_LONGEST)
    units, data = utf16("ab"), np.frombuffer(b"ab", np.uint8).copy()
    h = open_stream(a)
    try:
        assert N.lib().acgpu_stream_set_pipelined(h, 1) == N.OK
        for args in ((None, 0, 0), (units, 2, 0), (units, 2, 1)):
            rc, n, st = rep16(h, args[0], args[1], args[2], None, 0)
            assert rc == N.E_UNSUPPORTED and untouched_r(st)
        for args in ((None, 0, 0), (data, 2, 0), (data, 2, 1)):
            rc, n, st, ust = rep8(h, args[0], args[1], args[2], None, 0)
            assert rc == N.E_UNSUPPORTED and untouched_r(st) and untouched8(ust)
    finally:
        N.lib().acgpu_stream_close(h)
    # ... and a replace stream cannot be switched to the pipelined form
    h = open_stream(a)
    try:
        assert rep16(h, None, 0, 0, None, 0)[0] == N.OK
        assert N.lib().acgpu_stream_set_pipelined(h, 1) == N.E_INVALID
    finally:
        N.lib().acgpu_stream_close(h)


KINDS = {"match units": lambda h, final=0: feed16(h, None, 0, final),
         "match bytes": lambda h, final=0: feed8(h, None, 0, final),
         "replace units": lambda h, final=0: rep16(h, None, 0, final, None, 0)[0],
         "replace bytes": lambda h, final=0: rep8(h, None, 0, final, None, 0)[0]}


@pytest.mark.parametrize("later", sorted(KINDS))
@pytest.mark.parametrize("first", sorted(KINDS))
def test_the_first_feed_decides_which_of_the_four_kinds_a_stream_is(first, later):
    a = automaton(N.MODE_LONGEST)
    h = open_stream(a)
    try:
        assert KINDS[first](h) == N.OK  # a feed of length 0 decides it
        want = N.OK if later == first else N.E_INVALID
        assert KINDS[later](h) == want
        assert KINDS[later](h, 1) == want
        if later != first:  # the stream is still what it was, and open
            assert KINDS[first](h, 1) == N.OK
    finally:
        N.lib().acgpu_stream_close(h)


@pytest.mark.parametrize("mode", REPLACE_MODES)
def test_empty_feeds_need_no_device_and_nothing_follows_the_final_one(mode):
    a = automaton(mode)
    units, data = utf16("ab"), np.frombuffer(b"ab", np.uint8).copy()
    h = open_stream(a)
    try:
        for n_repl in (1, 2):
            rc, n, st = rep16(h, None, 0, 0, None, 0, n_repl=n_repl)
            assert (rc, n) == (N.OK, 0) and zero_r(st)
        assert rep16(h, None, 0, 0, None, 0, stats=False)[:2] == (N.OK, 0)
        rc, n, st = rep16(h, None, 0, 1, None, 0)
        assert (rc, n) == (N.OK, 0) and zero_r(st)
        for args in ((None, 0, 0), (None, 0, 1), (units, 2, 0)):  # the stream is finished
            rc, n, st = rep16(h, args[0], args[1], args[2], None, 0)
            assert rc == N.E_INVALID and untouched_r(st)
    finally:
        N.lib().acgpu_stream_close(h)
    h = open_stream(a)
    try:
        rc, n, st, ust = rep8(h, None, 0, 0, None, 0)
        assert (rc, n) == (N.OK, 0) and zero_r(st) and (ust.n_units, ust.first_bad, ust.ascii, ust.held) == (0, -1, 1, 0)
        assert rep8(h, None, 0, 0, None, 0, stats=False)[:2] == (N.OK, 0)
        rc, n, st, ust = rep8(h, None, 0, 1, None, 0, n_repl=2)
        assert (rc, n) == (N.OK, 0) and zero_r(st) and (ust.n_units, ust.first_bad, ust.ascii, ust.held) == (0, -1, 1, 0)
        for args in ((None, 0, 0), (None, 0, 1), (data, 2, 0)):
            rc, n, st, ust = rep8(h, args[0], args[1], args[2], None, 0)
            assert rc == N.E_INVALID and untouched_r(st) and untouched8(ust)
    finally:
        N.lib().acgpu_stream_close(h)
    # ... through the wrapper
    s = Stream(a)
    try:
        got = s.replace_feed(np.zeros(0, np.uint16), "#")
        assert got.shape == (0,) and got.dtype == np.uint16
        assert s.replace_feed("", ["x", "y"], final=True).size == 0
        with pytest.raises(N.AcgpuError) as e:
            s.replace_feed("", "#")
        assert e.value.code == N.E_INVALID
    finally:
        s.close()
    s = Stream(a)
    try:
        assert s.replace_feed_utf8(b"", b"#") == b"" and s.replace_feed_utf8(bytearray(), "#", final=True) == b""
        with pytest.raises(N.AcgpuError) as e:
            s.replace_feed_utf8(b"", "#")
        assert e.value.code == N.E_INVALID
    finally:
        s.close()


def test_a_detached_stream_is_invalid():
    a = automaton(N.MODE_LONGEST)
    h = open_stream(a)
    try:
        N.lib().acgpu_free(a.handle)
        a._h = None
        rc, n, st = rep16(h, None, 0, 0, None, 0)
        assert rc == N.E_INVALID and untouched_r(st)
        rc, n, st, ust = rep8(h, None, 0, 0, None, 0)
        assert rc == N.E_INVALID and untouched_r(st) and untouched8(ust)
    finally:
        N.lib().acgpu_stream_close(h)
