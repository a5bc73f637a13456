"""CPU-side checks of the chunked UTF-8 feed (include/acgpu.h: acgpu_stream_feed_utf8): the symbol and its stats struct, and
everything the entry decides before a device is touched -- the argument checks, the empty feeds, which kind of feed a stream
takes, the pipelined form and the feed after the last."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickSet, Automaton, Stream
from tests.helpers import WORD

vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
CANARY = (7, 7, 7, 7)
FILL = 0x5A5A5A5A


def open_stream(a):
    h = ctypes.c_void_p()
    assert N.lib().acgpu_stream_open(a.handle, ctypes.byref(h)) == N.OK
    return h


def feed8(h, data, n, final, kind, out, cap, n_out=True, base=True, stats=True):
    """-> (rc, n_out, base, stats)"""
    st = N.Utf8StreamStats(*CANARY)
    m, b = ctypes.c_uint64(99), ctypes.c_int64(-99)
    rc = N.lib().acgpu_stream_feed_utf8(h, data, n, final, kind, vp(out), cap, ctypes.byref(m) if n_out else None,
                                        ctypes.byref(b) if base else None, ctypes.byref(st) if stats else None)
    return rc, m.value, b.value, st


def feed16(h, units, n, final=0, kind=N.REC_MAP):
    """-> (rc, n_out)"""
    m, b = ctypes.c_uint64(99), ctypes.c_int64(-99)
    rc = N.lib().acgpu_stream_feed(h, vp(units), n, final, kind, None, 0, ctypes.byref(m), ctypes.byref(b))
    return rc, m.value


def untouched(st):
    return (st.n_units, st.first_bad, st.ascii, st.held) == CANARY


def test_the_library_exports_the_entry_and_binds_its_types():
    L = ctypes.CDLL(N.LIB_PATH)
    assert "acgpu_stream_feed_utf8" in N.SYMBOLS and hasattr(L, "acgpu_stream_feed_utf8")
    assert ctypes.sizeof(N.Utf8StreamStats) == 24
    assert [(f, getattr(N.Utf8StreamStats, f).offset) for f, _ in N.Utf8StreamStats._fields_] == [("n_units", 0), ("first_bad", 8), ("ascii", 16),
                                                                                                 ("held", 20)]
    assert N.lib().acgpu_abi_version() == N.ABI_VERSION == 5
    assert hasattr(Stream, "feed_utf8") and hasattr(AhoCorasickSet, "match_utf8_readable") and hasattr(AhoCorasickSet, "find_all_utf8_readable")


def test_argument_checks_come_before_any_device():
    a = Automaton(N.MODE_ALL, ["ab", "b"], True)
    data = ctypes.create_string_buffer(b"zabzab", 6)
    out = np.full((4, 3), FILL, np.int32)
    h = open_stream(a)
    try:
        calls = [feed8(None, data, 6, 0, N.REC_SET, out, 4),
                 feed8(h, data, 6, 0, N.REC_SET, out, 4, n_out=False),
                 feed8(h, data, 6, 0, N.REC_SET, out, 4, base=False),
                 feed8(h, None, 6, 0, N.REC_SET, out, 4),      # bytes to read, and no buffer
                 feed8(h, data, 6, 1, N.REC_MAP, None, 4),     # a capacity, and no array
                 # carried bytes + n_bytes stay below 2^31 (nothing is read before the check)
                 feed8(h, data, 1 << 31, 0, N.REC_MAP, out, 4), feed8(h, data, 1 << 40, 1, N.REC_SET, out, 4)]
        calls += [feed8(h, data, 6, 0, kind, out, 4) for kind in (0, 4, 10, 16, -8)]
        for i, (rc, n, base, st) in enumerate(calls):
            assert rc == N.E_INVALID and untouched(st), (i, rc)
        assert (out == FILL).all()
        # none of these has made the stream one of bytes: it still takes units (an empty feed: no device)
        assert feed16(h, None, 0) == (N.OK, 0)
    finally:
        N.lib().acgpu_stream_close(h)


@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_LONGEST, N.MODE_WHOLEWORD, N.MODE_SHORTEST, N.MODE_WWLONGEST])
def test_empty_feeds_need_no_device(mode):
    a = Automaton(mode, ["ab", "b"], True, word_chars=WORD if mode in (N.MODE_WHOLEWORD, N.MODE_WWLONGEST) else None)
    h = open_stream(a)
    try:
        for kind in (N.REC_MAP, N.REC_SET):
            rc, n, base, st = feed8(h, None, 0, 0, kind, None, 0)
            assert (rc, n, base) == (N.OK, 0, 0) and (st.n_units, st.first_bad, st.ascii, st.held) == (0, -1, 1, 0)
        assert feed8(h, None, 0, 0, N.REC_MAP, None, 0, stats=False)[:3] == (N.OK, 0, 0)
        rc, n, base, st = feed8(h, None, 0, 1, N.REC_MAP, None, 0)
        assert (rc, n, base) == (N.OK, 0, 0) and (st.n_units, st.first_bad, st.ascii, st.held) == (0, -1, 1, 0)
        # the stream is finished: a feed after the final one, of either kind and any length
        data = ctypes.create_string_buffer(b"ab", 2)
        for args in ((None, 0, 0), (None, 0, 1), (data, 2, 0)):
            rc, n, base, st = feed8(h, args[0], args[1], args[2], N.REC_MAP, None, 0)
            assert rc == N.E_INVALID and untouched(st)
        assert feed16(h, None, 0)[0] == N.E_INVALID
    finally:
        N.lib().acgpu_stream_close(h)
    # ... through the wrapper
    s = Stream(a, with_ids=True)
    try:
        got = s.feed_utf8(b"")
        assert got.shape == (0, 3) and got.dtype == np.int64
        assert s.feed_utf8(bytearray(), final=True).shape == (0, 3)
        with pytest.raises(N.AcgpuError) as e:
            s.feed_utf8(b"")
        assert e.value.code == N.E_INVALID
    finally:
        s.close()


def test_the_first_feed_decides_the_kind():
    a = Automaton(N.MODE_LONGEST, ["ab", "b"], True)
    units = np.zeros(1, np.uint16)
    h = open_stream(a)
    try:
        assert feed8(h, None, 0, 0, N.REC_MAP, None, 0)[0] == N.OK  # a feed of length 0 decides it
        assert feed16(h, None, 0)[0] == N.E_INVALID
        assert feed16(h, units, 1, final=1)[0] == N.E_INVALID
        assert N.lib().acgpu_stream_set_pipelined(h, 1) == N.E_INVALID  # a stream of bytes has no pipelined form
        assert feed8(h, None, 0, 0, N.REC_MAP, None, 0)[0] == N.OK      # it is still a stream of bytes, and open
    finally:
        N.lib().acgpu_stream_close(h)
    h = open_stream(a)
    try:
        assert feed16(h, None, 0) == (N.OK, 0)
        data = ctypes.create_string_buffer(b"ab", 2)
        for args in ((None, 0, 0), (None, 0, 1), (data, 2, 0)):
            rc, n, base, st = feed8(h, args[0], args[1], args[2], N.REC_MAP, None, 0)
            assert rc == N.E_INVALID and untouched(st)
        assert feed16(h, None, 0) == (N.OK, 0)  # it is still a stream of units
    finally:
        N.lib().acgpu_stream_close(h)


def test_a_pipelined_stream_is_unsupported():
    a = Automaton(N.MODE_ALL, ["ab"], True)
    h = open_stream(a)
    try:
        assert N.lib().acgpu_stream_set_pipelined(h, 1) == N.OK
        data = ctypes.create_string_buffer(b"ab", 2)
        for args in ((None, 0, 0), (data, 2, 0), (data, 2, 1)):
            rc, n, base, st = feed8(h, args[0], args[1], args[2], N.REC_MAP, None, 0)
            assert rc == N.E_UNSUPPORTED and untouched(st)
    finally:
        N.lib().acgpu_stream_close(h)
    s = Stream(a, with_ids=False, pipelined=True)
    try:
        with pytest.raises(N.AcgpuError) as e:
            s.feed_utf8(b"ab")
        assert e.value.code == N.E_UNSUPPORTED
    finally:
        s.close()


def test_a_detached_stream_is_invalid():
    a = Automaton(N.MODE_ALL, ["ab"], True)
    h = open_stream(a)
    try:
        N.lib().acgpu_free(a.handle)
        a._h = None
        rc, n, base, st = feed8(h, None, 0, 0, N.REC_MAP, None, 0)
        assert rc == N.E_INVALID and untouched(st)
    finally:
        N.lib().acgpu_stream_close(h)
