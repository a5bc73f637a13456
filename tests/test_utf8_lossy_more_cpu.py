"""CPU-side checks of lossy replace and the lossy streams (include/acgpu.h: acgpu_replace_utf8_lossy, acgpu_replace_batch_utf8_lossy,
acgpu_stream_feed_utf8_lossy, acgpu_stream_replace_utf8_lossy): the symbols and the new stats struct, everything the entries decide
before a device is touched -- every refusal of their strict counterparts, with outputs and stats untouched; the empty text, batch
and feeds; the policy as a part of the stream's kind -- the facade's errors= keyword, and the Python splice that the GPU tests take
their expected bytes from."""
import codecs
import ctypes
import os

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import (AhoCorasickMap, AhoCorasickSet, Automaton, LongestMatchMap, LongestMatchSet, ShortestMatchSet, Stream,
                                     WholeWordLongestMatchMap, WholeWordMatchSet, utf16)
from oracle.oracle import FAM_LONGEST, Oracle
from tests.helpers import WORD
from tests.utf8_lossy_ref import ALPHABET, TABLE, damaged, decode_replace

vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if isinstance(x, np.ndarray) else x  # (None and ctypes buffers as they are)
CANARY = 0xA5
LOSSY_CANARY = (7, 7, 7, 7, 7)
LOSSY_PRESET = (0, 0, -1, 0, 1)
STREAM_CANARY = (7, 7, 7, 7)
STREAM_PRESET = (0, 0, 1, 0)
REPLACE_MODES = [N.MODE_LONGEST, N.MODE_SHORTEST, N.MODE_WHOLEWORD, N.MODE_WWLONGEST]
NEW = ("acgpu_replace_utf8_lossy", "acgpu_replace_batch_utf8_lossy", "acgpu_stream_feed_utf8_lossy", "acgpu_stream_replace_utf8_lossy")


def automaton(mode, kws=("ab", "b"), cs=True):
    return Automaton(mode, list(kws), cs, word_chars=WORD if mode in (N.MODE_WHOLEWORD, N.MODE_WWLONGEST) else None)


def table(repls):
    """-> (bytes, offsets) in the layout the entries read"""
    parts = [np.frombuffer(r.encode(), np.uint8) for r in repls]
    off = np.zeros(len(parts) + 1, np.uint64)
    off[1:] = np.cumsum([p.size for p in parts])
    return np.concatenate(parts + [np.zeros(1, np.uint8)]), off


def fields(st):
    return tuple(getattr(st, f) for f, _ in type(st)._fields_)


def offs(*v):
    return np.array(v, dtype=np.uint64)


def replace(a, data, n_bytes, r_bytes, off, n_repl, out, cap, n_out=True):
    """acgpu_replace_utf8_lossy -> (rc, n_out, replace stats, lossy stats)"""
    no = ctypes.c_uint64(99)
    st, ust = N.ReplaceStats(7, 7, 7, 7), N.Utf8LossyStats(*LOSSY_CANARY)
    rc = N.lib().acgpu_replace_utf8_lossy(a.handle if a else None, vp(data), n_bytes, vp(r_bytes), vp(off), n_repl, vp(out), cap,
                                          ctypes.byref(no) if n_out else None, ctypes.byref(st), ctypes.byref(ust))
    return rc, no.value, st, ust


def replace_batch(a, data, offsets, n_hay, r_bytes, off, n_repl, out, cap, out_off, n_out=True):
    """acgpu_replace_batch_utf8_lossy -> (rc, n_out, replace stats, lossy stats)"""
    no = ctypes.c_uint64(99)
    st, ust = N.ReplaceStats(7, 7, 7, 7), N.Utf8LossyStats(*LOSSY_CANARY)
    rc = N.lib().acgpu_replace_batch_utf8_lossy(a.handle if a else None, vp(data), vp(offsets), n_hay, vp(r_bytes), vp(off), n_repl, vp(out), cap,
                                                vp(out_off), ctypes.byref(no) if n_out else None, ctypes.byref(st), ctypes.byref(ust))
    return rc, no.value, st, ust


def open_stream(a):
    h = ctypes.c_void_p()
    assert N.lib().acgpu_stream_open(a.handle, ctypes.byref(h)) == N.OK
    return h


def feed(h, data, n, final, kind, out, cap, n_out=True, base=True, lossy=True):
    """acgpu_stream_feed_utf8[_lossy] -> (rc, n_out, base, stats)"""
    st = N.Utf8LossyStreamStats(*STREAM_CANARY) if lossy else N.Utf8StreamStats(*STREAM_CANARY)
    m, b = ctypes.c_uint64(99), ctypes.c_int64(-99)
    entry = N.lib().acgpu_stream_feed_utf8_lossy if lossy else N.lib().acgpu_stream_feed_utf8
    rc = entry(h, vp(data), n, final, kind, vp(out), cap, ctypes.byref(m) if n_out else None, ctypes.byref(b) if base else None, ctypes.byref(st))
    return rc, m.value, b.value, st


def replace_feed(h, data, n, final, r_bytes, off, n_repl, out, cap, n_out=True, lossy=True):
    """acgpu_stream_replace_utf8[_lossy] -> (rc, n_out, stream stats, replace stats)"""
    ust = N.Utf8LossyStreamStats(*STREAM_CANARY) if lossy else N.Utf8StreamStats(*STREAM_CANARY)
    rst = N.ReplaceStats(7, 7, 7, 7)
    m = ctypes.c_uint64(99)
    entry = N.lib().acgpu_stream_replace_utf8_lossy if lossy else N.lib().acgpu_stream_replace_utf8
    rc = entry(h, vp(data), n, final, vp(r_bytes), vp(off), n_repl, vp(out), cap, ctypes.byref(m) if n_out else None, ctypes.byref(ust), ctypes.byref(rst))
    return rc, m.value, ust, rst


def feed16(h):
    m, b = ctypes.c_uint64(99), ctypes.c_int64(-99)
    return N.lib().acgpu_stream_feed(h, None, 0, 0, N.REC_MAP, None, 0, ctypes.byref(m), ctypes.byref(b))


def test_the_library_exports_the_entries_and_binds_their_types():
    L = ctypes.CDLL(N.LIB_PATH)
    for name in NEW:
        assert name in N.SYMBOLS and hasattr(L, name), name
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "acgpu.h")).read()
    for name in NEW:
        assert "int %s(" % name in hdr, name
    assert N.lib().acgpu_replace_utf8_lossy.argtypes[-1] == ctypes.POINTER(N.Utf8LossyStats)
    assert N.lib().acgpu_replace_batch_utf8_lossy.argtypes[-1] == ctypes.POINTER(N.Utf8LossyStats)
    assert N.lib().acgpu_stream_feed_utf8_lossy.argtypes[-1] == ctypes.POINTER(N.Utf8LossyStreamStats)
    assert N.lib().acgpu_stream_replace_utf8_lossy.argtypes[-2:] == [ctypes.POINTER(N.Utf8LossyStreamStats), ctypes.POINTER(N.ReplaceStats)]
    assert ctypes.sizeof(N.Utf8LossyStreamStats) == 24
    assert [(f, getattr(N.Utf8LossyStreamStats, f).offset) for f, _ in N.Utf8LossyStreamStats._fields_] == [
        ("n_units", 0), ("n_replaced", 8), ("ascii", 16), ("held", 20)]
    assert N.lib().acgpu_abi_version() == N.ABI_VERSION == 5


# ---- replace and batch replace --------------------------------------------------------------------------------------------------------
def test_replace_argument_checks_come_before_any_device():
    a = automaton(N.MODE_LONGEST, ["ab", "", "b", "ab"])
    data = np.frombuffer(b"zab\x80", np.uint8)
    r_bytes, off = table(["x", "y", "z", "w"])
    out = np.full(16, CANARY, np.uint8)
    r6, off6 = table(["x"] * 6)
    calls = [replace(None, data, 4, r_bytes, off, 4, out, 16), replace(a, None, 4, r_bytes, off, 4, out, 16),
             replace(a, data, 4, r_bytes, off, 4, out, 16, n_out=False), replace(a, data, 4, r_bytes, off, 4, None, 16),
             replace(a, data, 4, r_bytes, np.array([0, 2, 1, 3, 4], np.uint64), 4, out, 16), replace(a, data, 4, r_bytes, None, 4, out, 16)]
    calls += [replace(a, data, n, r_bytes, off, 4, out, 16) for n in (1 << 31, (1 << 31) + 5, 1 << 40)]
    calls += [replace(a, data, 4, r6, off6, n_repl, out, 16) for n_repl in (0, 2, 3, 5, 6)]
    for i, (rc, n, st, ust) in enumerate(calls):
        assert rc == N.E_INVALID and fields(ust) == LOSSY_CANARY and st.n_records == 7, (i, rc)
    assert (out == CANARY).all()


def test_batch_replace_argument_checks_come_before_any_device():
    a = automaton(N.MODE_LONGEST)
    data = np.frombuffer(b"zab\x80ab", np.uint8)
    r_bytes, off = table(["x"])
    r6, off6 = table(["x"] * 6)
    out = np.full(16, CANARY, np.uint8)
    out_off = np.full(3, 77, np.uint64)
    o = offs(0, 4, 6)
    calls = [replace_batch(None, data, o, 2, r_bytes, off, 1, out, 16, out_off), replace_batch(a, data, None, 2, r_bytes, off, 1, out, 16, out_off),
             replace_batch(a, data, o, 2, r_bytes, off, 1, out, 16, out_off, n_out=False), replace_batch(a, data, o, 2, r_bytes, off, 1, out, 16, None),
             replace_batch(a, data, o, 2, r_bytes, off, 1, None, 16, out_off), replace_batch(a, None, o, 2, r_bytes, off, 1, out, 16, out_off),
             replace_batch(a, data, offs(0, 5, 4), 2, r_bytes, off, 1, out, 16, out_off), replace_batch(a, data, offs(4, 2, 6), 2, r_bytes, off, 1, out, 16, out_off),
             replace_batch(a, data, offs(0, 1 << 31), 1, r_bytes, off, 1, out, 16, out_off),
             replace_batch(a, data, offs(0, 3, (1 << 31) - 2), 2, r_bytes, off, 1, out, 16, out_off),
             replace_batch(a, data, o, 2, r_bytes, None, 1, out, 16, out_off)]
    calls += [replace_batch(a, data, o, 2, r6, off6, n_repl, out, 16, out_off) for n_repl in (0, 3, 6)]
    for i, (rc, n, st, ust) in enumerate(calls):
        assert rc == N.E_INVALID and fields(ust) == LOSSY_CANARY and st.n_records == 7, (i, rc)
    assert (out == CANARY).all() and (out_off == 77).all()


@pytest.mark.parametrize("cs", [True, False])
def test_mode_all_and_unpaired_surrogates_are_unsupported_before_any_device(cs):
    data = np.frombuffer("a😀b ab".encode() + b"\x80", np.uint8)
    r_bytes, off = table(["#"])
    r6, off6 = table(["x"] * 6)
    out = np.full(32, CANARY, np.uint8)
    out_off = np.full(3, 77, np.uint64)
    o = offs(0, 6, data.size)
    autos = [automaton(N.MODE_ALL, cs=cs)]
    for kws in (["\ud83d", "ab"], ["ab", "\ude00"], ["x\ud83d", "ab"], ["\ude00\ud83d"], ["😀\ud83d"]):
        autos += [Automaton(N.MODE_SHORTEST, kws, cs), Automaton(N.MODE_LONGEST, kws, cs)]
    for a in autos:
        rc, n, st, ust = replace(a, data, data.size, r_bytes, off, 1, out, 32)
        assert rc == N.E_UNSUPPORTED and fields(ust) == LOSSY_CANARY and st.n_records == 7
        rc, n, st, ust = replace_batch(a, data, o, 2, r_bytes, off, 1, out, 32, out_off)
        assert rc == N.E_UNSUPPORTED and fields(ust) == LOSSY_CANARY and st.n_records == 7
        h = open_stream(a)
        try:
            rc, n, ust, rst = replace_feed(h, data, data.size, 0, r_bytes, off, 1, out, 32)
            assert rc == N.E_UNSUPPORTED and fields(ust) == STREAM_CANARY and rst.n_records == 7
        finally:
            N.lib().acgpu_stream_close(h)
    # (the table is checked first, as for the strict entries)
    assert replace(autos[0], data, data.size, r6, off6, 3, out, 32)[0] == N.E_INVALID
    assert replace_batch(autos[0], data, o, 2, r6, off6, 3, out, 32, out_off)[0] == N.E_INVALID
    assert (out == CANARY).all() and (out_off == 77).all()
    with pytest.raises(N.AcgpuError) as e:
        autos[0].replace_utf8(b"zab\x80", "#", errors="replace")
    assert e.value.code == N.E_UNSUPPORTED
    with pytest.raises(N.AcgpuError) as e:
        autos[0].replace_batch_utf8([b"zab\x80"], "#", errors="replace")
    assert e.value.code == N.E_UNSUPPORTED


@pytest.mark.parametrize("mode", REPLACE_MODES)
def test_an_empty_text_and_an_empty_batch_need_no_device(mode):
    a = automaton(mode)
    r_bytes, off = table(["x"])
    for data in (None, np.frombuffer(b"\x80", np.uint8)):
        rc, n, st, ust = replace(a, data, 0, r_bytes, off, 1, None, 0)
        assert (rc, n) == (N.OK, 0) and (st.n_records, st.units_out, st.pieces) == (0, 0, 0) and fields(ust) == LOSSY_PRESET
    data = np.frombuffer(b"\x80y", np.uint8)
    for buf, o, n_hay in ((None, offs(0), 0), (data, offs(1), 0), (None, offs(0, 0, 0, 0), 3), (data, offs(2, 2), 1), (data, offs(1, 1, 1), 2)):
        out_off = np.full(n_hay + 1, 77, np.uint64)
        rc, n, st, ust = replace_batch(a, buf, o, n_hay, r_bytes, off, 1, None, 0, out_off)
        assert (rc, n) == (N.OK, 0) and (st.n_records, st.units_out, st.pieces) == (0, 0, 0) and fields(ust) == LOSSY_PRESET
        assert (out_off == 0).all()
    got, st = a.replace_utf8(b"", "x", errors="replace")
    assert got.shape == (0,) and got.dtype == np.uint8 and st["units_out"] == 0
    got, out_off, st = a.replace_batch_utf8([b"", b""], "x", errors="replace")
    assert got.shape == (0,) and out_off.tolist() == [0, 0, 0]
    assert LongestMatchSet(["ab"], True).replace_utf8(b"", "x", errors="replace") == b""
    assert LongestMatchMap(["ab"], ["v"], True).replace_batch_utf8([b"", b""], errors="replace") == [b"", b""]


# ---- the stream feeds ---------------------------------------------------------------------------------------------------------------
def test_feed_argument_checks_come_before_any_device():
    a = automaton(N.MODE_ALL)
    data = ctypes.create_string_buffer(b"zab\x80ab", 6)
    out = np.full((4, 3), 0x5A5A5A5A, np.int32)
    h = open_stream(a)
    try:
        calls = [feed(None, data, 6, 0, N.REC_SET, out, 4), feed(h, data, 6, 0, N.REC_SET, out, 4, n_out=False),
                 feed(h, data, 6, 0, N.REC_SET, out, 4, base=False), feed(h, None, 6, 0, N.REC_SET, out, 4), feed(h, data, 6, 1, N.REC_MAP, None, 4),
                 feed(h, data, 1 << 31, 0, N.REC_MAP, out, 4), feed(h, data, 1 << 40, 1, N.REC_SET, out, 4)]
        calls += [feed(h, data, 6, 0, kind, out, 4) for kind in (0, 4, 10, 16, -8)]
        for i, (rc, n, base, st) in enumerate(calls):
            assert rc == N.E_INVALID and fields(st) == STREAM_CANARY, (i, rc)
        assert (out == 0x5A5A5A5A).all()
        assert feed16(h) == N.OK  # none of these has made the stream one of bytes: it still takes units
    finally:
        N.lib().acgpu_stream_close(h)
    h = open_stream(a)
    try:
        assert N.lib().acgpu_stream_set_pipelined(h, 1) == N.OK
        for args in ((None, 0, 0), (data, 2, 1)):
            rc, n, base, st = feed(h, args[0], args[1], args[2], N.REC_MAP, None, 0)
            assert rc == N.E_UNSUPPORTED and fields(st) == STREAM_CANARY
    finally:
        N.lib().acgpu_stream_close(h)


def test_replace_feed_argument_checks_come_before_any_device():
    a = automaton(N.MODE_LONGEST, ["ab", "", "b", "ab"])
    data = ctypes.create_string_buffer(b"zab\x80", 4)
    r_bytes, off = table(["x", "y", "z", "w"])
    r6, off6 = table(["x"] * 6)
    out = np.full(16, CANARY, np.uint8)
    h = open_stream(a)
    try:
        calls = [replace_feed(None, data, 4, 0, r_bytes, off, 4, out, 16), replace_feed(h, data, 4, 0, r_bytes, off, 4, out, 16, n_out=False),
                 replace_feed(h, None, 4, 0, r_bytes, off, 4, out, 16), replace_feed(h, data, 4, 1, r_bytes, off, 4, None, 16),
                 replace_feed(h, data, 1 << 31, 0, r_bytes, off, 4, out, 16), replace_feed(h, data, 1 << 40, 1, r_bytes, off, 4, out, 16),
                 replace_feed(h, data, 4, 0, r_bytes, np.array([0, 2, 1, 3, 4], np.uint64), 4, out, 16), replace_feed(h, data, 4, 0, r_bytes, None, 4, out, 16)]
        calls += [replace_feed(h, data, 4, 0, r6, off6, n_repl, out, 16) for n_repl in (0, 2, 3, 5, 6)]
        for i, (rc, n, ust, rst) in enumerate(calls):
            assert rc == N.E_INVALID and fields(ust) == STREAM_CANARY and rst.n_records == 7, (i, rc)
        assert (out == CANARY).all()
        assert feed16(h) == N.OK  # the stream has no kind yet
    finally:
        N.lib().acgpu_stream_close(h)
    h = open_stream(a)
    try:
        assert N.lib().acgpu_stream_set_pipelined(h, 1) == N.OK
        rc, n, ust, rst = replace_feed(h, data, 4, 0, r_bytes, off, 4, out, 16)
        assert rc == N.E_UNSUPPORTED and fields(ust) == STREAM_CANARY and (out == CANARY).all()
    finally:
        N.lib().acgpu_stream_close(h)


@pytest.mark.parametrize("mode", [N.MODE_ALL] + REPLACE_MODES)
def test_empty_feeds_need_no_device(mode):
    a = automaton(mode)
    r_bytes, off = table(["x"])
    data = ctypes.create_string_buffer(b"ab", 2)
    h = open_stream(a)
    try:
        for kind in (N.REC_MAP, N.REC_SET):
            rc, n, base, st = feed(h, None, 0, 0, kind, None, 0)
            assert (rc, n, base) == (N.OK, 0, 0) and fields(st) == STREAM_PRESET
        rc, n, base, st = feed(h, None, 0, 1, N.REC_MAP, None, 0)  # the end of a stream that holds nothing
        assert (rc, n, base) == (N.OK, 0, 0) and fields(st) == STREAM_PRESET
        for args in ((None, 0, 0), (None, 0, 1), (data, 2, 0)):  # the stream is finished
            rc, n, base, st = feed(h, args[0], args[1], args[2], N.REC_MAP, None, 0)
            assert rc == N.E_INVALID and fields(st) == STREAM_CANARY
    finally:
        N.lib().acgpu_stream_close(h)
    if mode == N.MODE_ALL:
        return
    h = open_stream(a)
    try:
        rc, n, ust, rst = replace_feed(h, None, 0, 0, r_bytes, off, 1, None, 0)
        assert (rc, n) == (N.OK, 0) and fields(ust) == STREAM_PRESET and (rst.n_records, rst.units_out) == (0, 0)
        rc, n, ust, rst = replace_feed(h, None, 0, 1, r_bytes, off, 1, None, 0)
        assert (rc, n) == (N.OK, 0) and fields(ust) == STREAM_PRESET and (rst.n_records, rst.units_out) == (0, 0)
        rc, n, ust, rst = replace_feed(h, data, 2, 0, r_bytes, off, 1, None, 0)
        assert rc == N.E_INVALID and fields(ust) == STREAM_CANARY
    finally:
        N.lib().acgpu_stream_close(h)
    s = Stream(a)
    try:
        assert s.feed_utf8(b"", errors="replace").shape == (0, 3)
        assert s.feed_utf8(bytearray(), final=True, errors="replace").shape == (0, 3)
    finally:
        s.close()
    s = Stream(a)
    try:
        assert s.replace_feed_utf8(b"", "x", errors="replace") == b"" and s.replace_feed_utf8(b"", "x", final=True, errors="replace") == b""
    finally:
        s.close()


def test_the_policy_is_part_of_the_streams_kind():
    a = automaton(N.MODE_LONGEST)
    r_bytes, off = table(["x"])
    data = ctypes.create_string_buffer(b"ab", 2)
    out = np.full(16, CANARY, np.uint8)
    recs = np.full((4, 3), 0x5A5A5A5A, np.int32)
    # (first feed, then every entry that must refuse the stream: match or replace, lossy or not)
    first = {"feed lossy": lambda h: feed(h, None, 0, 0, N.REC_MAP, None, 0)[0],
             "feed strict": lambda h: feed(h, None, 0, 0, N.REC_MAP, None, 0, lossy=False)[0],
             "replace lossy": lambda h: replace_feed(h, None, 0, 0, r_bytes, off, 1, None, 0)[0],
             "replace strict": lambda h: replace_feed(h, None, 0, 0, r_bytes, off, 1, None, 0, lossy=False)[0]}
    later = {"feed lossy": lambda h, n, f: feed(h, data if n else None, n, f, N.REC_MAP, recs, 4),
             "feed strict": lambda h, n, f: feed(h, data if n else None, n, f, N.REC_MAP, recs, 4, lossy=False),
             "replace lossy": lambda h, n, f: replace_feed(h, data if n else None, n, f, r_bytes, off, 1, out, 16),
             "replace strict": lambda h, n, f: replace_feed(h, data if n else None, n, f, r_bytes, off, 1, out, 16, lossy=False)}
    for kind in first:
        h = open_stream(a)
        try:
            assert first[kind](h) == N.OK, kind  # a feed of length 0 decides it
            for other in later:
                if other == kind:
                    continue
                for n, f in ((0, 0), (0, 1), (2, 0), (2, 1)):
                    res = later[other](h, n, f)
                    assert res[0] == N.E_INVALID and fields(res[-2] if other.startswith("replace") else res[-1]) == STREAM_CANARY, (kind, other, n, f)
            assert feed16(h) == N.E_INVALID
            assert first[kind](h) == N.OK, kind  # it is still a stream of its kind, and open
        finally:
            N.lib().acgpu_stream_close(h)
    assert (out == CANARY).all() and (recs == 0x5A5A5A5A).all()


def test_a_stream_remembers_its_policy_without_a_native_call():
    a = automaton(N.MODE_LONGEST)
    for first, second in (("strict", "replace"), ("replace", "strict")):
        for mk in (lambda s, e: s.feed_utf8(b"", errors=e), lambda s, e: s.replace_feed_utf8(b"", "x", errors=e)):
            s = Stream(a)
            try:
                mk(s, first)
                handle, s._h = s._h, None  # a native call would now fail on the handle
                try:
                    with pytest.raises(ValueError, match="errors"):
                        mk(s, second)
                finally:
                    s._h = handle
                mk(s, first)
            finally:
                s.close()


def test_errors_is_strict_or_replace_on_every_new_method_and_checked_before_a_native_call():
    a = automaton(N.MODE_LONGEST, ["ab"])
    sets = [LongestMatchSet(["ab"], True), ShortestMatchSet(["ab"], True), WholeWordMatchSet(["ab"], True), AhoCorasickSet(["ab"], True)]
    maps = [LongestMatchMap(["ab"], ["v"], True), WholeWordLongestMatchMap(["ab"], ["v"], True), AhoCorasickMap(["ab"], ["v"], True)]
    calls = [lambda e: a.replace_utf8(None, "x", errors=e), lambda e: a.replace_batch_utf8(None, "x", errors=e)]
    for f in sets + maps:
        arg = ("x",) if f in sets else ()
        calls += [lambda e, f=f, arg=arg: f.replace_utf8(None, *arg, errors=e), lambda e, f=f, arg=arg: f.replace_batch_utf8(None, *arg, errors=e),
                  lambda e, f=f, arg=arg: f.replace_utf8_readable(None, *arg, errors=e), lambda e, f=f: f.match_utf8_readable(None, None, errors=e),
                  lambda e, f=f: f.find_all_utf8_readable(None, errors=e)]
    s = Stream(a)
    handle, s._h = s._h, None
    try:
        calls += [lambda e: s.feed_utf8(b"ab", errors=e), lambda e: s.replace_feed_utf8(b"ab", "x", errors=e)]
        for call in calls:
            for e in ("ignore", "Replace", None, "surrogateescape"):
                with pytest.raises(ValueError, match="errors"):
                    call(e)
        assert s._errors is None  # a refused keyword fixes no policy
    finally:
        s._h = handle
        s.close()


# ---- the reference of the GPU tests ---------------------------------------------------------------------------------------------------
def lossy_records(orc, data):
    """the oracle's Map records on the reference's decoded text, in bytes of `data` through the reference's per-unit table"""
    text, off, length, replaced = decode_replace(data)
    if not text:
        return np.zeros((0, 3), np.int32)
    recs = orc.match(utf16(text), cap=max(1024, 8 * len(off)))
    want = recs.copy()
    if len(recs):
        want[:, 0] = off[recs[:, 0]]
        want[:, 1] = off[recs[:, 1] - 1] + length[recs[:, 1] - 1]
    return want


def splice(data, brecs, repls):
    """data[0:s_0] + repl[id_0] + data[e_0:s_1] + ... over the ORIGINAL bytes"""
    if len(brecs):
        assert (brecs[:, 0] < brecs[:, 1]).all() and (brecs[1:, 0] >= brecs[:-1, 1]).all() and brecs[-1, 1] <= len(data)
    parts, last = [], 0
    for s, e, k in brecs.tolist():
        parts += [data[last:s], repls[k] if isinstance(repls, list) else repls]
        last = e
    return b"".join(parts + [data[last:]])


def test_the_splice_reference():
    kws = ["ab", "é", "q", "�", "�b"]
    repls = [b"<1>", "É".encode(), b"", b"?", b"#"]
    orc = Oracle(FAM_LONGEST, kws, True, None, None, map_flavour=True)
    # well-formed input: the two rules coincide -- splicing the bytes is replacing in the decoded text
    for text in ("", "ab", "xabéq€😀ab", "q" * 40 + "😀é" * 9 + "ab", "no match here"):
        data = text.encode()
        got = splice(data, lossy_records(orc, data), repls)
        # (no replacement holds a keyword, so replacing one keyword after the other is replacing them all at once)
        assert got == text.replace("ab", "<1>").replace("é", "É").replace("q", "").encode(), text
        assert data.decode("utf-8", "replace") == text
    # every row of the table: its subparts are the records of the U+FFFD keyword, removed and nothing else
    for row, spans in TABLE:
        recs = lossy_records(orc, b"x" + row + b"y")
        assert [r[:2] for r in recs.tolist()] == [[s + 1, e + 1] for s, e in spans], row
        got = splice(b"x" + row + b"y", recs, repls)
        rest = bytearray(b"x" + row + b"y")
        for s, e in reversed(spans):
            rest[s + 1:e + 1] = b"?"
        assert got == bytes(rest), row
    # outside the matches the bytes stay as they are, ill-formed ones included; "�b" takes the subpart's bytes with the b
    data = b"ab\xc0ab\xe2\x82b \xf5q"
    assert splice(data, lossy_records(Oracle(FAM_LONGEST, ["ab", "q"], True, None, None, map_flavour=True), data), [b"<1>", b""]) == b"<1>\xc0<1>\xe2\x82b \xf5"
    assert splice(data, lossy_records(orc, data), repls) == b"<1>?<1># ?"


def held_ref(fed):
    """the claim rule on the bytes fed so far: the last unit of their lossy decoding is held back when it is a subpart that begins
    with a byte that can lead a sequence (C2..F4) and ends where the bytes end -- a subpart is a lead with all it has claimed, and
    at the end of the bytes no present byte has failed it.  No lead looks more than 3 bytes ahead: the last three bytes decide."""
    tail = bytes(fed[-3:])
    _, off, length, replaced = decode_replace(tail)
    return int(length[-1]) if len(off) and replaced[-1] and 0xC2 <= tail[int(off[-1])] <= 0xF4 else 0


def test_the_held_reference_is_cpythons_incremental_decoder_but_for_a_cut_surrogate():
    rng = np.random.default_rng(515)
    bufs = damaged(rng, "aé€😀 q中Ж".encode() * 8, n_buffers=1500, max_len=40)
    bufs += [bytes(ALPHABET[int(i)] for i in rng.integers(0, len(ALPHABET), int(n))) for n in rng.integers(1, 12, 1500)]
    seen = set()
    for b in bufs:
        d = codecs.getincrementaldecoder("utf-8")("replace")
        d.decode(b)
        cpython = len(d.getstate()[0])
        _, off, length, replaced = decode_replace(b)
        whole = int(length[-1]) if len(off) and replaced[-1] and 0xC2 <= b[int(off[-1])] <= 0xF4 else 0  # the rule on ALL the bytes
        assert held_ref(b) == whole, b
        if len(b) >= 2 and b[-2] == 0xED and 0xA0 <= b[-1] <= 0xBF:
            assert (held_ref(b), cpython) == (0, 2), b  # decided now: two U+FFFD
        else:
            assert held_ref(b) == cpython, b
        seen.add(held_ref(b))
    assert seen == {0, 1, 2, 3}
