"""CPU-side checks of the UTF-8 batch entries (include/acgpu.h: acgpu_match_batch_utf8, acgpu_summary_batch_utf8): the symbols
and their stats struct, everything they decide before a device is touched, and the host helpers of the facade."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickMap, AhoCorasickSet, Automaton, Utf8Error, utf8_line_offsets

vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
CANARY = (7, 7, 7, 7)
FILL = 0x5A5A5A5A


def _match(a, data, off, n, kind, out, cap, n_out=True, stats=True):
    """-> (rc, n_out, stats)"""
    st = N.Utf8BatchStats(*CANARY)
    m = ctypes.c_uint64(99)
    rc = N.lib().acgpu_match_batch_utf8(a.handle if a else None, data, vp(off), n, kind, vp(out), cap, ctypes.byref(m) if n_out else None,
                                        ctypes.byref(st) if stats else None)
    return rc, m.value, st


def _summary(a, data, off, n, out, stats=True):
    """-> (rc, summary stats, stats)"""
    st = N.Utf8BatchStats(*CANARY)
    sst = N.SummaryStats(7, 7, 7, 7)
    rc = N.lib().acgpu_summary_batch_utf8(a.handle if a else None, data, vp(off), n, vp(out), ctypes.byref(sst), ctypes.byref(st) if stats else None)
    return rc, sst, st


def untouched(st):
    return (st.n_units, st.first_bad, st.bad_haystack, st.ascii) == CANARY


def offs(*v):
    return np.array(v, dtype=np.uint64)


def test_the_library_exports_the_entries_and_binds_their_types():
    L = ctypes.CDLL(N.LIB_PATH)
    for name in ("acgpu_match_batch_utf8", "acgpu_summary_batch_utf8"):
        assert name in N.SYMBOLS and hasattr(L, name)
    assert ctypes.sizeof(N.Utf8BatchStats) == 24
    assert [(f, getattr(N.Utf8BatchStats, f).offset) for f, _ in N.Utf8BatchStats._fields_] == [("n_units", 0), ("first_bad", 8), ("bad_haystack", 16),
                                                                                               ("ascii", 20)]
    assert N.lib().acgpu_abi_version() == N.ABI_VERSION == 5


def test_utf8_error_names_the_haystack():
    e = Utf8Error(3, haystack=2)
    assert isinstance(e, ValueError) and (e.start, e.haystack) == (3, 2) and "2" in str(e) and "3" in str(e)
    e = Utf8Error(12)
    assert (e.start, e.haystack) == (12, None)


def test_match_argument_checks_come_before_any_device():
    a = Automaton(N.MODE_ALL, ["ab", "b"], True)
    data = ctypes.create_string_buffer(b"zabzab", 6)
    off = offs(0, 4, 6)
    out = np.full((4, 4), FILL, np.int32)
    calls = [_match(None, data, off, 2, N.REC_SET, out, 4),
             _match(a, None, off, 2, N.REC_SET, out, 4),                  # bytes to read, and no buffer
             _match(a, data, None, 2, N.REC_SET, out, 4),                 # no offsets
             _match(a, data, off, 2, N.REC_SET, out, 4, n_out=False),
             _match(a, data, off, 2, N.REC_SET, None, 4),                 # a capacity, and no array
             _match(a, data, offs(0, 5, 4), 2, N.REC_MAP, out, 4),        # descending offsets
             _match(a, data, offs(4, 2, 6), 2, N.REC_MAP, out, 4)]
    calls += [_match(a, data, off, 2, kind, out, 4) for kind in (0, 4, 10, 16, -8)]
    # the span, and the span plus one separator per haystack, stay below 2^31 (nothing is read before the check)
    calls += [_match(a, data, offs(0, 1 << 31), 1, N.REC_MAP, out, 4), _match(a, data, offs(5, 5 + (1 << 31) - 1), 1, N.REC_MAP, out, 4),
              _match(a, data, offs(0, 3, (1 << 31) - 2), 2, N.REC_MAP, out, 4), _match(a, data, offs(0, 1 << 40), 1, N.REC_SET, out, 4)]
    for i, (rc, n, st) in enumerate(calls):
        assert rc == N.E_INVALID and untouched(st), (i, rc)
    assert (out == FILL).all()


def test_summary_argument_checks_come_before_any_device():
    a = Automaton(N.MODE_LONGEST, ["ab", "b"], True)
    data = ctypes.create_string_buffer(b"zabzab", 6)
    off = offs(0, 4, 6)
    out = np.zeros(2, dtype=N.SUMMARY_DTYPE)
    out[:] = (77, 7, 7, 7, 7)
    calls = [_summary(None, data, off, 2, out), _summary(a, None, off, 2, out), _summary(a, data, None, 2, out), _summary(a, data, off, 2, None),
             _summary(a, data, offs(0, 5, 4), 2, out), _summary(a, data, offs(0, 1 << 31), 1, out),
             _summary(a, data, offs(0, 3, (1 << 31) - 2), 2, out), _summary(a, data, offs(0, 1 << 40), 1, out)]
    for i, (rc, sst, st) in enumerate(calls):
        assert rc == N.E_INVALID and untouched(st) and sst.n_records == 7, (i, rc)
    assert all(tuple(r) == (77, 7, 7, 7, 7) for r in out.tolist())


@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_LONGEST, N.MODE_SHORTEST])
def test_no_haystacks_and_empty_haystacks_need_no_device(mode):
    a = Automaton(mode, ["ab", "b"], True)
    data = ctypes.create_string_buffer(b"xy", 2)
    for buf, off, n in ((None, offs(0), 0), (data, offs(1), 0), (None, offs(0, 0, 0, 0), 3), (data, offs(2, 2), 1), (data, offs(1, 1, 1), 2)):
        rc, m, st = _match(a, buf, off, n, N.REC_MAP, None, 0)
        assert (rc, m) == (N.OK, 0) and (st.n_units, st.first_bad, st.bad_haystack, st.ascii) == (0, -1, 0, 1)
        assert _match(a, buf, off, n, N.REC_SET, None, 0, stats=False)[:2] == (N.OK, 0)
        out = np.zeros(max(n, 1), dtype=N.SUMMARY_DTYPE)
        out[:] = (77, 7, 7, 7, 7)
        rc, sst, st = _summary(a, buf, off, n, out if n else None)
        assert rc == N.OK and (st.n_units, st.first_bad, st.bad_haystack, st.ascii) == (0, -1, 0, 1)
        assert (sst.n_records, sst.n_matched, sst.pieces, sst.rescans) == (0, 0, 0, 0)
        assert [tuple(r) for r in out[:n].tolist()] == [(0, -1, -1, -1, 0)] * n
        assert _summary(a, buf, off, n, out if n else None, stats=False)[0] == N.OK
    # ... through the wrappers
    for datas in ([], [b""], [b"", bytearray(), memoryview(b"")]):
        got = a.match_batch_utf8(datas, with_ids=True)
        assert got.shape == (0, 4) and got.dtype == np.int32
        assert a.match_batch_utf8(datas, with_ids=False).shape == (0, 3)
        s, st = a.summary_batch_utf8(datas)
        assert s.dtype == N.SUMMARY_DTYPE and [tuple(r) for r in s.tolist()] == [(0, -1, -1, -1, 0)] * len(datas) and st["n_records"] == 0
    assert a.match_batch_utf8(b"", with_ids=True, offsets=[0, 0, 0]).shape == (0, 4)
    s = AhoCorasickSet(["ab"], True)
    assert s.find_all_batch_utf8([b"", b""]).shape == (0, 3) and s.contains_batch_utf8([b"", b""]).tolist() == [False, False]
    assert s.count_matches_batch_utf8([]).tolist() == [] and s.first_batch_utf8([b""]) == [None]
    m = AhoCorasickMap(["ab"], ["v"], True)
    assert m.find_all_batch_utf8([b""]).shape == (0, 4) and m.first_batch_utf8(b"", offsets=[0, 0]) == [None]
    seen = []
    s.match_batch_utf8([b"", b""], lambda *x: seen.append(x) or True)
    m.match_batch_utf8([], lambda *x: seen.append(x) or True)
    assert seen == []
    with pytest.raises(TypeError):
        s.contains_batch_utf8([b"", None])


def test_line_offsets_against_splitlines():
    texts = ["", "\n", "one line", "one line\n", "a\nbé\n\n😀 c\nlast", "a\nbé\n\n😀 c\nlast\n", "\n\n\n", "\nx", "x" * 100 + "\n" + "é" * 40]
    for text in texts:
        data = text.encode("utf-8")
        lines = data.splitlines(keepends=True)
        assert b"".join(lines) == data and not any(c in data for c in b"\r\x0b\x0c\x1c\x1d\x1e\x85")
        for form in (data, bytearray(data), memoryview(data), np.frombuffer(data, np.uint8)):
            off = utf8_line_offsets(form)
            assert off.dtype == np.uint64 and off.ndim == 1
            o = off.tolist()
            assert [data[o[i]:o[i + 1]] for i in range(len(o) - 1)] == lines, (text, o)
            assert o[0] == 0 and o[-1] == len(data)
    assert utf8_line_offsets(b"").tolist() == [0]
