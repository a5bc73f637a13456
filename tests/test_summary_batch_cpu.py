"""CPU-side checks of the batch summary entry (include/acgpu.h: acgpu_summary_batch_u16): everything it decides before a device is
touched -- argument checks, the empty batch, the failure without a device -- the layout of its records and the Python methods."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import (AhoCorasickMap, AhoCorasickSet, Automaton, LongestMatchMap, ShortestMatchSet, WholeWordLongestMatchMap,
                                     WholeWordMatchSet, _pack)
from tests.helpers import WORD

vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
KWS = ["abc", "", "b", "abc"]  # an empty keyword and a duplicate
HAYS = ["zabcz", "", "b", "zz"]
CANARY = (0x1122334455667788, 0x5A5A5A5A, 0x6B6B6B6B, 0x7C7C7C7C, 0x0D0D0D0D)


def canary(n):
    out = np.zeros(n, dtype=N.SUMMARY_DTYPE)
    out[:] = CANARY
    return out


def untouched(out):
    return all(tuple(int(x) for x in row) == CANARY for row in out.tolist())


def _call(a, units, off, n_hay, out, stats=True):
    """-> (rc, stats)"""
    st = N.SummaryStats(7, 7, 7, 7)
    rc = N.lib().acgpu_summary_batch_u16(a.handle if a else None, vp(units), vp(off), n_hay, vp(out), ctypes.byref(st) if stats else None)
    return rc, st


def test_layout_of_a_summary():
    assert N.SUMMARY_DTYPE.itemsize == ctypes.sizeof(N.BatchSummary) == 24
    for name, offset, size in (("n_matches", 0, 8), ("start", 8, 4), ("end", 12, 4), ("keyword_id", 16, 4), ("reserved", 20, 4)):
        assert N.SUMMARY_DTYPE.fields[name][1] == getattr(N.BatchSummary, name).offset == offset, name
        assert N.SUMMARY_DTYPE.fields[name][0].itemsize == getattr(N.BatchSummary, name).size == size, name
    assert N.SUMMARY_DTYPE["n_matches"] == np.uint64 and N.SUMMARY_DTYPE["start"] == np.int32
    assert ctypes.sizeof(N.SummaryStats) == 24
    assert "acgpu_summary_batch_u16" in N.SYMBOLS


def test_argument_checks_leave_out_untouched():
    a = Automaton(N.MODE_ALL, KWS, True)
    units, off = _pack(HAYS)
    out = canary(len(HAYS) + 2)
    assert _call(None, units, off, len(HAYS), out)[0] == N.E_INVALID
    assert _call(None, units, np.zeros(1, np.uint64), 0, out)[0] == N.E_INVALID
    assert _call(a, units, None, len(HAYS), out)[0] == N.E_INVALID
    assert _call(a, units, None, 0, out)[0] == N.E_INVALID
    assert _call(a, units, off, len(HAYS), None)[0] == N.E_INVALID  # NULL out with haystacks to report on
    assert _call(a, None, off, len(HAYS), out)[0] == N.E_INVALID   # units to read, and no array
    assert _call(a, units, np.array([0, 5, 4, 6, 8], np.uint64), 4, out)[0] == N.E_INVALID  # descending offsets
    assert _call(a, units, np.array([3, 0], np.uint64), 1, out)[0] == N.E_INVALID
    # units + haystacks of 2^31 or more: the concatenation would not fit a call (nothing is read before the check)
    for total, n_hay in (((1 << 31) - 1, 1), ((1 << 31) - 2, 2), (1 << 31, 1), (1 << 40, 1)):
        big = np.zeros(n_hay + 1, np.uint64)
        big[-1] = total
        assert _call(a, units, big, n_hay, out)[0] == N.E_INVALID, (total, n_hay)
    assert untouched(out)


@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_LONGEST, N.MODE_WHOLEWORD, N.MODE_SHORTEST, N.MODE_WWLONGEST])
def test_an_empty_batch_needs_no_device(mode):
    a = Automaton(mode, ["ab", "b"], True, word_chars=WORD if mode in (N.MODE_WHOLEWORD, N.MODE_WWLONGEST) else None)
    out = canary(2)
    for o in (out, None):
        rc, st = _call(a, None, np.zeros(1, np.uint64), 0, o)
        assert rc == N.OK and (st.n_records, st.n_matched, st.pieces, st.rescans) == (0, 0, 0, 0)
    assert _call(a, None, np.full(1, 12, np.uint64), 0, out, stats=False)[0] == N.OK  # (no stats wanted, a first offset that is not 0)
    assert untouched(out)
    got, st = a.summary_batch([])
    assert got.dtype == N.SUMMARY_DTYPE and got.shape == (0,) and st == {"n_records": 0, "n_matched": 0, "pieces": 0, "rescans": 0}


def test_python_methods_on_an_empty_list():
    sets = [AhoCorasickSet(KWS, True), ShortestMatchSet(KWS, False), WholeWordMatchSet(["ab"], True)]
    maps = [AhoCorasickMap(KWS, [1, 2, 3, 4], True), LongestMatchMap(KWS, "wxyz", False), WholeWordLongestMatchMap(["a b"], [None], True)]
    for m in sets + maps:
        c = m.contains_batch([])
        assert c.dtype == np.bool_ and c.shape == (0,)
        n = m.count_matches_batch([])
        assert n.dtype == np.uint64 and n.shape == (0,)
        assert m.first_batch([]) == []
        assert m.contains_batch(iter(())).shape == (0,)
        with pytest.raises(TypeError):
            m.contains_batch(["ab", None])


def test_without_a_device_the_call_fails_as_the_batch_match_call_does():
    a = Automaton(N.MODE_ALL, KWS, True)
    units, off = _pack(HAYS)
    recs = np.zeros((16, 4), np.int32)
    n_recs = ctypes.c_uint64(0)
    rc_match = N.lib().acgpu_match_batch_u16(a.handle, vp(units), vp(off), len(HAYS), N.REC_MAP, vp(recs), 16, ctypes.byref(n_recs))
    out = canary(len(HAYS) + 1)
    rc, st = _call(a, units, off, len(HAYS), out)
    assert rc == rc_match
    if rc != N.OK:  # no device: nothing was written, and the wrappers raise the library's error
        assert rc in (N.E_NODEVICE, N.E_HIP) and untouched(out)
        with pytest.raises(N.AcgpuError):
            a.summary_batch(HAYS)
        for call in ("contains_batch", "count_matches_batch", "first_batch"):
            with pytest.raises(N.AcgpuError):
                getattr(AhoCorasickSet(KWS, True), call)(HAYS)
    else:  # listener order: "b" ends before "abc" does; the duplicate keyword reports its last index
        assert [tuple(r) for r in out[:4].tolist()] == [(2, 2, 3, 2, 0), (0, -1, -1, -1, 0), (1, 0, 1, 2, 0), (0, -1, -1, -1, 0)]
        assert untouched(out[4:]) and (st.n_records, st.n_matched) == (3, 2)
        assert recs[:n_recs.value].tolist() == [[0, 2, 3, 2], [0, 1, 4, 3], [2, 0, 1, 2]]
