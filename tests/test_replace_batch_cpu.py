"""CPU-side checks of the batch replace entry (include/acgpu.h: acgpu_replace_batch_u16): everything it decides before a device
is touched -- argument checks, ACGPU_MODE_ALL, the empty batch, the failure without a device -- and the Python methods."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickSet, Automaton, LongestMatchMap, LongestMatchSet, _pack, utf16

vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
KWS = ["ab", "", "b", "ab"]  # an empty keyword and a duplicate
HAYS = ["zabz", "", "b"]


def _call(a, units, off, n_hay, r_units, r_off, n_repl, out, cap, out_off, n_out=True):
    """-> (rc, n_out, stats)"""
    no = ctypes.c_uint64(77)
    st = N.ReplaceStats()
    rc = N.lib().acgpu_replace_batch_u16(a.handle if a else None, vp(units), vp(off), n_hay, vp(r_units), vp(r_off), n_repl, vp(out), cap,
                                         vp(out_off), ctypes.byref(no) if n_out else None, ctypes.byref(st))
    return rc, no.value, st


def test_argument_checks():
    a = Automaton(N.MODE_LONGEST, KWS, True)
    units, off = _pack(HAYS)
    r_units, r_off = _pack(["x", "y", "z", "w"])
    out = np.zeros(16, np.uint16)
    oo = np.zeros(len(HAYS) + 1, np.uint64)
    args = (units, off, len(HAYS), r_units, r_off, 4, out, 16, oo)
    assert _call(None, *args)[0] == N.E_INVALID
    for at in (1, 6, 8):  # NULL offsets, out (with a capacity), out_offsets
        bad = list(args)
        bad[at] = None
        assert _call(a, *bad)[0] == N.E_INVALID, at
    assert _call(a, *args, n_out=False)[0] == N.E_INVALID
    assert _call(a, None, off, len(HAYS), r_units, r_off, 4, out, 16, oo)[0] == N.E_INVALID  # units to read, and no array
    # descending offsets
    assert _call(a, units, np.array([0, 4, 3, 5], np.uint64), 3, r_units, r_off, 4, out, 16, oo)[0] == N.E_INVALID
    # a replacement table of the wrong size, one whose offsets descend
    units6, off6 = _pack(["x"] * 6)
    for n_repl in (0, 2, 3, 5):
        assert _call(a, units, off, len(HAYS), units6, off6, n_repl, out, 16, oo)[0] == N.E_INVALID, n_repl
    assert _call(a, units, off, len(HAYS), r_units, np.array([0, 2, 1, 3, 4], np.uint64), 4, out, 16, oo)[0] == N.E_INVALID
    # units + haystacks of 2^31 or more: the concatenation would not fit a call (nothing is read before the check)
    for total, n_hay in (((1 << 31) - 1, 1), ((1 << 31) - 2, 2), (1 << 31, 1), (1 << 40, 1)):
        big = np.zeros(n_hay + 1, np.uint64)
        big[-1] = total
        assert _call(a, units, big, n_hay, r_units, r_off, 4, out, 16, np.zeros(n_hay + 1, np.uint64))[0] == N.E_INVALID, (total, n_hay)
    assert (out == 0).all()


def test_mode_all_is_unsupported_before_any_device_call():
    a = Automaton(N.MODE_ALL, KWS, True)
    units, off = _pack(HAYS)
    out = np.full(16, 0xBEEF, np.uint16)
    oo = np.zeros(len(HAYS) + 1, np.uint64)
    for repl in (["x", "y", "z", "w"], ["#"]):
        r_units, r_off = _pack(repl)
        assert _call(a, units, off, len(HAYS), r_units, r_off, len(repl), out, 16, oo)[0] == N.E_UNSUPPORTED
        assert _call(a, units, off, 0, r_units, r_off, len(repl), out, 16, oo)[0] == N.E_UNSUPPORTED
    assert (out == 0xBEEF).all()
    with pytest.raises(N.AcgpuError) as e:
        AhoCorasickSet(KWS, True).replace_batch(HAYS, "#")
    assert e.value.code == N.E_UNSUPPORTED


def test_an_empty_batch_needs_no_device():
    a = Automaton(N.MODE_LONGEST, KWS, True)
    r_units, r_off = _pack(["#"])
    oo = np.full(1, 99, np.uint64)
    rc, n_out, st = _call(a, None, np.zeros(1, np.uint64), 0, r_units, r_off, 1, None, 0, oo)
    assert rc == N.OK and n_out == 0 and oo[0] == 0 and st.n_records == 0 and st.units_out == 0
    units, off, st = a.replace_batch([], "#")
    assert units.size == 0 and off.tolist() == [0] and st["units_out"] == 0
    assert LongestMatchSet(KWS, True).replace_batch([], "#") == []
    assert LongestMatchMap(KWS, ["1", "2", "3", "4"], True).replace_batch([]) == []


def test_without_a_device_the_call_fails_as_the_replace_call_does():
    a = Automaton(N.MODE_LONGEST, KWS, True)
    hay = utf16("zabz")
    r_units, r_off = _pack(["#"])
    one = np.full(16, 0xBEEF, np.uint16)
    n_one = ctypes.c_uint64(0)
    rc_one = N.lib().acgpu_replace_u16(a.handle, vp(hay), 4, vp(r_units), vp(r_off), 1, vp(one), 16, ctypes.byref(n_one), None)
    units, off = _pack(HAYS)
    out = np.full(16, 0xBEEF, np.uint16)
    oo = np.zeros(len(HAYS) + 1, np.uint64)
    rc, n_out, st = _call(a, units, off, len(HAYS), r_units, r_off, 1, out, 16, oo)
    assert rc == rc_one
    if rc != N.OK:  # no device: nothing was written, and the wrappers raise the library's error
        assert rc in (N.E_NODEVICE, N.E_HIP) and (out == 0xBEEF).all()
        with pytest.raises(N.AcgpuError):
            a.replace_batch(HAYS, "#")
        with pytest.raises(N.AcgpuError):
            LongestMatchSet(KWS, True).replace_batch(HAYS, "#")
    else:
        assert out[:n_out].tolist() == utf16("z#z#").tolist() and (out[n_out:] == 0xBEEF).all()
        assert oo.tolist() == [0, 3, 3, 4] and st.n_records == 2 and st.units_out == 4


def test_wrappers_check_their_lists():
    a = Automaton(N.MODE_LONGEST, KWS, True)
    with pytest.raises(ValueError):
        a.replace_batch(HAYS, ["x", "y"])
    with pytest.raises(TypeError):
        LongestMatchSet(KWS, True).replace_batch(["zabz", None], "#")
    with pytest.raises(TypeError):
        LongestMatchMap(KWS, [1, 2, 3, 4], True).replace_batch(HAYS)
