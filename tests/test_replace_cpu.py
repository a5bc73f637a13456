"""CPU-side checks of the replace entries (include/acgpu.h: acgpu_replace_u16 / acgpu_replace_device): everything they decide
before a device is touched -- argument checks, ACGPU_MODE_ALL, the failure without a device -- and the tunable of the slabs."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickMap, AhoCorasickSet, Automaton, LongestMatchSet, _pack, utf16

vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
KWS = ["ab", "", "b", "ab"]  # an empty keyword and a duplicate


def _shard(n, d_hay=0x1000, own=None, text_begin=1, text_end=1):
    sh = N.Shard()
    sh.d_hay = d_hay
    sh.n_units = n
    sh.own_begin, sh.own_end = (0, n) if own is None else own
    sh.text_begin, sh.text_end = text_begin, text_end
    return sh


def _host(a, hay, n, units, off, n_repl, out, cap, n_out=True):
    no = ctypes.c_uint64(0)
    st = N.ReplaceStats()
    return N.lib().acgpu_replace_u16(a.handle if a else None, vp(hay), n, vp(units), vp(off), n_repl, vp(out), cap,
                                     ctypes.byref(no) if n_out else None, ctypes.byref(st))


def _device(a, sh, units, off, n_repl, d_out, cap):
    no = ctypes.c_uint64(0)
    st = N.ReplaceStats()
    return N.lib().acgpu_replace_device(a.handle if a else None, ctypes.byref(sh) if sh is not None else None, vp(units), vp(off),
                                        n_repl, d_out, cap, ctypes.byref(no), None, ctypes.byref(st))


def test_argument_checks():
    a = Automaton(N.MODE_LONGEST, KWS, True)
    hay = utf16("zabz")
    units, off = _pack(["x", "y", "z", "w"])
    out = np.zeros(16, np.uint16)
    assert _host(None, hay, 4, units, off, 4, out, 16) == N.E_INVALID
    assert _host(a, None, 4, units, off, 4, out, 16) == N.E_INVALID
    assert _host(a, hay, 4, units, off, 4, None, 16) == N.E_INVALID
    assert _host(a, hay, 4, units, off, 4, out, 16, n_out=False) == N.E_INVALID
    assert _host(a, hay, 1 << 31, units, off, 4, out, 16) == N.E_INVALID
    units6, off6 = _pack(["x"] * 6)
    for n_repl in (0, 2, 3, 5):
        assert _host(a, hay, 4, units6, off6, n_repl, out, 16) == N.E_INVALID, n_repl
        assert _device(a, _shard(4), units6, off6, n_repl, 0x2000, 16) == N.E_INVALID, n_repl
    # offsets that descend, more than 2^31 replacement units
    assert _host(a, hay, 4, units, np.array([0, 2, 1, 3, 4], np.uint64), 4, out, 16) == N.E_INVALID
    assert _host(a, hay, 4, units, np.array([0, (1 << 31) + 1], np.uint64), 1, out, 16) == N.E_INVALID
    assert (out == 0).all()
    # the device entry: NULL shard, a misaligned d_out, a shard that is not the whole text
    assert _device(a, None, units, off, 4, 0x2000, 16) == N.E_INVALID
    assert _device(a, _shard(4), units, off, 4, 0x2002, 16) == N.E_INVALID
    assert _device(a, _shard(4), units, off, 4, None, 16) == N.E_INVALID
    assert _device(a, _shard(1 << 31), units, off, 4, 0x2000, 16) == N.E_INVALID
    for sh in (_shard(64, own=(8, 64)), _shard(64, own=(0, 56)), _shard(64, text_begin=0), _shard(64, text_end=0)):
        assert _device(a, sh, units, off, 4, 0x2000, 16) == N.E_UNSUPPORTED


def test_mode_all_is_unsupported_before_any_device_call():
    a = Automaton(N.MODE_ALL, KWS, True)
    hay = utf16("zabz")
    out = np.full(16, 0xBEEF, np.uint16)
    for repl in (["x", "y", "z", "w"], ["#"]):
        units, off = _pack(repl)
        assert _host(a, hay, 4, units, off, len(repl), out, 16) == N.E_UNSUPPORTED
        assert _device(a, _shard(4), units, off, len(repl), 0x2000, 16) == N.E_UNSUPPORTED
    assert (out == 0xBEEF).all()
    for m in (AhoCorasickSet(KWS, True), AhoCorasickMap(KWS, ["1", "2", "3", "4"], True)):
        with pytest.raises(N.AcgpuError) as e:
            m.replace("zabz", "#")
        assert e.value.code == N.E_UNSUPPORTED


def test_without_a_device_the_call_fails_as_the_match_call_does():
    a = Automaton(N.MODE_LONGEST, KWS, True)
    hay = utf16("zabz")
    recs = np.zeros((8, 3), np.int32)
    n_out = ctypes.c_uint64(0)
    rc_match = N.lib().acgpu_match_u16(a.handle, vp(hay), 4, N.REC_MAP, vp(recs), 8, ctypes.byref(n_out))
    units, off = _pack(["#"])
    out = np.full(16, 0xBEEF, np.uint16)
    rc = _host(a, hay, 4, units, off, 1, out, 16)
    assert rc == rc_match
    if rc != N.OK:  # no device: nothing was written, and the wrappers raise the library's error
        assert rc in (N.E_NODEVICE, N.E_HIP) and (out == 0xBEEF).all()
        with pytest.raises(N.AcgpuError):
            a.replace_host(hay, "#")
        with pytest.raises(N.AcgpuError):
            LongestMatchSet(KWS, True).replace("zabz", "#")
    else:
        assert out[:3].tolist() == [ord("z"), ord("#"), ord("z")] and (out[3:] == 0xBEEF).all()


def test_wrapper_checks_the_replacement_list():
    a = Automaton(N.MODE_LONGEST, KWS, True)
    with pytest.raises(ValueError):
        a.replace_host(utf16("zabz"), ["x", "y"])


def test_slab_tunable_exists_with_its_default():
    assert N.set_tunable("replace_slab_units", 1000) == 1 << 25
    assert N.set_tunable("replace_slab_units", 1 << 25) == 1000
