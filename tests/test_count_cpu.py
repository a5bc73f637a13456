"""CPU-side checks of the counting entries (include/acgpu.h: acgpu_count_u16 / acgpu_count_device): the argument checks that need
no device, and the failure of a valid call without one."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickSet, Automaton, utf16


def _vp(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def test_count_argument_checks_without_device():
    L = N.lib()
    a = Automaton(N.MODE_ALL, ["ab", "", "b", "ab"], True)  # four keywords given: an empty one and a duplicate keep their slots
    hay = utf16("zabz")
    counts = np.full(4, 77, np.uint64)
    st = N.CountStats()
    assert L.acgpu_count_u16(None, _vp(hay), 4, _vp(counts), 4, ctypes.byref(st)) == N.E_INVALID
    assert L.acgpu_count_u16(a.handle, None, 4, _vp(counts), 4, ctypes.byref(st)) == N.E_INVALID
    assert L.acgpu_count_u16(a.handle, _vp(hay), 4, None, 4, ctypes.byref(st)) == N.E_INVALID
    for wrong in (0, 2, 3, 5):  # (2: the distinct non-empty keywords -- not what n_counts means)
        assert L.acgpu_count_u16(a.handle, _vp(hay), 4, _vp(counts), wrong, None) == N.E_INVALID
    assert L.acgpu_count_u16(a.handle, _vp(hay), 1 << 31, _vp(counts), 4, None) == N.E_INVALID
    sh = N.Shard()
    sh.d_hay, sh.n_units, sh.own_begin, sh.own_end, sh.text_begin, sh.text_end = 4096, 4, 0, 4, 1, 1
    d_counts = ctypes.c_void_p(1 << 20)  # (never dereferenced: every call below is refused first)
    assert L.acgpu_count_device(None, ctypes.byref(sh), d_counts, 4, None, None) == N.E_INVALID
    assert L.acgpu_count_device(a.handle, None, d_counts, 4, None, None) == N.E_INVALID
    assert L.acgpu_count_device(a.handle, ctypes.byref(sh), None, 4, None, None) == N.E_INVALID
    assert L.acgpu_count_device(a.handle, ctypes.byref(sh), ctypes.c_void_p((1 << 20) + 4), 4, None, None) == N.E_INVALID  # 8-byte alignment
    assert L.acgpu_count_device(a.handle, ctypes.byref(sh), d_counts, 3, None, None) == N.E_INVALID
    sh.n_units = sh.own_end = 1 << 31
    assert L.acgpu_count_device(a.handle, ctypes.byref(sh), d_counts, 4, None, None) == N.E_INVALID
    assert (counts == 77).all()
    # the tunables exist, with their defaults
    for name in ("states_chunk_log2", "count_form"):
        assert N.set_tunable(name, 0) == 0


def test_count_fails_loudly_without_device_and_leaves_counts_alone():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    L = N.lib()
    a = Automaton(N.MODE_ALL, ["ab", "b"], True)
    hay = utf16("zabz")
    out = np.zeros((16, 3), np.int32)
    n = ctypes.c_uint64(0)
    rc_match = L.acgpu_match_u16(a.handle, _vp(hay), 4, N.REC_MAP, _vp(out), 16, ctypes.byref(n))
    counts = np.full(2, 77, np.uint64)
    rc = L.acgpu_count_u16(a.handle, _vp(hay), 4, _vp(counts), 2, None)
    assert rc == rc_match and rc in (N.E_NODEVICE, N.E_HIP)
    assert (counts == 77).all()
    with pytest.raises(N.AcgpuError) as e:
        a.count_host(hay)
    assert e.value.code == rc
    with pytest.raises(N.AcgpuError):
        AhoCorasickSet(["ab"], True).count("zabz")
