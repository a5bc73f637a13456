"""CPU-side checks of the UTF-8 entry (include/acgpu.h: acgpu_match_utf8): the symbol and its error code, everything it decides
before a device is touched, and the host restatement of the mapping rule (strings.utf8_unit_offsets)."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickSet, Automaton, Utf8Error, utf8_unit_offsets, utf16

vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
CANARY = (7, 7, 7, 7)


def _call(a, data, n_bytes, kind, out, cap, n_out=True, stats=True):
    """-> (rc, n_out, stats)"""
    st = N.Utf8Stats(*CANARY)
    n = ctypes.c_uint64(99)
    rc = N.lib().acgpu_match_utf8(a.handle if a else None, data, n_bytes, kind, vp(out), cap, ctypes.byref(n) if n_out else None,
                                  ctypes.byref(st) if stats else None)
    return rc, n.value, st


def test_the_library_exports_the_entry_and_binds_its_types():
    assert "acgpu_match_utf8" in N.SYMBOLS and hasattr(ctypes.CDLL(N.LIB_PATH), "acgpu_match_utf8")
    assert N.E_ENCODING == -8 and ctypes.sizeof(N.Utf8Stats) == 24
    assert [(f, getattr(N.Utf8Stats, f).offset) for f, _ in N.Utf8Stats._fields_] == [("n_units", 0), ("first_bad", 8), ("ascii", 16), ("reserved", 20)]
    assert issubclass(Utf8Error, ValueError) and Utf8Error(12).start == 12


def test_strerror_knows_the_new_code():
    msgs = {code: N.lib().acgpu_strerror(code).decode() for code in range(-9, 1)}
    assert "UTF-8" in msgs[N.E_ENCODING]
    assert msgs[N.E_ENCODING] not in [m for c, m in msgs.items() if c != N.E_ENCODING]  # a message of its own
    assert msgs[-9] == "unknown error"


def test_argument_checks_come_before_any_device():
    a = Automaton(N.MODE_ALL, ["ab", "b"], True)
    data = ctypes.create_string_buffer(b"zabz", 4)
    out = np.full((4, 3), 0x5A5A5A5A, np.int32)
    assert _call(None, data, 4, N.REC_SET, out, 4)[0] == N.E_INVALID
    assert _call(a, None, 4, N.REC_SET, out, 4)[0] == N.E_INVALID           # bytes to read, and no buffer
    assert _call(a, data, 4, N.REC_SET, out, 4, n_out=False)[0] == N.E_INVALID
    assert _call(a, data, 4, N.REC_SET, None, 4)[0] == N.E_INVALID          # a capacity, and no array
    for kind in (0, 4, 10, 16, -8):
        assert _call(a, data, 4, kind, out, 4)[0] == N.E_INVALID, kind
    for n_bytes in (1 << 31, (1 << 31) + 5, 1 << 40):                       # (nothing is read before the check)
        assert _call(a, data, n_bytes, N.REC_MAP, out, 4)[0] == N.E_INVALID, n_bytes
    assert (out == 0x5A5A5A5A).all()


@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_LONGEST, N.MODE_SHORTEST])
def test_an_empty_text_needs_no_device(mode):
    a = Automaton(mode, ["ab", "b"], True)
    for data in (None, ctypes.create_string_buffer(b"x", 1)):
        rc, n, st = _call(a, data, 0, N.REC_MAP, None, 0)
        assert (rc, n) == (N.OK, 0) and (st.n_units, st.first_bad, st.ascii, st.reserved) == (0, -1, 1, 0)
    assert _call(a, None, 0, N.REC_SET, None, 0, stats=False)[:2] == (N.OK, 0)
    for data in (b"", bytearray(), memoryview(b""), np.zeros(0, np.uint8)):
        got = a.match_utf8(data, with_ids=True)
        assert got.shape == (0, 3) and got.dtype == np.int32
    assert AhoCorasickSet(["ab"], True).find_all_utf8(b"").shape == (0, 2)


def test_unit_offsets_against_a_loop_over_the_characters():
    text = "aé€😀z߿ࠀ￿\U00010000\U0010ffff" * 3 + "Grüße, Ελλάδα, Москва, 東京, 𝒜𝓃𝓈 ﻿."
    data = text.encode("utf-8")
    want, pos = [], 0
    for ch in text:
        enc = ch.encode("utf-8")
        want += [pos] * (2 if len(enc) == 4 else 1)
        pos += len(enc)
    assert {len(ch.encode("utf-8")) for ch in text} == {1, 2, 3, 4} and pos == len(data)
    for form in (data, bytearray(data), memoryview(data), np.frombuffer(data, np.uint8)):
        got = utf8_unit_offsets(form)
        assert got.dtype == np.int64 and got.tolist() == want
    assert len(want) == utf16(text).size
    assert utf8_unit_offsets(b"").shape == (0,) and utf8_unit_offsets(b"abc").tolist() == [0, 1, 2]
