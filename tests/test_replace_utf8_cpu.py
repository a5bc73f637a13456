"""CPU-side checks of the UTF-8 replace entry (include/acgpu.h: acgpu_replace_utf8): the symbol, and everything it decides before
a device is touched -- argument checks, ACGPU_MODE_ALL, keywords with an unpaired surrogate, the empty text -- and the wrapper's
check of the replacement list."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, LongestMatchMap, LongestMatchSet
from tests.helpers import WORD

vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
KWS = ["ab", "", "b", "ab"]  # an empty keyword and a duplicate
CANARY = 0xA5


def table(repls):
    """-> (bytes, offsets) in the layout the entry reads"""
    parts = [np.frombuffer(r.encode(), np.uint8) for r in repls]
    off = np.zeros(len(parts) + 1, np.uint64)
    off[1:] = np.cumsum([p.size for p in parts])
    return np.concatenate(parts + [np.zeros(1, np.uint8)]), off


def call(a, data, n_bytes, r_bytes, off, n_repl, out, cap, n_out=True, stats=True):
    """-> (rc, n_out, replace stats, utf8 stats)"""
    no = ctypes.c_uint64(99)
    st, ust = N.ReplaceStats(), N.Utf8Stats(7, 7, 7, 7)
    rc = N.lib().acgpu_replace_utf8(a.handle if a else None, vp(data), n_bytes, vp(r_bytes), vp(off), n_repl, vp(out), cap,
                                    ctypes.byref(no) if n_out else None, ctypes.byref(st) if stats else None,
                                    ctypes.byref(ust) if stats else None)
    return rc, no.value, st, ust


def test_the_library_exports_the_entry():
    assert "acgpu_replace_utf8" in N.SYMBOLS and hasattr(ctypes.CDLL(N.LIB_PATH), "acgpu_replace_utf8")
    assert N.lib().acgpu_abi_version() == 5


def test_argument_checks_come_before_any_device_and_leave_out_untouched():
    a = Automaton(N.MODE_LONGEST, KWS, True)
    data = np.frombuffer(b"zabz", np.uint8)
    r_bytes, off = table(["x", "y", "z", "w"])
    out = np.full(16, CANARY, np.uint8)
    assert call(None, data, 4, r_bytes, off, 4, out, 16)[0] == N.E_INVALID
    assert call(a, None, 4, r_bytes, off, 4, out, 16)[0] == N.E_INVALID              # bytes to read, and no buffer
    assert call(a, data, 4, r_bytes, off, 4, out, 16, n_out=False)[0] == N.E_INVALID
    assert call(a, data, 4, r_bytes, off, 4, None, 16)[0] == N.E_INVALID             # a capacity, and no array
    for n_bytes in (1 << 31, (1 << 31) + 5, 1 << 40):                                # (nothing is read before the check)
        assert call(a, data, n_bytes, r_bytes, off, 4, out, 16)[0] == N.E_INVALID, n_bytes
    r6, off6 = table(["x"] * 6)
    for n_repl in (0, 2, 3, 5, 6):
        assert call(a, data, 4, r6, off6, n_repl, out, 16)[0] == N.E_INVALID, n_repl
    assert call(a, data, 4, r_bytes, np.array([0, 2, 1, 3, 4], np.uint64), 4, out, 16)[0] == N.E_INVALID  # descending offsets
    assert call(a, data, 4, r_bytes, None, 4, out, 16)[0] == N.E_INVALID
    assert (out == CANARY).all()


def test_mode_all_is_unsupported_before_any_device_call():
    a = Automaton(N.MODE_ALL, KWS, True)
    data = np.frombuffer(b"zabz", np.uint8)
    out = np.full(16, CANARY, np.uint8)
    for repls in (["x", "y", "z", "w"], ["#"]):
        r_bytes, off = table(repls)
        assert call(a, data, 4, r_bytes, off, len(repls), out, 16)[0] == N.E_UNSUPPORTED
    r6, off6 = table(["x"] * 6)
    assert call(a, data, 4, r6, off6, 2, out, 16)[0] == N.E_INVALID  # (the table is checked first, as check_table does)
    assert (out == CANARY).all()
    with pytest.raises(N.AcgpuError) as e:
        a.replace_utf8(b"zabz", "#")
    assert e.value.code == N.E_UNSUPPORTED


@pytest.mark.parametrize("cs", [True, False])
def test_keywords_with_an_unpaired_surrogate_are_refused(cs):
    data = np.frombuffer("a😀b ab".encode(), np.uint8)
    r_bytes, off = table(["#"])
    out = np.full(32, CANARY, np.uint8)
    for kws in (["\ud83d", "ab"], ["ab", "\ude00"], ["x\ud83d", "ab"], ["\ude00\ud83d"], ["😀\ud83d"]):
        a = Automaton(N.MODE_SHORTEST, kws, cs)
        assert call(a, data, data.size, r_bytes, off, 1, out, 32)[0] == N.E_UNSUPPORTED, kws
        assert call(Automaton(N.MODE_LONGEST, kws, cs), data, data.size, r_bytes, off, 1, out, 32)[0] == N.E_UNSUPPORTED, kws
    assert (out == CANARY).all()
    # well-formed keywords are served: the return code is acgpu_match_utf8's on the same input, OK or the no-device error
    for kws in (["😀", "ab"], ["a😀b"], ["😀😀"]):
        a = Automaton(N.MODE_SHORTEST, kws, cs)
        recs = np.zeros((16, 3), np.int32)
        n = ctypes.c_uint64(0)
        rc_match = N.lib().acgpu_match_utf8(a.handle, vp(data), data.size, N.REC_MAP, vp(recs), 16, ctypes.byref(n), None)
        rc = call(a, data, data.size, r_bytes, off, 1, out, 32)[0]
        assert rc == rc_match and rc != N.E_UNSUPPORTED, kws
        if rc != N.OK:
            assert rc in (N.E_NODEVICE, N.E_HIP) and (out == CANARY).all()


@pytest.mark.parametrize("mode", [N.MODE_LONGEST, N.MODE_SHORTEST, N.MODE_WHOLEWORD, N.MODE_WWLONGEST])
def test_an_empty_text_needs_no_device(mode):
    a = Automaton(mode, ["ab", "b"], True, word_chars=WORD if mode in (N.MODE_WHOLEWORD, N.MODE_WWLONGEST) else None)
    r_bytes, off = table(["x"])
    for data in (None, np.frombuffer(b"x", np.uint8)):
        rc, n, st, ust = call(a, data, 0, r_bytes, off, 1, None, 0)
        assert (rc, n) == (N.OK, 0) and (st.n_records, st.units_out, st.pieces) == (0, 0, 0)
        assert (ust.n_units, ust.first_bad, ust.ascii, ust.reserved) == (0, -1, 1, 0)
    assert call(a, None, 0, r_bytes, off, 1, None, 0, stats=False)[:2] == (N.OK, 0)
    for data in (b"", bytearray(), memoryview(b""), np.zeros(0, np.uint8)):
        got, st = a.replace_utf8(data, "x")
        assert got.shape == (0,) and got.dtype == np.uint8 and st["units_out"] == 0
    assert LongestMatchSet(["ab"], True).replace_utf8(b"", "x") == b""
    assert LongestMatchMap(["ab"], ["v"], True).replace_utf8(b"") == b""


def test_wrapper_checks_the_replacement_list():
    a = Automaton(N.MODE_LONGEST, KWS, True)
    for bad in (["x", "y"], ["x"] * 5, []):
        with pytest.raises(ValueError):
            a.replace_utf8(b"zabz", bad)
    # a str is encoded as UTF-8, bytes-like entries are taken as they are
    r_bytes, off, n_repl = a._replacements_utf8(["é", b"\xff", bytearray(b"ab"), np.array([1, 2, 3], np.uint8)])
    assert n_repl == 4 and off.tolist() == [0, 2, 3, 5, 8] and r_bytes[:8].tobytes() == "é".encode() + b"\xffab\x01\x02\x03"
    assert a._replacements_utf8("€")[1].tolist() == [0, 3] and a._replacements_utf8(b"\x80")[2] == 1
