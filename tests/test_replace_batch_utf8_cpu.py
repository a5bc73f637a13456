"""CPU-side checks of the UTF-8 batch replace entry (include/acgpu.h: acgpu_replace_batch_utf8): the symbol, and everything it
decides before a device is touched -- the argument checks of acgpu_match_batch_utf8 and acgpu_replace_utf8 together,
ACGPU_MODE_ALL, keywords with an unpaired surrogate, batches without a byte -- the wrapper's check of the replacement list and
the facade on empty batches."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, LongestMatchMap, LongestMatchSet, ShortestMatchSet, WholeWordMatchSet
from tests.helpers import WORD

vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
KWS = ["ab", "", "b", "ab"]  # an empty keyword and a duplicate
CANARY = 0xA5
OFF_CANARY = 0x7777777777777777
UST_CANARY = (7, 7, 7, 7)
SYMBOL = "acgpu_replace_batch_utf8"


def table(repls):
    """-> (bytes, offsets) in the layout the entry reads"""
    parts = [np.frombuffer(r.encode(), np.uint8) for r in repls]
    off = np.zeros(len(parts) + 1, np.uint64)
    off[1:] = np.cumsum([p.size for p in parts])
    return np.concatenate(parts + [np.zeros(1, np.uint8)]), off


def offs(*v):
    return np.array(v, dtype=np.uint64)


def call(a, data, off, n, r_bytes, r_off, n_repl, out, cap, out_off="canary", n_out=True, stats=True):
    """-> (rc, n_out, out_offsets, replace stats, utf8 batch stats)"""
    no = ctypes.c_uint64(99)
    st, ust = N.ReplaceStats(7, 7, 7, 7), N.Utf8BatchStats(*UST_CANARY)
    oo = np.full(n + 1, OFF_CANARY, np.uint64) if isinstance(out_off, str) else out_off
    rc = getattr(N.lib(), SYMBOL)(a.handle if a else None, vp(data), vp(off), n, vp(r_bytes), vp(r_off), n_repl, vp(out), cap, vp(oo),
                                  ctypes.byref(no) if n_out else None, ctypes.byref(st) if stats else None, ctypes.byref(ust) if stats else None)
    return rc, no.value, oo, st, ust


def untouched(oo, ust):
    return (oo is None or (oo == OFF_CANARY).all()) and (ust.n_units, ust.first_bad, ust.bad_haystack, ust.ascii) == UST_CANARY


def test_the_library_exports_the_entry():
    assert SYMBOL in N.SYMBOLS and hasattr(ctypes.CDLL(N.LIB_PATH), SYMBOL)
    assert N.lib().acgpu_abi_version() == N.ABI_VERSION == 5


def test_argument_checks_come_before_any_device_and_leave_out_and_the_offsets_untouched():
    a = Automaton(N.MODE_LONGEST, KWS, True)
    data = np.frombuffer(b"zabzab", np.uint8)
    off = offs(0, 4, 6)
    r_bytes, r_off = table(["x", "y", "z", "w"])
    out = np.full(16, CANARY, np.uint8)
    r6, off6 = table(["x"] * 6)
    calls = [call(None, data, off, 2, r_bytes, r_off, 4, out, 16),
             call(a, data, None, 2, r_bytes, r_off, 4, out, 16),                         # no offsets
             call(a, data, off, 2, r_bytes, r_off, 4, out, 16, n_out=False),
             call(a, data, off, 2, r_bytes, r_off, 4, out, 16, out_off=None),            # no out_offsets
             call(a, data, off, 2, r_bytes, r_off, 4, None, 16),                         # a capacity, and no array
             call(a, data, offs(0, 5, 4), 2, r_bytes, r_off, 4, out, 16),                # descending offsets
             call(a, data, offs(4, 2, 6), 2, r_bytes, r_off, 4, out, 16),
             call(a, None, off, 2, r_bytes, r_off, 4, out, 16),                          # a byte to read, and no buffer
             call(a, None, offs(0, 0, 1), 2, r_bytes, r_off, 4, out, 16)]
    # a bad table: a wrong count, descending offsets, no offsets, units to read and no array
    calls += [call(a, data, off, 2, r6, off6, n_repl, out, 16) for n_repl in (0, 2, 3, 5, 6)]
    calls += [call(a, data, off, 2, r_bytes, offs(0, 2, 1, 3, 4), 4, out, 16), call(a, data, off, 2, r_bytes, None, 4, out, 16),
              call(a, data, off, 2, None, r_off, 4, out, 16)]
    # the span, and the span plus one separator per haystack, stay below 2^31 (nothing is read before the check)
    calls += [call(a, data, offs(0, 1 << 31), 1, r_bytes, r_off, 4, out, 16), call(a, data, offs(5, 5 + (1 << 31) - 1), 1, r_bytes, r_off, 4, out, 16),
              call(a, data, offs(0, 3, (1 << 31) - 2), 2, r_bytes, r_off, 4, out, 16), call(a, data, offs(0, 1 << 40), 1, r_bytes, r_off, 4, out, 16)]
    for i, (rc, n, oo, st, ust) in enumerate(calls):
        assert rc == N.E_INVALID and untouched(oo, ust) and st.n_records == 7, (i, rc)
    assert (out == CANARY).all()


def test_mode_all_is_unsupported_before_any_device_call():
    a = Automaton(N.MODE_ALL, KWS, True)
    data = np.frombuffer(b"zabzab", np.uint8)
    off = offs(0, 4, 6)
    out = np.full(16, CANARY, np.uint8)
    for repls in (["x", "y", "z", "w"], ["#"]):
        r_bytes, r_off = table(repls)
        rc, _, oo, _, ust = call(a, data, off, 2, r_bytes, r_off, len(repls), out, 16)
        assert rc == N.E_UNSUPPORTED and untouched(oo, ust)
        assert call(a, None, offs(0, 0), 1, r_bytes, r_off, len(repls), None, 0)[0] == N.E_UNSUPPORTED  # (an empty batch too)
    r6, off6 = table(["x"] * 6)
    assert call(a, data, off, 2, r6, off6, 2, out, 16)[0] == N.E_INVALID  # (the table is checked first, as check_table does)
    assert (out == CANARY).all()
    with pytest.raises(N.AcgpuError) as e:
        a.replace_batch_utf8([b"zabz", b"ab"], "#")
    assert e.value.code == N.E_UNSUPPORTED


@pytest.mark.parametrize("cs", [True, False])
def test_keywords_with_an_unpaired_surrogate_are_refused(cs):
    datas = ["a😀b ab".encode(), b"", "😀".encode()]
    data = np.frombuffer(b"".join(datas), np.uint8)
    off = np.cumsum([0] + [len(d) for d in datas], dtype=np.uint64)
    r_bytes, r_off = table(["#"])
    out = np.full(32, CANARY, np.uint8)
    for kws in (["\ud83d", "ab"], ["ab", "\ude00"], ["x\ud83d", "ab"], ["\ude00\ud83d"], ["😀\ud83d"]):
        for mode in (N.MODE_SHORTEST, N.MODE_LONGEST):
            rc, _, oo, _, ust = call(Automaton(mode, kws, cs), data, off, 3, r_bytes, r_off, 1, out, 32)
            assert rc == N.E_UNSUPPORTED and untouched(oo, ust), kws
        r2, off2 = table(["#", "#", "#"])
        assert call(Automaton(N.MODE_LONGEST, kws, cs), data, off, 3, r2, off2, 3, out, 32)[0] == N.E_INVALID  # (the table first)
    assert (out == CANARY).all()
    # well-formed keywords are served: the return code is acgpu_match_batch_utf8's on the same input, OK or the no-device error
    for kws in (["😀", "ab"], ["a😀b"], ["😀😀"]):
        a = Automaton(N.MODE_SHORTEST, kws, cs)
        recs = np.zeros((16, 4), np.int32)
        n = ctypes.c_uint64(0)
        rc_match = N.lib().acgpu_match_batch_utf8(a.handle, vp(data), vp(off), 3, N.REC_MAP, vp(recs), 16, ctypes.byref(n), None)
        rc, _, oo, _, _ = call(a, data, off, 3, r_bytes, r_off, 1, out, 32)
        assert rc == rc_match and rc != N.E_UNSUPPORTED, kws
        if rc != N.OK:
            assert rc in (N.E_NODEVICE, N.E_HIP) and (out == CANARY).all() and (oo[1:] == OFF_CANARY).all()


@pytest.mark.parametrize("mode", [N.MODE_LONGEST, N.MODE_SHORTEST, N.MODE_WHOLEWORD, N.MODE_WWLONGEST])
def test_no_haystacks_and_empty_haystacks_need_no_device(mode):
    a = Automaton(mode, ["ab", "b"], True, word_chars=WORD if mode in (N.MODE_WHOLEWORD, N.MODE_WWLONGEST) else None)
    r_bytes, r_off = table(["x"])
    data = np.frombuffer(b"xy", np.uint8)
    for buf, off, n in ((None, offs(0), 0), (data, offs(1), 0), (None, offs(0, 0, 0, 0), 3), (data, offs(2, 2), 1), (data, offs(1, 1, 1), 2)):
        rc, m, oo, st, ust = call(a, buf, off, n, r_bytes, r_off, 1, None, 0)
        assert (rc, m) == (N.OK, 0) and oo.tolist() == [0] * (n + 1)
        assert (st.n_records, st.units_out, st.pieces, st.rescans) == (0, 0, 0, 0)
        assert (ust.n_units, ust.first_bad, ust.bad_haystack, ust.ascii) == (0, -1, 0, 1)
        rc, m, oo, _, _ = call(a, buf, off, n, r_bytes, r_off, 1, None, 0, stats=False)
        assert (rc, m) == (N.OK, 0) and oo.tolist() == [0] * (n + 1)
    # ... through the wrapper
    for datas in ([], [b""], [b"", bytearray(), memoryview(b"")]):
        got, out_off, st = a.replace_batch_utf8(datas, "x")
        assert got.shape == (0,) and got.dtype == np.uint8 and out_off.tolist() == [0] * (len(datas) + 1) and st["units_out"] == 0
    got, out_off, _ = a.replace_batch_utf8(b"", "x", offsets=[0, 0, 0])
    assert got.size == 0 and out_off.tolist() == [0, 0, 0]


def test_wrapper_checks_the_replacement_list():
    a = Automaton(N.MODE_LONGEST, KWS, True)
    for bad in (["x", "y"], ["x"] * 5, []):
        with pytest.raises(ValueError):
            a.replace_batch_utf8([b"zabz", b""], bad)
    with pytest.raises(ValueError):
        a.replace_batch_utf8(b"zabz", "x", offsets=[0, 9])  # offsets past the buffer
    with pytest.raises(ValueError):
        a.replace_batch_utf8(b"zabz", "x", offsets=[])


def test_the_facade_on_empty_batches():
    s = LongestMatchSet(["ab"], True)
    m = LongestMatchMap(["ab"], ["v"], True)
    for x, args in ((s, ("x",)), (s, (b"x",)), (m, ()), (m, (["y"],)), (m, (b"#",)), (ShortestMatchSet(["ab"], False), ("",)),
                    (WholeWordMatchSet(["ab"], True), ("é",))):
        assert x.replace_batch_utf8([], *args) == []
        assert x.replace_batch_utf8([b"", b""], *args) == [b"", b""]
        assert x.replace_batch_utf8([bytearray(), memoryview(b""), np.zeros(0, np.uint8)], *args) == [b"", b"", b""]
        assert x.replace_batch_utf8(b"", *args, offsets=[0, 0]) == [b""]
    with pytest.raises(TypeError):
        s.replace_batch_utf8([b"", None], "x")
