"""CPU-side checks of the lossy UTF-8 entries (include/acgpu.h: acgpu_match_utf8_lossy, acgpu_match_batch_utf8_lossy,
acgpu_summary_batch_utf8_lossy): the symbols and their stats struct, everything they decide before a device is touched, the
facade's errors= keyword, and the reference decoder the GPU tests take their expected values from (tests/utf8_lossy_ref.py)
against CPython's own errors="replace"."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickMap, AhoCorasickSet, Automaton, utf16
from tests.utf8_lossy_ref import ALPHABET, TABLE, damaged, decode_replace, spans

vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
CANARY = (7, 7, 7, 7, 7)
PRESET = (0, 0, -1, 0, 1)
FILL = 0x5A5A5A5A


def fields(st):
    return tuple(getattr(st, f) for f, _ in N.Utf8LossyStats._fields_)


def _text(a, data, n, kind, out, cap, n_out=True):
    st = N.Utf8LossyStats(*CANARY)
    m = ctypes.c_uint64(99)
    rc = N.lib().acgpu_match_utf8_lossy(a.handle if a else None, data, n, kind, vp(out), cap, ctypes.byref(m) if n_out else None, ctypes.byref(st))
    return rc, m.value, st


def _batch(a, data, off, n, kind, out, cap, n_out=True):
    st = N.Utf8LossyStats(*CANARY)
    m = ctypes.c_uint64(99)
    rc = N.lib().acgpu_match_batch_utf8_lossy(a.handle if a else None, data, vp(off), n, kind, vp(out), cap, ctypes.byref(m) if n_out else None,
                                              ctypes.byref(st))
    return rc, m.value, st


def _summary(a, data, off, n, out):
    st = N.Utf8LossyStats(*CANARY)
    sst = N.SummaryStats(7, 7, 7, 7)
    rc = N.lib().acgpu_summary_batch_utf8_lossy(a.handle if a else None, data, vp(off), n, vp(out), ctypes.byref(sst), ctypes.byref(st))
    return rc, sst, st


def offs(*v):
    return np.array(v, dtype=np.uint64)


def test_the_library_exports_the_entries_and_binds_their_types():
    L = ctypes.CDLL(N.LIB_PATH)
    for name in ("acgpu_match_utf8_lossy", "acgpu_match_batch_utf8_lossy", "acgpu_summary_batch_utf8_lossy"):
        assert name in N.SYMBOLS and hasattr(L, name)
        assert getattr(N.lib(), name).argtypes[-1] == ctypes.POINTER(N.Utf8LossyStats)
    assert ctypes.sizeof(N.Utf8LossyStats) == 32
    assert [(f, getattr(N.Utf8LossyStats, f).offset) for f, _ in N.Utf8LossyStats._fields_] == [
        ("n_units", 0), ("n_replaced", 8), ("first_replaced", 16), ("first_haystack", 24), ("ascii", 28)]
    assert N.lib().acgpu_abi_version() == N.ABI_VERSION == 5


def test_text_argument_checks_come_before_any_device():
    a = Automaton(N.MODE_ALL, ["ab", "b"], True)
    data = ctypes.create_string_buffer(b"zab\x80ab", 7)
    out = np.full((4, 3), FILL, np.int32)
    calls = [_text(None, data, 7, N.REC_SET, out, 4), _text(a, None, 7, N.REC_SET, out, 4), _text(a, data, 7, N.REC_SET, out, 4, n_out=False),
             _text(a, data, 7, N.REC_SET, None, 4), _text(a, data, 1 << 31, N.REC_MAP, out, 4), _text(a, data, 1 << 40, N.REC_MAP, out, 4)]
    calls += [_text(a, data, 7, kind, out, 4) for kind in (0, 4, 10, 16, -8)]
    for i, (rc, n, st) in enumerate(calls):
        assert rc == N.E_INVALID and fields(st) == CANARY, (i, rc)
    assert (out == FILL).all()


def test_batch_argument_checks_come_before_any_device():
    a = Automaton(N.MODE_LONGEST, ["ab", "b"], True)
    data = ctypes.create_string_buffer(b"zab\x80ab", 7)
    off = offs(0, 4, 7)
    out = np.full((4, 4), FILL, np.int32)
    calls = [_batch(None, data, off, 2, N.REC_SET, out, 4), _batch(a, None, off, 2, N.REC_SET, out, 4), _batch(a, data, None, 2, N.REC_SET, out, 4),
             _batch(a, data, off, 2, N.REC_SET, out, 4, n_out=False), _batch(a, data, off, 2, N.REC_SET, None, 4),
             _batch(a, data, offs(0, 5, 4), 2, N.REC_MAP, out, 4), _batch(a, data, offs(4, 2, 6), 2, N.REC_MAP, out, 4),
             _batch(a, data, offs(0, 1 << 31), 1, N.REC_MAP, out, 4), _batch(a, data, offs(0, 3, (1 << 31) - 2), 2, N.REC_MAP, out, 4)]
    calls += [_batch(a, data, off, 2, kind, out, 4) for kind in (0, 4, 10, 16, -8)]
    for i, (rc, n, st) in enumerate(calls):
        assert rc == N.E_INVALID and fields(st) == CANARY, (i, rc)
    assert (out == FILL).all()
    sums = np.zeros(2, dtype=N.SUMMARY_DTYPE)
    sums[:] = (77, 7, 7, 7, 7)
    calls = [_summary(None, data, off, 2, sums), _summary(a, None, off, 2, sums), _summary(a, data, None, 2, sums), _summary(a, data, off, 2, None),
             _summary(a, data, offs(0, 5, 4), 2, sums), _summary(a, data, offs(0, 1 << 31), 1, sums)]
    for i, (rc, sst, st) in enumerate(calls):
        assert rc == N.E_INVALID and fields(st) == CANARY and sst.n_records == 7, (i, rc)
    assert all(tuple(r) == (77, 7, 7, 7, 7) for r in sums.tolist())


@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_LONGEST, N.MODE_SHORTEST])
def test_an_empty_text_and_empty_haystacks_need_no_device(mode):
    a = Automaton(mode, ["ab", "b"], True)
    data = ctypes.create_string_buffer(b"\x80y", 2)
    for buf in (None, data):
        rc, m, st = _text(a, buf, 0, N.REC_MAP, None, 0)
        assert (rc, m) == (N.OK, 0) and fields(st) == PRESET
    for buf, off, n in ((None, offs(0), 0), (data, offs(1), 0), (None, offs(0, 0, 0, 0), 3), (data, offs(2, 2), 1), (data, offs(1, 1, 1), 2)):
        rc, m, st = _batch(a, buf, off, n, N.REC_MAP, None, 0)
        assert (rc, m) == (N.OK, 0) and fields(st) == PRESET
        sums = np.zeros(max(n, 1), dtype=N.SUMMARY_DTYPE)
        sums[:] = (77, 7, 7, 7, 7)
        rc, sst, st = _summary(a, buf, off, n, sums)
        assert rc == N.OK and fields(st) == PRESET and (sst.n_records, sst.n_matched, sst.pieces, sst.rescans) == (0, 0, 0, 0)
        assert all(tuple(r) == (0, -1, -1, -1, 0) for r in sums[:n].tolist())
    assert a.match_utf8(b"", with_ids=True, errors="replace").shape == (0, 3)
    assert a.match_batch_utf8([b"", b""], with_ids=False, errors="replace").shape == (0, 3)
    assert a.summary_batch_utf8([b"", b""], errors="replace")[0].tolist() == [(0, -1, -1, -1, 0)] * 2


def test_errors_is_strict_or_replace_and_is_checked_before_a_native_call():
    a = Automaton(N.MODE_ALL, ["ab"], True)
    s, m = AhoCorasickSet(["ab"], True), AhoCorasickMap(["ab"], ["v"], True)
    calls = [lambda e: a.match_utf8(None, with_ids=True, errors=e), lambda e: a.match_batch_utf8(None, with_ids=True, errors=e),
             lambda e: a.summary_batch_utf8(None, errors=e)]
    for f in (s, m):
        calls += [lambda e, f=f: f.find_all_utf8(b"ab", errors=e), lambda e, f=f: f.match_utf8(b"ab", lambda *r: True, errors=e),
                  lambda e, f=f: f.find_all_batch_utf8([b"ab"], errors=e), lambda e, f=f: f.match_batch_utf8([b"ab"], lambda *r: True, errors=e),
                  lambda e, f=f: f.contains_batch_utf8([b"ab"], errors=e), lambda e, f=f: f.count_matches_batch_utf8([b"ab"], errors=e),
                  lambda e, f=f: f.first_batch_utf8([b"ab"], errors=e)]
    for call in calls:
        for e in ("ignore", "Replace", None, "surrogateescape"):
            with pytest.raises(ValueError, match="errors"):
                call(e)


def test_the_reference_decoder_on_the_table():
    for row, want in TABLE:
        text, off, length, replaced = decode_replace(row)
        assert text == row.decode("utf-8", "replace"), row
        assert spans(row) == want, row
        assert len(off) == len(length) == len(replaced) == len(utf16(text))
    assert decode_replace(b"")[0] == "" and spans(b"abc") == []
    # both units of a surrogate pair stand for the four bytes of their code point
    text, off, length, replaced = decode_replace("a😀".encode() + b"\xe2\x82")
    assert (off.tolist(), length.tolist(), replaced.tolist()) == ([0, 1, 1, 5], [1, 4, 4, 2], [False, False, False, True])
    # a haystack of a batch is decoded alone
    assert spans(b"a\xc3") == [(1, 2)] and spans(b"\xa9b") == [(0, 1)]


def test_the_reference_decoder_is_cpythons_replace_on_random_strings():
    rng = np.random.default_rng(4242)
    valid = "aé€😀 q中Ж".encode() * 8
    bufs = damaged(rng, valid, n_buffers=3000, max_len=60)
    bufs += [bytes(ALPHABET[int(i)] for i in rng.integers(0, len(ALPHABET), int(n))) for n in rng.integers(0, 40, 3000)]
    lens = set()
    for b in bufs:
        text, off, length, replaced = decode_replace(b)
        assert text == b.decode("utf-8", "replace"), b
        n = len(utf16(text))
        assert len(off) == len(length) == len(replaced) == n
        if n:
            # the units tile the buffer in order: every byte belongs to exactly one code point or subpart
            first = np.flatnonzero(np.r_[True, off[1:] != off[:-1]])
            assert off[0] == 0 and (off[first][1:] == (off + length)[first][:-1]).all() and off[-1] + length[-1] == len(b)
            assert ((length == 4) == np.isin(np.arange(n), np.flatnonzero((utf16(text) & 0xF800) == 0xD800))).all()
            assert (utf16(text)[replaced] == 0xFFFD).all() and (length[replaced] <= 3).all()
            lens |= set(length[replaced].tolist())
        else:
            assert b == b""
    assert len(bufs) >= 5000 and lens == {1, 2, 3}
