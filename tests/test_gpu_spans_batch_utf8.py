"""GPU tests of acgpu_spans_batch_utf8 / acgpu_spans_batch_utf8_lossy (include/acgpu.h; csrc/acgpu_spans.hip: the merge over virtual
coordinates, k_span_tag over voff; csrc/acgpu_utf8.hip: k_utf8_batch_vmap, k_utf8_batch_vpos, k_utf8_batch_voff).  The cases and the
reference are those of tests/test_gpu_cover_batch_utf8.py: for every haystack on its own the CPU oracle's records on the decoded
text, mapped to bytes, through tests/spans_ref.merge -- never the code under test.  As a second assertion only, the rows of a
haystack equal acgpu_spans_utf8 on it alone.  Every call has a sentinel behind cap and offsets[0] != 0."""
import ctypes
import importlib

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickSet, Utf8Error, utf16, utf8_line_offsets
from ahocorasick_amd.unicode_tables import word_chars_from_list
from tests import test_gpu_cover as V
from tests import test_gpu_cover_batch as CB
from tests import test_gpu_cover_batch_utf8 as B8
from tests.spans_ref import merge
from tests.test_gpu_utf8 import pair

S = importlib.import_module("ahocorasick_amd.spans")  # (the package's name `spans` is the function)

pytestmark = pytest.mark.gpu

MODES = B8.MODES
SENTINEL = 0x5A5A5A5A
vp = B8.vp
pieces = B8.pieces
records = B8.records


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in B8.DEFAULTS:
        N.set_tunable(k, v)


def spans_raw(a, datas, cap, errors="strict"):
    """acgpu_spans_batch_utf8[_lossy] into a buffer with a sentinel behind cap (in spans) -> (the triples written, rc, n_out, stats, utf8 stats)"""
    buf, off = B8.packed(datas)
    out = np.full((cap + 16, 3), SENTINEL, np.int32)
    name = "acgpu_spans_batch_utf8" + ("_lossy" if errors == "replace" else "")
    n_out, st, ust = ctypes.c_uint64(77), N.SpansStats(), N.UTF8_STATS[name]()
    rc = getattr(N.lib(), name)(a.handle, vp(buf), vp(off), len(datas), vp(out), cap, ctypes.byref(n_out), ctypes.byref(st), ctypes.byref(ust))
    assert (out[cap:] == SENTINEL).all(), "written at or beyond cap"
    return out[:min(cap, n_out.value)], rc, int(n_out.value), st, ust


def same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.int32, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (what, bad[:5], got[bad[:5]], want[bad[:5]])


def check(a, datas, recs, errors="strict", singles=8):
    """the entry with exactly the capacity the result needs against the reference, then up to `singles` haystacks against
    spans_utf8 -> (the expected triples, the call's stats)"""
    want = B8.spans_batch_ref8(datas, recs)
    got, rc, n_out, st, ust = spans_raw(a, datas, len(want), errors)
    assert rc == N.OK and n_out == len(want), (rc, n_out, len(want))
    same(got, want, "batch")
    assert (st.n_records, st.n_spans) == (sum(len(r) for r in recs), len(want)), (st.n_records, st.n_spans)
    for i in range(0, len(datas), max(1, len(datas) // singles)):
        same(S.spans_utf8(a, datas[i], errors=errors), want[want[:, 0] == i][:, 1:], "haystack %d alone" % i)
    return want, st


# ---- 1. the seam --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kws,texts", B8.SEAMS)
def test_a_span_never_reaches_across_two_haystacks(kws, texts):
    a, orc = pair(N.MODE_ALL, kws)
    datas = [t.encode() for t in texts]
    recs = records(orc, datas)
    want, st = check(a, datas, recs, singles=len(datas))
    if len(texts) == 2:
        n = len(kws[0].encode())
        assert want.tolist() == [[0, 1, 1 + n], [1, 0, n]]  # two spans ...
        assert S.spans_utf8(a, b"".join(datas)).tolist() == [[1, 1 + 2 * n]]  # ... where the joined text has one
    else:
        assert want.tolist() == [[i, 0, len(d)] for i, d in enumerate(datas)]  # every haystack wholly covered


@pytest.mark.parametrize("p", [None, 1, 16])
def test_a_lone_low_surrogate_against_four_byte_characters_at_the_seams(p):
    lo = utf16("😀")[1:]
    s = AhoCorasickSet([lo, "ab"], True)
    a, orc = pair(N.MODE_ALL, [lo, "ab"])
    datas = [t.encode() for t in ("a😀", "😀a", "😀", "😀", "", "😀😀", "ab😀", "😀ab", "x")]
    recs = records(orc, datas)
    pieces(p)
    want, st = check(s.automaton, datas, recs, singles=len(datas))
    assert want[:4].tolist() == [[0, 1, 5], [1, 0, 4], [2, 0, 4], [3, 0, 4]]


# ---- 2. empty haystacks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [None, 16])
def test_empty_haystacks(p):
    a, orc = pair(N.MODE_ALL, ["ab", "b", "é€"])
    some = [t.encode() for t in ("xab", "é€b", "..", "abé€", "b")]
    E = [b""]
    pieces(p)
    for datas in (E + some, some + E, some[:2] + E + some[2:], some[:1] + E * 2 + some[1:3] + E * 300 + some[3:] + E * 2, E * 2 + some + E * 300,
                  E * 5, E, some[:1], some[1:2]):
        check(a, datas, records(orc, datas), singles=4)


# ---- 3. sequences, every family -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [None, 16])
@pytest.mark.parametrize("mode", MODES)
def test_mixed_batch_every_family(mode, p):
    kws, datas, recs = B8.mixed_case(mode)
    a, orc = pair(mode, kws)
    pieces(p)
    want, st = check(a, datas, recs)
    if p:
        assert st.pieces >= 50


@pytest.mark.parametrize("p", [None, 16])
@pytest.mark.parametrize("mode", MODES)
def test_ascii_batch_every_family(mode, p):
    """the branch without checkpoints: a unit of the scan's text is its virtual coordinate"""
    kws, hays, recs = CB.seam_case(mode) if p is None else CB.small_piece_case(mode)
    a = CB.automaton(mode, kws)
    pieces(p)
    check(a, B8.as_bytes(hays), B8.set_recs(recs))


# ---- 4. pieces ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_LONGEST, N.MODE_SHORTEST])
@pytest.mark.parametrize("p", [16, 1000])
def test_piece_boundaries_on_a_separator_inside_a_pair_and_among_empty_haystacks(p, mode):
    datas, recs = B8.boundary_case(p)
    a, orc = pair(mode, B8.PIECE_KWS)
    if mode != N.MODE_ALL:
        recs = records(orc, datas)
    pieces(p)
    want, st = check(a, datas, recs)
    assert st.pieces >= 5, st.pieces


@pytest.mark.parametrize("reservoir", [8 * N.REC_SET, 512 * N.REC_SET])
def test_a_full_reservoir(reservoir):
    rng = np.random.default_rng(55)
    kws = ["ab", "b", "bcd", "dd", "a", "abcd", "é", "dé"]
    alpha = list("abcd") + ["é"]
    datas = ["".join(alpha[int(i)] for i in rng.integers(0, len(alpha), int(n))).encode() for n in rng.integers(0, 60, 250)]
    N.set_tunable("cursor_reservoir_bytes", reservoir)
    a, orc = pair(N.MODE_ALL, kws)  # (a pool made under the tunable: a reservoir never shrinks)
    recs = records(orc, datas)
    assert sum(len(r) for r in recs) > 6 * 512
    want, st = check(a, datas, recs, singles=4)
    assert st.rescans > 0, (st.pieces, st.rescans)


def test_one_span_carried_through_several_pieces():
    datas, recs = B8.long_span_case()
    a, orc = pair(N.MODE_ALL, ["aa"])
    pieces(1000)
    want, st = check(a, datas, recs)
    assert st.pieces >= 20 and st.max_carry >= 1 and [40, 0, 10000] in want.tolist(), (st.pieces, st.max_carry)


# ---- 5. capacity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [None, 16])
def test_capacity_keeps_the_count_exact_and_the_sentinel(p):
    kws, datas, recs = B8.mixed_case(N.MODE_ALL)
    a, orc = pair(N.MODE_ALL, kws)
    want = B8.spans_batch_ref8(datas, recs)
    total = len(want)
    pieces(p)
    for cap in (total, total - 1, total // 2, 0):
        got, rc, n_out, st, _ = spans_raw(a, datas, cap)
        assert rc == (N.OK if cap == total else N.E_OVERFLOW) and n_out == total == st.n_spans, (cap, rc, n_out)
        same(got, want[:cap], "cap %d" % cap)


# ---- 6. encoding --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(7))
def test_strict_refuses_what_match_batch_utf8_refuses_and_touches_nothing(i):
    datas = B8.ill_formed_batches()[i]
    a, orc = pair(N.MODE_ALL, ["ab", "b", "é"])
    rc, want = B8.match_batch_stats(a, datas)
    assert rc == N.E_ENCODING
    buf, off = B8.packed(datas)
    out = np.full((64, 3), SENTINEL, np.int32)
    n_out, st, ust = ctypes.c_uint64(77), N.SpansStats(), N.Utf8BatchStats()
    rc = N.lib().acgpu_spans_batch_utf8(a.handle, vp(buf), vp(off), len(datas), vp(out), 48, ctypes.byref(n_out), ctypes.byref(st), ctypes.byref(ust))
    assert rc == N.E_ENCODING and n_out.value == 0 and (out == SENTINEL).all()
    assert [int(getattr(ust, f)) for f, _ in ust._fields_] == want
    with pytest.raises(Utf8Error) as e:
        S.spans_batch_utf8(a, datas)
    assert (e.value.haystack, e.value.start) == (ust.bad_haystack, ust.first_bad)
    good = [t.encode() for t in ("xab", "é€ab")]
    check(a, good, records(orc, good))  # the pool is as usable as before


@pytest.mark.parametrize("p", [None, 3])
@pytest.mark.parametrize("i", range(7))
def test_lossy_decodes_every_haystack_on_its_own(i, p):
    datas = B8.ill_formed_batches()[i]
    a, orc = pair(N.MODE_ALL, ["ab", "b", "é", "\ufffd\ufffd", "b\ufffd", "x\ufffd"])
    recs = records(orc, datas, "replace")
    pieces(p)
    check(a, datas, recs, errors="replace", singles=len(datas))
    rc, want_st = B8.match_batch_stats(a, datas, lossy=True)
    got, rc2, n_out, st, ust = spans_raw(a, datas, 64, errors="replace")
    assert rc == rc2 == N.OK and [int(getattr(ust, f)) for f, _ in ust._fields_] == want_st


# ---- 7. where the library makes one call per haystack -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", V.WORDY)
def test_fallback_word_table_that_is_not_fold_consistent(mode):
    rng = np.random.default_rng(9)
    alpha = np.array([ord(ch) for ch in "abxyABXY ,"], dtype=np.uint16)
    wc = word_chars_from_list("abcdxyABCD")  # X, Y are not word characters although x, y are
    kws = [alpha[rng.integers(0, 4, int(rng.integers(1, 5)))] for _ in range(12)]
    kws += [kws[2].copy()]
    a, orc = V.pair(mode, kws, cs=False, wc=wc)
    assert a.info()["fold_consistent"] == 0
    texts = ["".join(chr(int(u)) for u in alpha[rng.integers(0, len(alpha), int(n))]) for n in (0, 1, 40, 300, 7, 0, 120, 3, 12, 60, 0, 25)]
    datas = [(t[:len(t) // 2] + "é€" + t[len(t) // 2:] if len(t) > 20 else t).encode() for t in texts]
    recs = B8.unit_records(orc, datas)
    assert sum(len(r) for r in recs) > 5
    want, st = check(a, datas, recs, singles=len(datas))
    assert st.pieces == sum(1 for d in datas if len(d))  # a text per haystack
    got, rc, n_out, st, _ = spans_raw(a, datas, 3)  # overflow through the calls per haystack
    assert rc == N.E_OVERFLOW and n_out == len(want)
    same(got, want[:3], "overflow")
    bad = datas[:5] + [b"ab\xe2\x82"] + datas[5:]  # an ill-formed batch on this route: refused as on the other
    rc, want_st = B8.match_batch_stats(a, bad)
    got, rc2, n_out, st, ust = spans_raw(a, bad, 64)
    assert rc == rc2 == N.E_ENCODING and n_out == 0 and [int(getattr(ust, f)) for f, _ in ust._fields_] == want_st and ust.bad_haystack == 5
    check(a, datas, recs, errors="replace", singles=2)


def test_fallback_dictionary_without_a_free_unit():
    kws = [np.array([i], dtype=np.uint16) for i in range(65536)]
    a, orc = V.pair(N.MODE_ALL, kws)
    texts = ["\x05\x06", "\x07", "", "\uffff\x00\x01", "\u012c" * 9, "", "\x00", "é€", "\x01\x02\x03\x04", "\t" * 70, "", "😀a"]
    datas = [t.encode() for t in texts]
    want, st = check(a, datas, B8.unit_records(orc, datas), singles=len(datas))
    assert want.tolist() == [[i, 0, len(d)] for i, d in enumerate(datas) if d] and st.pieces == len(want)
    got, rc, n_out, st, ust = spans_raw(a, datas[:3] + [b"\xc3"] + datas[3:], 64)
    assert rc == N.E_ENCODING and (ust.bad_haystack, ust.first_bad) == (3, 0) and n_out == 0


# ---- 8. the Python surface ----------------------------------------------------------------------------------------------------
def test_python_function():
    kws, datas, recs = B8.mixed_case(N.MODE_ALL)
    a, orc = pair(N.MODE_ALL, kws)
    want = B8.spans_batch_ref8(datas, recs)
    same(S.spans_batch_utf8(a, datas), want)
    same(S.spans_batch_utf8(a, [memoryview(d) for d in datas]), want)
    buf = np.frombuffer(b"".join(datas), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.uint64)
    st = N.SpansStats()
    same(S.spans_batch_utf8(a, buf, offsets=off, stats=st), want)
    assert st.n_spans == len(want)
    tail = want[want[:, 0] >= 3].copy()
    tail[:, 0] -= 3
    same(S.spans_batch_utf8(a, buf, offsets=off[3:]), tail)  # (offsets[0] != 0)
    log = "ab\nxé\n\néx😀ab".encode()
    s = AhoCorasickSet(["ab", "é"], True)
    assert S.spans_batch_utf8(s, log, offsets=utf8_line_offsets(log)).tolist() == [[0, 0, 2], [1, 1, 3], [3, 0, 2], [3, 7, 9]]
    bad = list(datas[:7]) + [b"a\xffb"] + list(datas[7:])
    with pytest.raises(Utf8Error) as e:
        S.spans_batch_utf8(a, bad)
    assert (e.value.haystack, e.value.start) == (7, 1)
    same(S.spans_batch_utf8(a, bad, errors="replace"), B8.spans_batch_ref8(bad, records(orc, bad, "replace")))
