"""GPU tests of the batch cover entry (include/acgpu.h: acgpu_cover_batch_u16; csrc/acgpu_cover.hip: k_cover_batch_head,
k_cover_batch_merge, the plan over spans and separators, k_cover_batch_offsets, k_cover_emit<.., true>).  Every expected value is
tests/cover_batch_ref.py -- tests/cover_ref.cover_ref over tests/spans_ref.merge of the CPU oracle's records, haystack by haystack --
never the code under test; as a second assertion only, a haystack's part of the result equals acgpu_cover_u16 on it alone.  Every
call has a sentinel behind cap.  The cases are shared with tests/test_gpu_spans_batch.py."""
import functools
import importlib

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import utf16
from ahocorasick_amd.unicode_tables import word_chars_from_list
from tests import test_gpu_cover as V
from tests import test_gpu_replace_batch as RB
from tests import test_gpu_summary_batch as SB
from tests.cover_batch_ref import cover_batch_raw, cover_batch_ref, layout
from tests.spans_ref import merge

C = importlib.import_module("ahocorasick_amd.cover")  # (the package's name `cover` is the function)

pytestmark = pytest.mark.gpu

DEFAULTS = V.DEFAULTS
MODES = sorted(V.MODES)
T = N.COVER_TILE_UNITS
PIECE = RB.PIECE


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def n_spans_of(hays, recs):
    return sum(len(merge(r, len(h))) for h, r in zip(hays, recs))


def check(a, hays, recs, open="", close="", body="keep", fill="*", singles=32):
    """acgpu_cover_batch_u16 with exactly the capacity the result needs against the reference, then up to `singles` haystacks
    against acgpu_cover_u16 -> (the expected units, offsets, the call's stats)"""
    want, off = cover_batch_ref(hays, recs, utf16(open), utf16(close), body, int(utf16(fill)[0]))
    got, oo, rc, n_out, st = cover_batch_raw(a, hays, len(want), open, close, body, fill)
    assert rc == N.OK and n_out == len(want), (rc, n_out, len(want))
    assert oo.tolist() == off.tolist(), np.flatnonzero(oo != off)[:5]
    V.same(got, want, "batch")
    assert (st.n_records, st.n_spans, st.units_out) == (sum(len(r) for r in recs), n_spans_of(hays, recs), len(want)), (st.n_records, st.n_spans)
    for i in range(0, len(hays), max(1, len(hays) // singles)):
        part = want[int(off[i]):int(off[i + 1])]
        alone, rc, n_out, _ = V.host_raw(a, hays[i], len(part), open, close, body, fill)
        assert rc == N.OK and n_out == len(part)
        V.same(alone, part, "haystack %d alone" % i)
    return want, off, st


# ---- the cases (shared with the spans tests) ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam_case(mode):
    """the haystacks of tests/test_gpu_replace_batch.py::test_four_families_at_the_seams and 30 random ones -> (kws, wc, hays, recs)"""
    kws, alpha = SB.family_case(mode)
    rng = np.random.default_rng(100 + mode)
    word = mode in V.WORDY
    hays = ["", "zz zz" if word else "zzzz", "ab", "ab zz c" if word else "abzzc", "xa", "by", "ab", "c", "ab", "cd", "",
            " ab", "  ab", ", c", " ", ",", "", "", "d, "]
    table = utf16(alpha)
    hays = [utf16(h) for h in hays] + [table[rng.integers(0, len(table), int(ln))] for ln in rng.integers(0, 41, 30)]
    a, orc = V.pair(mode, kws)
    return kws, hays, SB.oracle_records(orc, hays)


@functools.lru_cache(maxsize=None)
def nested_case():
    """AhoCorasick with overlapping and nested keywords"""
    kws = ["ab", "b", "bcd", "dd"]
    rng = np.random.default_rng(77)
    table = utf16("abcd.")
    hays = [utf16(h) for h in ("", "ab", "abcd", "bcdd", "dd", "", "d", "d", "xab", "bcd", "a", "b")]
    hays += [table[rng.integers(0, len(table), int(ln))] for ln in rng.integers(0, 41, 30)]
    a, orc = V.pair(N.MODE_ALL, kws)
    return kws, hays, SB.oracle_records(orc, hays)


def seam_with_two_spans(hays, recs):
    """from the reference: a haystack whose last span ends at its last unit, directly followed by one whose first span starts at 0"""
    sp = [merge(r, len(h)) for h, r in zip(hays, recs)]
    return any(len(sp[i]) and len(sp[i + 1]) and sp[i][-1, 1] == len(hays[i]) and sp[i + 1][0, 0] == 0 for i in range(len(hays) - 1))


@functools.lru_cache(maxsize=None)
def piece_case(mode):
    """the lengths of tests/test_gpu_replace_batch.py::piece_lengths, 60 000 units in all -> (kws, hays, recs)"""
    kws, alpha = SB.family_case(mode)
    rng = np.random.default_rng(300 + mode)
    lens, marks = RB.piece_lengths(rng)
    table = utf16(alpha)
    hays = [table[rng.integers(0, len(table), ln)] for ln in lens]
    first = marks["starts_at_piece_start"]
    starts = np.concatenate([[0], np.cumsum([ln + 1 for ln in lens])])
    assert starts[first] == 4 * PIECE and starts[marks["sep_at_piece_end"] + 1] - 1 == 3 * PIECE
    assert max(len(k) for k in kws) - 1 >= 3  # (the last-unit families: the separator at 5 * PIECE - 3 lies in the units a piece withholds)
    hays[first][:4] = utf16({N.MODE_WWLONGEST: "  ab", N.MODE_WHOLEWORD: "abc "}.get(mode, "abcz"))
    a, orc = V.pair(mode, kws)
    recs = SB.oracle_records(orc, hays)
    assert len(recs[first]) and recs[first][0, 0] == 0
    return kws, hays, recs


@functools.lru_cache(maxsize=None)
def long_span_case():
    """keyword aa: a haystack of 10 000 a is ONE span, carried through the pieces of 4096 units and ending at a separator; about
    43 000 units in all, more than 10 such pieces"""
    rng = np.random.default_rng(5)
    table = utf16("a.")
    hays = [table[rng.integers(0, 2, int(ln))] for ln in rng.integers(0, 30, 60)]
    hays += [utf16("a" * 10000), utf16(""), utf16("aa"), utf16("a"), utf16("a" * 9000 + ".aa"), utf16("a" * 10000), utf16(".." + "a" * 12000)]
    hays += [table[rng.integers(0, 2, int(ln))] for ln in rng.integers(0, 30, 60)]
    a, orc = V.pair(N.MODE_ALL, ["aa"])
    return ["aa"], hays, SB.oracle_records(orc, hays)


@functools.lru_cache(maxsize=None)
def small_piece_case(mode):
    """about 600 units in all, for pieces of 16 units"""
    kws, alpha = SB.family_case(mode)
    rng = np.random.default_rng(600 + mode)
    table = utf16(alpha)
    hays = [table[rng.integers(0, len(table), int(ln))] for ln in (0, 0, 15, 16, 17, 1, 0, 31, 40, 0, 14, 100, 3, 3, 0, 64, 47, 90, 0, 0, 120, 8, 5)]
    a, orc = V.pair(mode, kws)
    return kws, hays, SB.oracle_records(orc, hays)


def automaton(mode, kws):
    return V.pair(mode, kws)[0]


def pieces(p):
    N.set_tunable("cursor_first_piece", p)
    N.set_tunable("cursor_max_piece", p)


# ---- 1. seams -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_five_families_at_the_seams(mode):
    kws, hays, recs = seam_case(mode)
    assert seam_with_two_spans(hays, recs)
    a = automaton(mode, kws)
    for body, open, close in V.USES:
        check(a, hays, recs, open, close, body, singles=len(hays))
        check(a, hays, recs, "" if open else "<", "" if close else ">", body, singles=4)
    # mask_batch: every result has its haystack's length
    units, out_off, st = C.cover_batch_units(a, hays, body="fill")
    lens = np.cumsum([0] + [len(h) for h in hays])
    assert out_off.tolist() == lens.tolist() and st["units_out"] == lens[-1]
    assert [len(t) for t in C.mask_batch(a, hays)] == [len(h) for h in hays]
    # the smallest batches: one haystack, one empty haystack
    for body, open, close in V.USES:
        check(a, hays[3:4], recs[3:4], open, close, body)
        check(a, hays[:1], recs[:1], open, close, body)


def test_overlapping_and_nested_keywords_at_the_seams():
    kws, hays, recs = nested_case()
    assert seam_with_two_spans(hays, recs)
    a = automaton(N.MODE_ALL, kws)
    for body, open, close in V.USES:
        check(a, hays, recs, open, close, body, singles=len(hays))
        check(a, hays, recs, "" if open else "<", "" if close else ">", body, singles=4)


def test_python_functions():
    kws, hays, recs = nested_case()
    a = automaton(N.MODE_ALL, kws)
    texts = [h.tobytes().decode("utf-16-le") for h in hays]
    to_list = lambda units, off: [units[int(off[i]):int(off[i + 1])].tobytes().decode("utf-16-le") for i in range(len(off) - 1)]
    for fn, (open, close, body) in ((lambda: C.mask_batch(a, texts, fill="#"), ("", "", "fill")), (lambda: C.highlight_batch(a, texts, "<b>", "</b>"), ("<b>", "</b>", "keep")),
                                    (lambda: C.redact_batch(a, texts, "[r]"), ("[r]", "", "drop"))):
        assert fn() == to_list(*cover_batch_ref(hays, recs, utf16(open), utf16(close), body, ord("#")))
    assert C.redact_batch(a, ["xab", "abx"], "R") == ["xR", "Rx"] and C.redact(a, "xababx", "R") == "xRx"
    units, out_off, st = C.cover_batch_units(a, hays, open="<<<<", close=">>>>", cap=16)  # the wrapper's one retry
    want, off = cover_batch_ref(hays, recs, utf16("<<<<"), utf16(">>>>"), "keep")
    assert (units == want).all() and out_off.tolist() == off.tolist()


# ---- 2. equal positions and dense separators ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_cap", [None, 0])
@pytest.mark.parametrize("body,open", [("drop", ""), ("keep", "<")])
def test_more_items_in_an_emit_tile_than_lds_holds(body, open, lds_cap):
    rng = np.random.default_rng(21)
    a, orc = V.pair(N.MODE_ALL, ["a", "b"])
    table = utf16("abz")
    hays = [table[rng.integers(0, 3, int(ln))] for ln in rng.integers(0, 2, 8000)]
    recs = SB.oracle_records(orc, hays)
    kinds, stretch, item_at = layout(hays, recs, len(open), 0, body)
    first_tile = int(((item_at >= 0) & (item_at < T)).sum())
    assert first_tile > N.COVER_LDS_SEGMENTS, first_tile
    if body == "drop":  # equal positions: a span and the separator that touches it, runs of separators
        assert (np.diff(item_at) == 0).sum() > 4000 and len(kinds) < T
    if lds_cap is not None:
        assert N.set_tunable("cover_lds_segments", lds_cap) == N.COVER_LDS_SEGMENTS
    want, off, st = check(a, hays, recs, open, "", body)
    if body == "drop":
        assert 0 < want.size < T and (want == ord("z")).all()


# ---- 3. the plan past one workgroup -------------------------------------------------------------------------------------------
def test_plan_workgroups_of_mixed_spans_and_separators():
    rng = np.random.default_rng(22)
    a, orc = V.pair(N.MODE_ALL, ["a", "bb", "c"])
    table = utf16("abcz")
    hays = [table[rng.integers(0, 4, int(ln))] for ln in rng.integers(1, 4, 5000)]
    recs = SB.oracle_records(orc, hays)
    assert n_spans_of(hays, recs) + len(hays) > 2 * N.PLAN_TILE
    want, off, st = check(a, hays, recs, "<#>", "", "drop")
    assert st.pieces == 1
    check(a, hays, recs, "<#>", "", "keep")


# ---- 4. pieces ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body,open,close", [("drop", "***", ""), ("keep", "<b>", "</b>")])
@pytest.mark.parametrize("mode", MODES)
def test_pieces(mode, body, open, close):
    kws, hays, recs = piece_case(mode)
    a = automaton(mode, kws)
    pieces(PIECE)
    want, off, st = check(a, hays, recs, open, close, body)
    assert st.pieces >= 10, st.pieces


@pytest.mark.parametrize("body,open,close", V.USES)
def test_one_span_carried_to_a_separator(body, open, close):
    kws, hays, recs = long_span_case()
    a = automaton(N.MODE_ALL, kws)
    pieces(PIECE)
    want, off, st = check(a, hays, recs, open, close, body, singles=8)
    assert st.pieces >= 10 and st.max_carry >= 1, (st.pieces, st.max_carry)


@pytest.mark.parametrize("body,open,close", [("drop", "", ""), ("keep", "<", ">")])
@pytest.mark.parametrize("mode", MODES)
def test_pieces_of_16_units(mode, body, open, close):
    kws, hays, recs = small_piece_case(mode)
    assert 500 < sum(len(h) + 1 for h in hays) < 900
    a = automaton(mode, kws)
    pieces(16)
    want, off, st = check(a, hays, recs, open, close, body, singles=4)
    assert st.pieces >= 30, st.pieces


# ---- 5. a full reservoir ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reservoir", [8 * N.REC_SET, 512 * N.REC_SET])
def test_a_full_reservoir(reservoir):
    rng = np.random.default_rng(55)
    kws = ["ab", "b", "bcd", "dd", "a", "abcd"]
    table = utf16("abcd")
    hays = [table[rng.integers(0, 4, int(ln))] for ln in rng.integers(0, 60, 250)]
    N.set_tunable("cursor_reservoir_bytes", reservoir)
    a, orc = V.pair(N.MODE_ALL, kws)  # (a pool made under the tunable: a reservoir never shrinks)
    recs = SB.oracle_records(orc, hays)
    assert sum(len(r) for r in recs) > 6 * 512
    for body, open, close in V.USES:
        want, off, st = check(a, hays, recs, open, close, body, singles=4)
        assert st.rescans > 0, (st.pieces, st.rescans)


# ---- 6. slabs -----------------------------------------------------------------------------------------------------------------
def windows_begin_inside(hays, recs, n_open, n_close, body, slab):
    """From the reference's layout alone: what a multiple of `slab` lies STRICTLY inside of -- "open", "body", "close", "text" --
    and "seam" where a window begins with a haystack's first unit, directly behind the dropped separator."""
    kinds, stretch, item_at = layout(hays, recs, n_open, n_close, body)
    total, found = len(kinds), set()
    sep_at, o = set(), 0
    for h, r in zip(hays, recs):
        o += len(h) + sum(n_open + n_close - (e - s if body == "drop" else 0) for s, e in merge(r, len(h)).tolist())
        sep_at.add(o)
    assert o == total
    for w in range(slab, total, slab):
        if stretch[w] == stretch[w - 1]:
            found.add(kinds[w])
        if w in sep_at:
            found.add("seam")
    return found, total


@pytest.mark.parametrize("slab", [8, 1000])
def test_windows_of_the_slabs(slab):
    rng = np.random.default_rng(66)
    kws = ["ab", "b", "bcd", "dd"]
    table = utf16("abcd....")
    hays = [table[rng.integers(0, len(table), int(ln))] for ln in rng.integers(0, 16, 3000)]
    a, orc = V.pair(N.MODE_ALL, kws)
    recs = SB.oracle_records(orc, hays)
    found, total = windows_begin_inside(hays, recs, 5, 4, "keep", slab)
    assert found == {"open", "body", "close", "text", "seam"} and total > 4 * T, (found, total)
    N.set_tunable("replace_slab_units", slab)
    check(a, hays, recs, "<<b>>", "<e/>", "keep", singles=4)
    found, total = windows_begin_inside(hays, recs, 5, 0, "drop", slab)
    assert found == {"open", "text", "seam"} and total > 4 * T, (found, total)
    check(a, hays, recs, "[...]", "", "drop", singles=4)


# ---- 7. overflow --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [None, 16])
def test_overflow_keeps_every_offset_exact_and_the_sentinel(p):
    kws, hays, recs = nested_case()
    a = automaton(N.MODE_ALL, kws)
    want, off = cover_batch_ref(hays, recs, utf16("<b>"), utf16("</b>"), "keep")
    total = len(want)
    assert total > sum(len(h) for h in hays)  # KEEP outgrows the text
    if p:
        pieces(p)
    for cap in (0, total // 2, total - 1, total):
        got, oo, rc, n_out, st = cover_batch_raw(a, hays, cap, "<b>", "</b>", "keep")
        assert rc == (N.OK if cap == total else N.E_OVERFLOW) and n_out == total and st.units_out == total, (cap, rc, n_out)
        assert oo.tolist() == off.tolist(), cap
        V.same(got, want[:cap], "cap %d" % cap)


# ---- 8. where the library makes one call per haystack -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", V.WORDY)
def test_fallback_word_table_that_is_not_fold_consistent(mode):
    rng = np.random.default_rng(9)
    alpha = np.array([ord(ch) for ch in "abxyABXY ,"], dtype=np.uint16)
    wc = word_chars_from_list("abcdxyABCD")  # X, Y are not word characters although x, y are
    kws = [alpha[rng.integers(0, 4, int(rng.integers(1, 5)))] for _ in range(12)]
    kws += [kws[2].copy()]
    a, orc = V.pair(mode, kws, cs=False, wc=wc)
    assert a.info()["fold_consistent"] == 0
    hays = [alpha[rng.integers(0, len(alpha), int(ln))] for ln in (0, 1, 40, 300, 7, 0, 120, 3, 12, 60, 0, 25)]
    recs = SB.oracle_records(orc, hays)
    assert sum(len(r) for r in recs) > 5
    for body, open, close in V.USES:
        want, off, st = check(a, hays, recs, open, close, body, singles=len(hays))
        assert st.pieces == sum(1 for h in hays if len(h))  # a text per haystack
    want, off = cover_batch_ref(hays, recs, utf16("<"), utf16(">"), "keep")
    got, oo, rc, n_out, st = cover_batch_raw(a, hays, int(off[3]) + 1, "<", ">", "keep")  # overflow through the calls per haystack
    assert rc == N.E_OVERFLOW and n_out == len(want) and oo.tolist() == off.tolist()
    V.same(got, want[:int(off[3]) + 1], "overflow")


def test_fallback_dictionary_without_a_free_unit():
    kws = [np.array([i], dtype=np.uint16) for i in range(65536)]
    a, orc = V.pair(N.MODE_ALL, kws)
    hays = [np.array(h, np.uint16) for h in ([5, 6], [7], [], [65535, 0, 1], [300] * 9, [], [0], [65535], [1, 2, 3, 4], [9] * 70, [], [8, 8])]
    recs = SB.oracle_records(orc, hays)
    assert sum(len(r) for r in recs) == sum(len(h) for h in hays)
    for body, open, close in V.USES:
        want, off, st = check(a, hays, recs, open, close, body, singles=len(hays))
        assert st.pieces == sum(1 for h in hays if len(h)) and st.n_spans == sum(1 for h in hays if len(h))


# ---- 9. the pool behind a batch call ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", V.WORDY)
def test_a_plain_call_behind_a_batch_call_starts_its_text_as_a_text(mode):
    """d.start_behind is the separator for as long as the batch's text is scanned, and -1 again behind every return: a text
    whose first units are a keyword is matched there only if the scan does not take position 0 for the unit behind a separator"""
    kws, hays, recs = seam_case(mode)
    a, orc = V.pair(mode, kws)
    text = utf16("ab cd, c ab" if mode == N.MODE_WWLONGEST else "abc dd, ab c")
    want = orc.match(text, cap=64)[:, :2]
    assert len(want) and want[0, 0] == 0
    for cap in (None, 3):  # behind a call that succeeded, and behind one that overflowed
        if cap is None:
            check(a, hays, recs, "<", ">", "keep", singles=1)
        else:
            assert cover_batch_raw(a, hays, cap, "<", ">", "keep")[2] == N.E_OVERFLOW
        got = a.match_host(text, False)
        assert got.tolist() == want.tolist()
