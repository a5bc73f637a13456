"""GPU tests of the batch spans entry (include/acgpu.h: acgpu_spans_batch_u16; csrc/acgpu_spans.hip: the merge over the
concatenation, k_span_tag behind every piece).  Every expected triple is tests/spans_ref.merge over the CPU oracle's records,
haystack by haystack (tests/cover_batch_ref.spans_batch_ref); as a second assertion only, a haystack's triples equal acgpu_spans_u16
on it alone.  Every call has a sentinel behind cap.  The cases are those of tests/test_gpu_cover_batch.py."""
import importlib

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import utf16
from ahocorasick_amd.unicode_tables import word_chars_from_list
from tests import test_gpu_cover as V
from tests import test_gpu_cover_batch as B
from tests import test_gpu_summary_batch as SB
from tests.cover_batch_ref import spans_batch_raw, spans_batch_ref

S = importlib.import_module("ahocorasick_amd.spans")  # (the package's name `spans` is the function)

pytestmark = pytest.mark.gpu

PIECE = B.PIECE


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in B.DEFAULTS:
        N.set_tunable(k, v)


def check(a, hays, recs, singles=32):
    """acgpu_spans_batch_u16 with exactly the capacity the result needs against the reference, then up to `singles` haystacks
    against acgpu_spans_u16 -> (the expected triples, the call's stats)"""
    want = spans_batch_ref(hays, recs)
    got, rc, n_out, st = spans_batch_raw(a, hays, len(want))
    assert rc == N.OK and n_out == len(want), (rc, n_out, len(want))
    assert got.shape == want.shape and (got == want).all(), np.flatnonzero((got != want).any(axis=1))[:5]
    assert (st.n_records, st.n_spans) == (sum(len(r) for r in recs), len(want)), (st.n_records, st.n_spans)
    for i in range(0, len(hays), max(1, len(hays) // singles)):
        assert S.spans(a, hays[i]).tolist() == want[want[:, 0] == i][:, 1:].tolist(), i
    return want, st


# ---- 1. seams -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", B.MODES)
def test_five_families_at_the_seams(mode):
    kws, hays, recs = B.seam_case(mode)
    assert B.seam_with_two_spans(hays, recs)
    a = B.automaton(mode, kws)
    want, st = check(a, hays, recs, singles=len(hays))
    assert (S.spans_batch(a, hays) == want).all()
    # the smallest batches: one haystack, one empty haystack
    check(a, hays[3:4], recs[3:4])
    want, st = check(a, hays[:1], recs[:1])
    assert len(want) == 0


def test_overlapping_and_nested_keywords_at_the_seams():
    kws, hays, recs = B.nested_case()
    assert B.seam_with_two_spans(hays, recs)
    a = B.automaton(N.MODE_ALL, kws)
    want, st = check(a, hays, recs, singles=len(hays))
    assert S.spans_batch(a, ["xab", "abx"]).tolist() == [[0, 1, 3], [1, 0, 2]] and S.spans(a, "xababx").tolist() == [[1, 5]]


# ---- 2. dense separators, more spans than one tile of the merge ---------------------------------------------------------------
def test_thousands_of_tiny_haystacks():
    rng = np.random.default_rng(21)
    a, orc = V.pair(N.MODE_ALL, ["a", "b"])
    table = utf16("abz")
    hays = [table[rng.integers(0, 3, int(ln))] for ln in rng.integers(0, 2, 8000)]
    recs = SB.oracle_records(orc, hays)
    want, st = check(a, hays, recs)
    assert len(want) > N.SPAN_TILE and st.pieces == 1


# ---- 4. pieces ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", B.MODES)
def test_pieces(mode):
    kws, hays, recs = B.piece_case(mode)
    a = B.automaton(mode, kws)
    B.pieces(PIECE)
    want, st = check(a, hays, recs)
    assert st.pieces >= 10, st.pieces


def test_one_span_carried_to_a_separator():
    kws, hays, recs = B.long_span_case()
    a = B.automaton(N.MODE_ALL, kws)
    B.pieces(PIECE)
    want, st = check(a, hays, recs, singles=8)
    assert st.pieces >= 10 and st.max_carry >= 1, (st.pieces, st.max_carry)
    i = next(i for i, h in enumerate(hays) if len(h) == 10000)
    assert want[want[:, 0] == i].tolist() == [[i, 0, 10000]] and sum(len(h) + 1 for h in hays) > 10 * PIECE


@pytest.mark.parametrize("mode", B.MODES)
def test_pieces_of_16_units(mode):
    kws, hays, recs = B.small_piece_case(mode)
    a = B.automaton(mode, kws)
    B.pieces(16)
    want, st = check(a, hays, recs, singles=4)
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
    want, st = check(a, hays, recs, singles=4)
    assert st.rescans > 0, (st.pieces, st.rescans)


# ---- 7. overflow --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [None, 16])
def test_overflow_is_exact_and_keeps_the_sentinel(p):
    kws, hays, recs = B.nested_case()
    a = B.automaton(N.MODE_ALL, kws)
    want = spans_batch_ref(hays, recs)
    total = len(want)
    assert total > 20
    if p:
        B.pieces(p)
    for cap in (0, total // 2, total - 1, total):
        got, rc, n_out, st = spans_batch_raw(a, hays, cap)
        assert rc == (N.OK if cap == total else N.E_OVERFLOW) and n_out == total and st.n_spans == total, (cap, rc, n_out)
        assert (got == want[:cap]).all(), cap


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
    want, st = check(a, hays, recs, singles=len(hays))
    assert st.pieces == sum(1 for h in hays if len(h))  # a text per haystack
    got, rc, n_out, st = spans_batch_raw(a, hays, 3)  # overflow through the calls per haystack
    assert rc == N.E_OVERFLOW and n_out == len(want) > 3 and (got == want[:3]).all()


def test_fallback_dictionary_without_a_free_unit():
    kws = [np.array([i], dtype=np.uint16) for i in range(65536)]
    a, orc = V.pair(N.MODE_ALL, kws)
    hays = [np.array(h, np.uint16) for h in ([5, 6], [7], [], [65535, 0, 1], [300] * 9, [], [0], [65535], [1, 2, 3, 4], [9] * 70, [], [8, 8])]
    recs = SB.oracle_records(orc, hays)
    want, st = check(a, hays, recs, singles=len(hays))
    assert want.tolist() == [[i, 0, len(h)] for i, h in enumerate(hays) if len(h)] and st.pieces == len(want)


# ---- 9. the pool behind a batch call ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", V.WORDY)
def test_a_plain_call_behind_a_batch_call_starts_its_text_as_a_text(mode):
    kws, hays, recs = B.seam_case(mode)
    a, orc = V.pair(mode, kws)
    text = utf16("ab cd, c ab" if mode == N.MODE_WWLONGEST else "abc dd, ab c")
    want = orc.match(text, cap=64)[:, :2]
    assert len(want) and want[0, 0] == 0
    check(a, hays, recs, singles=1)
    assert a.match_host(text, False).tolist() == want.tolist()
    assert spans_batch_raw(a, hays, 2)[1] == N.E_OVERFLOW
    assert a.match_host(text, False).tolist() == want.tolist()
