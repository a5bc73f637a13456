"""GPU tests of the spans entries (include/acgpu.h: acgpu_spans_u16 / acgpu_spans_device; csrc/acgpu_spans.hip: the suffix minimum,
the prefix count and the scatter behind every piece, and the carry between pieces).  Every expected value is
tests/spans_ref.py's merge -- a coverage bitmap -- of the CPU oracle's records; host and device entry in every case, the device
entry with a canary behind cap."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.spans import spans, spans_device
from ahocorasick_amd.strings import Automaton, utf16
from oracle.oracle import FAM_AC, FAM_LONGEST, FAM_SHORTEST, FAM_WHOLEWORD, FAM_WWLONGEST, Oracle
from tests.helpers import LOWER, WORD, fixture_inputs
from tests.spans_ref import merge
from tests.test_gpu_tiny_pieces import PIECES, family_case

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20)]
MODES = {N.MODE_ALL: FAM_AC, N.MODE_LONGEST: FAM_LONGEST, N.MODE_WHOLEWORD: FAM_WHOLEWORD, N.MODE_SHORTEST: FAM_SHORTEST,
         N.MODE_WWLONGEST: FAM_WWLONGEST}
WORDY = (N.MODE_WHOLEWORD, N.MODE_WWLONGEST)
T = N.SPAN_TILE  # kSpanTile of csrc/acgpu_spans.hip: the intervals one workgroup of the merge's scans takes (256 threads by 8)
CANARY = 0x5A5A5A5A
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def pieces(p):
    N.set_tunable("cursor_first_piece", p)
    N.set_tunable("cursor_max_piece", p)


def pair(mode, kws, cs=True, wc=None):
    if wc is None and mode in WORDY:
        wc = WORD
    return Automaton(mode, kws, cs, word_chars=wc), Oracle(MODES[mode], kws, case_sensitive=cs, lower=None if cs else LOWER, word_chars=wc)


def host_raw(a, hay, cap):
    """acgpu_spans_u16 into a buffer with a canary behind cap -> (the spans written, rc, n_out, stats)"""
    hay = utf16(hay)
    out = np.full((cap + 8, 2), CANARY, np.int32)
    n_out, st = ctypes.c_uint64(0), N.SpansStats()
    rc = N.lib().acgpu_spans_u16(a.handle, vp(hay if hay.size else np.zeros(1, np.uint16)), int(hay.size), vp(out), cap, ctypes.byref(n_out),
                                 ctypes.byref(st))
    assert (out[cap:] == CANARY).all(), "host: written at or beyond cap"
    return out[:min(cap, n_out.value)], rc, int(n_out.value), st


def device_raw(a, hay, cap):
    """acgpu_spans_device on the current torch stream, into a buffer with a canary behind cap -> (spans, rc, n_out, stats dict)"""
    import torch
    hay = utf16(hay)
    d_hay = torch.from_numpy(np.ascontiguousarray(hay if hay.size else np.zeros(8, np.uint16)).view(np.int16)).cuda()
    d_out = torch.full((2 * cap + 64,), CANARY, dtype=torch.int32, device="cuda")
    n_out, rc, st = spans_device(a, d_hay.data_ptr(), int(hay.size), d_out.data_ptr(), cap, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[2 * cap:] == CANARY).all(), "device: written at or beyond cap"
    return got[:2 * min(cap, n_out)].reshape(-1, 2), rc, n_out, st


def same(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (what, bad[:5], got[bad[:5]], want[bad[:5]])


def check_both(a, orc, hay, recs=None):
    """host and device entry against the merge of the oracle's records -> (the spans, the host entry's stats)"""
    hay = utf16(hay)
    if recs is None:
        recs = orc.match(hay, cap=max(1024, hay.size * 8))
    want = merge(recs[:, :2], int(hay.size))
    st = N.SpansStats()
    same(spans(a, hay, stats=st), want, "host")
    assert (st.n_records, st.n_spans) == (len(recs), len(want)), (st.n_records, st.n_spans, len(recs), len(want))
    got, rc, n_out, dst = device_raw(a, hay, len(want))
    assert rc == N.OK and n_out == len(want), (rc, n_out, len(want))
    same(got, want, "device")
    assert (dst["n_records"], dst["n_spans"]) == (len(recs), len(want)), dst
    return want, st


# ---- 1. fixtures ------------------------------------------------------------------------------------------------------------
FIXTURES = [("literal", N.MODE_LONGEST), ("literal", N.MODE_WHOLEWORD), ("literal", N.MODE_ALL), ("overlap2", N.MODE_LONGEST),
            ("overlap2", N.MODE_ALL), ("wwl4", N.MODE_WWLONGEST), ("shortest2", N.MODE_SHORTEST), ("readmeWholeWord", N.MODE_WHOLEWORD)]


@pytest.mark.parametrize("name,mode", FIXTURES)
def test_fixtures(fixtures, name, mode):
    fx = [f for f in fixtures if f["name"] == name][0]
    hay, kws = fixture_inputs(fx)
    kws = fx.get({N.MODE_SHORTEST: "S_keywords", N.MODE_WWLONGEST: "WWL_keywords"}.get(mode, "keywords"), kws)
    a, orc = pair(mode, kws)
    recs = orc.match(hay, cap=max(1024, len(hay) * 8))
    want, _ = check_both(a, orc, hay, recs)
    if (name, mode) == ("overlap2", N.MODE_LONGEST):
        assert [r[:2] for r in recs.tolist()[:2]] == [[1, 5], [5, 8]]  # two records that touch ...
        assert want.tolist()[0] == [1, 8]                               # ... are one span


# ---- 2. edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_LONGEST])
def test_edges(mode):
    a, orc = pair(mode, ["ab", "abc", "c"])
    base = "abzcabczzab"
    for n in (0, 1, 2, 7, 8, 9, len(base)):  # (length 2: the text is one span; 7: a span ends at n; all: one at unit 0)
        check_both(a, orc, base[:n])
    want, st = check_both(a, orc, "zzzz zzzz zzzz zzzz z")  # no match
    assert len(want) == 0 and st.n_records == 0
    want, _ = check_both(a, orc, "abc")  # the text is one span
    assert want.tolist() == [[0, 3]]
    a, orc = pair(mode, ["bc", "abcde"])
    want, _ = check_both(a, orc, "abcde")
    if mode == N.MODE_ALL:  # the first record, (1, 3), starts behind the span's start
        assert orc.match(utf16("abcde")).tolist()[0][:2] == [1, 3]
    assert want.tolist() == [[0, 5]]


# ---- 3. the tile seams of the two scans -------------------------------------------------------------------------------------
COUNTS = (T - 1, T, T + 1, 2 * T + 1, 3 * T)


@pytest.mark.parametrize("count", COUNTS)
def test_as_many_spans_as_records_at_the_tile_seams(count):
    a, orc = pair(N.MODE_ALL, ["a"])
    want, st = check_both(a, orc, "a." * count)
    assert st.n_records == count and len(want) == count


@pytest.mark.parametrize("count", COUNTS)
def test_one_span_of_all_records_at_the_tile_seams(count):
    # "a" * k under {a, aa} has 2 k - 1 records; an even count takes a "b" behind them and the keyword "ab", one record more
    a, orc = pair(N.MODE_ALL, ["a", "aa", "ab"])
    k = (count + 1) // 2
    hay = "a" * k + ("b" if count % 2 == 0 else "")
    want, st = check_both(a, orc, hay)
    assert st.n_records == count and want.tolist() == [[0, len(hay)]]


def random_dense(n_units):
    """20 keywords of 1 .. 6 units over "ab." and a random text of n_units over the same three -> (automaton, oracle, text, records)"""
    rng = np.random.default_rng(4306)  # (a seed under which the conditions asserted by the callers hold)
    kws, seen = [], set()
    while len(kws) < 20:
        k = "".join(rng.choice(list("ab."), int(rng.integers(1, 7))))
        if k not in seen:
            seen.add(k)
            kws.append(k)
    assert {len(k) for k in kws} == set(range(1, 7))
    hay = np.array([ord(c) for c in "ab."], np.uint16)[rng.choice(3, n_units, p=[0.3, 0.3, 0.4])]
    a, orc = pair(N.MODE_ALL, kws)
    recs = orc.match(hay, cap=hay.size * 8)
    return a, orc, hay, recs


@pytest.fixture(scope="module")
def random_case():
    return random_dense(12000)


def test_random_text_with_heads_on_every_lane_and_tile_position(random_case):
    a, orc, hay, recs = random_case
    assert 4 * T <= len(recs) <= 7 * T, len(recs)
    want = merge(recs[:, :2], hay.size)
    ends = recs[:, 1].astype(np.int64)
    assert (np.diff(ends) >= 0).all()
    heads = np.searchsorted(ends, want[:, 0], side="right")  # the first record that ends inside span k: the records' ends ascend
    assert {int(h) % 8 for h in heads} == set(range(8)) and {int(h) % 64 for h in heads} == set(range(64))
    on_tile = {int(h) % T for h in heads if h >= T}
    assert 0 in on_tile and T - 1 in on_tile, sorted(on_tile)[:3]
    check_both(a, orc, hay, recs)


# ---- 4. pieces and the carry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PIECES)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_tiny_pieces_every_family(mode, p):
    c = family_case(mode, True)
    a = Automaton(mode, c.kws, True, word_chars=c.wc)
    max_len = max(len(k) for k in c.kws)
    assert max_len == 41
    pieces(p)
    want, st = check_both(a, c.oracle, c.hay, c.recs)
    assert st.pieces >= c.hay.size // p and st.max_carry <= max_len // 2 + 2, (st.pieces, st.max_carry)
    if mode not in (N.MODE_ALL, N.MODE_SHORTEST):
        assert st.max_carry <= 1


@pytest.fixture(scope="module")
def covered_case():
    """AhoCorasick: keywords of 41 units that cover earlier, shorter matches -- "c" every 5 units in the one, every 2 units in the other"""
    sparse, dense = "abcab" * 8 + "a", "ca" * 20 + "c"
    kws = ["c", sparse, dense]
    hay = utf16("zz" + sparse + "zzz" + dense + "z" + sparse + dense + "zz" + "c" + "zzz")
    orc = Oracle(FAM_AC, kws)
    return kws, hay, orc, orc.match(hay, cap=hay.size * 8)


@pytest.mark.parametrize("p", PIECES)
def test_a_long_keyword_covers_earlier_matches_of_other_pieces(covered_case, p):
    kws, hay, orc, recs = covered_case
    # the regime, from the oracle's records: a record of 41 units with at least 4 records of one unit inside it that do not touch
    # each other, the first of which ends two pieces or more before the long one does (a piece owns the matches that END in it)
    r = recs[:, :2].astype(np.int64)
    long_ones = r[r[:, 1] - r[:, 0] == 41]
    reached = False
    for s, e in long_ones.tolist():
        inside = r[(r[:, 1] - r[:, 0] == 1) & (r[:, 0] >= s) & (r[:, 1] < e)]
        if len(inside) >= 4 and (np.diff(inside[:, 0]) >= 2).all() and (e - 1) // p >= (inside[0, 1] - 1) // p + 2:
            reached = True
    assert reached or 2 * p > 41 - 3, "no long record ends two pieces behind the first short one inside it"
    a = Automaton(N.MODE_ALL, kws, True)
    pieces(p)
    want, st = check_both(a, orc, hay, recs)
    assert 3 <= st.max_carry <= 41 // 2 + 2, st.max_carry
    assert len(want) == 4  # the four long keywords, of which the last two touch, and the lone "c": no "c" inside a long one is a span


# ---- 5. capacity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [None, 16])
def test_capacity(p):
    a, orc = pair(N.MODE_ALL, ["ab", "b", "bcd"])
    hay = utf16("ab.bcd..b.abab..bcdb.b..ab.b.bcd" * 3)
    want = merge(orc.match(hay, cap=hay.size * 8)[:, :2], hay.size)
    n = len(want)
    assert n >= 10
    if p:
        pieces(p)
    for cap in (0, 1, n - 1):
        for entry in (host_raw, device_raw):
            got, rc, n_out, st = entry(a, hay, cap)
            assert rc == N.E_OVERFLOW and n_out == n, (entry.__name__, cap, rc, n_out)
            same(got, want[:cap], entry.__name__)
    for entry in (host_raw, device_raw):
        got, rc, n_out, st = entry(a, hay, n)
        assert rc == N.OK and n_out == n
        same(got, want, entry.__name__)


# ---- 6. case folding and word characters ------------------------------------------------------------------------------------
def test_case_insensitive_all():
    a, orc = pair(N.MODE_ALL, ["Straße", "ab", "BCD", "é"], cs=False)
    check_both(a, orc, "xABcd STRAßE abé.É bCdab " * 40)


def test_wholeword_with_the_default_tables():
    a, orc = pair(N.MODE_WHOLEWORD, ["ab", "cd", "Éa"], cs=False)
    want, _ = check_both(a, orc, "AB cd,abcd éA-ab ab\tCD ab " * 40)
    assert len(want)
