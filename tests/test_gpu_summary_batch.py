"""GPU tests of the batch summary entry (include/acgpu.h: acgpu_summary_batch_u16; csrc/acgpu_summary.hip: k_batch_summary behind
every piece of the piece driver).  Every expected summary comes from the CPU oracle, haystack by haystack: the number of its
records and the first of them in listener order, or (-1, -1, -1)."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import (AhoCorasickMap, AhoCorasickSet, Automaton, LongestMatchMap, ShortestMatchMap, WholeWordLongestMatchMap,
                                     WholeWordMatchMap, WholeWordMatchSet, _pack, utf16)
from ahocorasick_amd.unicode_tables import word_chars_from_list
from oracle.oracle import FAM_AC, FAM_LONGEST, FAM_SHORTEST, FAM_WHOLEWORD, FAM_WWLONGEST, Oracle
from tests.helpers import LOWER, WORD

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20)]
MODES = {N.MODE_ALL: FAM_AC, N.MODE_LONGEST: FAM_LONGEST, N.MODE_WHOLEWORD: FAM_WHOLEWORD, N.MODE_SHORTEST: FAM_SHORTEST,
         N.MODE_WWLONGEST: FAM_WWLONGEST}
WORDY = (N.MODE_WHOLEWORD, N.MODE_WWLONGEST)
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def pair(mode, kws, cs=True, wc=None):
    if wc is None and mode in WORDY:
        wc = WORD
    return (Automaton(mode, kws, cs, word_chars=wc),
            Oracle(MODES[mode], kws, cs, None if cs else LOWER, wc, map_flavour=True))


def oracle_records(orc, hays):
    """the oracle's records of every haystack alone: computed once per case"""
    return [orc.match(h, cap=max(64, 8 * len(h))) for h in hays]


def summaries(recs):
    want = np.zeros(len(recs), dtype=N.SUMMARY_DTYPE)
    for i, r in enumerate(recs):
        want[i] = (len(r),) + (tuple(r[0].tolist()) if len(r) else (-1, -1, -1)) + (0,)
    return want


def check(a, hays, recs):
    """Automaton.summary_batch against the oracle -> the call's stats"""
    want = summaries(recs)
    got, st = a.summary_batch(hays)
    assert got.dtype == N.SUMMARY_DTYPE and got.shape == want.shape
    bad = [i for i in range(len(hays)) if got[i] != want[i]]
    assert not bad, (bad[:5], got[bad[:5]], want[bad[:5]])
    assert st["n_records"] == sum(len(r) for r in recs) and st["n_matched"] == sum(1 for r in recs if len(r)), st
    return st


def family_case(mode):
    """keywords and the alphabet of the random haystacks; the word matchers' texts have two non-word units"""
    if mode == N.MODE_WWLONGEST:  # " " and ", " have no word character: kept as they are, the root has a transition on them
        return ["ab", "ab cd", " ", "c", ", ", "abcd a", "ab"], "abcd ,"
    if mode == N.MODE_WHOLEWORD:
        return ["ab", "abc", "c", "dd", "abcda", "ab"], "abcd ,"
    if mode == N.MODE_ALL:
        return ["ab", "abc", "c", "bcd", "dd", "abcdab", "ab", "b"], "abcdz"
    return ["ab", "abc", "c", "bcd", "dd", "abcdab", "ab"], "abcdz"


def seam_case(mode):
    """-> (automaton, haystacks, the oracle's records): shared by the first two tests"""
    if mode not in _SEAMS:
        kws, alpha = family_case(mode)
        rng = np.random.default_rng(100 + mode)
        a, orc = pair(mode, kws)
        word = mode in WORDY
        hays = ["", "zz zz" if word else "zzzz", "ab",          # empty, no match, one that is a single match
                "ab zz c" if word else "abzzc",                   # a match as first units and one as last units
                "xa", "by", "ab", "c", "ab", "cd", "",            # joins that spell "ab", "abc", "ab cd": no match across
                " ab", "  ab", ", c", " ", ",", "", "", "d, ",    # WholeWordLongest: a haystack's first unit is a walk start
                "abc"]
        table = utf16(alpha)
        hays += [table[rng.integers(0, len(table), int(ln))] for ln in rng.integers(0, 41, 30)]
        _SEAMS[mode] = (a, hays, oracle_records(orc, hays))
    return _SEAMS[mode]


_SEAMS = {}


# ---- 1. five families at the seams between haystacks --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_five_families_at_the_seams(mode):
    a, hays, recs = seam_case(mode)
    assert len(recs[0]) == 0 and len(recs[1]) == 0 and len(recs[4]) == 0 and len(recs[10]) == 0
    assert len(recs[5]) == (1 if mode == N.MODE_ALL else 0)  # (its dictionary has "b")
    assert recs[3][-1, 1] == len(hays[3]) and len(recs[6]) and len(recs[7]) and len(recs[8])
    if mode == N.MODE_WWLONGEST:
        assert recs[11].tolist() == [] and recs[12].tolist() == [[0, 1, 2], [2, 4, 6]]
    if mode == N.MODE_ALL:
        # listener order is end ascending, then start ascending: in "abc" the keywords "ab" and "b" are reported before "abc"
        assert recs[19].tolist() == [[0, 2, 6], [1, 2, 7], [0, 3, 1], [2, 3, 2]]
        # With this dictionary the first record always has the lowest start too (every longer keyword begins with "ab" or "b",
        # which end no later than anything inside it).  Without "ab" it has not: "b" in "abc" is reported before "abc".
        a2, orc2 = pair(mode, ["abc", "b"])
        recs2 = oracle_records(orc2, hays)
        assert recs2[19].tolist() == [[1, 2, 1], [0, 3, 0]]
        late = [i for i, r in enumerate(recs2) if len(r) and r[0, 0] > r[:, 0].min()]
        assert late, "no haystack whose first record does not have the smallest start"
        check(a2, hays, recs2)
    st = check(a, hays, recs)
    assert st["pieces"] >= 1 and st["rescans"] == 0
    # one haystack, one empty haystack: the smallest batches
    check(a, hays[3:4], recs[3:4])
    check(a, hays[:1], recs[:1])


# ---- 2. agreement with the call that returns the records -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_agreement_with_the_batch_match_call(mode):
    a, hays, _ = seam_case(mode)
    tagged = a.match_batch(hays, with_ids=True)
    want = np.zeros(len(hays), dtype=N.SUMMARY_DTYPE)
    want[:] = (0, -1, -1, -1, 0)
    for h, s, e, k in tagged.tolist():
        if want[h]["n_matches"] == 0:
            want[h] = (1, s, e, k, 0)
        else:
            want["n_matches"][h] += 1
    got, st = a.summary_batch(hays)
    assert (got == want).all() and st["n_records"] == len(tagged)


# ---- 3. runs of every length against the kernel's waves and workgroups ---------------------------------------------------------
def test_runs_across_workgroups_and_waves():
    """AhoCorasick with a, aa, aaa, aaaa: a haystack of L units has 4 L - 6 records (L >= 4), so the runs end on and around the
    64-record waves and the 256-record workgroups, one run has thousands of records, and 200 short haystacks give runs of 0 to 3"""
    rng = np.random.default_rng(3)
    a, orc = pair(N.MODE_ALL, ["a", "aa", "aaa", "aaaa"])
    lens = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 0, 3] + rng.integers(0, 3, 200).tolist()
    hays = [np.full(int(ln), ord("a"), np.uint16) for ln in lens]
    recs = oracle_records(orc, hays)
    assert len(recs[8]) == 4 * 1000 - 6 and len(recs[1]) == 1 and len(recs[10]) == 6
    st = check(a, hays, recs)
    assert st["n_records"] > 7000


# ---- 4. runs across pieces -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_runs_across_pieces(mode):
    kws, alpha = family_case(mode)
    rng = np.random.default_rng(400 + mode)
    table = utf16(alpha)
    hays = [table[rng.integers(0, len(table), int(ln))] for ln in rng.integers(150, 401, 40)]
    # haystack 0 is cut by the first piece end (64) and its only record lies behind it: its first match comes from a later piece
    filler = ord(",") if mode in WORDY else ord("z")
    hays[0] = np.full(150, filler, np.uint16)
    hays[0][100] = ord("c")
    a, orc = pair(mode, kws)
    recs = oracle_records(orc, hays)
    assert recs[0].tolist() == [[100, 101, kws.index("c")]]
    # the ramp: 64 units, then 256 at a time (the density cap is far away with the default reservoir)
    starts = np.concatenate([[0], np.cumsum([len(h) + 1 for h in hays])])
    piece_ends = np.arange(64, starts[-1], 256)
    cut = 0
    for i, r in enumerate(recs):
        inside = piece_ends[(piece_ends > starts[i]) & (piece_ends < starts[i] + len(hays[i]))] - starts[i]
        cut += any((r[:, 1] <= b).any() and (r[:, 0] >= b).any() for b in inside)
    assert cut >= 10, cut  # haystacks with records on both sides of a piece end
    N.set_tunable("cursor_first_piece", 64)
    N.set_tunable("cursor_max_piece", 256)
    st = check(a, hays, recs)
    assert st["pieces"] >= 10 and st["rescans"] == 0, st


# ---- 5. a piece scanned again is summarised once -------------------------------------------------------------------------------
def test_rescans_count_nothing_twice():
    rng = np.random.default_rng(5)
    a, orc = pair(N.MODE_ALL, ["a", "aa", "aaa", "aaaa"])
    table = utf16("aaaz")
    hays = [table[rng.integers(0, 4, int(ln))] for ln in rng.integers(0, 61, 100)]
    assert 2500 < sum(len(h) for h in hays) < 3500
    recs = oracle_records(orc, hays)
    N.set_tunable("cursor_reservoir_bytes", 4096)  # 341 records
    st = check(a, hays, recs)
    assert st["rescans"] >= 1 and st["pieces"] > st["rescans"] and st["n_records"] > 3000, st


# ---- 6. where the library scans haystack by haystack ---------------------------------------------------------------------------
def test_fallback_dictionary_without_a_free_unit():
    kws = [np.array([i], dtype=np.uint16) for i in range(65536)]
    a, orc = pair(N.MODE_ALL, kws)
    hays = [np.array(h, np.uint16) for h in ([5, 6], [7], [], [65535, 0, 1], [300] * 9, [], [0], [65535], [1, 2, 3, 4], [9] * 70, [], [8, 8])]
    recs = oracle_records(orc, hays)
    assert sum(len(r) for r in recs) == sum(len(h) for h in hays)
    st = check(a, hays, recs)
    assert st["pieces"] == sum(1 for h in hays if len(h))  # a text per haystack


@pytest.mark.parametrize("mode", WORDY)
def test_fallback_word_table_that_is_not_fold_consistent(mode):
    rng = np.random.default_rng(9)
    alpha = np.array([ord(ch) for ch in "abxyABXY ,"], dtype=np.uint16)
    wc = word_chars_from_list("abcdxyABCD")  # X, Y are not word characters although x, y are
    kws = [alpha[rng.integers(0, 4, int(rng.integers(1, 5)))] for _ in range(12)]
    kws += [kws[2].copy()]
    a, orc = pair(mode, kws, cs=False, wc=wc)
    assert a.info()["fold_consistent"] == 0
    hays = [alpha[rng.integers(0, len(alpha), int(ln))] for ln in (0, 1, 40, 300, 7, 0, 120, 3, 12, 60, 0, 25)]
    recs = oracle_records(orc, hays)
    assert sum(len(r) for r in recs) > 5
    check(a, hays, recs)


# ---- 7. case folding and duplicate keywords through the facade -----------------------------------------------------------------
def test_case_insensitive_map_through_the_facade():
    rng = np.random.default_rng(7)
    words = ["straße", "naïve", "Zürich", "λόγος", "ΑΘΗΝΑ", "σοφία", "москва", "Привет", "мир", "data", "GPU"]
    values = ["[%d:%s]" % (i, w.upper()) for i, w in enumerate(words)]
    filler = ["und", "και", "или", "the", "x1"]

    def flip(w):
        return "".join(c.upper() if rng.integers(2) else c.lower() for c in w)

    def sentence(n):
        toks = [flip(words[int(rng.integers(len(words)))]) if rng.integers(3) == 0 else filler[int(rng.integers(len(filler)))] for _ in range(n)]
        return "".join(t + (" ", ", ", "-")[int(rng.integers(3))] for t in toks)
    hays = [sentence(int(n)) for n in rng.integers(0, 8, 150)]
    orc = Oracle(FAM_WHOLEWORD, words, False, LOWER, WORD, map_flavour=True)
    recs = oracle_records(orc, hays)
    n = [len(r) for r in recs]
    assert 20 < sum(1 for x in n if x) < 130 and max(n) > 1
    m = WholeWordMatchMap(words, values, False)
    contains, counts = m.contains_batch(hays), m.count_matches_batch(hays)
    assert contains.dtype == np.bool_ and contains.tolist() == [x > 0 for x in n]
    assert counts.dtype == np.uint64 and counts.tolist() == n
    assert m.first_batch(hays) == [(int(r[0, 0]), int(r[0, 1]), values[int(r[0, 2])]) if len(r) else None for r in recs]
    s = WholeWordMatchSet(words, False)
    assert s.first_batch(hays) == [(int(r[0, 0]), int(r[0, 1])) if len(r) else None for r in recs]
    assert s.contains_batch(hays).tolist() == contains.tolist()


@pytest.mark.parametrize("cls", [AhoCorasickMap, LongestMatchMap, ShortestMatchMap, WholeWordMatchMap, WholeWordLongestMatchMap])
def test_duplicate_keywords_report_the_value_that_won(cls):
    kws = ["ab", "cd", "ab", "e", "cd", "ab"]
    values = ["v%d" % i for i in range(len(kws))]
    hays = ["ab", "zz cd", "", "e ab", "zz"]
    m = cls(kws, values, True)
    first = {"ab": 0, "cd": 1, "e": 3} if cls is ShortestMatchMap else {"ab": 5, "cd": 4, "e": 3}
    assert m.first_batch(hays) == [(0, 2, values[first["ab"]]), (3, 5, values[first["cd"]]), None, (0, 1, values[first["e"]]), None]
    assert m.count_matches_batch(hays).tolist() == [1, 1, 0, 2, 0]
    assert m.contains_batch(hays).tolist() == [True, True, False, True, False]
    assert AhoCorasickSet(kws, True).first_batch(hays[:2]) == [(0, 2), (3, 5)]


# ---- 8. the stream rule ----------------------------------------------------------------------------------------------------------
def test_stream_rule():
    import torch
    a, hays, recs = seam_case(N.MODE_ALL)
    hay = np.concatenate([utf16(h) for h in hays] * 20)
    d_hay = torch.from_numpy(hay.view(np.int16)).cuda()
    cap = 4 * hay.size
    out_recs = torch.empty((cap, 3), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    tk, rc = a.match_device_begin(d_hay.data_ptr(), hay.size, True, out_recs.data_ptr(), cap, stream=stream.cuda_stream)
    assert rc == N.OK
    units, off = _pack(hays)
    out = np.zeros(len(hays), dtype=N.SUMMARY_DTYPE)
    out[:] = (77, 7, 7, 7, 7)
    rc = N.lib().acgpu_summary_batch_u16(a.handle, vp(units), vp(off), len(hays), vp(out), None)
    assert rc == N.E_INVALID and all(tuple(r) == (77, 7, 7, 7, 7) for r in out.tolist())
    m, rc, _ = a.match_device_end(tk)
    assert rc == N.OK and m > 0
    check(a, hays, recs)
