"""GPU tests of the count-batch entries (include/acgpu.h: acgpu_count_batch_u16 and its UTF-8 twins; csrc/acgpu_terms.hip:
k_terms_block, k_terms_place and k_terms_gather behind every piece of the piece driver; ahocorasick_amd/terms.py).  Every expected
matrix comes from the CPU oracle, haystack by haystack: np.unique of the id column of its records.  Comparison is exact."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd import terms
from ahocorasick_amd.strings import (AhoCorasickMap, Automaton, LongestMatchMap, ShortestMatchMap, Utf8Error, WholeWordLongestMatchMap,
                                     WholeWordMatchMap, _pack, utf16)
from ahocorasick_amd.unicode_tables import word_chars_from_list
from oracle.oracle import FAM_AC, FAM_LONGEST, FAM_SHORTEST, FAM_WHOLEWORD, FAM_WWLONGEST, Oracle
from tests.helpers import LOWER, WORD

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20)]
MODES = {N.MODE_ALL: FAM_AC, N.MODE_LONGEST: FAM_LONGEST, N.MODE_WHOLEWORD: FAM_WHOLEWORD, N.MODE_SHORTEST: FAM_SHORTEST,
         N.MODE_WWLONGEST: FAM_WWLONGEST}
WORDY = (N.MODE_WHOLEWORD, N.MODE_WWLONGEST)
B = N.TERMS_BLOCK
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


def matrix(recs):
    """the oracle's records per haystack -> (indptr, indices, data): np.unique of every haystack's id column"""
    rows = [np.unique(r[:, 2], return_counts=True) if len(r) else (np.zeros(0, np.int64), np.zeros(0, np.int64)) for r in recs]
    indptr = np.concatenate([[0], np.cumsum([len(u) for u, _ in rows])]).astype(np.int64)
    return indptr, np.concatenate([u for u, _ in rows]).astype(np.int32), np.concatenate([c for _, c in rows]).astype(np.uint32)


def same(got, want):
    assert [g.dtype for g in got] == [np.int64, np.int32, np.uint32]
    assert got[0].tolist() == want[0].tolist()
    assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()


def check(a, hays, recs):
    """terms.count_batch against the oracle -> the call's stats"""
    want = matrix(recs)
    st = N.CountBatchStats()
    same(terms.count_batch(a, hays, stats=st), want)
    assert st.n_records == sum(len(r) for r in recs) and st.n_terms == len(want[1]), (st.n_records, st.n_terms)
    assert st.n_terms <= st.n_entries <= st.n_records and st.reserved == 0
    assert st.rows_cut > 0 or st.n_entries == st.n_terms  # (entries are merged away only in cut rows)
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
    """-> (automaton, haystacks, the oracle's records): the haystack list of tests/test_gpu_summary_batch.py's seam_case"""
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
    assert len(recs[6]) and len(recs[7]) and len(recs[8])
    if mode == N.MODE_WWLONGEST:
        assert recs[11].tolist() == [] and recs[12].tolist() == [[0, 1, 2], [2, 4, 6]]
    st = check(a, hays, recs)
    assert st.pieces >= 1 and st.rescans == 0 and st.rows_cut == 0  # (far fewer than B records: no row is cut)
    got = terms.count_batch(a, hays)
    sums = [int(got[2][got[0][i]:got[0][i + 1]].sum()) for i in range(len(hays))]
    assert sums == a.summary_batch(hays)[0]["n_matches"].tolist()  # the row sums are count_matches_batch
    # one haystack, one empty haystack: the smallest batches
    check(a, hays[3:4], recs[3:4])
    st = check(a, hays[:1], recs[:1])
    assert (st.n_records, st.pieces) == (0, 0)  # (nothing to scan)


# ---- 2. runs against the edges of the blocks -------------------------------------------------------------------------------------
def aaaa():
    if "aaaa" not in _SEAMS:
        _SEAMS["aaaa"] = pair(N.MODE_ALL, ["a", "aa", "aaa", "aaaa"])
    return _SEAMS["aaaa"]


def runs_of_a(lens):
    """AhoCorasick over a, aa, aaa, aaaa: a haystack of L >= 4 a's has 4 L - 6 records, L = 3 has 6, 2 has 3, 1 has 1"""
    a, orc = aaaa()
    hays = [np.full(int(ln), ord("a"), np.uint16) for ln in lens]
    recs = oracle_records(orc, hays)
    assert [len(r) for r in recs] == [4 * ln - 6 if ln >= 4 else (0, 1, 3, 6)[ln] for ln in lens]
    return a, hays, recs


def test_a_run_that_ends_on_a_block_boundary_is_not_cut():
    a, hays, recs = runs_of_a([513, 1, 1, 5, 2])  # 2046 + 1 + 1 = B, then 14 and 3 in the second block
    assert sum(len(r) for r in recs[:3]) == B
    st = check(a, hays, recs)
    assert st.rows_cut == 0 and st.n_entries == st.n_terms == 4 + 1 + 1 + 4 + 2


def test_a_run_cut_by_a_block_boundary_with_the_same_keyword_on_both_sides():
    a, hays, recs = runs_of_a([513, 3, 4])  # records 2046 .. 2051 are haystack 1's: a, aa | a, aaa, aa, a
    assert len(recs[0]) == B - 2 and recs[1][:2, 2].tolist() == [0, 1] and 0 in recs[1][2:, 2].tolist()
    st = check(a, hays, recs)
    assert st.rows_cut >= 1 and st.n_entries > st.n_terms, (st.rows_cut, st.n_entries, st.n_terms)


def test_a_run_that_spans_four_blocks():
    a, hays, recs = runs_of_a([2, 1600, 3])
    assert len(recs[1]) > 3 * B
    st = check(a, hays, recs)
    assert st.rows_cut >= 1 and st.n_entries > st.n_terms, (st.rows_cut, st.n_entries, st.n_terms)


def test_a_block_with_more_runs_than_lanes():
    rng = np.random.default_rng(24)
    lens = rng.integers(1, 4, 300)
    lens[rng.choice(300, 20, replace=False)] = 0
    a, hays, recs = runs_of_a(lens.tolist())
    assert sum(1 for r in recs if len(r)) > 256 and sum(len(r) for r in recs) < B  # one block, 280 runs
    st = check(a, hays, recs)
    assert st.rows_cut == 0


@pytest.mark.parametrize("lens,total", [([513, 1, 1], B), ([513, 1], B - 1), ([513, 1, 1, 1], B + 1)])
def test_batches_of_a_block_of_records_one_less_and_one_more(lens, total):
    a, hays, recs = runs_of_a(lens)
    assert sum(len(r) for r in recs) == total
    st = check(a, hays, recs)
    assert st.n_records == total and st.rows_cut == 0


# ---- 3. many distinct keys per block ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_LONGEST])
def test_many_distinct_keys_per_block(mode):
    rng = np.random.default_rng(31)
    letters = "abcdefghijklmnop"
    kws = [x + y for x in letters for y in letters] + list(letters)
    a, orc = pair(mode, kws)
    table = utf16(letters)
    hays = [table[rng.integers(0, 16, int(ln))] for ln in rng.integers(0, 61, 120)]
    recs = oracle_records(orc, hays)
    st = check(a, hays, recs)
    assert st.n_terms > 1000 and (mode == N.MODE_LONGEST or st.n_records > 2 * B)  # (AhoCorasick: several blocks)


# ---- 4. a row no block can hold --------------------------------------------------------------------------------------------------
def test_a_row_with_more_distinct_keywords_than_a_block_has_records():
    rng = np.random.default_rng(41)
    alpha = np.arange(0x100, 0x140, dtype=np.uint16)
    kws = [np.array([x, y], np.uint16) for x in alpha for y in alpha]
    a, orc = pair(N.MODE_ALL, kws)
    hays = [alpha[[1, 2, 3]], alpha[rng.integers(0, 64, 20000)], alpha[[5, 5]]]
    recs = oracle_records(orc, hays)
    assert len(np.unique(recs[1][:, 2])) > B
    st = check(a, hays, recs)
    assert st.rows_cut == 1 and st.n_entries > st.n_terms > B


# ---- 5. across pieces ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_rows_across_pieces(mode):
    kws, alpha = family_case(mode)
    rng = np.random.default_rng(400 + mode)
    table = utf16(alpha)
    hays = [table[rng.integers(0, len(table), int(ln))] for ln in rng.integers(150, 401, 40)]
    a, orc = pair(mode, kws)
    recs = oracle_records(orc, hays)
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
    assert st.pieces >= 10 and st.rescans == 0, (st.pieces, st.rescans)


# ---- 6. a piece scanned again is reduced once --------------------------------------------------------------------------------------
def test_rescans_count_nothing_twice():
    rng = np.random.default_rng(5)
    a, orc = pair(N.MODE_ALL, ["a", "aa", "aaa", "aaaa"])  # (its own automaton: a pool's reservoir never shrinks)
    table = utf16("aaaz")
    hays = [table[rng.integers(0, 4, int(ln))] for ln in rng.integers(0, 61, 100)]
    assert 2500 < sum(len(h) for h in hays) < 3500
    recs = oracle_records(orc, hays)
    N.set_tunable("cursor_reservoir_bytes", 4096)  # 341 records
    st = check(a, hays, recs)
    assert st.rescans >= 1 and st.pieces > st.rescans and st.n_records > 3000, (st.rescans, st.pieces, st.n_records)


# ---- 7. where the library scans haystack by haystack ---------------------------------------------------------------------------
def test_fallback_dictionary_without_a_free_unit():
    kws = [np.array([i], dtype=np.uint16) for i in range(65536)]
    a, orc = pair(N.MODE_ALL, kws)
    hays = [np.array(h, np.uint16) for h in ([5, 6], [7], [], [65535, 0, 1], [300] * 9, [], [0], [65535], [1, 2, 3, 4], [9] * 70, [], [8, 8])]
    recs = oracle_records(orc, hays)
    assert sum(len(r) for r in recs) == sum(len(h) for h in hays)
    st = check(a, hays, recs)
    assert st.pieces == sum(1 for h in hays if len(h))  # a text per haystack


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


# ---- 8. capacity -------------------------------------------------------------------------------------------------------------------
def test_capacity_rule():
    a, hays, recs = runs_of_a([513, 3, 4, 700, 2])  # cut rows: n_terms < n_entries < n_records
    want = matrix(recs)
    n_records, n_hay = sum(len(r) for r in recs), len(hays)
    units, off = _pack(hays)
    C64, C32 = 0x1122334455667788, 0x5A5A5A5A

    def call(cap):
        row_ptr, ids, counts = np.full(n_hay + 2, C64, np.uint64), np.full(cap + 1, C32, np.uint32), np.full(cap + 1, C32, np.uint32)
        n_out, st = ctypes.c_uint64(0), N.CountBatchStats()
        rc = N.lib().acgpu_count_batch_u16(a.handle, vp(units), vp(off), n_hay, vp(row_ptr), vp(ids), vp(counts), cap, ctypes.byref(n_out),
                                           ctypes.byref(st))
        assert row_ptr[-1] == C64 and ids[-1] == C32 and counts[-1] == C32
        return rc, n_out.value, st, row_ptr, ids, counts

    rc, n_out, st, row_ptr, ids, counts = call(n_records)  # the record count always suffices
    assert rc == N.OK and n_out == st.n_terms == len(want[1]) and st.n_records == n_records
    assert row_ptr[:-1].tolist() == want[0].tolist() and ids[:n_out].tolist() == want[1].tolist() and counts[:n_out].tolist() == want[2].tolist()
    n_entries = st.n_entries
    assert st.n_terms < n_entries < n_records
    rc, n_out, st, row_ptr, ids, counts = call(n_entries - 1)
    assert rc == N.E_OVERFLOW and n_out == n_entries == st.n_entries and st.n_terms == 0
    assert (row_ptr == C64).all() and (ids == C32).all() and (counts == C32).all()
    rc, n_out, st, row_ptr, ids, counts = call(0)
    assert rc == N.E_OVERFLOW and n_out == n_entries and (row_ptr == C64).all()
    rc, n_out, st, row_ptr, ids, counts = call(n_entries)  # the reported size succeeds
    assert rc == N.OK and n_out == len(want[1]) and st.n_entries == n_entries
    assert row_ptr[:-1].tolist() == want[0].tolist() and ids[:n_out].tolist() == want[1].tolist() and counts[:n_out].tolist() == want[2].tolist()


# ---- 9. UTF-8 ----------------------------------------------------------------------------------------------------------------------
U8_WORDS = ["straße", "é", "日本", "😀", "a😀b", "naïve", "\ufffd", "ab", "b"]


def test_utf8_forms_equal_the_call_on_the_decoded_lines():
    rng = np.random.default_rng(91)
    a, orc = pair(N.MODE_ALL, U8_WORDS)
    atoms = ["straße", "é", "日本", "😀", "a😀b", "naïve", "ab", "b", " ", "x", "ü", "語", "𝄞", "\ufffd"]
    lines = ["".join(atoms[int(i)] for i in rng.integers(0, len(atoms), int(n))) for n in rng.integers(0, 12, 60)] + ["", "😀", "b"]
    datas = [ln.encode("utf-8") for ln in lines]
    assert any(len(d) > len(ln) for d, ln in zip(datas, lines))
    recs = oracle_records(orc, lines)
    want = matrix(recs)
    assert len(want[1]) > 100
    same(terms.count_batch(a, lines), want)
    st = N.CountBatchStats()
    same(terms.count_batch_utf8(a, datas, stats=st), want)
    assert st.n_records == sum(len(r) for r in recs)
    buf = b"".join(datas)
    offsets = np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.uint64)
    same(terms.count_batch_utf8(a, buf, offsets=offsets), want)
    same(terms.count_batch_utf8(a, datas, errors="replace"), want)  # (well-formed bytes: the lossy form changes nothing)
    # an ill-formed line: refused, with the place
    bad = datas[:7] + [b"ab\xe6\x97 b"] + datas[7:]
    with pytest.raises(Utf8Error) as ei:
        terms.count_batch_utf8(a, bad)
    assert (ei.value.haystack, ei.value.start) == (7, 2)


def test_lossy_utf8_equals_the_call_on_the_lines_decoded_with_replace():
    a, orc = pair(N.MODE_ALL, U8_WORDS)
    datas = [b"\xffab", b"a\xf0\x9f\x98b stra\xc3\x9fe", b"b\xe6\x97", "日本 😀".encode(), b"", b"\x80\x80b\xc3", "a😀b".encode()[:-2] + b"b",
             b"\xed\xa0\x80", "naïve \ufffd".encode(), b"ab"]
    lines = [d.decode("utf-8", "replace") for d in datas]
    assert lines[0][0] == lines[1][1] == lines[2][-1] == "\ufffd"  # stray bytes at a line's start, middle and end
    recs = oracle_records(orc, lines)
    want = matrix(recs)
    fffd = U8_WORDS.index("\ufffd")
    assert sum(int((r[:, 2] == fffd).sum()) for r in recs) >= 8  # the replaced subparts match the U+FFFD keyword
    same(terms.count_batch(a, lines), want)
    same(terms.count_batch_utf8(a, datas, errors="replace"), want)
    offsets = np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.uint64)
    same(terms.count_batch_utf8(a, b"".join(datas), offsets=offsets, errors="replace"), want)
    with pytest.raises(Utf8Error) as ei:
        terms.count_batch_utf8(a, datas)
    assert (ei.value.haystack, ei.value.start) == (0, 0)


# ---- 10. through the facade --------------------------------------------------------------------------------------------------------
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
    want = matrix(recs)
    assert len(want[1]) > 50 and want[2].max() > 1
    m = WholeWordMatchMap(words, values, False)
    got = terms.count_batch(m, hays)
    same(got, want)
    same(terms.count_batch(m.automaton, hays), want)
    same(terms.count_batch_utf8(m, [h.encode() for h in hays]), want)
    columns = np.bincount(got[1], weights=got[2], minlength=len(words)).astype(np.uint64)
    assert columns.tolist() == sum(m.count(h) for h in hays).tolist()


@pytest.mark.parametrize("cls", [AhoCorasickMap, LongestMatchMap, ShortestMatchMap, WholeWordMatchMap, WholeWordLongestMatchMap])
def test_duplicate_keywords_report_the_index_that_won(cls):
    kws = ["ab", "cd", "ab", "e", "cd", "ab"]
    values = ["v%d" % i for i in range(len(kws))]
    hays = ["ab", "zz cd", "", "e ab e", "zz"]
    m = cls(kws, values, True)
    won = {"ab": 0, "cd": 1, "e": 3} if cls is ShortestMatchMap else {"ab": 5, "cd": 4, "e": 3}
    got = terms.count_batch(m, hays)
    row3 = sorted([(won["e"], 2), (won["ab"], 1)])
    same(got, (np.array([0, 1, 2, 2, 4, 4]), np.array([won["ab"], won["cd"]] + [i for i, _ in row3]), np.array([1, 1] + [c for _, c in row3])))
    orc = Oracle(MODES[cls._MODE], kws, True, None, WORD if cls._MODE in WORDY else None, map_flavour=True)
    same(got, matrix(oracle_records(orc, hays)))
    columns = np.bincount(got[1], weights=got[2], minlength=len(kws)).astype(np.uint64)
    assert columns.tolist() == sum(m.count(h) for h in hays).tolist()


# ---- 11. the stream rule -----------------------------------------------------------------------------------------------------------
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
    row_ptr, ids, counts = np.full(len(hays) + 1, 77, np.uint64), np.full(4096, 77, np.uint32), np.full(4096, 77, np.uint32)
    n_out = ctypes.c_uint64(77)
    rc = N.lib().acgpu_count_batch_u16(a.handle, vp(units), vp(off), len(hays), vp(row_ptr), vp(ids), vp(counts), 4096, ctypes.byref(n_out), None)
    assert rc == N.E_INVALID and (row_ptr == 77).all() and (ids == 77).all() and (counts == 77).all() and n_out.value == 77
    m, rc, _ = a.match_device_end(tk)
    assert rc == N.OK and m > 0
    check(a, hays, recs)
