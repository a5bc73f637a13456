"""GPU tests of the UTF-8 batch entries (include/acgpu.h: acgpu_match_batch_utf8, acgpu_summary_batch_utf8; csrc/acgpu_utf8.hip:
k_utf8_batch_count, k_utf8_batch_write, k_utf8_batch_tag, k_summary_utf8_bytes around the unchanged scan).  Every expected record
comes from the CPU oracle on each haystack decoded alone, its positions mapped to bytes by the header's rule restated over the
haystack's code points (unit_map / to_bytes of tests/test_gpu_utf8.py, not the product's utf8_unit_offsets); equality is exact.
Expected error positions are CPython's: the first haystack whose .decode() fails, and its UnicodeDecodeError.start."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import (AhoCorasickMap, AhoCorasickSet, Automaton, LongestMatchMap, Utf8Error, WholeWordMatchMap, WholeWordMatchSet,
                                     utf8_line_offsets, utf16)
from ahocorasick_amd.unicode_tables import word_chars_from_list
from oracle.oracle import FAM_WHOLEWORD, Oracle
from tests.helpers import LOWER, WORD
from tests.test_gpu_utf8 import MODES, WORDY, filler, keywords_from, mixed_text, pair, to_bytes

pytestmark = pytest.mark.gpu

BLOCK = 4096  # bytes per workgroup of the transcoder (16 per lane)
RESERVOIR = ("cursor_reservoir_bytes", 256 << 20)
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
EMPTY = np.zeros((0, 3), np.int32)


def expected(orc, datas):
    """-> per haystack (records in units, records in bytes), from the oracle on each haystack decoded alone"""
    per = []
    for d in datas:
        text = bytes(d).decode("utf-8")
        if not text:
            per.append((EMPTY, EMPTY))
            continue
        recs = orc.match(utf16(text), cap=max(1024, 8 * len(text)))
        per.append((recs, to_bytes(recs, text)))
    return per


def tagged(per):
    rows = [np.column_stack([np.full(len(b), i, np.int32), b]) for i, (_, b) in enumerate(per) if len(b)]
    return np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 4), np.int32)


def summaries(per):
    want = np.zeros(len(per), dtype=N.SUMMARY_DTYPE)
    for i, (_, b) in enumerate(per):
        want[i] = (len(b),) + (tuple(b[0].tolist()) if len(b) else (-1, -1, -1)) + (0,)
    return want


def n_units_of(datas):
    return sum(len(utf16(bytes(d).decode("utf-8"))) for d in datas)


def check(a, per, datas, kinds=(True, False), offsets=None):
    """match_batch_utf8 (both record kinds) and summary_batch_utf8 against the oracle -> (batch stats, summary stats)"""
    want = tagged(per)
    st = N.Utf8BatchStats()
    arg = datas if offsets is None else b"".join(bytes(d) for d in datas)
    for with_ids in kinds:
        got = a.match_batch_utf8(arg, with_ids=with_ids, stats=st, offsets=offsets)
        w = want if with_ids else want[:, :3]
        assert got.shape == w.shape and got.dtype == np.int32, (got.shape, w.shape)
        bad = np.flatnonzero((got != w).any(axis=1))
        assert not len(bad), (bad[:5], got[bad[:5]], w[bad[:5]])
        assert (st.n_units, st.first_bad, st.bad_haystack) == (n_units_of(datas), -1, 0)
        assert st.ascii == int(all(max(bytes(d), default=0) < 0x80 for d in datas))
    ws = summaries(per)
    st2 = N.Utf8BatchStats()
    got, sst = a.summary_batch_utf8(arg, stats=st2, offsets=offsets)
    assert got.dtype == N.SUMMARY_DTYPE and got.shape == ws.shape
    bad = [i for i in range(len(ws)) if got[i] != ws[i]]
    assert not bad, (bad[:5], got[bad[:5]], ws[bad[:5]])
    assert sst["n_records"] == len(want) and sst["n_matched"] == sum(1 for _, b in per if len(b)), sst
    assert (st2.n_units, st2.first_bad, st2.bad_haystack, st2.ascii) == (st.n_units, -1, 0, st.ascii)
    return st, sst


def run(a, orc, datas, **kw):
    per = expected(orc, datas)
    check(a, per, datas, **kw)
    return per


def cut_up(rng, text, lo, hi, empties):
    """the characters of `text` as haystacks of lo..hi characters; about one in `empties` is empty.  A haystack that is not empty
    is cut behind a separator of mixed_text (a word has at most 6 characters), so that the word matchers find whole words"""
    out, i = [], 0
    while i < len(text):
        ln = 0 if rng.integers(empties) == 0 else int(rng.integers(lo, hi - 6))
        while 0 < ln and i + ln < len(text) and text[i + ln - 1] not in " ,·。\n":
            ln += 1
        assert ln <= hi
        out.append(text[i:i + ln].encode("utf-8"))
        i += ln
    return out


def keywords(rng, text, mode, cs):
    """keywords drawn from the text (with a duplicate); the word matchers, whose keywords are whole words, get four draws"""
    if mode not in WORDY:
        return keywords_from(rng, text[:4000], mode, cs)
    return [k for i in range(4) for k in keywords_from(rng, text[3000 * i:3000 * i + 3000], mode, cs)]


def conditions(per):
    n_recs = sum(len(b) for _, b in per)
    shifted = sum(1 for u, b in per if len(b) and b[0, 0] != u[0, 0])
    return n_recs, shifted, sum(1 for u, _ in per if not len(u))


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------
def parity_case(mode, cs):
    rng = np.random.default_rng(7000 + 10 * mode + cs)
    text = mixed_text(rng, 12000)
    kws = keywords(rng, text, mode, cs)
    return rng, text, kws


@pytest.mark.parametrize("cs", [True, False])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_parity_with_the_haystacks_decoded_one_by_one(mode, cs):
    rng, text, kws = parity_case(mode, cs)
    a, orc = pair(mode, kws, cs)
    datas = cut_up(rng, text, 0, 60, 12)[:400]
    per = expected(orc, datas)
    # the input's own conditions
    n_recs, shifted, without = conditions(per)
    assert len(datas) == 400 and n_recs >= 200 and shifted >= 20, (n_recs, shifted)
    assert sum(1 for d in datas if not d) >= 10 and without - sum(1 for d in datas if not d) >= 10
    assert {len(ch.encode()) for ch in text} == {1, 2, 3, 4}
    st, _ = check(a, per, datas)
    assert st.ascii == 0
    check(a, per, datas, kinds=(True,), offsets=np.cumsum([0] + [len(d) for d in datas], dtype=np.uint64))


@pytest.mark.parametrize("mode", sorted(MODES))
def test_parity_across_many_workgroups(mode):
    """one batch of about 300 000 bytes in about 6 000 haystacks: some 75 workgroups of the transcoder"""
    rng = np.random.default_rng(7100 + mode)
    text = mixed_text(rng, 170000)
    a, orc = pair(mode, keywords(rng, text, mode, True), True)
    datas = cut_up(rng, text, 0, 60, 12)
    assert 280000 < sum(len(d) for d in datas) < 340000 and 5000 < len(datas) < 7500
    per = expected(orc, datas)
    n_recs, shifted, _ = conditions(per)
    assert n_recs >= 200 and shifted >= 20
    check(a, per, datas)


# ---- 2. haystack boundaries against the transcoder's seams ---------------------------------------------------------------------
SEAMS = [s + d for s in (16, 1008, 1024, 4080, 4096, 8192) for d in range(-4, 5)]


def seam_pair():
    if not _SEAM:
        _SEAM.append(pair(N.MODE_ALL, ["😀", "\ud83d", "\ude00", "é", "€😀", "kw", "k", "ab"]))
    return _SEAM[0]


_SEAM = []


def test_a_boundary_at_every_offset_around_the_seams():
    """the cut lies at byte p exactly: a 4-byte character immediately before it and immediately behind it, and a keyword matches
    in the first and in the last unit of both neighbours"""
    a, orc = seam_pair()
    for p in SEAMS:
        left = "😀".encode() + filler(p - 8) + "😀".encode()
        right = "😀".encode() + filler(37) + "😀".encode()
        assert len(left) == p
        per = run(a, orc, [left, right], kinds=(True,))
        for (u, b), data in zip(per, (left, right)):
            n = len(utf16(data.decode()))
            assert (u[:, 0] == 0).any() and (u[:, 0] == 1).any() and (u[:, 1] == n).any() and (u[:, 0] == n - 1).any()
            assert (b[:, 0] == 0).any() and (b[:, 1] == len(data)).any()
    # all-ASCII twins of the same shapes
    for p in SEAMS:
        datas = [b"k" + b"a" * (p - 2) + b"k", b"kw" + b"a" * 30 + b"ab"]
        per = expected(orc, datas)
        assert len(per[0][1]) == 2 and len(per[1][1]) == 3
        st, _ = check(a, per, datas, kinds=(True,))
        assert st.ascii == 1


def test_one_filler_text_cut_at_every_seam_offset():
    """... and one text with all those boundaries at once, each rounded down to a code-point boundary of the filler (where two
    round to the same byte there is an empty haystack)"""
    a, orc = seam_pair()
    text = filler(8192 + 64)
    starts = np.flatnonzero((np.frombuffer(text, np.uint8) & 0xC0) != 0x80)
    cuts = [int(starts[np.searchsorted(starts, p, side="right") - 1]) for p in SEAMS]
    off = [0] + cuts + [len(text)]
    assert off == sorted(off) and len(set(off)) < len(off)
    datas = [text[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    per = run(a, orc, datas)
    assert sum(len(b) for _, b in per) > 2000


# ---- 3. separators against the checkpoint stride ---------------------------------------------------------------------------------
def test_separators_do_not_shift_the_checkpoints():
    """200 haystacks of 1 .. 40 units, cycling; from 4 units on a haystack begins and ends with an astral character that is a
    keyword (2 units: that character alone; 1 and 3 units: "é", "é😀")"""
    a, orc = seam_pair()
    mid = "aé€b中"
    texts = []
    for i in range(200):
        ln = i % 40 + 1
        texts.append({1: "é", 2: "😀", 3: "é😀"}.get(ln) or "😀" + (mid * 8)[:ln - 4] + "😀")
        assert len(utf16(texts[-1])) == ln
    datas = [t.encode() for t in texts]
    per = expected(orc, datas)
    pure0 = np.cumsum([0] + [len(utf16(t)) for t in texts])  # a haystack's first unit, separators not counted
    residues = set()
    for i, (u, _) in enumerate(per):
        residues |= set(((u[:, 0] + pure0[i]) % 32).tolist())
    assert residues == set(range(32))
    seps = [int(pure0[j + 1]) + j for j in range(len(texts))]  # where separator j stands in the text the scan sees
    assert any(s % 32 == 0 for s in seps)
    check(a, per, datas)


# ---- 4. empty haystacks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_len", [1, 2, 5])
def test_runs_of_empty_haystacks(run_len):
    a, orc = seam_pair()
    e = [b""] * run_len
    h = ["😀kw é".encode(), "ab€😀".encode(), "é".encode()]
    run(a, orc, e + h)                      # at the front
    run(a, orc, h[:1] + e + h[1:])          # in the middle
    run(a, orc, h + e)                      # at the end
    run(a, orc, e + h[:2] + e + h[2:] + e)
    for d in (-1, 0, 1):                    # at a seam of the transcoder's workgroups
        left = filler(BLOCK + d - 4) + "😀".encode()
        run(a, orc, [left] + e + ["😀ab".encode()], kinds=(True,))
    left = filler(BLOCK - 4) + "😀".encode()  # ... and at the buffer's end where that is a seam: no lane begins there
    run(a, orc, [left] + e, kinds=(True,))


def test_one_haystack_among_fifty_empty_ones_and_one_alone():
    a, orc = seam_pair()
    data = "kw😀 é ab €😀".encode()
    for at in (0, 17, 50):
        per = run(a, orc, [b""] * at + [data] + [b""] * (50 - at))
        assert len(per[at][1]) > 5
    for d in (data, filler(2 * BLOCK + 3), b"kw ab"):
        per = run(a, orc, [d])
        alone = a.match_utf8(d, with_ids=True)
        assert (tagged(per) == np.column_stack([np.zeros(len(alone), np.int32), alone])).all()


# ---- 5. nothing crosses a haystack ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_nothing_crosses_a_haystack(mode):
    a, orc = pair(mode, ["foo", "bar", "foobar", "ab", "éa"], True)
    per = run(a, orc, [b"a", b"b", b"foo", b"bar", "é".encode(), b"a", b"foo", b"", b"bar", b"ab"])
    assert [len(b) for _, b in per] == [0, 0, 1, 1, 0, 0, 1, 0, 1, 1]


# ---- 6. validation: differential against CPython -----------------------------------------------------------------------------------
def cpython_first(datas):
    """-> (the first haystack whose decode fails, UnicodeDecodeError.start in it), or None"""
    for i, d in enumerate(datas):
        try:
            bytes(d).decode("utf-8")
        except UnicodeDecodeError as e:
            return i, e.start
    return None


def refused(a, datas, with_ids=True):
    """the raw call on an ill-formed batch -> (bad_haystack, first_bad); out keeps its canary, nothing is reported"""
    buf = np.frombuffer(b"".join(datas) or b"\0", np.uint8)
    off = np.cumsum([0] + [len(d) for d in datas], dtype=np.uint64)
    kind = N.REC_MAP if with_ids else N.REC_SET
    out = np.full((16, kind // 4 + 1), 77, np.int32)
    n_out = ctypes.c_uint64(5)
    st = N.Utf8BatchStats(7, 7, 7, 7)
    rc = N.lib().acgpu_match_batch_utf8(a.handle, vp(buf), vp(off), len(datas), kind, vp(out), 16, ctypes.byref(n_out), ctypes.byref(st))
    assert rc == N.E_ENCODING and n_out.value == 0 and (out == 77).all() and (st.n_units, st.ascii) == (0, 0)
    sums = np.zeros(len(datas), dtype=N.SUMMARY_DTYPE)
    sums[:] = (77, 7, 7, 7, 7)
    st2 = N.Utf8BatchStats(7, 7, 7, 7)
    rc = N.lib().acgpu_summary_batch_utf8(a.handle, vp(buf), vp(off), len(datas), vp(sums), None, ctypes.byref(st2))
    assert rc == N.E_ENCODING and all(tuple(r) == (77, 7, 7, 7, 7) for r in sums.tolist())
    assert (st2.bad_haystack, st2.first_bad, st2.n_units, st2.ascii) == (st.bad_haystack, st.first_bad, 0, 0)
    return st.bad_haystack, st.first_bad


GOOD = ["kw😀 é".encode(), b"", "ab€😀".encode()]


def test_random_cuts_of_a_valid_text_fail_where_cpython_fails():
    a, orc = seam_pair()
    good = expected(orc, GOOD)
    text = mixed_text(np.random.default_rng(66), 5200).encode()
    assert 8000 < len(text) < 10500
    arr = np.frombuffer(text, np.uint8)
    inside = set()
    for seed in range(20):
        rng = np.random.default_rng(600 + seed)
        cuts = np.sort(rng.integers(0, len(text) + 1, 300)).tolist()
        off = [0] + cuts + [len(text)]
        datas = [text[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        want = cpython_first(datas)
        assert want is not None, seed
        assert refused(a, datas, with_ids=bool(seed & 1)) == want, (seed, want)
        # the sequence the failing cut fell into: the failure is a lead that haystack `i` truncates, or a continuation byte at its start
        p = off[want[0]] + want[1]
        while (arr[p] & 0xC0) == 0x80:
            p -= 1
        inside.add(1 + (arr[p] >= 0xC0) + (arr[p] >= 0xE0) + (arr[p] >= 0xF0))
        if seed % 5 == 0:
            check(a, good, GOOD, kinds=(True,))  # the same automaton answers a good batch
    assert inside >= {2, 3, 4}, inside
    with pytest.raises(Utf8Error) as e:
        a.match_batch_utf8(datas, with_ids=True)
    assert (e.value.haystack, e.value.start) == want
    with pytest.raises(Utf8Error) as e:
        a.summary_batch_utf8(datas)
    assert (e.value.haystack, e.value.start) == want
    check(a, good, GOOD)


HAND = [([b"a\xc3", b"\xa9b"], (0, 1)),
        ([b"ok", b"\xa9b"], (1, 0)),
        ([b"", b"\xf0\x9f", b"\x98\x80"], (1, 0)),
        ([b"x\xe2\x82", b"\xac"], (0, 1)),
        ([b"\xf0\x9f\x98", b"", b"\x80"], (0, 0)),
        (["é".encode()] * 7 + [b"ab\xe0\x80\xafcd", b"ok"], (7, 2)),      # an overlong form in haystack 7 of 9
        ([b"ok", b""] * 3 + ["€".encode(), b"abc\xed\xa0\x80", b"\x80"], (7, 3))]  # an encoded surrogate there


def test_hand_cases_and_the_same_with_the_cut_at_a_workgroup_seam():
    a, orc = seam_pair()
    good = expected(orc, GOOD)
    for datas, want in HAND:
        assert cpython_first(datas) == want
        assert refused(a, datas) == want, datas
        # the boundary behind the ill-formed haystack's failing sequence -- or in front of it -- at byte 4096 of the buffer
        at = sum(len(d) for d in datas[:want[0] + 1])
        for seam in (at, at - len(datas[want[0]])):
            moved = [filler(BLOCK - seam)] + datas
            assert cpython_first(moved) == (want[0] + 1, want[1])
            assert refused(a, moved, with_ids=False) == (want[0] + 1, want[1]), moved[1:]
    check(a, good, GOOD)
    # a whole buffer that is valid, cut inside a sequence, is refused; cut between the sequences it is not
    assert refused(a, [b"a\xc3", b"\xa9b"]) == (0, 1)
    run(a, orc, [b"a", b"\xc3\xa9b"])


# ---- 7. rescans in the summary -------------------------------------------------------------------------------------------------------
@pytest.fixture
def small_reservoir():
    N.set_tunable(RESERVOIR[0], 4096)  # 341 records
    yield
    N.set_tunable(*RESERVOIR)


def test_rescans_count_nothing_twice(small_reservoir):
    rng = np.random.default_rng(5)
    a, orc = pair(N.MODE_ALL, ["a", "aa", "aaa", "aaaa"])
    table = "aaazé"
    datas = ["".join(table[int(i)] for i in rng.integers(0, 5, int(ln))).encode() for ln in rng.integers(0, 61, 100)]
    assert 2500 < sum(len(d) for d in datas) < 4500 and n_units_of(datas) < sum(len(d) for d in datas)
    per = expected(orc, datas)
    ws = summaries(per)
    got, sst = a.summary_batch_utf8(datas)
    assert (got == ws).all()
    assert sst["rescans"] >= 1 and sst["pieces"] > sst["rescans"] and sst["n_records"] == sum(len(b) for _, b in per) > 1000, sst
    assert sum(1 for u, b in per if len(b) and b[0, 0] != u[0, 0]) >= 10


# ---- 8. where the library scans haystack by haystack ---------------------------------------------------------------------------------
def test_fallback_dictionary_without_a_free_unit():
    kws = [np.array([i], dtype=np.uint16) for i in range(65536)]
    a, orc = pair(N.MODE_ALL, kws)
    datas = [t.encode() for t in ["ab", "é", "", "zéa", "ü" * 9, "", "a", "ÿ", "abcd", "ñ" * 70, "", "éé"]]
    per = expected(orc, datas)
    assert sum(len(b) for _, b in per) == n_units_of(datas) < sum(len(d) for d in datas)
    _, sst = check(a, per, datas)
    assert sst["pieces"] == sum(1 for d in datas if d)  # a text per haystack
    ascii_datas = [b"ab", b"", b"xyz"]
    st, _ = check(a, expected(orc, ascii_datas), ascii_datas)
    assert st.ascii == 1
    assert refused(a, [b"ab", b"", b"a\xc3", b"\xa9b"]) == (2, 1)
    check(a, per, datas, kinds=(True,))


@pytest.mark.parametrize("mode", WORDY)
def test_fallback_word_table_that_is_not_fold_consistent(mode):
    rng = np.random.default_rng(9)
    alpha = "abxyABXY ,éÉ"
    wc = word_chars_from_list("abcdxyABCDéÉ")  # X, Y are not word characters although x, y are
    kws = ["".join(alpha[int(i)] for i in rng.integers(0, 4, int(rng.integers(1, 5)))) for _ in range(24)] + ["é", "aé"]
    kws += [kws[2]]
    a, orc = Automaton(mode, kws, False, word_chars=wc), Oracle(MODES[mode], kws, False, LOWER, wc, map_flavour=True)
    assert a.info()["fold_consistent"] == 0
    datas = ["".join(alpha[int(i)] for i in rng.integers(0, len(alpha), int(ln))).encode() for ln in (0, 1, 40, 300, 7, 0, 120, 3, 12, 60, 0, 25)]
    per = expected(orc, datas)
    assert sum(len(b) for _, b in per) > 5 and any(len(b) and b[0, 0] != u[0, 0] for u, b in per)
    check(a, per, datas, kinds=(True,))
    assert refused(a, [b"ab", "é".encode()[:1], "é".encode()[1:]]) == (1, 0)
    # Set records: the *Set class's loop (WholeWordLongestMatchSet does not fold in its skip loops: other records over this table)
    per_set = expected(Oracle(MODES[mode], kws, False, LOWER, wc), datas)
    got = a.match_batch_utf8(datas, with_ids=False)
    assert got.shape == (sum(len(b) for _, b in per_set), 3) and (got == tagged(per_set)[:, :3]).all()
    check(a, per, datas, kinds=(True,))


# ---- 9. capacity ---------------------------------------------------------------------------------------------------------------------
def test_overflow_reports_the_exact_count():
    a, orc = seam_pair()
    datas = ["aé€😀kw".encode()] * 300
    want = tagged(expected(orc, datas))
    buf = np.frombuffer(b"".join(datas), np.uint8)
    off = np.cumsum([0] + [len(d) for d in datas], dtype=np.uint64)
    n_out = ctypes.c_uint64(0)

    def call(out, cap):
        return N.lib().acgpu_match_batch_utf8(a.handle, vp(buf), vp(off), len(datas), N.REC_MAP, vp(out), cap, ctypes.byref(n_out), None)
    out = np.zeros((len(want), 4), np.int32)
    assert len(want) > 1500
    assert call(out, len(want) - 1) == N.E_OVERFLOW and n_out.value == len(want)
    assert call(None, 0) == N.E_OVERFLOW and n_out.value == len(want)
    assert call(out, len(want)) == N.OK and n_out.value == len(want) and (out == want).all()
    assert (a.match_batch_utf8(datas, with_ids=True, cap=1) == want).all()  # the wrapper's retry


# ---- 10. the facade --------------------------------------------------------------------------------------------------------------------
def test_facade_against_the_utf16_counterparts_on_the_decoded_lines():
    rng = np.random.default_rng(7)
    words = ["straße", "naïve", "Zürich", "λόγος", "ΑΘΗΝΑ", "σοφία", "москва", "Привет", "мир", "data", "GPU"]
    values = ["[%d:%s]" % (i, w.upper()) for i, w in enumerate(words)]
    fill = ["und", "και", "или", "the", "x1", "東京", "😀"]

    def flip(w):
        return "".join(c.upper() if rng.integers(2) else c.lower() for c in w)

    def sentence(n):
        toks = [flip(words[int(rng.integers(len(words)))]) if rng.integers(3) == 0 else fill[int(rng.integers(len(fill)))] for _ in range(n)]
        return "".join(t + (" ", ", ", "-")[int(rng.integers(3))] for t in toks)
    lines = [sentence(int(n)) for n in rng.integers(0, 8, 300)]
    datas = [ln.encode() for ln in lines]
    m, s = WholeWordMatchMap(words, values, False), WholeWordMatchSet(words, False)
    orc = Oracle(FAM_WHOLEWORD, words, False, LOWER, WORD, map_flavour=True)
    per = expected(orc, datas)
    want = tagged(per)
    assert len(want) > 100 and (want[:, 1:3] != tagged([(u, u) for u, _ in per])[:, 1:3]).any()
    assert (m.find_all_batch_utf8(datas) == want).all() and (s.find_all_batch_utf8(datas) == want[:, :3]).all()
    # the UTF-16 counterparts on the decoded lines: the same decisions, the same values, positions in units there
    assert m.contains_batch_utf8(datas).tolist() == m.contains_batch(lines).tolist()
    counts = m.count_matches_batch_utf8(datas)
    assert counts.dtype == np.uint64 and counts.tolist() == m.count_matches_batch(lines).tolist() == [len(b) for _, b in per]
    first16 = m.first_batch(lines)
    first8 = m.first_batch_utf8(datas)
    assert [f and f[2] for f in first8] == [f and f[2] for f in first16]
    assert first8 == [(int(b[0, 0]), int(b[0, 1]), values[int(b[0, 2])]) if len(b) else None for _, b in per]
    assert s.first_batch_utf8(datas) == [f and f[:2] for f in first8]
    # listeners: the haystack's own bytes, byte offsets into them; False ends that haystack's matches
    seen16, seen8 = [], []
    m.match_batch(lines, lambda h, b, e, v: seen16.append((utf16(h)[b:e].tobytes().decode("utf-16-le"), v)) and False)
    m.match_batch_utf8(datas, lambda h, b, e, v: seen8.append((bytes(h[b:e]).decode(), v, h in datas)) and False)
    assert seen8 == [(t, v, True) for t, v in seen16] and len(seen8) == int(m.contains_batch(lines).sum())
    seen = []
    s.match_batch_utf8(datas, lambda h, b, e: seen.append(bytes(h[b:e]).decode()) or True)
    assert len(seen) == len(want)
    # one buffer in place: the lines of a log file
    buf = "\n".join(lines).encode()
    off = utf8_line_offsets(buf)
    assert len(off) - 1 == len(buf.splitlines(keepends=True))
    line_recs = expected(orc, [buf[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)])
    assert (m.find_all_batch_utf8(buf, offsets=off) == tagged(line_recs)).all()
    assert m.contains_batch_utf8(buf, offsets=off).tolist() == [len(b) > 0 for _, b in line_recs]
    assert s.count_matches_batch_utf8(bytearray(buf), offsets=off).tolist() == [len(b) for _, b in line_recs]
    assert m.first_batch_utf8(memoryview(buf), offsets=off) == [(int(b[0, 0]), int(b[0, 1]), values[int(b[0, 2])]) if len(b) else None
                                                                 for _, b in line_recs]
    with pytest.raises(Utf8Error) as e:
        s.contains_batch_utf8([b"ok", b"gr\xc3", b"\xbc"])
    assert (e.value.haystack, e.value.start) == (1, 2)
    # the mid-pair rule, relative to the haystack
    assert AhoCorasickSet(["\ud83d", "\ude00"], True).find_all_batch_utf8([b"xy", "a😀b".encode()]).tolist() == [[1, 1, 5], [1, 1, 5]]
    mm = AhoCorasickMap(["\ud83d", "\ude00", "😀b"], ["hi", "lo", "both"], True)
    assert mm.find_all_batch_utf8(["é".encode(), "a😀b".encode()]).tolist() == [[1, 1, 5, 0], [1, 1, 5, 1], [1, 1, 6, 2]]
    assert LongestMatchMap(["é"], ["v"], True).first_batch_utf8(["aé".encode(), b""]) == [(1, 3, "v"), None]
