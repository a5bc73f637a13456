"""GPU tests of stream replace in UTF-16 units (include/acgpu.h: acgpu_stream_replace_u16; csrc/acgpu_stream.hip, and in
csrc/acgpu_replace.hip the pieces driven over a feed's owned range).  The expected text is the splice of the CPU oracle's records
for the WHOLE text (tests/helpers.py: splice), whatever the chunking; equality is exact."""
import ctypes
import io

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import (Automaton, LongestMatchMap, LongestMatchSet, ShortestMatchSet, Stream, WholeWordMatchMap, utf16)
from oracle.oracle import FAM_LONGEST, FAM_SHORTEST, FAM_WHOLEWORD, FAM_WWLONGEST, Oracle
from tests.helpers import LOWER, WORD, rand_case, splice

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20),
            ("replace_slab_units", 1 << 25)]
MODES = {N.MODE_LONGEST: FAM_LONGEST, N.MODE_WHOLEWORD: FAM_WHOLEWORD, N.MODE_SHORTEST: FAM_SHORTEST, N.MODE_WWLONGEST: FAM_WWLONGEST}
WORDY = (N.MODE_WHOLEWORD, N.MODE_WWLONGEST)
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def small_pieces():
    for k, v in (("cursor_first_piece", 64), ("cursor_max_piece", 256), ("cursor_reservoir_bytes", 4096), ("replace_slab_units", 1000)):
        N.set_tunable(k, v)


def pair(mode, kws, cs=True, wc=None):
    if wc is None and mode in WORDY:
        wc = WORD
    return (Automaton(mode, kws, cs, word_chars=wc),
            Oracle(MODES[mode], kws, case_sensitive=cs, lower=None if cs else LOWER, word_chars=wc, map_flavour=True))


def four_sets(kws):
    kws = [utf16(k) if k is not None else np.zeros(0, np.uint16) for k in kws]
    return {"longer": [np.concatenate([k, utf16("<+>")]) for k in kws], "shorter": [k[:len(k) // 2] for k in kws],
            "empty": ["" for _ in kws], "same": [np.full(len(k), ord("#"), np.uint16) for k in kws]}


def split(hay, cuts):
    edges = [0] + [int(c) for c in cuts] + [len(hay)]
    return [hay[edges[i]:edges[i + 1]] for i in range(len(edges) - 1)]


def feed_all(a, chunks, repls, final_in_last):
    """the chunks through one replace stream -> (the whole output, [(units fed so far, units delivered so far, stats dict) per feed])"""
    s = Stream(a)
    st = N.ReplaceStats()
    parts, log, fed = [], [], 0
    feeds = [(c, final_in_last and i == len(chunks) - 1) for i, c in enumerate(chunks)]
    if not final_in_last:
        feeds.append((np.zeros(0, np.uint16), True))
    try:
        for c, final in feeds:
            parts.append(s.replace_feed(c, repls, final=final, stats=st))
            fed += len(c)
            assert st.units_out == parts[-1].size
            log.append((fed, sum(p.size for p in parts), {f: int(getattr(st, f)) for f, _ in N.ReplaceStats._fields_}))
    finally:
        s.close()
    return np.concatenate(parts), log


def same(got, want, what):
    assert got.dtype == np.uint16 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert not len(bad), (what, bad[:5], got[bad[:5]], want[bad[:5]])


# ---- 1. parity over chunkings ------------------------------------------------------------------------------------------------
def parity_case(mode, cs):
    rng = np.random.default_rng(1800 + 10 * mode + cs)
    word = mode in WORDY
    kw_alpha = [ord(c) for c in ("abAB" if word or not cs else "abc")]
    hay_alpha = kw_alpha + ([32, 32, 32, 45] if word else [ord("d")])
    _, kws = rand_case(rng, kw_alpha, 60, 12, 0)
    kws += [kws[3].copy(), np.zeros(0, np.uint16)]
    hay = np.asarray(hay_alpha, np.uint16)[rng.integers(0, len(hay_alpha), 20011)]
    for at in range(30, hay.size - 20, 97):  # the long keywords too, as words of their own where words count
        k = kws[int(rng.integers(len(kws)))]
        hay[at:at + k.size] = k
        if word:
            hay[at - 1] = hay[at + k.size] = 32
    return kws, hay


@pytest.mark.parametrize("cs", [True, False])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_parity_over_chunkings(mode, cs):
    rng = np.random.default_rng(1900 + 10 * mode + cs)
    kws, hay = parity_case(mode, cs)
    a, orc = pair(mode, kws, cs)
    recs = orc.match(hay, cap=hay.size * 2)
    lens = recs[:, 1] - recs[:, 0]
    assert len(recs) > 500 and lens.min() == 1 and max(len(k) for k in kws) == 12
    assert lens.max() == 12 or mode == N.MODE_SHORTEST  # (a one-unit keyword ends every longer one's match)
    sets = dict(four_sets(kws), one="[*]")
    wants = {name: splice(hay, recs, r) for name, r in sets.items()}
    for name, r in sets.items():  # the whole text in one call says the same
        same(a.replace_host(hay, r)[0], wants[name], ("replace_host", name))
    n, s0 = hay.size, 7000
    few = [("no cut", [hay]), ("one cut", split(hay, [n // 2 + 1])), ("twelve cuts", split(hay, sorted(set(rng.integers(1, n, 12).tolist()))))]
    many = [("one-unit chunks", split(hay, range(s0, s0 + 301))),
            ("empty chunks", [hay[:0], hay[:s0 + 1], hay[:0], hay[:0], hay[s0 + 1:s0 + 2], hay[:0], hay[s0 + 2:], hay[:0]]),
            ("chunks shorter than the keywords", split(hay, range(s0, s0 + 601, 2)))]
    many += [("cut at %d" % c, split(hay, [c])) for c in range(s0, s0 + 300)]
    names = sorted(sets)
    runs = [(what, chunks, name) for what, chunks in few for name in names]
    runs += [(what, chunks, names[i % len(names)]) for i, (what, chunks) in enumerate(many)]  # (every set at every kind of seam)
    for i, (what, chunks, name) in enumerate(runs):
        assert sum(len(c) for c in chunks) == n
        got, log = feed_all(a, chunks, sets[name], final_in_last=i % 2 == 0)
        same(got, wants[name], (what, name))
        assert sum(st["n_records"] for _, _, st in log) == len(recs), (what, name)


# ---- 2. a match longer than several chunks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [N.MODE_LONGEST, N.MODE_WHOLEWORD])
def test_a_match_longer_than_several_chunks(mode):
    rng = np.random.default_rng(2)
    long_kw = "".join("abAB"[int(i)] for i in rng.integers(0, 4, 40))
    kws = [long_kw, "ab", "b", long_kw[:17]]
    repls = ["<" + "=" * 23 + ">", "(1)", "", "<17>"]
    text = "zz ab " + long_kw + " b " + long_kw + " " + long_kw[:17] + " zab " + long_kw + " " + long_kw[:39] + " ab"
    hay = utf16(text)
    a, orc = pair(mode, kws)
    recs = orc.match(hay)
    whole = recs[recs[:, 2] == 0]
    assert len(whole) == 3 and ((whole[:, 1] - whole[:, 0]) == 40).all()
    want = splice(hay, recs, repls)
    for first in range(1, 8):  # every phase of the 7-unit chunks against the matches
        chunks = split(hay, range(first, hay.size, 7))
        assert max(len(c) for c in chunks) == 7
        got, log = feed_all(a, chunks, repls, final_in_last=first % 2 == 0)
        same(got, want, first)
        # where each 40-unit match's replacement lies in the output: no feed ends inside it, and the feed that delivers it comes
        # when the match's last unit has been fed -- so neither half a replacement nor a part of the match's text was delivered
        ends = [delivered for _, delivered, _ in log]
        for s, e, k in whole.tolist():
            p0 = splice(hay[:s], recs[recs[:, 1] <= s], repls).size
            p1 = p0 + len(repls[0])
            assert not any(p0 < d < p1 for d in ends), (first, s, ends)
            assert all(delivered <= p0 for fed, delivered, _ in log if fed < e), (first, s)
        assert sum(st["n_records"] for _, _, st in log) == len(recs)


# ---- 3. many pieces inside one feed ------------------------------------------------------------------------------------------------
def test_many_pieces_inside_one_feed():
    """Pieces of 64 .. 256 units, a reservoir of 4096 bytes (341 Map records) and slabs of 1000 units: every feed is many pieces.
    With those figures no piece can overflow the reservoir -- the records of these families do not overlap, so 256 owned units
    hold at most 256 of them -- and a rescan is therefore provoked by a second run with pieces of up to 4096 units, the figures of
    tests/test_gpu_replace.py::test_piece_halo_and_slab_seams: the text begins with a stretch without matches, over which the
    ramp reaches its largest piece before it knows a density."""
    rng = np.random.default_rng(3)
    _, kws = rand_case(rng, [ord(c) for c in "abc"], 50, 9, 0)
    hay = np.asarray([ord(c) for c in "abcd"], np.uint16)[rng.integers(0, 4, 50000)]
    hay[:1500] = ord("z")
    repls = [utf16("<" + "=" * (i % 6) + ">") if i % 3 else np.zeros(0, np.uint16) for i in range(len(kws))]
    a, orc = pair(N.MODE_LONGEST, kws)
    recs = orc.match(hay, cap=hay.size * 2)
    assert len(recs) > 0.1 * hay.size
    want = splice(hay, recs, repls)
    small_pieces()
    got, log = feed_all(a, split(hay, [16001, 33000]), repls, final_in_last=True)
    same(got, want, "three feeds")
    assert all(st["pieces"] > 10 for _, _, st in log), log
    assert sum(st["n_records"] for _, _, st in log) == len(recs)
    N.set_tunable("cursor_max_piece", 4096)
    a = Automaton(N.MODE_LONGEST, kws, True)  # (a pool whose reservoir has not grown yet)
    got, log = feed_all(a, split(hay, [16001, 33000]), repls, final_in_last=False)
    same(got, want, "three feeds, larger pieces")
    assert all(st["pieces"] > 1 for _, _, st in log[:3]) and sum(st["rescans"] for _, _, st in log) >= 1, log
    assert sum(st["n_records"] for _, _, st in log) == len(recs)


# ---- 4. overflow ---------------------------------------------------------------------------------------------------------------------
def test_overflow_commits_nothing():
    rng = np.random.default_rng(4)
    _, kws = rand_case(rng, [ord(c) for c in "abc"], 30, 6, 0)
    hay = np.asarray([ord(c) for c in "abcd"], np.uint16)[rng.integers(0, 4, 9000)]
    sets = four_sets(kws)
    a, orc = pair(N.MODE_LONGEST, kws)
    chunks = split(hay, [3000, 6001])
    for name in ("longer", "shorter"):
        repls = sets[name]
        want = splice(hay, orc.match(hay, cap=hay.size), repls)
        plain, log = feed_all(a, chunks, repls, final_in_last=True)
        same(plain, want, name)
        units, off, n_repl = a._replacements(repls)
        h = ctypes.c_void_p()
        assert N.lib().acgpu_stream_open(a.handle, ctypes.byref(h)) == N.OK
        parts = []
        try:
            for i, c in enumerate(chunks):
                need = log[i][1] - (log[i - 1][1] if i else 0)  # what this feed delivers in the uninterrupted run
                for cap in ([0, need - 1, need] if i == 1 else [need]):
                    out = np.full(need + 64, 0x5A5A, np.uint16)
                    n_out, st = ctypes.c_uint64(0), N.ReplaceStats()
                    rc = N.lib().acgpu_stream_replace_u16(h, vp(c), c.size, 1 if i == 2 else 0, vp(units), vp(off), n_repl, vp(out) if cap else None,
                                                          cap, ctypes.byref(n_out), ctypes.byref(st))
                    assert rc == (N.OK if cap == need else N.E_OVERFLOW), (name, i, cap, rc)
                    assert n_out.value == need and st.units_out == need, (name, i, cap, n_out.value, need)
                    assert (out[cap:] == 0x5A5A).all(), "written at or beyond cap"
                parts.append(out[:need])
        finally:
            N.lib().acgpu_stream_close(h)
        same(np.concatenate(parts), want, (name, "after the overflows"))


# ---- 5. latency bound -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_without_matches_a_feed_withholds_at_most_max_len_plus_one_units(mode):
    rng = np.random.default_rng(5 + mode)
    kws = ["ab", "abbab", "b", "babababa"]
    max_len = 8
    hay = np.asarray([ord(c) for c in "xyz ,"], np.uint16)[rng.integers(0, 5, 5000)]
    a, orc = pair(mode, kws)
    assert len(orc.match(hay)) == 0 and a.info()["max_keyword_len"] == max_len
    cuts = sorted(set(rng.integers(1, hay.size, 30).tolist()) | set(range(2000, 2040)) | {2050, 2059, 2069})
    got, log = feed_all(a, split(hay, cuts), "#", final_in_last=False)
    same(got, hay, "no match, no change")
    for fed, delivered, st in log[:-1]:
        assert fed - (max_len + 1) <= delivered <= fed, (fed, delivered)
    assert log[-1][1] == hay.size


# ---- 6. interleaving ----------------------------------------------------------------------------------------------------------------------
def test_other_calls_between_the_feeds_of_a_stream():
    rng = np.random.default_rng(6)
    _, kws = rand_case(rng, [ord(c) for c in "abc"], 30, 6, 0)
    alpha = np.asarray([ord(c) for c in "abcd"], np.uint16)
    hay, other, third = (alpha[rng.integers(0, 4, n)] for n in (12000, 7000, 5000))
    sets = four_sets(kws)
    a, orc = pair(N.MODE_LONGEST, kws)
    recs = orc.match(hay, cap=hay.size)
    recs3 = orc.match(third, cap=third.size)
    s1, s2 = Stream(a), Stream(a)
    p1, p2, between = [], [], []
    try:
        c1, c2 = split(hay, range(1000, hay.size, 1000)), split(other, range(600, other.size, 600))
        assert len(c1) == len(c2) == 12
        for i in range(12):
            p1.append(s1.replace_feed(c1[i], sets["longer"], final=i == 11))
            between.append(a.replace_host(third, sets["same"])[0])
            p2.append(s2.replace_feed(c2[i], sets["empty"], final=i == 11))
            got = a.match_host(third, with_ids=True)
            assert got.shape == recs3.shape and (got == recs3).all()
    finally:
        s1.close()
        s2.close()
    same(np.concatenate(p1), splice(hay, recs, sets["longer"]), "the stream")
    same(np.concatenate(p2), splice(other, orc.match(other, cap=other.size), sets["empty"]), "the second stream")
    want3 = splice(third, recs3, sets["same"])
    for b in between:
        same(b, want3, "replace_host between the feeds")


# ---- 7. a word table that is not fold-consistent ---------------------------------------------------------------------------------------------
def test_word_table_that_is_not_fold_consistent_follows_the_readable_loops():
    """the tables and dictionaries of test_gpu_parity.py::test_stream_fold_inconsistent_wholeword_folds_in_every_lookup: the stream
    rewrites by the records of match(Readable), which folds in every lookup, not by those of match(String)"""
    rng = np.random.default_rng(91)
    alpha = np.array([ord(c) for c in "abxyABXY ,."], dtype=np.uint16)
    differ = 0
    for wchars in ("ABXYxy", "abxyAB"):
        wc = np.zeros(65536, np.uint8)
        for ch in wchars:
            wc[ord(ch)] = 1
        for it in range(12):
            pool = [ord(c) for c in wchars]
            kws = [np.array([pool[int(j)] for j in rng.integers(0, len(pool), int(rng.integers(1, 5)))], dtype=np.uint16) for _ in range(10)]
            hay = alpha[rng.integers(0, len(alpha), int(rng.integers(1, 4000)))]
            a = Automaton(N.MODE_WHOLEWORD, kws, False, word_chars=wc)
            assert a.info()["fold_consistent"] == 0
            orc = Oracle(FAM_WHOLEWORD, kws, case_sensitive=False, lower=LOWER, word_chars=wc)
            recs = orc.match_readable(hay, 7, positions=True)
            repls = ["<%d>" % i for i in range(len(kws))]
            want = splice(hay, recs, repls)
            want_string = splice(hay, orc.match(hay), repls)
            differ += want.size != want_string.size or bool((want != want_string).any())
            for cuts in ([], [hay.size // 2], sorted(set(rng.integers(0, hay.size, 6).tolist())), list(range(1, min(hay.size, 40), 3))):
                got, log = feed_all(a, split(hay, cuts), repls, final_in_last=len(cuts) % 2 == 0)
                same(got, want, (wchars, it, list(cuts)[:4]))
                assert sum(st["n_records"] for _, _, st in log) == len(recs)
    assert differ >= 1  # (the test tells the two loops apart)


# ---- 8. the facade -------------------------------------------------------------------------------------------------------------------------
def test_replace_readable_of_a_set_and_a_map():
    rng = np.random.default_rng(8)
    words = ["he", "she", "hers", "ü", "€5", "😀", "ü😀", "s"]
    values = ["[%d]" % i for i in range(len(words))]
    text = "".join(("she said: ünï €5 and 😀 ushers, ü😀 hers. ", "😀😀 x ", "his ")[int(i)] for i in rng.integers(0, 3, 400))
    s, m = LongestMatchSet(words, True), LongestMatchMap(words, values, True)
    for chunk_chars in (1, 7, 1000, 1 << 22):
        parts = list(s.replace_readable(io.StringIO(text), "***", chunk_chars=chunk_chars))
        assert all(isinstance(p, str) for p in parts) and "".join(parts) == s.replace(text, "***")
        assert "".join(m.replace_readable(io.StringIO(text), chunk_chars=chunk_chars)) == m.replace(text)
    assert "".join(m.replace_readable(iter([text[:11], text[11:12], utf16(text[12:])]), "")) == m.replace(text, "")
    assert "".join(ShortestMatchSet(words, True).replace_readable([text], "_")) == ShortestMatchSet(words, True).replace(text, "_")
    w = WholeWordMatchMap(["she", "hers"], ["SHE", "HERS"], False)
    assert "".join(w.replace_readable(io.StringIO(text), chunk_chars=5)) == w.replace(text)
    # units that split a pair: the str pieces still join to the text
    units = utf16(text)
    assert "".join(s.replace_readable(split(units, range(1, 400)), "***")) == s.replace(text, "***")
    # closing the generator early closes the stream and leaves the automaton usable
    g = s.replace_readable(io.StringIO(text), "***", chunk_chars=50)
    first = next(g)
    assert s.replace(text, "***").startswith(first)
    g.close()
    assert s.replace(text, "***") == "".join(s.replace_readable([text], "***"))
