"""GPU tests of the batch replace entry (include/acgpu.h: acgpu_replace_batch_u16; csrc/acgpu_replace.hip: k_replace_merge,
k_replace_batch_offsets over the plan and the emit of the replace calls).  Every expected text is the Python splice of the CPU
oracle's records, haystack by haystack: hay[e_{-1}:s_0] + repl[id_0] + hay[e_0:s_1] + ... + hay[e_{k-1}:n]."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, WholeWordMatchMap, _pack, _to_str, utf16
from ahocorasick_amd.unicode_tables import word_chars_from_list
from oracle.oracle import FAM_LONGEST, FAM_SHORTEST, FAM_WHOLEWORD, FAM_WWLONGEST, Oracle
from tests.helpers import LOWER, WORD, splice

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("replace_slab_units", 1 << 25)]
MODES = {N.MODE_LONGEST: FAM_LONGEST, N.MODE_WHOLEWORD: FAM_WHOLEWORD, N.MODE_SHORTEST: FAM_SHORTEST, N.MODE_WWLONGEST: FAM_WWLONGEST}
WORDY = (N.MODE_WHOLEWORD, N.MODE_WWLONGEST)
CANARY = 0x5A5A
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def oracle_records(orc, hays):
    """the oracle's records of every haystack alone: computed once per case, shared by its replacement sets"""
    return [orc.match(h, cap=max(64, 2 * len(h))) for h in hays]


def expected(hays, recs, repls):
    """-> (units, out_offsets, n_records)"""
    parts = [splice(h, r, repls) for h, r in zip(hays, recs)]
    off = np.zeros(len(parts) + 1, np.uint64)
    off[1:] = np.cumsum([p.size for p in parts], dtype=np.uint64)
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint16)), off, sum(len(r) for r in recs)


def check(a, hays, recs, repls):
    """Automaton.replace_batch against the oracle splice -> (the expected units, offsets, the call's stats)"""
    want, off, n_rec = expected(hays, recs, repls)
    got, got_off, st = a.replace_batch(hays, repls)
    assert got_off.tolist() == off.tolist()
    assert got.shape == want.shape and (got == want).all()
    assert st["n_records"] == n_rec and st["units_out"] == want.size, st
    return want, off, st


def pair(mode, kws, cs=True, wc=None, map_flavour=False):
    if wc is None and mode in WORDY:
        wc = WORD
    return (Automaton(mode, kws, cs, word_chars=wc),
            Oracle(MODES[mode], kws, case_sensitive=cs, lower=None if cs else LOWER, word_chars=wc, map_flavour=map_flavour))


def five_sets(kws):
    kws = [utf16(k) for k in kws]
    return {"longer": [np.concatenate([k, utf16("<+>")]) for k in kws], "shorter": [k[:len(k) // 2] for k in kws],
            "empty": ["" for _ in kws], "same": [np.full(len(k), ord("#"), np.uint16) for k in kws], "single": "<*>"}


def family_case(mode):
    """keywords and the alphabet of the random haystacks; the word matchers' texts have two non-word units"""
    if mode == N.MODE_WWLONGEST:  # " " and ", " have no word character: kept as they are, the root has a transition on them
        return ["ab", "ab cd", " ", "c", ", ", "abcd a", "ab"], "abcd ,"
    if mode == N.MODE_WHOLEWORD:
        return ["ab", "abc", "c", "dd", "abcda", "ab"], "abcd ,"
    return ["ab", "abc", "c", "bcd", "dd", "abcdab", "ab"], "abcdz"


# ---- 1. four families at the seams between haystacks --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_four_families_at_the_seams(mode):
    kws, alpha = family_case(mode)
    rng = np.random.default_rng(100 + mode)
    a, orc = pair(mode, kws)
    word = mode in WORDY
    hays = ["", "zz zz" if word else "zzzz", "ab",          # empty, no match, one that is a single match
            "ab zz c" if word else "abzzc",                   # a match as first units and one as last units
            "xa", "by", "ab", "c", "ab", "cd", "",            # joins that spell "ab", "abc", "ab cd": no match across
            " ab", "  ab", ", c", " ", ",", "", "", "d, "]    # WholeWordLongest: a haystack's first unit is a walk start
    table = utf16(alpha)
    hays += [table[rng.integers(0, len(table), int(ln))] for ln in rng.integers(0, 41, 30)]
    recs = oracle_records(orc, hays)
    assert len(recs[0]) == 0 and len(recs[1]) == 0 and recs[2].tolist()[0][:2] == [0, 2] and len(recs[2]) == 1
    assert recs[3][0, 0] == 0 and recs[3][-1, 1] == len(hays[3]) and len(recs[4]) == 0 and len(recs[5]) == 0
    if mode == N.MODE_WWLONGEST:
        # the walk from a first space swallows the word behind it (in a text, "ab" behind a space is reported: recs[3]), or
        # reports the keyword " "
        assert recs[11].tolist() == [] and recs[12].tolist() == [[0, 1, 2], [2, 4, 6]]
    for label, repls in five_sets(kws).items():
        check(a, hays, recs, repls)
    # one haystack, one empty haystack: the smallest batches
    check(a, hays[3:4], recs[3:4], "#")
    check(a, hays[:1], recs[:1], "#")


# ---- 2. separators dense enough to leave LDS ----------------------------------------------------------------------------------
def test_more_separators_in_an_emit_tile_than_lds_holds():
    """8000 haystacks of 0 or 1 units and deleting replacements: well over 3072 segments in the one 2048-unit tile of the output"""
    rng = np.random.default_rng(21)
    a, orc = pair(N.MODE_LONGEST, ["a", "b"])
    table = utf16("abz")
    hays = [table[rng.integers(0, 3, int(ln))] for ln in rng.integers(0, 2, 8000)]
    recs = oracle_records(orc, hays)
    want, off, st = check(a, hays, recs, ["", ""])
    assert 0 < want.size < 2048 and (want == ord("z")).all() and st["n_records"] + len(hays) > 3072
    check(a, hays, recs, "")


def test_plan_workgroups_of_mixed_records_and_separators():
    rng = np.random.default_rng(22)
    a, orc = pair(N.MODE_LONGEST, ["a", "bb", "c"])
    table = utf16("abcz")
    hays = [table[rng.integers(0, 4, int(ln))] for ln in rng.integers(1, 4, 5000)]
    recs = oracle_records(orc, hays)
    want, off, st = check(a, hays, recs, ["<aaaa>", "<bbbbbbbbbbbbbbbbb>", "c2"])
    assert st["n_records"] > 2048 and want.size > 4 * sum(len(h) for h in hays) // 2


# ---- 3. pieces ------------------------------------------------------------------------------------------------------------------
PIECE = 4096


def piece_lengths(rng):
    """Haystack lengths, 60 000 units in all.  With pieces of 4096 units of the concatenation (a separator behind every haystack):
    piece ends inside a 10 000-unit haystack; a separator AT a piece end (the next piece's first unit); a separator as a piece's
    last unit (the haystack behind it starts exactly at a piece start); a separator 3 units in front of a piece end -- within
    max_len - 1 of it for Shortest -- and empty haystacks around that end."""
    lens, pos = [], 0  # pos: the concatenation's units so far

    def add(ln):
        nonlocal pos
        lens.append(int(ln))
        pos += int(ln) + 1

    def separator_at(target):
        while target - pos > 130:
            add(rng.integers(20, 61))
        rest = target - pos  # two haystacks: l1 + 1 + l2 == rest
        add(rest // 2)
        add(target - pos)
        assert pos - 1 == target

    marks = {}
    add(10000)
    separator_at(3 * PIECE)
    marks["sep_at_piece_end"] = len(lens) - 1
    separator_at(4 * PIECE - 1)
    marks["starts_at_piece_start"] = len(lens)  # the next haystack
    separator_at(5 * PIECE - 3)
    for _ in range(4):
        add(0)  # separators at 5 * PIECE - 2 .. + 1
    add(10000)
    add(0)
    add(10000)
    while sum(lens) < 60000 - 130:
        add(rng.integers(20, 61))
    add(60000 - sum(lens))
    assert sum(lens) == 60000
    return lens, marks


@pytest.mark.parametrize("mode", sorted(MODES))
def test_pieces(mode):
    kws, alpha = family_case(mode)
    rng = np.random.default_rng(300 + mode)
    lens, marks = piece_lengths(rng)
    table = utf16(alpha)
    hays = [table[rng.integers(0, len(table), ln)] for ln in lens]
    first = marks["starts_at_piece_start"]
    starts = np.concatenate([[0], np.cumsum([ln + 1 for ln in lens])])
    assert starts[first] == 4 * PIECE and starts[marks["sep_at_piece_end"] + 1] - 1 == 3 * PIECE
    assert max(len(k) for k in kws) - 1 >= 3  # (Shortest: the separator at 5 * PIECE - 3 lies in the units a piece withholds)
    hays[first][:4] = utf16({N.MODE_WWLONGEST: "  ab", N.MODE_WHOLEWORD: "abc "}.get(mode, "abcz"))  # ("  ab": the keyword " " only where a walk starts)
    a, orc = pair(mode, kws)
    recs = oracle_records(orc, hays)
    assert len(recs[first]) and recs[first][0, 0] == 0
    repls = five_sets(kws)
    N.set_tunable("cursor_first_piece", PIECE)
    N.set_tunable("cursor_max_piece", PIECE)
    for label in ("longer", "empty", "single"):
        want, off, st = check(a, hays, recs, repls[label])
        assert st["pieces"] > 1, st
    N.set_tunable("replace_slab_units", 1000)
    check(a, hays, recs, repls["shorter"])


# ---- 4. overflow and the canary -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slab", [8, 1024, 1 << 25])
def test_overflow_keeps_every_offset_exact_and_the_canary(slab):
    rng = np.random.default_rng(41)
    kws, alpha = family_case(N.MODE_LONGEST)
    a, orc = pair(N.MODE_LONGEST, kws)
    table = utf16(alpha)
    hays = [table[rng.integers(0, len(table), int(ln))] for ln in rng.integers(0, 41, 200)]
    recs = oracle_records(orc, hays)
    repls = five_sets(kws)["longer"]
    want, off, n_rec = expected(hays, recs, repls)
    need = int(want.size)
    inside = next(int(off[i]) + 1 for i in range(50, 200) if off[i + 1] - off[i] > 2)
    N.set_tunable("replace_slab_units", slab)
    units, h_off = _pack(hays)
    r_units, r_off, n_repl = a._replacements(repls)
    for cap, rc_want in ((0, N.E_OVERFLOW), (need - 1, N.E_OVERFLOW), (inside, N.E_OVERFLOW), (int(off[120]), N.E_OVERFLOW), (need, N.OK)):
        out = np.full(need + 64, CANARY, np.uint16)
        oo = np.full(len(hays) + 1, 99, np.uint64)
        n_out, st = ctypes.c_uint64(0), N.ReplaceStats()
        rc = N.lib().acgpu_replace_batch_u16(a.handle, vp(units), vp(h_off), len(hays), vp(r_units), vp(r_off), n_repl, vp(out) if cap else None,
                                             cap, vp(oo), ctypes.byref(n_out), ctypes.byref(st))
        assert rc == rc_want and n_out.value == need and st.units_out == need and st.n_records == n_rec, (cap, rc)
        assert oo.tolist() == off.tolist(), cap
        assert (out[cap:] == CANARY).all(), cap
        if rc == N.OK:
            assert (out[:need] == want).all()
    got, got_off, st = a.replace_batch(hays, repls, cap=16)  # the wrapper's one retry
    assert (got == want).all() and got_off.tolist() == off.tolist()


# ---- 5. where the library makes one call per haystack ---------------------------------------------------------------------------
def test_fallback_dictionary_without_a_free_unit():
    kws = [np.array([i], dtype=np.uint16) for i in range(65536)]
    a, orc = pair(N.MODE_LONGEST, kws)
    hays = [np.array(h, np.uint16) for h in ([5, 6], [7], [], [65535, 0, 1], [300] * 9)]
    recs = oracle_records(orc, hays)
    assert sum(len(r) for r in recs) == sum(len(h) for h in hays)
    check(a, hays, recs, "<#>")
    check(a, hays, recs, [np.array([i ^ 1] * (i % 3), np.uint16) for i in range(65536)])
    want, off, _ = expected(hays, recs, "<#>")
    units, h_off = _pack(hays)
    r_units, r_off, n_repl = a._replacements("<#>")
    for cap in (0, int(off[1]), int(off[1]) + 1):  # overflow through the calls per haystack: exact offsets, nothing behind cap
        out = np.full(int(want.size) + 8, CANARY, np.uint16)
        oo = np.zeros(len(hays) + 1, np.uint64)
        n_out = ctypes.c_uint64(0)
        rc = N.lib().acgpu_replace_batch_u16(a.handle, vp(units), vp(h_off), len(hays), vp(r_units), vp(r_off), n_repl, vp(out), cap, vp(oo),
                                             ctypes.byref(n_out), None)
        assert rc == N.E_OVERFLOW and n_out.value == want.size and oo.tolist() == off.tolist() and (out[cap:] == CANARY).all()


def test_fallback_word_table_that_is_not_fold_consistent():
    rng = np.random.default_rng(9)
    alpha = np.array([ord(ch) for ch in "abxyABXY ,"], dtype=np.uint16)
    wc = word_chars_from_list("abcdxyABCD")  # X, Y are not word characters although x, y are
    kws = [alpha[rng.integers(0, 4, int(rng.integers(1, 5)))] for _ in range(12)]
    kws += [kws[2].copy()]
    a, orc = pair(N.MODE_WHOLEWORD, kws, cs=False, wc=wc, map_flavour=True)
    assert a.info()["fold_consistent"] == 0
    hays = [alpha[rng.integers(0, len(alpha), int(ln))] for ln in (0, 1, 40, 300, 7, 0, 120)]
    recs = oracle_records(orc, hays)
    assert sum(len(r) for r in recs) > 5
    check(a, hays, recs, ["<%d>" % i for i in range(len(kws))])


# ---- 6. case folding through the facade -----------------------------------------------------------------------------------------
def test_case_insensitive_map_through_the_facade():
    rng = np.random.default_rng(6)
    words = ["straße", "naïve", "Zürich", "λόγος", "ΑΘΗΝΑ", "σοφία", "москва", "Привет", "мир", "data", "GPU"]
    values = ["[%d:%s]" % (i, w.upper()) for i, w in enumerate(words)]
    filler = ["und", "και", "или", "the", "x1"]

    def flip(w):
        return "".join(c.upper() if rng.integers(2) else c.lower() for c in w)

    def sentence(n):
        toks = [flip(words[int(rng.integers(len(words)))]) if rng.integers(3) else filler[int(rng.integers(len(filler)))] for _ in range(n)]
        return "".join(t + (" ", ", ", "-")[int(rng.integers(3))] for t in toks)
    hays = [sentence(int(n)) for n in rng.integers(0, 12, 150)]
    orc = Oracle(FAM_WHOLEWORD, words, case_sensitive=False, lower=LOWER, word_chars=WORD)
    recs = oracle_records(orc, hays)
    assert sum(len(r) for r in recs) > 100
    m = WholeWordMatchMap(words, values, False)
    assert m.replace_batch(hays) == [_to_str(splice(h, r, values)) for h, r in zip(hays, recs)]
    assert m.replace_batch(hays, "") == [_to_str(splice(h, r, "")) for h, r in zip(hays, recs)]
