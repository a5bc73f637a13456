"""GPU tests of the match cursor (include/acgpu.h: acgpu_cursor_*): one match(String) call handed out in pages and scanned
piece by piece.  The pages, concatenated, must be what acgpu_match_u16 returns (and the oracle) for every family, record kind,
page size and piece size; the scan must stop where the pages taken stop; a text with more records than a Java int[] holds must
drain page by page."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd import synth
from ahocorasick_amd.strings import Automaton, Cursor, utf16
from ahocorasick_amd.unicode_tables import word_chars_from_list
from oracle.oracle import FAM_AC, FAM_LONGEST, FAM_SHORTEST, FAM_WHOLEWORD, FAM_WWLONGEST, Oracle
from tests.helpers import LOWER, WORD, rand_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20), ("all_form", 0),
            ("count_form", 0)]
MODES = {N.MODE_ALL: FAM_AC, N.MODE_LONGEST: FAM_LONGEST, N.MODE_WHOLEWORD: FAM_WHOLEWORD, N.MODE_SHORTEST: FAM_SHORTEST,
         N.MODE_WWLONGEST: FAM_WWLONGEST}


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def pieces(first, largest=None):
    N.set_tunable("cursor_first_piece", first)
    N.set_tunable("cursor_max_piece", largest or first)


def drain(auto, hay, ids, cap):
    """every page of a cursor, concatenated, and its final stats"""
    with Cursor(auto, hay, ids) as c:
        pages = []
        while True:
            p = c.next(cap)
            assert len(p) <= cap
            if not len(p):
                break
            pages.append(p)
        st = c.stats()
        assert len(c.next(cap)) == 0  # (done stays done)
    assert st["done"] == 1 and st["records_buffered"] == 0
    return (np.concatenate(pages) if pages else np.zeros((0, 3 if ids else 2), np.int32)), st


def _case(mode, cs, seed, n):
    """(automaton, oracle, haystack, max_len) over a small alphabet: overlaps, prefixes, fail chains"""
    rng = np.random.default_rng(seed)
    word = mode in (N.MODE_WHOLEWORD, N.MODE_WWLONGEST)
    kw_alpha = [ord(c) for c in "abAB"] if word else [ord(c) for c in "abcA"]
    hay_alpha = kw_alpha + [32, 32, 45] if word else kw_alpha
    _, kws = rand_case(rng, kw_alpha, 60, 7 if word else 12, 0)
    if mode == N.MODE_WWLONGEST:
        kws += [np.concatenate([kws[i], np.array([32], np.uint16), kws[i + 1]]) for i in range(0, 20, 2)]
    hay = np.asarray(hay_alpha, np.uint16)[rng.integers(0, len(hay_alpha), n)]
    wc = WORD if word else None
    auto = Automaton(mode, kws, cs, word_chars=wc)
    orc = Oracle(MODES[mode], kws, case_sensitive=cs, lower=None if cs else LOWER, word_chars=wc)
    return auto, orc, hay, max(len(k) for k in kws)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("cs", [True, False])
def test_pages_equal_match_u16_and_the_oracle(mode, cs):
    """All five families x Set / Map x case-sensitive / not, pieces of 1000-3000 units, page caps 1 .. 2^20."""
    auto, orc, hay, ml = _case(mode, cs, 100 + mode * 2 + cs, (1 << 16) + 123)
    want = orc.match(hay, cap=hay.size * 16)
    assert len(want) > 500
    for ids in (True, False):
        ref = auto.match_host(hay, ids)
        assert (ref == (want if ids else want[:, :2])).all()
        for first, largest in ((1000, 3000), (1777, 1777)):
            pieces(first, largest)
            for cap in (ml, 4096, 1 << 20):
                got, st = drain(auto, hay, ids, cap)
                assert got.shape == ref.shape and (got == ref).all(), (ids, first, cap)
                assert st["pieces"] >= hay.size // largest and st["records_delivered"] == len(ref)
        # page caps 1 and 3 on a shorter text (every page is one launch and one copy)
        short = hay[:9000]
        ref_s = auto.match_host(short, ids)
        pieces(1000, 3000)
        for cap in (1, 3):
            got, _ = drain(auto, short, ids, cap)
            assert got.shape == ref_s.shape and (got == ref_s).all(), (ids, cap)


def test_seams_of_the_chain_families_and_long_keywords():
    """Piece boundaries placed on purpose (pieces of 1000 units), the shapes of test_gpu_multi's share seams."""
    pieces(1000)
    a, b, c = ord("a"), ord("b"), ord("c")
    # Longest: a keyword that covers whole pieces (the match before swallows them: nothing reported, the chain passes through)
    rng = np.random.default_rng(5)
    hay = np.where(rng.integers(0, 4, 12000) > 0, a, b).astype(np.uint16)
    big = hay[2500:8300].copy()
    kws = [big, np.array([a], np.uint16), np.array([a, b], np.uint16), np.array([b, a, a], np.uint16)]
    want = Oracle(FAM_LONGEST, kws).match(hay)
    auto = Automaton(N.MODE_LONGEST, kws, True)
    assert int((want[:, 1] - want[:, 0]).max()) == 5800
    for ids in (True, False):
        got, _ = drain(auto, hay, ids, 1000)
        assert (got == (want if ids else want[:, :2])).all()
    # Shortest: the restart position travels through pieces without matches
    hay = np.full(9000, c, np.uint16)
    for at in (1990, 1998, 3996, 3999, 4001, 6999):
        hay[at:at + 8] = [a, b, a, b, a, b, a, b]
    kws = [np.array([a, b, a], np.uint16), np.array([b, a, b], np.uint16)]
    want = Oracle(FAM_SHORTEST, kws).match(hay)
    got, _ = drain(Automaton(N.MODE_SHORTEST, kws, True), hay, True, 7)
    assert got.shape == want.shape and (got == want).all()
    # WholeWord: words straddling seams and reaching into the right halo (words of up to 40 units)
    rng = np.random.default_rng(6)
    words = [np.full(int(n), a if i % 2 else b, np.uint16) for i, n in enumerate(rng.integers(1, 41, 900))]
    parts = []
    for w in words:
        parts += [w, np.array([32] * int(rng.integers(1, 3)), np.uint16)]
    hay = np.concatenate(parts)
    kws = [w for w in words[::3]]
    want = Oracle(FAM_WHOLEWORD, kws, word_chars=WORD).match(hay)
    got, _ = drain(Automaton(N.MODE_WHOLEWORD, kws, True, word_chars=WORD), hay, True, 4096)
    assert len(want) > 100 and got.shape == want.shape and (got == want).all()
    # WholeWordLongest: walks over several words that cross seams
    kws2 = [np.concatenate([words[i], np.array([32], np.uint16), words[i + 1]]) for i in range(0, 600, 2)] + kws
    orc = Oracle(FAM_WWLONGEST, kws2, word_chars=WORD)
    want = orc.match(hay)
    got, _ = drain(Automaton(N.MODE_WWLONGEST, kws2, True, word_chars=WORD), hay, True, 4096)
    assert len(want) > 100 and got.shape == want.shape and (got == want).all()
    # AhoCorasick: keywords longer than a piece (a left halo of 1499 units)
    hay = synth.haystack(7, 20000, table=synth.ALPHA_LOWER[:3])
    kws = [hay[3000:4500].copy(), hay[9990:11490].copy(), hay[100:103].copy()]
    want = Oracle(FAM_AC, kws).match(hay)
    got, _ = drain(Automaton(N.MODE_ALL, kws, True), hay, True, 100)
    assert got.shape == want.shape and (got == want).all() and int((want[:, 1] - want[:, 0]).max()) == 1500


def test_fold_inconsistent_tables_take_the_sequential_form():
    """WholeWord (Set and Map) and WholeWordLongestSet over a table that is not fold-consistent: one piece, the same records."""
    pieces(1000)
    rng = np.random.default_rng(9)
    alpha = np.array([ord(ch) for ch in "abxyABXY ,"], dtype=np.uint16)
    wc = word_chars_from_list("abcdxyABCD")  # X, Y are not word characters although x, y are
    hay = alpha[rng.integers(0, len(alpha), 30000)]
    kws = [alpha[rng.integers(0, 4, int(rng.integers(1, 5)))] for _ in range(12)]
    for mode, flavours in ((N.MODE_WHOLEWORD, (True, False)), (N.MODE_WWLONGEST, (False,))):
        auto = Automaton(mode, kws + ([np.concatenate([kws[0], [32], kws[1]]).astype(np.uint16)] if mode == N.MODE_WWLONGEST else []),
                         False, word_chars=wc)
        assert auto.info()["fold_consistent"] == 0
        for ids in flavours:
            ref = auto.match_host(hay, ids)
            got, st = drain(auto, hay, ids, 333)
            assert len(ref) > 100 and got.shape == ref.shape and (got == ref).all()
            assert st["pieces"] == 1


@pytest.mark.parametrize("n", [0, 1, 2, 4095, 4096])
def test_small_texts(n):
    auto, orc, hay, _ = _case(N.MODE_ALL, True, 3, 4096)
    hay = hay[:n]
    for ids in (True, False):
        ref = auto.match_host(hay, ids)
        got, st = drain(auto, hay, ids, 5)
        assert got.shape == ref.shape and (got == ref).all()
        assert st["scan_end"] == n


def test_early_stop_scans_only_the_first_piece():
    """A 2^28-unit text whose first matches lie in the first 2^20 units: one next(16) scans the first piece only."""
    n = 1 << 28
    hay = np.full(n, 32, np.uint16)
    kws = ["ab", "abc", "bca", "c"]
    pre = synth.haystack(11, 1 << 19, table=np.array([97, 98, 99, 32], np.uint16))
    hay[:pre.size] = pre
    want = Oracle(FAM_AC, kws).match(pre)
    for mode, ids in ((N.MODE_ALL, True), (N.MODE_WHOLEWORD, False)):
        auto = Automaton(mode, kws, True, word_chars=WORD if mode == N.MODE_WHOLEWORD else None)
        with Cursor(auto, hay, ids) as c:
            page = c.next(16)
            st = c.stats()
        assert st["scan_end"] <= (1 << 20) + 3 + 1 and st["pieces"] - st["rescans"] == 1 and len(page) >= 1
        if mode == N.MODE_ALL:
            assert len(page) == 16 and (page == want[:16]).all()


def test_reservoir_pressure_rescans_and_nomem():
    """A 64 KiB reservoir under a dense dictionary: pieces are rescanned smaller, the records stay exact; a budget below
    max_len records cannot hold one unit's records: ACGPU_E_NOMEM."""
    kws = ["a" * L for L in range(1, 17)]
    hay = np.full(40000, ord("a"), np.uint16)
    hay[::997] = ord("b")
    auto = Automaton(N.MODE_ALL, kws, True)
    ref = auto.match_host(hay, True)
    N.set_tunable("cursor_reservoir_bytes", 64 << 10)
    got, st = drain(auto, hay, True, 5000)
    assert st["rescans"] > 0 and got.shape == ref.shape and (got == ref).all()
    N.set_tunable("cursor_reservoir_bytes", 15 * 8)
    with Cursor(auto, hay, False) as c:
        with pytest.raises(N.AcgpuError) as e:
            while len(c.next(4096)):
                pass
        assert e.value.code == N.E_NOMEM
        with pytest.raises(N.AcgpuError):  # after a failed next only close is valid
            c.next(1)


def _dense_all():
    from tests.test_gpu_count import _family_case
    kws, hay = _family_case(N.MODE_ALL, True, 300 + N.MODE_ALL * 2 + 1, 20000)
    return lambda: Automaton(N.MODE_ALL, kws, True), hay, len(kws)


def _whole_word_not_fold_consistent():
    rng = np.random.default_rng(9)
    alpha = np.array([ord(ch) for ch in "abxyABXY ,"], dtype=np.uint16)
    wc = word_chars_from_list("abcdxyABCD")  # X, Y are not word characters although x, y are
    hay = alpha[rng.integers(0, len(alpha), 20000)]
    kws = [alpha[rng.integers(0, 4, int(rng.integers(1, 5)))] for _ in range(12)]
    kws += [kws[2].copy()]
    return lambda: Automaton(N.MODE_WHOLEWORD, kws, False, word_chars=wc), hay, len(kws)


@pytest.mark.parametrize("case", [_dense_all, _whole_word_not_fold_consistent])
def test_cursor_and_count_plan_the_same_pieces(case):
    """A cursor drained in one page per piece and a counting call, each on a fresh automaton (an empty reservoir), pieces of
    64 .. 4096 units through a reservoir of 500 Map records, every piece through records: the same pieces and the same rescans.
    The dense ALL text overflows its reservoir at least once; the WholeWord table that is not fold-consistent is one piece."""
    fresh, hay, n_kw = case()
    ref = fresh().match_host(hay, True)
    want = np.bincount(ref[:, 2], minlength=n_kw).astype(np.uint64)
    pieces(64, 4096)
    N.set_tunable("cursor_reservoir_bytes", 6000)
    N.set_tunable("all_form", 1)
    N.set_tunable("count_form", 1)
    got, cst = drain(fresh(), hay, True, len(ref) + 1)
    counts, nst = fresh().count_host(hay)
    plans = (cst["pieces"], cst["rescans"]), (nst["pieces"], nst["rescans"])
    print("plan", case.__name__, plans)
    assert plans[0] == plans[1]
    assert len(ref) > 100 and got.shape == ref.shape and (got == ref).all()
    assert (counts == want).all() and nst["units_direct"] == 0
    if case is _dense_all:
        assert cst["rescans"] >= 1
    else:
        assert cst["pieces"] - cst["rescans"] == 1 and nst["pieces"] - nst["rescans"] == 1


def test_more_records_than_a_java_int_array_holds():
    """Keywords a .. a^32 over 'a' x 2^26: 32 n - 496 records (4.3e9 ints as a Java int[]), drained in pages of 2^24 records,
    every page checked against the closed form: at end e, starts e - L for L = min(e, 32) down to 1."""
    n = 1 << 26
    auto = Automaton(N.MODE_ALL, ["a" * L for L in range(1, 33)], True)
    hay = np.full(n, ord("a"), np.uint16)
    head = np.array([(e - L, e) for e in range(1, 33) for L in range(e, 0, -1)], np.int64)  # the first 528 records
    total = 0
    with Cursor(auto, hay, False) as c:
        while True:
            p = c.next(1 << 24)
            if not len(p):
                break
            g = np.arange(total, total + len(p), dtype=np.int64)
            e = 33 + (g - 528) // 32
            start = e - 32 + (g - 528) % 32
            small = g < 528
            if small.any():
                start[small], e[small] = head[g[small], 0], head[g[small], 1]
            assert (p[:, 0] == start).all() and (p[:, 1] == e).all(), total
            total += len(p)
            del p
        st = c.stats()
    assert total == 32 * n - 496 and st["records_delivered"] == total and total * 2 > 2 ** 31


def test_cursors_share_an_automaton_with_match_calls():
    auto, orc, hay, _ = _case(N.MODE_LONGEST, True, 21, 50000)
    hay2 = hay[::-1].copy()
    ref1, ref2, ref3 = auto.match_host(hay, True), auto.match_host(hay2, True), auto.match_host(hay[:5000], True)
    pieces(1500, 6000)
    c1, c2 = Cursor(auto, hay, True), Cursor(auto, hay2, True)
    got1, got2 = [], []
    while True:
        p1 = c1.next(700)
        assert (auto.match_host(hay[:5000], True) == ref3).all()
        p2 = c2.next(900)
        got1.append(p1)
        got2.append(p2)
        if not len(p1) and not len(p2):
            break
    c1.close()
    c2.close()
    assert (np.concatenate(got1) == ref1).all() and (np.concatenate(got2) == ref2).all()


def test_facades_page_long_haystacks():
    """StringSet / StringMap.match on a >= 2^22-unit text page through the cursor: the listener hears find_all's records; a
    listener that returns False after 5 records gets exactly the first 5."""
    from ahocorasick_amd import (AhoCorasickMap, AhoCorasickSet, LongestMatchMap, ShortestMatchSet, WholeWordLongestMatchSet,
                                 WholeWordMatchMap)
    table = np.array([ord(ch) for ch in "abcd  "], dtype=np.uint16)
    hay = synth.haystack(31, (1 << 22) + 77, table=table)
    kws = ["ab", "abc", "bca", "c", "dab", "a b", "cd"]
    ids = list(range(len(kws)))
    objs = [AhoCorasickSet(kws, True), AhoCorasickMap(kws, ids, False), LongestMatchMap(kws, ids, True), ShortestMatchSet(kws, True),
            WholeWordMatchMap([k for k in kws if " " not in k], ids, True), WholeWordLongestMatchSet(kws, True)]
    for o in objs:
        want = o.find_all(hay)
        got = []
        if want.shape[1] == 3:
            o.match(hay, lambda h, s, e, v: got.append((s, e, v)) or True)
        else:
            o.match(hay, lambda h, s, e: got.append((s, e)) or True)
        assert len(want) > 1000 and np.array_equal(np.array(got, np.int32).reshape(want.shape), want), type(o).__name__
        first = []
        if want.shape[1] == 3:
            o.match(hay, lambda h, s, e, v: first.append((s, e, v)) or len(first) < 5)
        else:
            o.match(hay, lambda h, s, e: first.append((s, e)) or len(first) < 5)
        assert np.array_equal(np.array(first, np.int32), want[:5])


def test_jni_cursor_glue_over_the_library_returns_the_ctypes_pages(tmp_path):
    """tests/jni_min/cursor_env.c (mock JNIEnv + acgpu_jni_cursor.c) linked against libacgpu.so: the flattened pages of the native
    methods are the ctypes binding's."""
    N.lib()
    jdir = os.path.join(ROOT, "tests", "jni_min")
    so = str(tmp_path / "libjhc.so")
    libdir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fPIC", "-shared", "-I", jdir, "-I",
                           os.path.join(ROOT, "include"), "-o", so, os.path.join(jdir, "cursor_env.c"), "-L", libdir,
                           "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + libdir])
    L = ctypes.CDLL(so)
    vp, ll, ci = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    L.jh_exception_class.restype = ctypes.c_char_p
    L.jh_build.restype = ll
    L.jh_build.argtypes = [ci, vp, vp, vp, ci, ci, vp, vp, ci]
    L.jh_free.argtypes = [ll]
    L.jh_release.argtypes = [vp]
    L.jh_cursor_open.restype = ll
    L.jh_cursor_open.argtypes = [ll, vp, ll, ci]
    L.jh_cursor_next.restype = ll
    L.jh_cursor_next.argtypes = [ll, ci, ctypes.POINTER(vp)]
    L.jh_cursor_close.argtypes = [ll]
    L.jh_violations.restype = ll
    from ahocorasick_amd.strings import _pack
    kws = synth.random_keywords(5, 800, 2, 9, table=synth.ALPHA_LOWER[:8])
    hay = synth.haystack(6, 300000, table=synth.ALPHA_LOWER[:8])
    units, off = _pack(kws)
    h = L.jh_build(N.MODE_ALL, units.ctypes.data, off.ctypes.data, None, len(kws), 1, None, None, 65536)
    assert h != 0
    want = Automaton(N.MODE_ALL, kws, True).match_host(hay, True)
    pieces(20000, 80000)
    c = L.jh_cursor_open(h, hay.ctypes.data, hay.size, 1)
    assert c != 0, L.jh_exception_class()
    got = []
    while True:
        p = ctypes.c_void_p()
        k = L.jh_cursor_next(c, 5000, ctypes.byref(p))
        assert k >= 0, L.jh_exception_class()
        if k:
            got.append(np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_int32)), shape=(int(k),)).copy())
        L.jh_release(p)
        if k == 0:
            break
        assert k <= 5000 * 3
    L.jh_cursor_close(c)
    L.jh_free(h)
    got = np.concatenate(got).reshape(-1, 3)
    assert len(want) > 10000 and got.shape == want.shape and (got == want).all() and L.jh_violations() == 0


def test_cursor_next_and_stats_check_their_arguments_on_a_device():
    """cap 0, NULL out or n_out: ACGPU_E_INVALID before anything is scanned (needs an open cursor, so a device)."""
    L = N.lib()
    a = Automaton(N.MODE_ALL, ["ab"], True)
    with Cursor(a, utf16("zabz" * 100), False) as c:
        out = np.zeros(16, np.int32)
        n = ctypes.c_uint64(0)
        vp = out.ctypes.data_as(ctypes.c_void_p)
        assert L.acgpu_cursor_next(c._h, vp, 0, ctypes.byref(n)) == N.E_INVALID
        assert L.acgpu_cursor_next(c._h, None, 4, ctypes.byref(n)) == N.E_INVALID
        assert L.acgpu_cursor_next(c._h, vp, 4, None) == N.E_INVALID
        assert L.acgpu_cursor_get_stats(c._h, None) == N.E_INVALID
