"""CPU-side checks of caller-supplied fold tables (tests/fold_tables.py): every named table crosses the limit it is named for, by a
restatement of the builder's counts and by the builder's own where a hook returns them; every structure the builder derives from
lower[] gives lower[] back for all 65536 units; the table simulations of tests/test_native_cpu.py and the oracle agree under every
table; the oracle itself is pinned to oracle/brute.py under every table; and the inputs of tests/test_gpu_fold_tables.py meet their
coverage floors and notice a table that is wrong in one unit -- with the oracle alone, no device."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton
from oracle import brute
from oracle.oracle import FAM_AC, FAM_LONGEST, FAM_SHORTEST, FAM_WHOLEWORD, FAM_WWLONGEST, Oracle
from tests import fold_tables as F
from tests.test_native_cpu import (_perfect_tables, _simulate_all, _simulate_wholeword, _simulate_wholeword_perfect, _tables,
                                   _wordhash_tables)

CUSTOM = [t for t in F.TABLES if t != "java"]
AC_KIND = {"java": "cyrillic", "wide": "mixed", "manydeltas": "mixed", "huge": "huge", "scatter": "scatter", "farpartner": "far_low",
           "rotate": "rotate", "inconsistent": "mixed"}


def _ww(table, kws=("a",)):
    T, word = F.fold_table(table)
    return Automaton(N.MODE_WHOLEWORD, list(kws), False, word_chars=word, lower=T)


def _ac(table, rng, n_kw=None):
    T, _ = F.fold_table(table)
    kws = F.dictionary(AC_KIND[table], table, rng)[:n_kw]
    return kws, Automaton(N.MODE_ALL, kws, False, lower=T)


# ---- thresholds -----------------------------------------------------------------------------------------------------------------

def test_every_table_crosses_the_limit_it_is_named_for():
    st = {t: F.table_stats(*F.fold_table(t)) for t in F.TABLES}
    # (k_wwl_walk keeps at most 24 fold pages in LDS, k_ww_pp / k_ww_tile at most 64; the byte pages hold at most 128 deltas and 64 pages)
    assert st["java"] == {"fold_pages": 18, "deltas": 79, "byte_pages": 54, "idempotent": True, "fold_consistent": True}
    assert 24 < st["wide"]["fold_pages"] <= 64 and st["wide"]["deltas"] <= 128 and st["wide"]["byte_pages"] > 64
    assert st["manydeltas"]["fold_pages"] <= 24 and st["manydeltas"]["deltas"] > 128 and st["manydeltas"]["byte_pages"] is None
    assert st["huge"]["fold_pages"] > 64
    assert st["inconsistent"]["fold_pages"] == st["wide"]["fold_pages"] and not st["inconsistent"]["fold_consistent"]
    assert not st["rotate"]["idempotent"]
    for t in F.TABLES:
        assert st[t]["fold_consistent"] == (t != "inconsistent"), t
        assert st[t]["idempotent"] == (t != "rotate"), t
    # which form of k_wwl_walk a table takes (the profile's name does not say): the page count is the evidence
    assert [t for t in ("java", "manydeltas", "wide", "huge", "inconsistent") if st[t]["fold_pages"] <= 24] == ["java", "manydeltas"]
    T, _ = F.fold_table("rotate")
    a, b, c, d = F.ROT
    assert (T[a], T[b], T[c], T[d]) == (b, c, d, a) and T[ord("e")] == 0 and T[0xFFFF] == ord("f") and T[0xD800] == ord("g")
    T, _ = F.fold_table("farpartner")
    top, low = np.array(F.FAR_TOP), np.array(F.FAR_LOW)
    assert (T[top - 0x20] == top).all() and (T[top] == top).all() and top[-1] > 0xFF00          # partner below, both near the top
    assert (T[low + 0x50] == low).all() and (T[low] == low).all() and low[0] + 0x50 > low[-1]   # partner above
    pre_top = np.flatnonzero(np.isin(T, top) & ~np.isin(np.arange(65536), top))
    assert set(pre_top.tolist()) == set((top - 0x20).tolist())                                  # no exceptions: the checks accept
    pre_low = np.flatnonzero(np.isin(T, low) & ~np.isin(np.arange(65536), np.concatenate([low, low + 0x50])))
    assert (pre_low < 0x0400).sum() >= 5                                                        # exceptions in the low zone: they refuse


@pytest.mark.parametrize("table", F.TABLES)
def test_the_builders_counts_equal_the_restated_ones(table):
    T, word = F.fold_table(table)
    st = F.table_stats(T, word)
    a = _ww(table)
    n_pages = ctypes.c_uint32(0)
    N.check(N.lib().acgpu_debug_wordhash(a.handle, None, None, None, None, None, ctypes.byref(n_pages), None, None), "n_pages")
    assert n_pages.value == st["fold_pages"]
    built = st["fold_consistent"] and st["byte_pages"] is not None and st["byte_pages"] <= 64
    assert _perfect_tables(a)[2] == (st["byte_pages"] if built else 0)
    assert a.info()["fold_consistent"] == (0 if table == "inconsistent" else 1)
    wwl = Automaton(N.MODE_WWLONGEST, ["a b"], False, word_chars=word, lower=T)
    assert wwl.info()["fold_consistent"] == (0 if table == "inconsistent" else 1)


def test_scatter_class_tables_do_not_fit_where_the_kernels_keep_them():
    """dfa_pages (16-bit classes: 256 + 512 bytes per distinct page) are dropped beyond 32 KB.  cls_pages (bytes: 256 + 256 per distinct
    page) go to LDS when they fit behind the filter rows in the tile kernel's static array (csrc/acgpu_tile.hip: rows32, ACGPU_FILTER_WORDS
    words; the rows are acgpu_info.filter_bits / 8 bytes, the pages start at the next multiple of 16): with the 50-unit dictionary they
    do (the no_class_pages twin is the table in global memory), with the bucketed one they do not.  All restated from cls_lut, which
    has one distinct page per page the table's rule touches."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(N.LIB_PATH), "..", "csrc", "acgpu_tile.hip")).read()
    lds = 4 * int(re.search(r"#define ACGPU_FILTER_WORDS (\d+)", src).group(1))
    assert lds == 88064
    kws, a = _ac("scatter", np.random.default_rng(1))
    cls = _tables(a)[1]
    n = F.distinct_pages(cls)
    assert n >= 200 and 256 + n * 512 > 32 * 1024 and 256 + n * 256 >= 50 * 1024
    assert a.info()["n_classes"] == 51 and a.info()["dense"] == 1
    rows = (a.info()["filter_bits"] // 8 + 15) & ~15
    assert a.info()["filter_k"] == 3 and rows + 256 + n * 256 <= lds
    T, _ = F.fold_table("scatter")
    kws = F.dictionary("scatter_bucketed", "scatter", np.random.default_rng(1))
    a = Automaton(N.MODE_ALL, kws, False, lower=T)
    n = F.distinct_pages(_tables(a)[1])  # (bucketed: a page of tile_lut differs wherever the page of cls_lut does, or two units share a bucket)
    rows = (a.info()["filter_bits"] // 8 + 15) & ~15
    assert a.info()["n_classes"] == 301 and a.info()["filter_k"] == 3 and rows == 64 * 64 * 8
    assert n >= 220 and rows + 256 + (n - 8) * 256 > lds  # (even if eight pages fell together in the buckets)
    # the tables of the state forms' cases, for contrast: the pages are kept (k_ac_states and k_longest_follow need them)
    kws, a = _ac("huge", np.random.default_rng(1))
    n = F.distinct_pages(_tables(a)[1])
    assert 50 <= n and 256 + n * 512 <= 32 * 1024


# ---- reconstruction --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", F.TABLES)
def test_fold_pages_and_byte_pages_give_the_table_back(table):
    T, word = F.fold_table(table)
    a = _ww(table)
    _, _, pgidx, pages, _ = _wordhash_tables(a)
    u = np.arange(65536)
    got = (u + pages[pgidx[u >> 8].astype(np.int64) * 256 + (u & 255)]) & 0xffff
    assert (got == T).all(), np.flatnonzero(got != T)[:8]
    _, _, n_pages, _, _, idx, bpages, delta = _perfect_tables(a)
    if n_pages:
        e = bpages[idx[u >> 8].astype(np.int64) * 256 + (u & 255)].astype(np.int64)
        assert ((e & 1) == (word != 0)).all()
        assert (((u + delta[e >> 1]) & 0xffff) == T).all()


@pytest.mark.parametrize("table", F.TABLES)
def test_cls_lut_is_the_class_of_the_folded_unit(table):
    T, _ = F.fold_table(table)
    kws, a = _ac(table, np.random.default_rng(2))
    cls = _tables(a)[1]
    used = np.unique(np.concatenate([T[k] for k in kws]))
    cls_of = np.zeros(65536, np.int64)
    cls_of[used] = np.arange(1, len(used) + 1)
    assert a.info()["n_classes"] == len(used) + 1
    assert (cls == cls_of[T]).all(), np.flatnonzero(cls != cls_of[T])[:8]


# ---- the table simulations against the oracle ----------------------------------------------------------------------------------

def _small_text(rng, table, kws, word, n=2000, minimal=False):
    T, _ = F.fold_table(table)
    return F.preimage_text(rng, T, kws, n, [b for b in (160, 1024) if b < n - 128], word, minimal=minimal, n_plants=120, plane=False,
                           every_preimage=False)[0]  # (too short for a plant per preimage unit: the GPU cases' texts have those)


@pytest.mark.parametrize("table", CUSTOM)
def test_table_simulations_reproduce_the_oracle_under_a_custom_table(table):
    T, word = F.fold_table(table)
    rng = np.random.default_rng(F.TABLES.index(table) + 40)
    kws = F.dictionary("ww_short", table, rng)
    hay = _small_text(rng, table, kws, word)
    a = Automaton(N.MODE_WHOLEWORD, kws, False, word_chars=word, lower=T)
    if table != "inconsistent":  # (the hash tables are what the position-parallel kernels probe: fold-consistent tables)
        want = Oracle(FAM_WHOLEWORD, kws, case_sensitive=False, lower=T, word_chars=word).match(hay).tolist()
        assert len(want) >= 100
        assert _simulate_wholeword(a, hay, word, False) == want
        if _perfect_tables(a)[2]:
            assert _simulate_wholeword_perfect(a, hay, False) == want
    else:  # ... and here over wordChars o toLowerCase, the scan that folds in every lookup (acgpu.h: the Readable loops)
        want = Oracle(FAM_WHOLEWORD, kws, case_sensitive=False, lower=T, word_chars=word).match_readable(hay, positions=True).tolist()
        assert len(want) >= 100
        assert _simulate_wholeword(a, hay, word[T], False) == want
    kws, a = _ac(table, rng)
    hay = _small_text(rng, table, kws, None)
    want = Oracle(FAM_AC, kws, case_sensitive=False, lower=T).match(hay).tolist()
    assert len(want) >= 100 and _simulate_all(a, hay) == want


# ---- the oracle pinned to the closed forms ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", CUSTOM)
def test_oracle_equals_the_closed_forms_under_a_custom_table(table):
    """oracle/brute.py folds both sides once and compares; its word matchers are stated for fold-consistent tables, so
    "inconsistent" (which is "wide" with another word table) is pinned for the three families without word characters."""
    T, word = F.fold_table(table)
    rng = np.random.default_rng(F.TABLES.index(table) + 70)
    n_records = 0
    for rep in range(6):
        kws = F.dictionary(AC_KIND[table], table, rng)[:40] + [k[:2] for k in F.dictionary(AC_KIND[table], table, rng)[:10]]
        for fam, closed, minimal in ((FAM_AC, brute.ac_all, False), (FAM_LONGEST, brute.longest, False), (FAM_SHORTEST, brute.shortest, True)):
            hay = _small_text(rng, table, kws, None, n=300, minimal=minimal)
            got = Oracle(fam, kws, case_sensitive=False, lower=T).match(hay).tolist()
            assert got == [list(m) for m in closed(hay, kws, False, T)], (table, fam, rep)
            n_records += len(got)
        if table == "inconsistent":
            continue
        for kind, fam in (("ww_short", FAM_WHOLEWORD), ("phrases", FAM_WWLONGEST)):
            kws = F.dictionary(kind, table, rng)[::5]
            hay = _small_text(rng, table, kws, word, n=300).copy()
            hay[rng.integers(0, hay.size, 40)] = F.SPACE
            got = Oracle(fam, kws, case_sensitive=False, lower=T, word_chars=word).match(hay).tolist()
            if fam == FAM_WHOLEWORD:
                want = brute.wholeword(hay, kws, word, False, T)
            else:
                want = brute.wwlongest(hay, kws, word, case_sensitive=False, lower=T)
            assert got == [list(m) for m in want], (table, fam, rep)
            n_records += len(got)
    assert n_records >= 200


# ---- the inputs of the GPU cases ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(F.CASES))
def test_gpu_case_inputs_meet_the_coverage_floors(name):
    kws, hay, spans, T, word = F.case_inputs(name)
    want = F.case_records(name)
    assert hay.size == F.N_UNITS + 65536 and len(kws) <= 2000
    assert len(want) >= 1000
    # records that hold a raw unit beyond ASCII that folds to another unit
    moved = np.concatenate([[0], np.cumsum((T[hay] != hay) & (hay >= 0x80))])
    assert ((moved[want[:, 1]] - moved[want[:, 0]]) > 0).mean() >= 0.30
    have = set(map(tuple, want[:, :2].tolist()))
    assert all(sp in have for sp in spans)
    # every preimage unit of every keyword unit inside at least one record (word matchers: the preimages that are word characters
    # wherever the unit has one -- a keyword is validated on its raw units, and a run holds nothing else)
    alpha = np.unique(np.concatenate([T[k] for k in kws]))
    need = np.isin(T, alpha)
    if word is not None:
        w = word != 0
        has_word = np.zeros(65536, bool)
        has_word[T[w]] = True
        need &= w | ~has_word[T]
    cover = np.zeros(hay.size + 1, np.int64)
    np.add.at(cover, want[:, 0], 1)
    np.add.at(cover, want[:, 1], -1)
    inside = np.zeros(65536, bool)
    inside[hay[np.cumsum(cover[:-1]) > 0]] = True
    assert not (need & ~inside).any(), np.flatnonzero(need & ~inside)[:8]


@pytest.mark.parametrize("name", list(F.CASES))
def test_gpu_case_records_change_with_one_unit_of_the_table(name):
    """A scan that folded one preimage unit of a planted keyword out of the alphabet reports other records: the case's text tells a
    wrong fold of that unit from a right one.  The wrong fold is the haystack's alone, as on the device, where the dictionary was
    folded by the host: every occurrence of the unit in the text is replaced by a private-use unit, which folds to itself, is in no
    alphabet and is no word character.  (The same wrong entry given to the oracle's own table would fold the dictionary with it, and a
    unit that is its own only preimage would then still match itself.)"""
    kws, hay, spans, T, word = F.case_inputs(name)
    want = F.case_records(name)
    rng = np.random.default_rng(len(name) * 7 + 1)
    planted = np.unique(np.concatenate([hay[s:e] for s, e in spans]))
    r = int(planted[rng.integers(0, len(planted))])
    assert T[0xE000] == 0xE000 and not np.isin(0xE000, np.concatenate([T[k] for k in kws])) and (word is None or not word[0xE000])
    wrong = np.where(hay == r, 0xE000, hay).astype(np.uint16)
    got = F.case_oracle(name).match(wrong, cap=1 << 20)
    assert got.shape != want.shape or (got != want).any(), (name, hex(r))

def test_keywords_that_differ_only_in_trailing_nul_word_units_are_refused_loudly():
    """The hashes of a word run go over its packed units, zero beyond its end: with U+0000 as a word character "a", "a\\0" and "a\\0\\0"
    hash alike, the two-choice table has two slots for them, and acgpu_build says ACGPU_E_UNSUPPORTED -- no automaton that would report
    other records.  This pins a known limitation of the builder as a loud refusal, not a contract: a builder that placed such
    keywords would be right, and this test would then change.  (Why "rotate", where e folds to U+0000, is paired with a word table in which neither is a word character.)"""
    word = np.array(F.fold_table("java")[1])
    word[0] = 1
    kws = [np.array([97] + [0] * k, np.uint16) for k in range(3)]
    for mode in (N.MODE_WHOLEWORD, N.MODE_WWLONGEST):
        assert Automaton(mode, kws[:2], True, word_chars=word).info()["n_keywords"] == 2
        with pytest.raises(N.AcgpuError) as e:
            Automaton(mode, kws, True, word_chars=word)
        assert e.value.code == N.E_UNSUPPORTED
