"""Caller-supplied fold tables for the tests (test code only).  acgpu_build takes lower[65536] from the caller, and the device folds
through structures the builder derives from it (fold pages, byte pages, class tables and their pages, folded range classes, merged
stretches), each with a limit and a fallback.  The tables here are the shipped one changed by a short rule so that a limit is
crossed; table_stats() restates the builder's counts, preimage_text() builds a text that sends every unit of the plane and every
preimage of the dictionary's units through the lookups, and CASES names the dictionary / table / tunables of every GPU case, so that
tests/test_fold_tables_cpu.py can check the inputs with the oracle alone and tests/test_gpu_fold_tables.py runs exactly those."""
import functools

import numpy as np

from ahocorasick_amd import _native as N
from oracle.oracle import FAM_AC, FAM_LONGEST, FAM_SHORTEST, FAM_WHOLEWORD, FAM_WWLONGEST, Oracle
from tests.helpers import LOWER, WORD

N_UNITS = (1 << 16) + 777
# (tests/test_gpu_tile_forms.py: a lane, a tile, a second-level tile, a region and the seam at 2^16)
BOUNDARIES = [160, 1024, 2048, 3 * 2048, 16384, 32768, 65536]
SPACE, BANG = 0x20, 0x21
TABLES = ("java", "wide", "manydeltas", "huge", "scatter", "farpartner", "rotate", "inconsistent")

SCATTER_ALPHA = list(range(0x4E00, 0x4E00 + 300, 6))  # 50 units in more stretches than the range arithmetic merges: the class table
FAR_TOP = list(range(0xFF41, 0xFF5B))                 # fullwidth a..z, partner range U+FF21.. (the shipped table's own pairs)
FAR_LOW = list(range(0x0250, 0x026A))                 # partner range above it at U+02A0.. (this table's rule)
WIDE_PAGES = list(range(0x50, 0x5C))                  # CJK pages: word characters throughout, nothing folds there in the shipped table
MANY_PAGES = list(range(0x60, 0x65))
HUGE_PAGES = list(range(0x4E, 0x80))
ROT = [ord(c) for c in "abcd"]


def _u(s):
    return np.array([ord(c) for c in s], dtype=np.uint16)


@functools.lru_cache(maxsize=None)
def fold_table(name):
    """(lower uint16[65536], word uint8[65536]) of a named table; both read-only.  Except for "inconsistent" the word table is
    the default one made fold-consistent with the table: word[r] = word[lower[r]], repeated until it holds for every unit."""
    T = np.asarray(LOWER, dtype=np.uint16).copy()
    if name in ("wide", "inconsistent"):  # 12 more fold pages, each its own pattern (and its own delta): 30 fold pages, 66 byte pages
        for k, pg in enumerate(WIDE_PAGES):
            T[(pg << 8) | (k + 1)] = pg << 8
    elif name == "manydeltas":  # 5 more fold pages with 12 deltas each that no other unit has: 23 fold pages, 139 deltas
        for j, pg in enumerate(MANY_PAGES):
            for i in range(1, 13):
                T[(pg << 8) | (16 * j + i)] = pg << 8
    elif name == "huge":  # 50 more fold pages: 68
        for k, pg in enumerate(HUGE_PAGES):
            T[(pg << 8) | (k + 1)] = pg << 8
    elif name == "scatter":
        # two units in each of 222 pages fold onto the 50 units of SCATTER_ALPHA, at in-page offsets that differ from page to page
        # (37 is odd: p -> 37 p + 11 mod 256 is one to one), so the class tables have as many distinct pages
        n_pre = np.bincount(LOWER, minlength=65536)
        free = (LOWER == np.arange(65536)) & (n_pre == 1)  # units that fold to themselves and that nothing else folds to
        for p in range(0x20, 0x100):
            if p in (0x4E, 0x4F):
                continue
            for o, t in (((p * 37 + 11) & 255, p % 50), ((p * 101 + 3) & 255, (p + 17) % 50)):
                while not free[(p << 8) | o]:
                    o = (o + 1) & 255
                T[(p << 8) | o] = SCATTER_ALPHA[t]
    elif name == "farpartner":
        for i, f in enumerate(FAR_LOW):
            T[0x02A0 + i] = f
    elif name == "rotate":  # not idempotent: a -> b -> c -> d -> a; e -> U+0000; U+FFFF -> f; a high surrogate -> g
        for i, c in enumerate(ROT):
            T[c] = ROT[(i + 1) % 4]
        T[ord("e")] = 0
        T[0xFFFF] = ord("f")
        T[0xD800] = ord("g")
    elif name != "java":
        raise KeyError(name)
    word = np.asarray(WORD, dtype=np.uint8).copy()
    for _ in range(4):  # ("rotate": e folds to U+0000 and E to e, so neither is a word character)
        word = word[T]
    if name == "inconsistent":  # U+5001 folds to the word character U+5000 and is none itself, the same on two more pages
        word[[0x5001, 0x5102, 0x5203]] = 0
    T.setflags(write=False)
    word.setflags(write=False)
    return T, word


def table_stats(T, word):
    """The builder's counts restated (acgpu_build.cpp, "the fold table as shared pages" and "word-character bit and fold delta in
    one byte"): distinct pages of 256 deltas with the all-zero page counted whether it occurs or not, distinct deltas, distinct byte
    pages (None: more than 128 deltas -- the pages cannot be built at all), and the two properties of the pair."""
    T = np.asarray(T, dtype=np.uint16)
    u = np.arange(65536, dtype=np.int64)
    delta = ((T.astype(np.int64) - u) & 0xffff).astype(np.uint16)
    pages = {delta[p * 256:(p + 1) * 256].tobytes() for p in range(256)} | {bytes(512)}
    deltas = list(dict.fromkeys(delta.tolist()))  # in the builder's order of first occurrence
    byte_pages = None
    if len(deltas) <= 128:
        idx = np.zeros(65536, np.int64)
        idx[deltas] = np.arange(len(deltas))
        e = (idx[delta] << 1) | (np.asarray(word)[u] != 0)
        byte_pages = len({e[p * 256:(p + 1) * 256].tobytes() for p in range(256)})
    w = np.asarray(word) != 0
    return {"fold_pages": len(pages), "deltas": len(deltas), "byte_pages": byte_pages,
            "idempotent": bool((T[T] == T).all()), "fold_consistent": bool((w == w[T]).all())}


def distinct_pages(lut):
    """distinct 256-entry pages of a 65536-entry table (what cls_pages / dfa_pages hold once each)"""
    lut = np.asarray(lut)
    return len({lut[p * 256:(p + 1) * 256].tobytes() for p in range(256)})


def preimages(T):
    """folded unit -> array of the raw units that fold to it"""
    T = np.asarray(T, dtype=np.uint16)
    order = np.argsort(T, kind="stable")
    cuts = np.flatnonzero(np.diff(T[order])) + 1
    return {int(T[g[0]]): g.astype(np.uint16) for g in np.split(order, cuts)}


def spell(rng, pre, folded, word=None, force=None):
    """a raw spelling of a string of folded units: every unit a random one of its preimages (word: word characters only; force =
    (position, raw unit): that one as given)"""
    out = np.empty(len(folded), np.uint16)
    for i, f in enumerate(np.asarray(folded).tolist()):
        c = pre[f]
        if word is not None and (np.asarray(word)[c] != 0).any():
            c = c[np.asarray(word)[c] != 0]
        out[i] = c[rng.integers(0, len(c))]
    if force is not None:
        out[force[0]] = force[1]
    return out


def _minimal(folded_kws):
    """indices of the keywords that hold no other keyword inside them (Shortest reports such a keyword whole)"""
    keys = [k.tobytes() for k in folded_kws]
    have = set(keys)
    out = []
    for i, k in enumerate(folded_kws):
        n = len(k)
        inner = (k[a:b].tobytes() for a in range(n) for b in range(a + 1, n + 1) if b - a < n)
        if not any(s in have for s in inner):
            out.append(i)
    return out


def preimage_text(rng, T, kws, n, boundaries, word=None, minimal=False, n_plants=1400, plane=True, every_preimage=True):
    """(text, planted spans).  The text is n + 65536 units:
      (a) one copy of arange(65536), behind the first n - 64 units: every unit of the plane goes through every lookup once;
      (b) random units, half of them from the full preimage of the dictionary's folded units under T (every raw r with T[r] in
          the alphabet), the others units that fold next to the alphabet, separators, U+0000, U+FFFF and surrogates;
      (c) keywords spelt in a random mixture of their preimages: for every preimage unit one keyword that holds it there, more at
          random up to n_plants, one across every boundary and one ending at the text's last unit -- each between two '!' (in
          no keyword, no word character), so that every family reports the planted span itself.
    kws are the dictionary's raw keywords; minimal: plant only keywords that hold no other keyword (Shortest); plane = False: a
    text of n units without (a), for the loops written in Python; every_preimage = False: without the one plant per preimage unit
    (the random plants only), for texts too short to hold them."""
    T = np.asarray(T, dtype=np.uint16)
    pre = preimages(T)
    folded = [T[np.asarray(k, dtype=np.uint16)] for k in kws]
    alpha = np.unique(np.concatenate(folded))
    full = np.flatnonzero(np.isin(T, alpha)).astype(np.uint16)
    near = np.unique(np.concatenate([(alpha.astype(np.int64) + d) & 0xffff for d in (-1, 1, -256, 256, 32, -32)])).astype(np.uint16)
    near_pre = np.flatnonzero(np.isin(T, near) & ~np.isin(T, alpha)).astype(np.uint16)
    other = np.concatenate([near_pre, np.array([SPACE, SPACE, SPACE, BANG, 0x00E9, 0x0000, 0xFFFF, 0xD800, 0xDFFF, 0x3002], np.uint16)])
    total = n + 65536 if plane else n
    hay = np.where(rng.random(total) < 0.55, full[rng.integers(0, len(full), total)], other[rng.integers(0, len(other), total)]).astype(np.uint16)
    a0 = n - 64
    if plane:
        hay[a0:a0 + 65536] = np.arange(65536, dtype=np.uint16)
    ok = _minimal(folded) if minimal else list(range(len(kws)))
    holds = {}
    for i in ok:
        for j, f in enumerate(folded[i].tolist()):
            holds.setdefault(f, []).append((i, j))
    plants = []  # (keyword index, forced (position, raw unit) or None)
    for f in alpha.tolist():
        for r in pre[f].tolist() if every_preimage else []:
            if f in holds and (word is None or word[r] or not np.asarray(word)[pre[f]].any()):  # (word matchers: spelt in word characters)
                # (where it can be, in a keyword that is spelt with ANOTHER preimage there: the plant then matches by the fold of r alone)
                at = [(i, j) for i, j in holds[f] if int(kws[i][j]) != r] or holds[f]
                i, j = at[int(rng.integers(0, len(at)))]
                plants.append((i, (j, r)))
    while len(plants) < n_plants:
        plants.append((ok[int(rng.integers(0, len(ok)))], None))
    order = rng.permutation(len(plants))
    spans = []

    def put(s, i, force=None):
        k = spell(rng, pre, folded[i], word, force)
        hay[s:s + k.size] = k
        hay[s - 1] = BANG
        if s + k.size < total:
            hay[s + k.size] = BANG
        spans.append((s, s + k.size))

    zones = [(b - 48, b + 48) for b in boundaries]
    pos = 8
    for p in order.tolist():
        i, force = plants[p]
        L = len(folded[i])
        pos += 1 + int(rng.integers(0, 6))
        for lo, hi in zones:
            if pos + L + 1 > lo and pos - 1 < hi:
                pos = hi + 1
        if not plane and pos + L + 1 >= a0:
            break
        assert pos + L + 1 < a0, "the plants do not fit in front of the copy of the plane"
        put(pos, i, force)
        pos += L + 1
    for q, b in enumerate(boundaries):
        i = ok[(7 * q) % len(ok)]
        L = len(folded[i])
        put(b - 1 if L == 1 else b - (L + 1) // 2, i)
    i = ok[(7 * len(boundaries)) % len(ok)]
    put(total - len(folded[i]), i)
    return hay, spans


# ---- the dictionaries -----------------------------------------------------------------------------------------------------------

def _words(rng, pre, alpha, n, lo, hi, word=None):
    """n distinct random strings over the folded alphabet, each in a random raw spelling"""
    alpha = np.asarray(alpha, dtype=np.uint16)
    seen = {}
    for _ in range(n):
        f = alpha[rng.integers(0, len(alpha), int(rng.integers(lo, hi + 1)))]
        seen.setdefault(f.tobytes(), f)
    return [spell(rng, pre, f, word) for f in seen.values()]


def word_alphabet(name):
    """Latin, Greek, Cyrillic and CJK units as the table folds them, the targets of the table's own rule among them"""
    T, _ = fold_table(name)
    own = np.unique(T[np.flatnonzero(T != LOWER)])
    base = np.concatenate([_u("abcdefghik"), np.array([0x00E9, 0x03B1, 0x03B2, 0x03B3, 0x03B4, 0x0430, 0x0431, 0x0432, 0x0433, 0x4E2D, 0x9FA0], np.uint16)])
    a = np.unique(np.concatenate([base, own[:12].astype(np.uint16)]))
    return a[fold_table(name)[1][a] != 0]


# name -> (family, mode, table, dictionary, tunables of the build, tunables of the call, what prof["scan_kernel"] must say)
# a kernel given as "=x": equal to x; "^x": starts with x; "!x": does not start with x; a callable: called with the name; None: any
def _fold_range_form(k):  # (tests/test_gpu_parity.py: folded range classes with the packed filter; not the merged stretches)
    if not k.startswith("k_ac_tile<"):
        return False
    a = k.split("<")[1].rstrip(">").split(", ")
    return a[1] == "false" and len(a) >= 6 and a[4] == "false" and a[5] == "true"


def _merged_form(k):
    if not k.startswith("k_ac_tile<"):
        return False
    a = k.split("<")[1].rstrip(">").split(", ")
    return len(a) >= 6 and a[1:6] == ["false", "false", "false", "true", "true"]


def _no_range_form(k):
    return k.startswith("k_ac_tile<") and not _fold_range_form(k) and not _merged_form(k)


STATES_ALWAYS, FOLLOW_ALWAYS_NO_BITS = 6, 5
CASES = {}
for _t, _short, _long in (("java", "^k_ww_pp<3,", "=k_ww_tile<1>"), ("wide", "^k_ww_pp<1,", "=k_ww_tile<1>"),
                          ("manydeltas", "^k_ww_pp<1,", "=k_ww_tile<1>"), ("huge", "=k_ww_tile<2>", "=k_ww_tile<2>"),
                          ("inconsistent", None, None)):
    CASES["ww_short_" + _t] = (FAM_WHOLEWORD, N.MODE_WHOLEWORD, _t, "ww_short", {}, {}, _short)
    CASES["ww_long_" + _t] = (FAM_WHOLEWORD, N.MODE_WHOLEWORD, _t, "ww_long", {}, {}, _long)
for _t in ("java", "manydeltas", "wide", "huge", "inconsistent"):
    CASES["wwl_" + _t] = (FAM_WWLONGEST, N.MODE_WWLONGEST, _t, "phrases", {}, {}, None)
for _f, _fam, _mode, _call, _k in (("tile", FAM_AC, N.MODE_ALL, {"force_kernel": 2}, "^k_ac_tile<"),
                                   ("dfa", FAM_AC, N.MODE_ALL, {"force_kernel": 1}, "^k_ac_dfa<"),
                                   ("longest", FAM_LONGEST, N.MODE_LONGEST, {}, None),
                                   ("shortest", FAM_SHORTEST, N.MODE_SHORTEST, {}, None)):
    _tile = _f == "tile"
    CASES[_f + "_range_java"] = (_fam, _mode, "java", "cyrillic", {}, _call, _fold_range_form if _tile else _k)
    CASES[_f + "_range_far_top"] = (_fam, _mode, "farpartner", "far_top", {}, _call, _fold_range_form if _tile else _k)
    CASES[_f + "_range_far_low"] = (_fam, _mode, "farpartner", "far_low", {}, _call, _no_range_form if _tile else _k)
    CASES[_f + "_merged_java"] = (_fam, _mode, "java", "two_scripts", {}, _call, _merged_form if _tile else _k)
    CASES[_f + "_scatter"] = (_fam, _mode, "scatter", "scatter", {}, _call, "=k_ac_tile<3, false, true, false>" if _tile else _k)
    CASES[_f + "_scatter_no_pages"] = (_fam, _mode, "scatter", "scatter", {"no_class_pages": 1}, _call, "=k_ac_tile<3, false, true, false>" if _tile else _k)
    CASES[_f + "_sparse_wide"] = (_fam, _mode, "wide", "mixed", {"force_sparse": 1}, _call, "=k_ac_scan_sparse" if _f == "dfa" else None)
    CASES[_f + "_rotate"] = (_fam, _mode, "rotate", "rotate", {}, _call, _k)
# cls_pages that do not fit behind the tile kernel's filter rows: bucketed classes (K = 3: 32 KB of rows) over 300 units, 225 distinct pages
for _b in ({}, {"no_class_pages": 1}):
    CASES["tile_scatter_bucketed" + ("_no_pages" if _b else "")] = (FAM_AC, N.MODE_ALL, "scatter", "scatter_bucketed", _b, {"force_kernel": 2},
                                                                     "=k_ac_tile<3, false, true, false, true>")
# the scans that read dfa_pages and have no form without them: tables whose class pages fit (k_ac_states: 51 distinct pages;
# k_longest_follow, which has 12 KB for rows and pages: 13), and "scatter", with which these forms cannot be taken
CASES["states_huge"] = (FAM_AC, N.MODE_ALL, "huge", "huge", {}, {"all_form": STATES_ALWAYS}, "=k_ac_states")
CASES["states_scatter"] = (FAM_AC, N.MODE_ALL, "scatter", "scatter", {}, {"all_form": STATES_ALWAYS}, "!k_ac_states")
CASES["follow_wide"] = (FAM_LONGEST, N.MODE_LONGEST, "wide", "wide_targets", {}, {"longest_form": FOLLOW_ALWAYS_NO_BITS}, "=k_longest_follow")
CASES["follow_scatter"] = (FAM_LONGEST, N.MODE_LONGEST, "scatter", "scatter", {}, {"longest_form": FOLLOW_ALWAYS_NO_BITS}, "!k_longest_follow")
# every tunable a case may set, with the value it goes back to
KNOBS = [("force_kernel", 0), ("all_form", 0), ("longest_form", 0), ("no_class_pages", 0), ("force_sparse", 0)]


def dictionary(kind, table, rng):
    """the raw keywords of a case"""
    T, word = fold_table(table)
    pre = preimages(T)
    if kind in ("ww_short", "ww_long"):
        kws = _words(rng, pre, word_alphabet(table), 300, 1, 16, word)
        if kind == "ww_long":  # more than 32 units: k_ww_tile
            a = word_alphabet(table)
            kws.append(spell(rng, pre, a[rng.integers(0, len(a), 40)], word))
        return kws
    if kind == "phrases":  # words, and two words with a space between them
        ws = _words(rng, pre, word_alphabet(table), 200, 1, 9, word)
        sp = np.array([SPACE], np.uint16)
        two = [np.concatenate([ws[int(rng.integers(0, len(ws)))], sp, ws[int(rng.integers(0, len(ws)))]]) for _ in range(150)]
        return ws + two
    alpha = {"cyrillic": list(range(0x0430, 0x044A)), "far_top": FAR_TOP, "far_low": FAR_LOW,
             "two_scripts": list(range(ord("b"), ord("i"))) + list(range(0x03B1, 0x03B8)),  # (without i: U+0130 lies in the low zone of Greek)
             "scatter": SCATTER_ALPHA, "scatter_bucketed": list(range(0x4E00, 0x4E00 + 300)), "mixed": word_alphabet(table).tolist(),
             "rotate": ROT + [0, ord("f"), ord("g"), ord("h")],
             "huge": [pg << 8 for pg in HUGE_PAGES], "wide_targets": [pg << 8 for pg in WIDE_PAGES]}[kind]
    kws = _words(rng, pre, alpha, 2000 if kind == "scatter_bucketed" else 300, 3 if kind == "scatter_bucketed" else 4, 9)
    if kind in ("huge", "wide_targets"):  # (every unit a keyword: no selective filter, the dictionaries k_longest_follow is for)
        kws += [spell(rng, pre, [f]) for f in alpha]
    return kws


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(keywords, text, planted spans, lower, word or None) of a case; the same arrays for every caller"""
    fam, _, table, kind, _, _, _ = CASES[name]
    T, word = fold_table(table)
    rng = np.random.default_rng(sum(map(ord, name)) * 977 + 5)
    kws = dictionary(kind, table, rng)
    ww = fam in (FAM_WHOLEWORD, FAM_WWLONGEST)
    hay, spans = preimage_text(rng, T, kws, N_UNITS, BOUNDARIES, word if ww else None, minimal=fam == FAM_SHORTEST)
    hay.setflags(write=False)
    return kws, hay, spans, T, (word if ww else None)


def case_oracle(name, lower=None):
    """the oracle of a case, built with the case's table (or with `lower` in its place); Map records"""
    fam = CASES[name][0]
    kws, _, _, T, word = case_inputs(name)
    return Oracle(fam, kws, case_sensitive=False, lower=T if lower is None else lower, word_chars=word, map_flavour=(fam == FAM_WWLONGEST))


@functools.lru_cache(maxsize=None)
def case_records(name):
    """the oracle's records of a case's text, computed once"""
    want = case_oracle(name).match(case_inputs(name)[1], cap=1 << 20)
    want.setflags(write=False)
    return want
