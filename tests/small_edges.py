"""The inputs of the one-launch edge suites (tests/test_gpu_one_launch_edges.py, tests/test_one_launch_inputs_cpu.py): short host
texts for k_small<MODE> (csrc/acgpu_small.hip) at the edges of its lists -- kSmallMaxRecs occurrences, kSmallMaxLen units per
keyword, kSmallMaxUnits units of text, the lane seams p = t + k * 1024, the last round of the Longest pointer doubling, WholeWord
runs on the seams and at both ends of the text, U+0000 against the zero padding, units from 0x8000 on, duplicates after folding.

One function per case builds the dictionary and the texts, takes the records from the CPU oracle and ASSERTS that the input reaches
what it is for -- from the text, the dictionary and the oracle alone.  Whether the one launch may answer a call (`one_launch`)
restates its gate (match_host_text and small_call_supported) on the same evidence: 1 .. 4096 units, no keyword beyond 256 units, a
family with a kernel there, a fold-consistent word table, and for ALL / SHORTEST at most 4096 occurrences of ALL keywords -- counted
by Oracle(FAM_AC) on the same dictionary.  Test code only; nothing here touches the library."""
import functools

import numpy as np

from ahocorasick_amd import synth
from ahocorasick_amd.strings import utf16
from oracle.oracle import FAM_AC, FAM_LONGEST, FAM_SHORTEST, FAM_WHOLEWORD, FAM_WWLONGEST, Oracle
from tests.helpers import LOWER, WORD

MAX_UNITS, MAX_RECS, MAX_LEN, BLOCK = 4096, 4096, 256, 1024  # kSmallMaxUnits, kSmallMaxRecs, kSmallMaxLen, kSmallBlock
SEAMS = (1024, 2048, 3072)  # lane t walks from t, t + 1024, t + 2048 and t + 3072
FAMILY = {"all": FAM_AC, "longest": FAM_LONGEST, "wholeword": FAM_WHOLEWORD, "shortest": FAM_SHORTEST, "wwlongest": FAM_WWLONGEST}
A, B, X, SPACE = ord("a"), ord("b"), ord("x"), 32


def units(*parts):
    """str, lists of units and arrays, joined"""
    return np.concatenate([utf16(p) if isinstance(p, str) else np.asarray(p, dtype=np.uint16).reshape(-1) for p in parts] +
                          [np.zeros(0, np.uint16)]).astype(np.uint16)


class Dictionary:
    """keywords with their case rule and tables; shared by the cases that use it (an automaton is built once per family)"""

    def __init__(self, kws, cs=True, word=None, lower=None):
        self.kws = [units(k) for k in kws]
        self.cs = cs
        self.word = word
        self.lower = None if cs else (LOWER if lower is None else lower)

    def fold(self, u):
        u = np.asarray(u, dtype=np.uint16)
        return u if self.cs else self.lower[u].astype(np.uint16)

    def folded(self):
        return [tuple(self.fold(k).tolist()) for k in self.kws]

    def max_len(self):
        return max(len(k) for k in self.kws)

    def oracle(self, family):
        return Oracle(family, self.kws, case_sensitive=self.cs, lower=self.lower,
                      word_chars=self.word if family in (FAM_WHOLEWORD, FAM_WWLONGEST) else None)

    def occurrences(self, hay):
        """how many occurrences of ANY keyword the text holds: what k_small counts in n_found for ALL and SHORTEST"""
        return len(self.oracle(FAM_AC).match(hay, cap=2 * MAX_RECS))


class Case:
    """One call: family, dictionary, text, the oracle's records, and whether the one launch answers it.
    why (one_launch False): "records" | "max_len" | "fold" | "family" | "units" -- checked here, on the input alone."""

    def __init__(self, name, mode, d, hay, why=None):
        self.name, self.mode, self.d, self.why = name, mode, d, why
        self.one_launch = why is None
        self.hay = units(hay)
        self.hay.setflags(write=False)
        self.recs = d.oracle(FAMILY[mode]).match(self.hay)
        self.recs.setflags(write=False)
        n = self.hay.size
        held = 1 <= n <= MAX_UNITS and d.max_len() <= MAX_LEN and mode != "wwlongest"
        if mode == "wholeword":
            held = held and (d.cs or bool((d.word == d.word[d.lower]).all()))
        self.n_all = d.occurrences(self.hay) if mode in ("all", "shortest") else None
        if self.n_all is not None:
            held = held and self.n_all <= MAX_RECS
        assert held == self.one_launch, (name, mode, n, d.max_len(), self.n_all)
        if why is not None:
            assert {"records": self.n_all is not None and self.n_all > MAX_RECS, "max_len": d.max_len() > MAX_LEN, "units": n > MAX_UNITS,
                    "family": mode == "wwlongest", "fold": mode == "wholeword" and not d.cs and bool((d.word != d.word[d.lower]).any())}[why], (name, why)

    def __repr__(self):
        return "%s[%s]" % (self.name, self.mode)


def spans(c):
    return [(s, e) for s, e, _ in c.recs.tolist()]


# ---- a. the record lists, full and one beyond ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_a():
    """a^1 .. a^90 and b over x a^90 x [b x [b x]]: 90 * 91 / 2 = 4095 occurrences inside the run, up to 90 with one end, and 0, 1 or 2
    more -- `m > kSmallMaxRecs` at 4095, 4096 and 4097, the counting sort with `recs` and `sorted` full, the rank loop with 90
    occurrences in one end.  And the plain full list: a on a^4096."""
    d = Dictionary([np.full(k, A, np.uint16) for k in range(1, 91)] + ["b"])
    one = Dictionary(["a"])
    out = []
    for mode in ("all", "shortest"):
        for extra in (0, 1, 2):
            hay = units([X], np.full(90, A), [X], [B, X] * extra)
            c = Case("a_%d" % (4095 + extra), mode, d, hay, why="records" if extra == 2 else None)
            assert c.n_all == 4095 + extra
            ends = np.bincount(d.oracle(FAM_AC).match(hay, cap=2 * MAX_RECS)[:, 1])
            assert ends.max() == 90 and (ends > 8).sum() >= 80  # more than 8 occurrences share an end
            assert len(c.recs) == (c.n_all if mode == "all" else 90 + extra)
            out.append(c)
        c = Case("a_full", mode, one, np.full(MAX_UNITS, A))
        assert c.n_all == MAX_RECS == len(c.recs) and c.hay.size == MAX_UNITS
        out.append(c)
    return out


# ---- b. keywords of 255, 256 and 257 units ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_b():
    """Keywords of 255 and 256 units over {a, b} with short prefixes and suffixes of theirs, planted in x's: from unit 0, across 1024,
    2048 and 3072, and up to the last unit of texts of 4096, 4095 and 1025 units -- walks of 256 steps over the lane seams and onto
    unit n.  The same with a keyword of 257 units in the dictionary, and that keyword alone: not the one launch's."""
    rng = np.random.default_rng(5100)
    k255, k256, k257 = (np.array([A, B], np.uint16)[rng.integers(0, 2, ln)] for ln in (255, 256, 257))
    short = [k256[:7], k256[-7:], k255[:4], k255[-4:], k256[:1]]
    d256 = Dictionary([k255, k256] + short)
    d257 = Dictionary([k255, k256, k257] + short)
    alone = Dictionary([k257])
    assert (d256.max_len(), d257.max_len(), alone.max_len()) == (256, 257, 257)

    def text(n, plants):
        hay = np.full(n, X, np.uint16)
        for p, k in plants:
            assert (hay[max(p - 1, 0):p + len(k) + 1] == X).all() and p + len(k) <= n
            hay[p:p + len(k)] = k
        return hay

    texts = {4096: text(4096, [(0, k256), (300, k255), (924, k256), (1793, k256), (2300, k257), (3071, k255), (3840, k256)]),
             4095: text(4095, [(0, k255), (1023, k256), (2047, k256), (2400, k257), (2817, k256), (3840, k255)]),
             1025: text(1025, [(0, k256), (400, k257), (769, k256)])}
    out = []
    for n, hay in texts.items():
        for mode in ("all", "shortest", "longest"):
            c = Case("b_%d" % n, mode, d256, hay)
            out.append(c)
            if mode == "shortest":
                continue
            long_ones = [(s, e) for s, e in spans(c) if e - s >= 255]
            assert (0, 256 if n != 4095 else 255) in long_ones and any(e == n for _, e in long_ones), (n, mode)
            for seam in SEAMS:
                assert seam > n or any(s < seam < e for s, e in long_ones), (n, mode, seam)
            if n != 1025:  # a walk that starts on the last unit in front of a seam, one that crosses it with its last unit
                assert any(s % BLOCK == BLOCK - 1 for s, _ in long_ones) and any(e % BLOCK == 1 for _, e in long_ones)
    for mode in ("all", "shortest", "longest"):
        c = Case("b_257", mode, d257, texts[4096], why="max_len")
        assert mode == "shortest" or (2300, 2557) in spans(c)
        out.append(c)
    out.append(Case("b_257_alone", "all", alone, texts[1025], why="max_len"))
    assert spans(out[-1]) == [(400, 657)]
    return out


# ---- c. a large dictionary -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_c():
    """20 000 random keywords of 3 to 12 letters (a hashed goto table of some 150 000 edges: probe sequences of every length) over
    4096 random letters with 200 plants, one every 20 units: keywords whole, with their last unit changed, without it."""
    kws = synth.random_keywords(5200, 20000, 3, 12)
    d = Dictionary(kws)
    rng = np.random.default_rng(5201)
    hay = synth.haystack(5202, MAX_UNITS).copy()
    whole = []
    for i in range(200):
        k = kws[int(rng.integers(len(kws)))].copy()
        p = 20 * i + int(rng.integers(0, 8))
        kind = 0 if i in (0, 199) else i % 4  # (the first plant begins the text, the last one ends it: both whole)
        if i == 0:
            p = 0
        if i == 199:
            p = MAX_UNITS - len(k)
        if kind == 2:
            k[-1] = A + (int(k[-1]) - A + 1 + int(rng.integers(25))) % 26
        elif kind == 3:
            k = k[:-1]
        else:
            whole.append((p, p + len(k)))
        hay[p:p + len(k)] = k
    out = [Case("c_large", mode, d, hay) for mode in ("all", "longest")]
    assert len(kws) == 20000 and out[0].n_all <= MAX_RECS and out[0].n_all >= 300, out[0].n_all
    got = set(spans(out[0]))
    assert all(w in got for w in whole) and (0, whole[0][1]) in got and whole[-1][1] == MAX_UNITS
    assert len(out[1].recs) >= 200
    return out


# ---- d. the depth of the Longest chain -------------------------------------------------------------------------------------------
D_LENGTHS = (1, 2, 3, 1023, 1024, 1025, 4095, 4096)


@functools.lru_cache(maxsize=None)
def case_d():
    """{b, bb} on x^(n - 1) b: every jump of the chain is 1 and its only match is the last unit -- the mark reaches it in the LAST
    round of the pointer doubling (`span < n`), at n = 2^k and 2^k +- 1.  On x^(n - 2) bb the last jump is 2, onto n.  A keyword of
    256 units every 300: jumps of 256 between runs of single steps."""
    d = Dictionary(["b", "bb"])
    out = []
    for n in D_LENGTHS:
        c = Case("d_b_%d" % n, "longest", d, units(np.full(n - 1, X), "b"))
        assert c.recs.tolist() == [[n - 1, n, 0]] and not np.isin(c.hay[:n - 1], [B]).any()
        out.append(c)
    for n in (2, 3, 1024, 1025, 4096):
        c = Case("d_bb_%d" % n, "longest", d, units(np.full(n - 2, X), "bb"))
        assert c.recs.tolist() == [[n - 2, n, 1]]
        out.append(c)
    rng = np.random.default_rng(5300)
    k256 = np.array([ord("c"), ord("d")], np.uint16)[rng.integers(0, 2, 256)]
    d3 = Dictionary(["b", "bb", k256])
    hay = np.full(MAX_UNITS, X, np.uint16)
    at = list(range(0, 3301, 300)) + [MAX_UNITS - 256]
    for p in at:
        hay[p:p + 256] = k256
    hay[260], hay[270:272], hay[3838] = B, B, B
    c = Case("d_jumps", "longest", d3, hay)
    assert [s for s, e in spans(c) if e - s == 256] == at and len(c.recs) == len(at) + 3 and c.recs[-1, 1] == MAX_UNITS
    out.append(c)
    return out


# ---- e. WholeWord runs -----------------------------------------------------------------------------------------------------------
def runs(hay, word=WORD):
    """the maximal stretches of word characters -> [(start, end)]"""
    w = np.concatenate([[False], word[np.asarray(hay, dtype=np.uint16)].astype(bool), [False]])
    edge = np.flatnonzero(w[1:] != w[:-1])
    return list(zip(edge[0::2].tolist(), edge[1::2].tolist()))


def lay(n, plants):
    """spaces with the plants in them, at least one space between two"""
    hay = np.full(n, SPACE, np.uint16)
    for p, k in plants:
        assert p + len(k) <= n and (hay[max(p - 1, 0):p + len(k) + 1] == SPACE).all(), p
        hay[p:p + len(k)] = k
    return hay


@functools.lru_cache(maxsize=None)
def case_e(cs):
    """Keywords of 1, 2, 31 and 200 letters in spaces.  Runs that start at 0, 1023, 1024 and 1025, end at 1024, 2048, 3072 and on the
    text's last unit (`wordf[min(pos, kSmallMaxUnits)]` reads the zero behind it), runs of a keyword and one letter more -- inside
    the text and as its last unit -- and of a keyword without its last letter, neighbours with one space between them.
    Case-insensitive: the keywords and every plant in a case of their own."""
    rng = np.random.default_rng(5400 + cs)
    low = np.arange(A, A + 26, dtype=np.uint16)
    w1, w2, w31, w200 = units("q"), units("ab"), low[rng.integers(0, 26, 31)], low[rng.integers(0, 26, 200)]
    z = units("z")

    def cased(k):
        """case-insensitive: every other letter or so in upper case"""
        k = units(k)
        return k if cs else np.where((rng.integers(0, 2, len(k)) == 1) & (k >= A) & (k < A + 26), k - 32, k).astype(np.uint16)

    d = Dictionary([cased(k) for k in (w1, w2, w31, w200)], cs=cs, word=WORD)
    more = lambda k: units(k, z)
    texts = {
        "A": lay(4096, [(0, w2), (3, w31), (35, w1), (40, more(w2)), (50, more(w1)), (60, more(w31)), (100, w31[:-1]), (140, w2[:-1]),
                        (150, more(w200)), (360, w200[:-1]), (600, w200), (1023, w1), (1025, w2), (1848, w200), (2950, w200), (4065, w31)]),
        "B": lay(4095, [(0, w200), (1024, w200), (2017, w31), (2049, w2), (3071, w2), (4060, more(w31)), (4094, w1)]),
        "C": lay(3073, [(0, more(w31)), (993, w31), (1025, w31[:-1]), (2047, w1), (2872, w200)]),
        "D": lay(1024, [(0, w1), (2, w1), (824, w200)]),
        "E": lay(202, [(1, more(w200))]),
        "F": lay(200, [(1, w200[:-1])]),
        "G": lay(1, [(0, w1)]),
    }
    kw_set = set(d.folded())
    out, starts, ends, at_n, plus, minus, neighbours = [], set(), set(), 0, set(), set(), 0
    for name, hay in texts.items():
        hay = cased(hay)
        c = Case("e_%s_%s" % ("cs" if cs else "ci", name), "wholeword", d, hay)
        exact = []
        for s, e in runs(hay):
            f = tuple(d.fold(hay[s:e]).tolist())
            if f in kw_set:
                exact.append((s, e))
            elif f[:-1] in kw_set:
                plus.add((len(f) - 1, e == hay.size))
            elif any(k[:-1] == f for k in kw_set):
                minus.add((len(f) + 1, e == hay.size))
        assert spans(c) == exact, (name, spans(c), exact)  # a record is a run that is a keyword, nothing else
        starts |= {s for s, _ in exact}
        ends |= {e for _, e in exact}
        at_n += bool(exact) and exact[-1][1] == hay.size
        neighbours += sum(1 for (_, e0), (s1, _) in zip(exact, exact[1:]) if e0 + 1 == s1)
        out.append(c)
    assert {0, 1023, 1024, 1025} <= starts and set(SEAMS) <= ends and at_n >= 4 and neighbours >= 4
    assert plus >= {(1, False), (2, False), (31, False), (200, False), (200, True)} and minus >= {(2, False), (31, False), (200, False), (200, True)}
    if not cs:
        assert any((c.hay != LOWER[c.hay]).any() for c in out) and any((k != LOWER[k]).any() for k in d.kws)
    return out


@functools.lru_cache(maxsize=None)
def case_e_refused():
    """Calls on short texts that are not the one launch's: a word table that is not fold-consistent (A and B are word characters,
    a and b are not), WholeWordLongest, and one unit more than 4096."""
    wc = np.zeros(65536, np.uint8)
    for ch in "ABx":
        wc[ord(ch)] = 1
    out = [Case("e_fold_inconsistent", "wholeword", Dictionary(["A", "AB", "x"], cs=False, word=wc), "AB x A ab", why="fold"),
           Case("e_wwlongest", "wwlongest", Dictionary(["ab", "ab cd"], word=WORD), "ab cd ab x", why="family"),
           Case("e_4097_units", "all", Dictionary(["a"]), units(np.full(MAX_UNITS, X), "a"), why="units")]
    assert out[1].hay.size == 10 and spans(out[1]) == [(0, 5), (6, 8)] and spans(out[2]) == [(4096, 4097)]
    return out


# ---- f. units --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_f():
    """U+0000 in keywords against the zeros behind unit n (texts that end in a, in a 0 and in 0 0, none a multiple of four units
    long); units of 0x8000 and above through edge_key; three keywords that are one after folding."""
    out = []
    zero = Dictionary([[A, 0], [0], [0, 0, B], [A]])
    tails = {"a": [X, A, 0, 0, B, 0, X, 0, A], "a0": [X, 0, 0, B, X, A, 0], "00": [A, X, 0, 0, B, A, 0, 0, 0, 0]}
    for name, hay in tails.items():
        assert len(hay) % 4 != 0
        for mode in ("all", "shortest", "longest"):
            c = Case("f_zero_%s" % name, mode, zero, hay)
            assert max(e for _, e in spans(c)) == len(hay) and all(e <= len(hay) for _, e in spans(c))
            out.append(c)
    high = np.array([0x8000, 0xD800, 0xDFFF, 0xFFFF, 0x4E2D], np.uint16)
    rng = np.random.default_rng(5500)
    kws = [high[rng.integers(0, 5, int(rng.integers(1, 5)))] for _ in range(12)] + [high[[3]], high[[1, 2]], high[[2, 1]]]
    hay = high[rng.integers(0, 5, 601)]
    for mode, cs in (("all", True), ("all", False), ("shortest", True), ("longest", True)):
        c = Case("f_high_%s" % ("cs" if cs else "ci"), mode, Dictionary(kws, cs=cs), hay)
        assert len(c.recs) >= 100 and set(np.unique(hay).tolist()) == set(high.tolist())
        out.append(c)
    for mode in ("all", "shortest", "longest", "wholeword"):
        d = Dictionary(["Ab", "aB", "AB"], cs=False, word=WORD if mode == "wholeword" else None)
        c = Case("f_folded_duplicates", mode, d, "ab Ab,AB aB abab ab")
        assert len(set(d.folded())) == 1 and len(c.recs) >= 5
        # the reference keeps the last duplicate's value, ShortestMatch the first one's
        assert set(c.recs[:, 2].tolist()) == ({0} if mode == "shortest" else {2}), (mode, c.recs.tolist())
        out.append(c)
    return out


# ---- g. two automata in turn on one pool -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_g():
    """One round of calls: an ALL automaton and a WholeWord automaton in turn, on 4096 units and then on 5.  The 5-unit texts follow
    4096-unit ones in the same pinned block: behind their last unit lie stale letters, behind their records stale records."""
    all_a, ww = Dictionary(["a"]), Dictionary(["ab"], word=WORD)
    out = [Case("g_all_4096", "all", all_a, np.full(MAX_UNITS, A)),
           Case("g_ww_4096", "wholeword", ww, units("ab ", np.full(MAX_UNITS - 3, A))),
           Case("g_all_5", "all", all_a, "aa ab"),
           Case("g_ww_5", "wholeword", ww, "aa ab")]
    assert [len(c.recs) for c in out] == [MAX_RECS, 1, 3, 1] and [c.hay.size for c in out] == [4096, 4096, 5, 5]
    assert spans(out[3]) == [(3, 5)]  # the run ends on the text's last unit: what lies behind it must not lengthen it
    return out


GROUPS = {
    "a_record_lists": case_a,
    "b_long_keywords": case_b,
    "c_large_dictionary": case_c,
    "d_longest_chain": case_d,
    "e_wholeword_cs": functools.partial(case_e, True),
    "e_wholeword_ci": functools.partial(case_e, False),
    "e_refused": case_e_refused,
    "f_units": case_f,
    "g_alternating": case_g,
}
