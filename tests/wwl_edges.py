"""The shared dictionary and text of the WholeWordLongest edge suites (tests/test_gpu_wwlongest_edges.py, tests/test_wwlongest_table_cpu.py)
and what can be said about them without a device: a plain trie of the trimmed, folded keywords, the walk starts of a text, and
the regime the oracle's records reach.  Test code only; nothing here touches the library."""
import functools

import numpy as np

from oracle.oracle import FAM_WWLONGEST, Oracle, trim
from tests.helpers import LOWER, WORD

# Latin, Latin-1 and Greek pairs: every unit folds onto another one of the alphabet or is the folded form itself
ALPHA = np.array([ord(c) for c in "abAB"] + [0x00E9, 0x00C9, 0x03B1, 0x0391], dtype=np.uint16)
SWAP = {int(x): int(y) for x, y in zip(ALPHA[[0, 1, 2, 3, 4, 5, 6, 7]], ALPHA[[2, 3, 0, 1, 5, 4, 7, 6]])}
SP = np.array([32], np.uint16)
COMMA_SP = np.array([44, 32], np.uint16)
FIRST_LENS = (1, 2, 5, 11, 12, 13, 14, 16, 17, 24, 40)
INLINE = 12  # kWwInlineUnits: the longest first word the first-word table settles
SEEDS = {True: 4100, False: 4101}  # case_sensitive -> seed; chosen so that regime() holds (asserted by both suites)
CLASSES = ("single_short", "single_long", "phrase_short", "phrase_long", "first_12", "first_13", "carried")


def cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.uint16) for p in parts]).astype(np.uint16)


def other_unit(rng, u):
    """a unit of the alphabet that is not u"""
    while True:
        c = int(ALPHA[int(rng.integers(len(ALPHA)))])
        if c != int(u):
            return c


def edge_dictionary(rng):
    """-> (keywords, first words).  First words of every length in FIRST_LENS: three drawn at random, for each of those (from 2
    units on) one that shares all but its last unit, and one that is a proper prefix of a first word of the next length.  Every
    first word stands in up to four forms -- alone, first + " " + second, first + " " + w + ", " + w -- every fourth one ONLY
    inside phrases and every fourth one only alone; a few keywords are given twice."""
    firsts, seen = [], set()

    def add(w):
        if tuple(w.tolist()) in seen:
            return False
        seen.add(tuple(w.tolist()))
        firsts.append(w.astype(np.uint16))
        return True

    bases = {}
    for ln in FIRST_LENS:
        bases[ln] = []
        for _ in range(2 if ln == 1 else 3):
            while True:
                w = ALPHA[rng.integers(0, len(ALPHA), ln)]
                if add(w):
                    break
            bases[ln].append(w)
            if ln >= 2:
                s = w.copy()
                s[-1] = other_unit(rng, s[-1])
                add(s)
    for ln, nxt in zip(FIRST_LENS[:-1], FIRST_LENS[1:]):
        add(bases[nxt][0][:ln])  # a proper prefix of another first word
    kws = []
    for i, f in enumerate(firsts):
        phrase_only = i % 4 == 3
        if not phrase_only:
            kws.append(f)
        if i % 4 == 1:  # alone only: a walk ends on it (unless it is another first word's prefix)
            continue
        if phrase_only or i % 3 != 0:
            second = firsts[int(rng.integers(len(firsts)))] if rng.integers(3) == 0 else ALPHA[rng.integers(0, len(ALPHA), int(rng.integers(1, 6)))]
            kws.append(cat(f, SP, second))
        if phrase_only or i % 3 != 1:
            w = ALPHA[rng.integers(0, len(ALPHA), int(rng.integers(1, 5)))]
            kws.append(cat(f, SP, w, COMMA_SP, w))
    # duplicates: "last one wins" for first words that end a walk, first words that go on, and phrases
    for i in (1, 5, 9, 13, 17, 0, 2, 4, 8):  # (1 mod 4: alone only -- a keyword id in the first-word table)
        kws.append(firsts[i].copy())
    for j in rng.choice(len(kws), 4, replace=False):
        kws.append(kws[int(j)].copy())
    return kws, firsts


def edge_text(rng, kws, n_tokens, flips):
    """Tokens with one or two spaces between them: a keyword; a keyword with one unit changed (anywhere, the last unit, units 12,
    13 and 14); one unit longer; one unit shorter; with `flips`, a keyword with the case of some units flipped."""
    parts = []
    for _ in range(n_tokens):
        k = kws[int(rng.integers(len(kws)))].copy()
        kind = int(rng.integers(0, 10 if flips else 8))
        if kind in (2, 3):
            where = [int(rng.integers(len(k))), len(k) - 1] + [p for p in (11, 12, 13) if p < len(k)]
            p = where[int(rng.integers(len(where)))]
            k[p] = other_unit(rng, k[p])
        elif kind == 4:
            k = cat(k, [ALPHA[int(rng.integers(len(ALPHA)))]])
        elif kind == 5 and len(k) > 1:
            k = k[:-1]
        elif kind >= 8:
            flip = rng.integers(0, 2, len(k)) == 1
            k = np.array([SWAP.get(int(u), int(u)) if f else int(u) for u, f in zip(k, flip)], np.uint16)
        parts += [k, SP if rng.integers(2) else cat(SP, SP)]
    return cat(*parts[:-1])  # (ends inside or at the end of a word)


def fold_units(units, cs):
    u = np.asarray(units, dtype=np.uint16)
    return u if cs else LOWER[u].astype(np.uint16)


class Trie:
    """A plain trie of the trimmed, folded keywords: children[node] = {unit: node}, kw[node] = the id of the LAST keyword that
    ends there (-1: none), depth[node]."""

    def __init__(self, kws, cs, word=WORD):
        self.cs = cs
        self.children, self.kw, self.depth = [{}], [-1], [0]
        for i, k in enumerate(kws):
            t = fold_units(trim(k, word), cs).tolist()
            if not t:
                continue
            node = 0
            for u in t:
                nxt = self.children[node].get(u)
                if nxt is None:
                    nxt = len(self.children)
                    self.children[node][u] = nxt
                    self.children.append({})
                    self.kw.append(-1)
                    self.depth.append(self.depth[node] + 1)
                node = nxt
            self.kw[node] = i

    def walk_stop(self, folded, start):
        """where a walk from `start` leaves the trie (or the text ends)"""
        node, i = 0, start
        while i < len(folded):
            nxt = self.children[node].get(folded[i])
            if nxt is None:
                break
            node, i = nxt, i + 1
        return i

    def word_paths(self, word=WORD):
        """{units of an all-word path: (node, is a keyword, goes on with a non-word unit)} over every depth"""
        out, stack = {}, [(0, ())]
        while stack:
            node, path = stack.pop()
            if node:
                out[path] = (node, self.kw[node] >= 0, any(not word[u] for u in self.children[node]))
            for u, c in self.children[node].items():
                if word[u]:
                    stack.append((c, path + (u,)))
        return out


def walk_starts(hay, word=WORD, text_begin=True):
    """positions the scan can start a walk at: word characters whose left neighbour is none, and position 0 of the text"""
    w = word[np.asarray(hay, dtype=np.uint16)].astype(bool)
    s = w.copy()
    s[1:] &= ~w[:-1]
    if text_begin and len(s):
        s[0] = True
    return np.flatnonzero(s)


def record_classes(recs, hay, trie, word=WORD):
    """{class: number of records} from the oracle's records, the text and the dictionary alone (CLASSES):
    single / phrase: the record holds no / a non-word unit; short / long: its first word has at most / more than 12 units;
    carried: the walk from the record's start follows the trie for at least two units past the record's end before it leaves
    -- what is reported is the fail match carried along a longer keyword."""
    hay = np.asarray(hay, dtype=np.uint16)
    folded = fold_units(hay, trie.cs).tolist()
    w = word[hay].astype(bool)
    out = dict.fromkeys(CLASSES, 0)
    for s, e, _ in recs.tolist():
        nonword = np.flatnonzero(~w[s:e])
        first = int(nonword[0]) if len(nonword) else e - s
        kind = ("phrase" if len(nonword) else "single") + ("_short" if first <= INLINE else "_long")
        out[kind] += 1
        if first == INLINE:
            out["first_12"] += 1
        if first == INLINE + 1:
            out["first_13"] += 1
        if trie.walk_stop(folded, s) >= e + 2:
            out["carried"] += 1
    return out


class Case:
    pass


@functools.lru_cache(maxsize=None)
def edge_case(cs, n_tokens=1500):
    """The edge dictionary, the edge text and the oracle's records of one case rule: computed once, shared, never changed."""
    c = Case()
    rng = np.random.default_rng(SEEDS[cs])
    c.cs = cs
    c.kws, c.firsts = edge_dictionary(rng)
    c.hay = edge_text(rng, c.kws, n_tokens, flips=not cs)
    c.hay.setflags(write=False)
    c.oracle = oracle_for(c.kws, cs)
    c.recs = c.oracle.match(c.hay, cap=c.hay.size)
    c.recs.setflags(write=False)
    c.trie = Trie(c.kws, cs)
    return c


def oracle_for(kws, cs, map_flavour=False):
    return Oracle(FAM_WWLONGEST, kws, case_sensitive=cs, lower=LOWER, word_chars=WORD, map_flavour=map_flavour)


def regime(c, at_least=20):
    """Asserts that the edge text reaches every class of record_classes() at least `at_least` times, whatever a device answers."""
    assert c.hay.size <= 40000, c.hay.size
    counts = record_classes(c.recs, c.hay, c.trie)
    for k in CLASSES:
        assert counts[k] >= at_least, (c.cs, k, counts)
    return counts
