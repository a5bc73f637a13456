"""The inputs of the selection edge suites (tests/test_gpu_selection_edges.py, tests/test_selection_inputs_cpu.py) and a plain model of
the selection itself: run_selection (csrc/acgpu_hostrun.hip) takes the ordered all-matches list, works out a successor per record
(k_short_next / k_long_next, csrc/acgpu_shortest.hip), marks the chain from the entry (mark_chain), and scatters the marked records
(k_short_emit).  Here the list is Oracle(FAM_AC)'s -- end ascending, longest first -- and the successors, the head, the chain and the
jumps are restated over it in a few lines of numpy, with a pure-Python twin for the lists short enough to loop over.

One function per case builds the dictionary and the text and ASSERTS that the input reaches what it is for -- the number of
records M, the chain's length, the head's index, the largest jump, the records per end -- from the model and the oracle alone.
Test code only; nothing here touches the library."""
import functools

import numpy as np

from ahocorasick_amd import synth
from ahocorasick_amd.strings import utf16
from oracle.oracle import FAM_AC, FAM_LONGEST, FAM_SHORTEST, Oracle
from tests.helpers import LOWER

BLOCK = 256               # csrc/acgpu_shortest.hip launch_shortest_select / launch_longest_select / launch_chain_mark: `block(256), grid((M + 1 + 255) / 256)`
MARKS_PER_LAUNCH = 8      # csrc/acgpu_shortest.hip `constexpr int kRoundLog = 3`: k_short_round marks 2^3 chain elements per marked one, `reach <<= kRoundLog`
SCAN_TILE = 2048          # csrc/acgpu_kernels.hip `constexpr int kScanTile = 2048`: the prefix sum over the marks under k_short_emit
MARK_TILE = 512           # csrc/acgpu_hostrun.hip mark_chain `const uint32_t tile_units = 512`: indices per lane of the one pass
JUMP_BLOCK = 64           # csrc/acgpu_wwlongest.hip k_wwl_jumps `blockmax[k >> 6]`: one farthest landing per 64 indices
ONE_PASS_MAX_JUMP = 60000  # csrc/acgpu_hostrun.hip mark_chain `if (max_jump > 60000) one_pass = false`
ONE_PASS_EARLY_FROM = 64  # csrc/acgpu_hostrun.hip mark_chain `(tunables().tile_debug & kSelMarkOnePassEarly) ? 64u : (1u << 22)`
SYNC_SET = 16             # csrc/acgpu_longest.hip `#define ACGPU_SYNC_SET 16`: the distinct landings k_longest_sync follows per tile
MARK_DEFAULT, MARK_DOUBLING, MARK_ONE_PASS_EARLY = 0, 2097152, 4194304  # tile_debug: csrc/acgpu_kernels.h kSelMarkDoubling, kSelMarkOnePassEarly
ALL_MARKERS = (MARK_DEFAULT, MARK_DOUBLING, MARK_ONE_PASS_EARLY)
SHORT_TEXT = 4096         # csrc/acgpu_small.h kSmallMaxUnits: the host entry answers a text of up to 4096 units with k_small

A, B, C = ord("a"), ord("b"), ord("c")
SEAM_M = (1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 32767, 32768, 32769)


def units(*parts):
    """str, lists of units and arrays, joined"""
    return np.concatenate([utf16(p) if isinstance(p, str) else np.asarray(p, dtype=np.uint16).reshape(-1) for p in parts] +
                          [np.zeros(0, np.uint16)]).astype(np.uint16)


# ---- the model -------------------------------------------------------------------------------------------------------------------
def shortest_next(recs):
    """nxt[k]: the first later record that starts at or after record k's end, M if there is none.  A record that starts at or
    after e_k ends behind it, so it IS later in the list: the smallest index among the records with start >= e_k."""
    M = len(recs)
    s, e = recs[:, 0].astype(np.int64), recs[:, 1].astype(np.int64)
    by_start = np.argsort(s, kind="stable")
    first_index_from = np.minimum.accumulate(np.append(by_start, M)[::-1])[::-1]  # the smallest index among the starts from here on
    return first_index_from[np.searchsorted(s[by_start], e, side="left")]


def shortest_head(recs, entry):
    """the first record of the list that starts at or after the entry, M if there is none"""
    at = np.flatnonzero(recs[:, 0] >= entry)
    return int(at[0]) if len(at) else len(recs)


def longest_next(recs, limit):
    """nxt[k]: among the records with e_k <= start < limit the one with the smallest start, the longest at that start; M if none"""
    return longest_from(recs, recs[:, 1], limit)


def longest_from(recs, pos, limit):
    M = len(recs)
    s, e = recs[:, 0].astype(np.int64), recs[:, 1].astype(np.int64)
    order = np.lexsort((-e, s))  # start ascending, the longest first
    at = np.searchsorted(s[order], np.asarray(pos, dtype=np.int64), side="left")
    cand = np.append(order, M)[at]
    start = np.append(s, limit)[cand]
    return np.where(start < limit, cand, M)


def longest_head(recs, entry, limit):
    return int(longest_from(recs, [entry], limit)[0])


def shortest_next_plain(recs):
    """shortest_next as two loops"""
    rows = recs.tolist()
    M = len(rows)
    return np.array([next((j for j in range(k + 1, M) if rows[j][0] >= rows[k][1]), M) for k in range(M)], dtype=np.int64)


def longest_next_plain(recs, limit):
    """longest_next as two loops"""
    rows = recs.tolist()
    M = len(rows)
    out = []
    for k in range(M):
        best = M
        for j in range(M):
            s, e = rows[j][0], rows[j][1]
            if s >= rows[k][1] and s < limit and (best == M or s < rows[best][0] or (s == rows[best][0] and e > rows[best][1])):
                best = j
        out.append(best)
    return np.array(out, dtype=np.int64)


def chain(nxt, head):
    """the indices head, nxt[head], nxt[nxt[head]], ... below M"""
    M, out, k = len(nxt), [], int(head)
    while k < M:
        out.append(k)
        k = int(nxt[k])
    return np.array(out, dtype=np.int64)


def jumps(nxt):
    """nxt[k] - k: what k_wwl_jumps hands the one pass as lengths (a record without a successor jumps to M)"""
    return np.asarray(nxt, dtype=np.int64) - np.arange(len(nxt))


def fold(u, cs):
    u = np.asarray(u, dtype=np.uint16)
    return u if cs else LOWER[u].astype(np.uint16)


def first_duplicate(kws, cs):
    """keyword index -> the index of the first keyword that is the same after folding: ShortestMatchMap keeps the first
    duplicate's value, AhoCorasickMap the last one's"""
    seen, out = {}, []
    for i, k in enumerate(kws):
        out.append(seen.setdefault(tuple(fold(utf16(k), cs).tolist()), i))
    return np.array(out, dtype=np.int32)


class Dictionary:
    """keywords with their case rule and the three oracles over them"""

    def __init__(self, kws, cs=True):
        self.kws = [units(k) for k in kws]
        self.cs = cs
        self.lower = None if cs else LOWER
        self.max_len = max(len(k) for k in self.kws)
        self.first = first_duplicate(self.kws, cs)
        self._oracles = {}

    def oracle(self, family):
        if family not in self._oracles:
            self._oracles[family] = Oracle(family, self.kws, case_sensitive=self.cs, lower=self.lower)
        return self._oracles[family]

    def all_records(self, hay):
        """the all-matches list of the text: every occurrence, end ascending, longest first"""
        hay = units(hay)
        return self.oracle(FAM_AC).match(hay, cap=max(1024, 4 * hay.size))


FAMILY = {"shortest": FAM_SHORTEST, "longest": FAM_LONGEST}


class Selection:
    """What run_selection has to do on one shard of a text, from the oracle's all-matches list and the model alone.
    own = (begin, end) of the shard, entry = its chain entry.  SHORTEST selects among the occurrences whose last unit lies in the
    shard; LONGEST among those that end in it or in the max_len - 1 units behind it, and only those that start before its end.
      .all    the list the selection runs over        .M          its length
      .nxt    every record's successor (M: none)     .head       the index of the chain's first record (M: none)
      .chain  the indices of the selected records    .recs       the selected records, ids as the family reports them
      .exit   the chain exit the call reports        .max_jump   the largest nxt[k] - k"""

    def __init__(self, d, family, hay, all_recs=None, own=None, entry=None):
        hay = units(hay)
        n = hay.size
        self.own = (0, n) if own is None else own
        self.entry = self.own[0] if entry is None else entry
        lo, hi = self.own
        full = d.all_records(hay) if all_recs is None else all_recs
        if family == "shortest":
            keep = (full[:, 1] > lo) & (full[:, 1] <= hi)
        else:
            keep = (full[:, 1] > lo) & (full[:, 1] <= min(n, hi + d.max_len - 1))
        self.all = full[keep]
        self.M = len(self.all)
        if family == "shortest":
            self.nxt = shortest_next(self.all)
            self.head = shortest_head(self.all, self.entry)
        else:
            self.nxt = longest_next(self.all, hi)
            self.head = longest_head(self.all, self.entry, hi) if self.entry < hi else self.M
        self.chain = chain(self.nxt, self.head)
        self.recs = self.all[self.chain].copy()
        if family == "shortest":
            self.recs[:, 2] = d.first[self.recs[:, 2]]
        last = int(self.recs[-1, 1]) if len(self.recs) else None
        if family == "shortest":
            self.exit = self.entry if last is None else last
        else:
            self.exit = max(self.entry, hi) if last is None else max(last, hi)
        self.jumps = jumps(self.nxt)
        self.max_jump = int(self.jumps.max()) if self.M else 0

    def group_sizes(self):
        """how many records share each end"""
        return np.unique(self.all[:, 1], return_counts=True)[1]


class Case:
    """One whole-text call: family, dictionary, text, chain entry; the model's selection and the oracle's records of the family
    (a chain that enters at `entry` is the oracle's on the text from there on)."""

    def __init__(self, name, family, d, hay, entry=0, markers=ALL_MARKERS):
        self.name, self.family, self.d, self.entry, self.markers = name, family, d, entry, markers
        self.hay = units(hay)
        self.hay.setflags(write=False)
        self.sel = Selection(d, family, self.hay, entry=entry)
        self.want = d.oracle(FAMILY[family]).match(self.hay[entry:], cap=max(1024, self.hay.size))
        self.want[:, :2] += entry
        self.want.setflags(write=False)

    def __repr__(self):
        return "%s[%s]" % (self.name, self.family)


# ---- 1. record counts at the kernels' seams --------------------------------------------------------------------------------------
D_A = Dictionary(["a"])
D_A_B = Dictionary(["a", "b"])
D_AB_B = Dictionary(["ab", "b"])


@functools.lru_cache(maxsize=None)
def case_seams(M):
    """Exactly M records in three shapes: `a` on a^M -- every record on the chain, the chain as long as the list, the most launches
    the doubling can need; {a, b} on b^(M-1) a entered at its last unit -- the chain is the list's last record alone; {ab, b} on
    (ab)^(M/2) (an odd M: a `b` in front) -- selected and skipped records in turn."""
    full = Case("seam_full_%d" % M, "shortest", D_A, np.full(M, A))
    assert full.sel.M == M and len(full.sel.chain) == M and full.sel.head == 0 and full.sel.max_jump == 1
    one = Case("seam_one_%d" % M, "shortest", D_A_B, units(np.full(M - 1, B), "a"), entry=M - 1)
    assert one.sel.M == M and one.sel.chain.tolist() == [M - 1] and one.sel.head == M - 1
    alt = Case("seam_alternating_%d" % M, "shortest", D_AB_B, units("b" * (M % 2), "ab" * (M // 2)))
    assert alt.sel.M == M and len(alt.sel.chain) == (M + 1) // 2 and alt.sel.head == 0
    if M >= 4:
        assert set(np.diff(alt.sel.chain).tolist()) <= {1, 2} and (np.diff(alt.sel.chain) == 2).sum() >= M // 2 - 1
    return [full, one, alt]


# ---- 2. k_short_next's group search ----------------------------------------------------------------------------------------------
GROUP_K = 100


def group_position(sel):
    """per record with a successor: (the successor's place in its end group: 0 first, 1 middle, 2 last, -1 a group of one;
    how many end groups on the successor lies)"""
    ends = sel.all[:, 1]
    first = np.searchsorted(ends, ends, side="left")
    last = np.searchsorted(ends, ends, side="right") - 1
    group_no = np.cumsum(np.concatenate([[0], np.diff(ends) != 0]))
    k = np.flatnonzero(sel.nxt < sel.M)
    j = sel.nxt[k]
    place = np.where(first[j] == last[j], -1, np.where(j == first[j], 0, np.where(j == last[j], 2, 1)))
    return k, place, group_no[j] - group_no[k]


@functools.lru_cache(maxsize=None)
def case_groups(cs):
    """a^3 .. a^100, b, ab, aab, aaab, bab and two duplicates over a/b text with a-runs of 1 to 150 units: up to 98 records per
    end.  In `b aab` the record in front of the first a is followed by the FIRST record of the group [aab, ab, b], in `aaab` the
    a-keywords that end two units in front of the b by `ab`, a MIDDLE one, inside a run by a^3, the LAST of its group and three
    groups on.  The text ends in a^120 c^300: the records that end on the run's last three units have no successor, and the
    first of them stands some 290 records in front of the list's end.  Case-insensitive: keywords and text in mixed case."""
    rng = np.random.default_rng(6200 + cs)

    def cased(k):
        k = units(k)
        return k if cs else np.where(rng.integers(0, 2, len(k)) == 1, k - 32, k).astype(np.uint16)

    kws = [cased("a" * k) for k in range(3, GROUP_K + 1)] + [cased(k) for k in ("b", "ab", "aab", "aaab", "bab", "ab", "aaa")]
    d = Dictionary(kws, cs=cs)
    parts = [units("baab"), units("aaab")]
    while sum(len(p) for p in parts) < 3800:
        parts += [np.full(int(rng.choice([1, 2, 3, 5, 40, 110, 150])), A), np.full(int(rng.integers(1, 3)), B)]
    parts += [np.full(120, A), np.full(300, C)]
    c = Case("groups_%s" % ("cs" if cs else "ci"), "shortest", d, cased(units(*parts)))
    sel = c.sel
    assert c.hay.size > SHORT_TEXT and sel.group_sizes().max() == GROUP_K - 2 and (sel.group_sizes() >= 64).sum() >= 100
    k, place, groups_on = group_position(sel)
    assert {0, 1, 2, -1} <= set(place.tolist()), set(place.tolist())
    assert groups_on.max() >= 3 and (groups_on == 1).any()
    dead = np.flatnonzero(sel.nxt == sel.M)
    assert sel.M - int(dead[0]) > BLOCK, (sel.M, dead[0])  # no successor, and more than a block of records behind it
    dup = [i for i in range(len(kws)) if d.first[i] != i]
    assert len(dup) == 2 and set(d.first[dup].tolist()) <= set(c.want[:, 2].tolist()) and not set(dup) & set(c.want[:, 2].tolist())
    assert set(dup) & set(sel.all[:, 2].tolist())  # the all-matches list names the LAST duplicate, the selection the first
    if not cs:
        assert (c.hay != LOWER[c.hay]).any() and any((k != LOWER[k]).any() for k in d.kws)
    return c


# ---- 3. k_long_next's rules ------------------------------------------------------------------------------------------------------
LONG_PAD = 3000  # random keywords of 4 .. 9 letters: with them the suffix filter is selective (info()["tile_kernel"] == 1, asserted where it is used)
NESTED = ("qabc", "qabcde", "qabcdefghijk")  # at one start; the longest is the dictionary's longest keyword, 12 units
OUTER, INNER = "mnopqrstuv", "opqr"           # INNER starts later and ends earlier: earlier in the list, and it loses
HEAD, STRADDLE, TOUCH = "ghijkl", "jklwxyz", "wxyz"  # STRADDLE starts inside HEAD and reaches beyond it; TOUCH starts where HEAD ends
NEVER = "zyxwvutsrqponmlk"                    # 16 units, in no text: max_len 16 without a record that long


@functools.lru_cache(maxsize=None)
def long_dictionary(cs, with_never):
    hand = list(NESTED) + [OUTER, INNER, HEAD, STRADDLE, TOUCH] + ([NEVER] if with_never else [])
    if not cs:
        hand = [h.upper() if i % 2 else h.capitalize() for i, h in enumerate(hand)]
    pad = synth.random_keywords(6301, LONG_PAD, 4, 9)
    d = Dictionary([units(h) for h in hand] + list(pad), cs=cs)
    assert d.max_len == (16 if with_never else 12) and min(len(k) for k in d.kws) >= 4
    return d


def plant_padding(hay, d, at):
    """one of the dictionary's random keywords at each of the positions"""
    pad = d.kws[-LONG_PAD:]
    for i, p in enumerate(at):
        k = pad[(7 * i) % LONG_PAD]
        hay[p:p + len(k)] = k


def long_text(cs, d, n=6000):
    """random letters with the hand-made stretches planted: NESTED at unit 0, OUTER (with INNER inside), HEAD + TOUCH with
    STRADDLE across their seam, NESTED again touching an OUTER, and TOUCH on the text's last units; 80 of the random keywords in
    between, so that the list has more than the 64 records the early one pass asks for"""
    rng = np.random.default_rng(6310 + cs)
    hay = synth.haystack(6311, n).copy()
    plant_padding(hay, d, range(2500, 4500, 25))
    plants = [(0, NESTED[2]), (500, OUTER), (1000, HEAD + TOUCH), (1500, NESTED[2] + OUTER), (2000, NESTED[1]), (4700, HEAD + TOUCH + OUTER),
              (n - 4, TOUCH)]
    for p, k in plants:
        hay[p:p + len(k)] = utf16(k)
    if not cs:
        hay = np.where(rng.integers(0, 2, n) == 1, hay - 32, hay).astype(np.uint16)
    return hay


@functools.lru_cache(maxsize=None)
def case_long_rules(cs, with_never):
    """The sparse Longest on the planted text.  Asserted from the list and the model: the 12-unit keyword is selected at its start
    although two shorter ones there come earlier in the list, and it ends EXACTLY max_len behind the start (`e > cur_s + max_len`
    must not cut it off) -- or, with the 16-unit keyword that never occurs, four units inside that bound; INNER is in the list in
    front of OUTER and is not selected; STRADDLE is in the list in front of TOUCH with the same end, and TOUCH is selected; records
    touch end to start; one starts at unit 0 and one ends on the last unit."""
    d = long_dictionary(cs, with_never)
    c = Case("long_rules_%s%s" % ("cs" if cs else "ci", "_never" if with_never else ""), "longest", d, long_text(cs, d))
    sel, n = c.sel, c.hay.size
    assert n > SHORT_TEXT and ONE_PASS_EARLY_FROM <= sel.M <= n // 4 + 4096  # (run_longest_sparse's dense_limit: beyond it the walk)
    rows = sel.all[:, :2].tolist()
    got = c.sel.recs[:, :2].tolist()
    for s in (0, 1500):
        assert [rows.index([s, s + ln]) for ln in (4, 6, 12)] == sorted(rows.index([s, s + ln]) for ln in (4, 6, 12))
        assert [s, s + 12] in got and [s, s + 4] not in got and [s, s + 6] not in got
    assert (sel.all[:, 1] - sel.all[:, 0]).max() == 12 and d.max_len - 12 == (4 if with_never else 0)
    assert [2000, 2006] in got and [2000, 2004] not in got
    assert rows.index([502, 506]) < rows.index([500, 510]) and [500, 510] in got and [502, 506] not in got
    for s in (1000, 4700):
        assert rows.index([s + 3, s + 10]) + 1 == rows.index([s + 6, s + 10])  # same end: the longer one first
        assert [s, s + 6] in got and [s + 6, s + 10] in got and [s + 3, s + 10] not in got
    assert [4710, 4720] in got and [1512, 1522] in got  # three records touching end to start; two
    assert got[0] == [0, 12] and got[-1] == [n - 4, n] and sel.head > 0  # (the head is the THIRD record of the list)
    assert (np.asarray(got)[1:, 0] >= np.asarray(got)[:-1, 1]).all()
    return c


# ---- 4. shards: a cut on every unit ----------------------------------------------------------------------------------------------
CUT_BASE, CUT_UNITS = 2000, 40
D_CUT_SHORT = Dictionary(["abab", "ab", "ba", "bab", "b", "aabb", "bb", "bbaab", "ab"])


@functools.lru_cache(maxsize=None)
def case_cut(family, cs=True):
    """-> (dictionary, text, the cuts, the all-matches list of the whole text, the family's records).  Shortest: an a/b stretch of
    40 units with overlapping and nested occurrences in 3000 units of c with a few more occurrences on either side.  Longest:
    the planted stretches of long_text moved next to each other, cuts across all of them."""
    if family == "shortest":
        rng = np.random.default_rng(6400)
        hay = np.full(3000, C, np.uint16)
        hay[CUT_BASE:CUT_BASE + CUT_UNITS] = np.array([A, B], np.uint16)[rng.integers(0, 2, CUT_UNITS)]
        hay[CUT_BASE + 10:CUT_BASE + 19] = utf16("aabbaabab")
        for p in list(range(100, 340, 20)) + [1990, 2050] + list(range(2100, 2340, 20)) + [2990]:
            hay[p:p + 4] = utf16("abab")
        d = D_CUT_SHORT
    else:
        d = long_dictionary(cs, False)
        rng = np.random.default_rng(6410 + cs)
        hay = synth.haystack(6411, 6000).copy()
        plant_padding(hay, d, list(range(105, 1900, 25)) + list(range(2200, 4200, 25)))
        stretch = NESTED[2] + OUTER + HEAD + TOUCH + "xx" + NESTED[1]
        assert len(stretch) == CUT_UNITS
        hay[CUT_BASE:CUT_BASE + len(stretch)] = utf16(stretch)
        for p, k in ((0, NESTED[0]), (60, OUTER), (5000, HEAD), (5990, OUTER)):
            hay[p:p + len(k)] = utf16(k)
        if not cs:
            hay = np.where(rng.integers(0, 2, hay.size) == 1, hay - 32, hay).astype(np.uint16)
    full = d.all_records(hay)
    want = d.oracle(FAMILY[family]).match(hay)
    cuts = list(range(CUT_BASE - 1, CUT_BASE + CUT_UNITS + 2))
    inside = full[(full[:, 1] > CUT_BASE) & (full[:, 0] < CUT_BASE + CUT_UNITS)]
    assert len(inside) >= (30 if family == "shortest" else 9), len(inside)
    assert ((inside[:, None, 0] < inside[None, :, 0]) & (inside[None, :, 1] < inside[:, None, 1])).any()      # nested
    assert ((inside[:, None, 0] < inside[None, :, 0]) & (inside[None, :, 0] < inside[:, None, 1]) & (inside[:, None, 1] < inside[None, :, 1])).any()
    sel = want[(want[:, 1] > CUT_BASE) & (want[:, 0] < CUT_BASE + CUT_UNITS)]
    assert any(s < c < e for c in cuts for s, e in sel[:, :2].tolist()) and any(c == e for c in cuts for e in sel[:, 1].tolist())
    hay.setflags(write=False)
    return d, hay, cuts, full, want


def two_shards(d, family, hay, full, cut):
    """the model's selection of (0, cut) entered at 0 and of (cut, n) entered where the first one left"""
    left = Selection(d, family, hay, all_recs=full, own=(0, cut), entry=0)
    entry = left.exit if family == "shortest" else max(left.exit, cut)
    right = Selection(d, family, hay, all_recs=full, own=(cut, hay.size), entry=entry)
    return left, right


# ---- 5. capacity -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_capacity(family):
    """a text with a few hundred selected records among more that are not: the Shortest groups text, the Longest rules text"""
    c = case_groups(True) if family == "shortest" else case_long_rules(True, False)
    assert 20 <= len(c.want) < c.sel.M
    return c


# ---- 6. one pass, the head not at index 0 ----------------------------------------------------------------------------------------
HEAD_UNITS = 1100
HEAD_BLOCK = 12 * JUMP_BLOCK  # a 64-index block in the middle of the list
HEAD_ENTRIES = tuple(sorted({HEAD_UNITS - r for r in (1, MARK_TILE - 1, MARK_TILE, MARK_TILE + 1, 2 * MARK_TILE - 1, 2 * MARK_TILE, 2 * MARK_TILE + 1)} |
                            {HEAD_UNITS - 30, HEAD_BLOCK, HEAD_BLOCK + 5, HEAD_BLOCK + JUMP_BLOCK - 1}))


@functools.lru_cache(maxsize=None)
def case_head(entry):
    """`a` on a^1100 entered at `entry`: record k is (k, k + 1), so the head's index IS the entry and the one pass covers
    M - head indices: 1, 511 .. 513, 1023 .. 1025; a head in the list's last 64 indices; a head that is the first, a middle and
    the last index of its 64-index block (the last: the only one of that block on the chain).  And {ab, b} on b (ab)^549
    entered at the same unit: the head's index is the entry again, the jumps are 1 and 2."""
    one = Case("head_%d" % entry, "shortest", D_A, np.full(HEAD_UNITS, A), entry=entry, markers=(MARK_ONE_PASS_EARLY, MARK_DOUBLING))
    assert one.sel.M == HEAD_UNITS >= ONE_PASS_EARLY_FROM and one.sel.head == entry > 0 and len(one.sel.chain) == HEAD_UNITS - entry
    two = Case("head_alternating_%d" % entry, "shortest", D_AB_B, units("b", "ab" * (HEAD_UNITS // 2 - 1)), entry=entry,
               markers=(MARK_ONE_PASS_EARLY, MARK_DOUBLING))
    assert two.sel.M == HEAD_UNITS - 1 and two.sel.head == entry and two.sel.max_jump == 2
    return [one, two]


# ---- 7. / 8. one pass, jumps longer than a tile; both sides of 60000 --------------------------------------------------------------
JUMP_BRUTE_L = (3, 5, 8)        # short enough for the two loops
JUMP_TILE_L = (30, 100)         # jumps of some 960 and 10 200 indices: beyond one tile, beyond twenty
JUMP_LIMIT_L = (243, 244)       # the largest jumps on either side of 60000
JUMP_ENTRIES = (0, 1, 17)


def jump_text(L):
    """a^(4 L + 1) b a^(L + 3): 5 L + 5 units, a long run and one that holds ten records"""
    return units(np.full(4 * L + 1, A), "b", np.full(L + 3, A))


@functools.lru_cache(maxsize=None)
def case_jumps(L, entry=0):
    """Shortest over a^L .. a^2L on two a-runs: from the 2L-th unit of a run on L + 1 records share every end, and each of them is
    followed by the LAST record of the group L ends on -- the first record of a group jumps over L^2 + 2 L indices.  The records
    of one group land on one index, so what enters a 512-index tile are the landings of the L or so groups in front of it: more
    than k_longest_sync's 16 from L = 30 on, no synchronisation point, and one lane carries the chain over tile after tile.  The
    number of records, the largest jump and the landings per tile are the model's, not the formula's.  entry: the chain enters
    there instead of at unit 0, on another record of every group it meets."""
    d = Dictionary([np.full(k, A, np.uint16) for k in range(L, 2 * L + 1)])
    c = Case("jumps_%d_%d" % (L, entry), "shortest", d, jump_text(L), entry=entry, markers=(MARK_ONE_PASS_EARLY, MARK_DOUBLING))
    assert c.sel.group_sizes().max() == L + 1 and (c.sel.head > 0) == (entry > 0) and d.max_len == 2 * L and c.hay.size == 5 * L + 5
    assert (c.sel.all[:, 0] > 4 * L + 1).sum() == 10  # the records of the second run
    return c


CROWD = 1100  # more than two tiles of records under one jump


@functools.lru_cache(maxsize=None)
def case_far_jump_over_a_crowd():
    """a, cd, d and a^i c for i = 1 .. 1100 on a^1100 c d a^700: every a is selected, and the last one in front of the c is followed
    by cd -- 1101 indices on, over the 1100 records a^i c, which all end on the c and all land on d, ONE index behind cd and not
    on the chain.  A tile of the one pass begins among them, more than 512 indices behind the jumping a: only a look-back of the
    whole jump sees the landing on cd; a shorter one finds d alone and takes it for the synchronisation point."""
    d = Dictionary(["a", "cd", "d"] + [units(np.full(i, A), "c") for i in range(1, CROWD + 1)])
    c = Case("far_jump_over_a_crowd", "shortest", d, units(np.full(CROWD, A), "cd", np.full(700, A)),
             markers=(MARK_ONE_PASS_EARLY, MARK_DOUBLING))
    sel = c.sel
    k = int(np.argmax(sel.jumps))
    x = int(sel.nxt[k])
    on_chain = set(sel.chain.tolist())
    assert sel.head == 0 and k in on_chain and x in on_chain and x - k == CROWD + 1 == sel.max_jump
    assert (sel.nxt[k + 1:x] == x + 1).all() and x + 1 not in on_chain and sel.all[x].tolist()[:2] == [CROWD, CROWD + 2]
    assert any(k + MARK_TILE < tb <= x for tb in range(MARK_TILE, sel.M, MARK_TILE))  # (the head is index 0: tiles begin at 512 t)
    assert len(c.want) == CROWD + 1 + 700
    return c


def landings_into_tiles(sel):
    """per 512-index tile behind the head's: on how many distinct indices at or behind the tile's first the records in front of it land"""
    out = []
    for tb in range(sel.head + MARK_TILE, sel.M, MARK_TILE):
        land = sel.nxt[:tb]
        out.append(len(np.unique(land[land >= tb])))
    return out


