"""GPU tests of the piece driver (csrc/acgpu_pieces.hip: scan_next_piece) where a piece is SHORTER than a keyword: pieces of
1 .. 40 units under keywords of up to 41.  A match then spans several whole pieces, a piece holds no complete match, the left halo
is longer than the piece, a Shortest piece withholds more units than it owns (replace_limit, csrc/acgpu_replace.hip), the first-unit
families' `done` runs ahead of the next piece, and the chain passes through pieces that hold neither end of the current match.
Cursor, count, replace (host and device entry) and batch replace, every family, against ONE Oracle.match over the whole text;
that the text reaches the regime is asserted from the oracle's records alone, before any device call."""
import functools

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, utf16
from oracle.oracle import FAM_AC, FAM_LONGEST, FAM_SHORTEST, FAM_WHOLEWORD, FAM_WWLONGEST, Oracle
from tests.helpers import LOWER, WORD, splice
from tests.test_gpu_cursor import drain
from tests.test_gpu_replace import replace_device
from tests.test_gpu_replace_batch import expected as batch_expected

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20),
            ("replace_slab_units", 1 << 25)]
MODES = {N.MODE_ALL: FAM_AC, N.MODE_LONGEST: FAM_LONGEST, N.MODE_WHOLEWORD: FAM_WHOLEWORD, N.MODE_SHORTEST: FAM_SHORTEST,
         N.MODE_WWLONGEST: FAM_WWLONGEST}
REPLACING = [m for m in sorted(MODES) if m != N.MODE_ALL]  # (AhoCorasick's records overlap: cursor and count only)
WORDY = (N.MODE_WHOLEWORD, N.MODE_WWLONGEST)
PIECES = (1, 2, 3, 7, 16, 40)
LONG = (9, 23, 41)
SEEDS = {(N.MODE_WWLONGEST, True): 7100}  # (mode, case_sensitive) -> seed, where the default one does not meet the conditions of regime()


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def pieces(p):
    N.set_tunable("cursor_first_piece", p)
    N.set_tunable("cursor_max_piece", p)


def _free_of(rng, length, alpha, factors):
    """a random string of `length` units over alpha that contains none of `factors`: unit by unit, stepping back at a dead end"""
    factors = [tuple(f.tolist()) for f in factors if len(f)]
    out, tried = [], [set()]
    while len(out) < length:
        left = [c for c in alpha if c not in tried[-1]]
        if not left:
            out.pop()
            tried.pop()
            continue
        c = left[int(rng.integers(len(left)))]
        tried[-1].add(c)
        cand = tuple(out) + (c,)
        if any(cand[-len(f):] == f for f in factors if len(f) <= len(cand)):
            continue
        out.append(c)
        tried.append(set())
    return np.array(out, np.uint16)


def _flip(rng, units):
    """every letter in upper or lower case at random"""
    u = units.copy()
    up = (rng.integers(0, 2, u.size) == 1) & (u >= ord("a")) & (u <= ord("z"))
    u[up] -= 32
    return u


class Case:
    pass


@functools.lru_cache(maxsize=None)
def family_case(mode, cs):
    """Keywords, the text, its cut into 60 haystacks, the oracle's records of both and the replacement sets -- computed once per
    family and case rule, shared by every piece size and never changed."""
    c = Case()
    rng = np.random.default_rng(SEEDS.get((mode, cs), 7000 + 2 * mode + cs))
    word = mode in WORDY
    a, b, ch = ord("a"), ord("b"), ord("c")
    # about 12 short keywords of 1 .. 5 units.  Shortest: the one 1-unit keyword is "c" and the others have 3 units or more, so
    # that strings over {a, b} exist that hold none of them -- the long keywords (otherwise Shortest never reports those).
    if mode == N.MODE_SHORTEST:
        shorts = [np.array([ch], np.uint16)]
        lens = [3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5]
    else:
        shorts = [np.array([x], np.uint16) for x in ((a,) if word else (ch,))]
        lens = [2, 2, 2, 3, 3, 3, 4, 4, 5, 5, 5]
    seen = {tuple(s.tolist()) for s in shorts}
    while len(shorts) < 12:
        k = np.array([a, b, ch], np.uint16)[rng.integers(0, 3, lens[len(shorts) - 1])]
        if tuple(k.tolist()) not in seen:
            seen.add(tuple(k.tolist()))
            shorts.append(k)
    longs = []
    for ln in LONG:  # (no long keyword holds a shorter one either)
        longs.append(_free_of(rng, ln, [a, b], shorts + longs) if mode == N.MODE_SHORTEST else
                     _free_of(rng, ln, [a, b, ch], longs))
    kws = shorts + longs + [shorts[4].copy()]  # one duplicate
    if mode == N.MODE_WWLONGEST:  # two keywords with an inner space
        kws += [np.concatenate([shorts[2], [32], shorts[5]]).astype(np.uint16), np.concatenate([shorts[0], [32], longs[0]]).astype(np.uint16)]
    # the text: every long keyword 6 times, in random order, random units between them; in front of and behind a planted keyword
    # a unit that no keyword has (a match that reaches into the keyword from the left would hide it from the chain families)
    if word:  # words, 6 in 10 of them short keywords, with " ", ", ", "," or "-" (a word character: it joins two words) behind each
        fence = 32

        def filler(n_units):
            out = []
            while sum(len(x) for x in out) < n_units:
                out.append(shorts[int(rng.integers(12))] if rng.integers(10) < 6 else np.array([a, b, ch], np.uint16)[rng.integers(0, 3, int(rng.integers(1, 5)))])
                out.append(utf16((" ", " ", ", ", ",", "-")[int(rng.integers(5))]))
            return np.concatenate(out)[:n_units]
    else:  # random units, 7 in 100 of them none that a keyword has
        fence = ord("d")

        def filler(n_units):
            return np.array([a, b, ch, fence, 0x2603], np.uint16)[rng.choice(5, n_units, p=[0.31, 0.31, 0.31, 0.05, 0.02])]
    plants = [i % 3 for i in range(18)]
    rng.shuffle(plants)
    parts = []
    for i in plants:
        parts += [filler(int(rng.integers(8, 28))), [fence], longs[i], [fence]]
    if mode == N.MODE_WWLONGEST:
        parts += [kws[-1], [fence], kws[-2], [ord(",")]]
    parts.append(filler(12))
    hay = np.concatenate(parts).astype(np.uint16)
    if not cs:
        hay = _flip(rng, hay)
        kws = [_flip(rng, k) for k in kws]
    assert 700 <= hay.size <= 900, hay.size
    c.kws, c.hay, c.wc = kws, hay, (WORD if word else None)
    c.oracle = Oracle(MODES[mode], kws, case_sensitive=cs, lower=None if cs else LOWER, word_chars=c.wc)
    c.recs = c.oracle.match(hay, cap=hay.size * 8)
    # 60 haystacks of 0 .. 40 units that are the text cut at 59 places: with pieces of 1 .. 40 units of the concatenation the
    # separators land inside pieces, at their ends and next to them
    lens = rng.integers(0, 41, 60)
    lens[[3, 4, 30, 59]] = 0
    while lens.sum() != hay.size:
        i = int(rng.integers(60))
        if i not in (3, 4, 30, 59):
            lens[i] = min(40, max(0, lens[i] + int(np.sign(hay.size - lens.sum()))))
    cuts = np.concatenate([[0], np.cumsum(lens)])
    c.hays = [hay[cuts[i]:cuts[i + 1]] for i in range(60)]
    c.hay_recs = [c.oracle.match(h, cap=64 + 8 * len(h)) for h in c.hays] if mode != N.MODE_ALL else None
    i_long = 12 + 2  # the keyword of 41 units
    c.repls = {"empty": ["" for _ in kws],
               "cycle": [("0123456789ABCDEFG" * 2)[i % 17:i % 17 + i % 18] for i in range(len(kws))],
               "one of 300": [("{" + "=" * 298 + "}") if i == i_long else "<%d>" % i for i in range(len(kws))]}
    assert [len(r) for r in c.repls["cycle"]] == [i % 18 for i in range(len(kws))] and len(c.repls["one of 300"][i_long]) == 300
    assert len(kws[i_long]) == 41
    return c


def regime(mode, c):
    """What the oracle's records alone say about the text: it reaches the regime these tests are about, whatever the device
    answers.  -> {piece size: records that span a piece seam}"""
    recs, n = c.recs.astype(np.int64), c.hay.size
    s, e = recs[:, 0], recs[:, 1]
    ln = e - s
    for want in LONG:
        assert (ln == want).sum() >= 6, (want, int((ln == want).sum()))  # every planted long keyword is reported where it stands
    spanning = {}
    for p in PIECES:
        spanning[p] = int((s // p != (e - 1) // p).sum())
        if p <= 16:
            assert spanning[p] >= 5, (p, spanning[p])
        if p <= 7:  # the whole pieces inside [s, e): from the first piece start at or behind s
            assert (e // p - (s + p - 1) // p).max() >= 3, p
        if mode == N.MODE_SHORTEST:
            # a record that ends in the max_len - 1 units a piece withholds in front of its end q < n (its end, not q - (max_len -
            # 1), is then the limit); the records that START there and end behind q are the seam-spanning ones above
            q = (e + p - 1) // p * p
            assert ((q - e < max(LONG) - 1) & (q < n)).any() and spanning[p] >= 1, p
    covered = np.zeros(n, bool)
    for x, y in zip(s.tolist(), e.tolist()):
        covered[x:y] = True
    assert covered.sum() >= 0.1 * n, covered.sum()
    return spanning


def automaton(mode, cs, c):
    return Automaton(mode, c.kws, cs, word_chars=c.wc)


def page_cap(n_recs):
    cap = next(k for k in (7, 11, 13) if n_recs % k)
    assert n_recs > cap and n_recs % cap
    return cap


# ---- the CPU side of every case: collected with the GPU tests, and what chooses the seeds -----------------------------------------
def seam_counts():
    """{(mode, cs): {piece size: seam-spanning records}} of every case (python -c 'import tests.test_gpu_tiny_pieces as t;
    print(t.seam_counts())' on a machine without a device)"""
    return {(m, cs): regime(m, family_case(m, cs)) for m in sorted(MODES) for cs in (True, False)}


# ---- 1. cursor and count --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PIECES)
@pytest.mark.parametrize("cs", [True, False])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_cursor_and_count(mode, cs, p):
    c = family_case(mode, cs)
    regime(mode, c)
    n, want = c.hay.size, c.recs
    auto = automaton(mode, cs, c)
    pieces(p)
    for ids in (True, False):
        got, st = drain(auto, c.hay, ids, page_cap(len(want)))
        ref = want if ids else want[:, :2]
        assert got.shape == ref.shape and (got == ref).all(), ids
        assert st["pieces"] >= n // p and st["records_delivered"] == len(want), st
    counts, st = auto.count_host(c.hay)
    assert (counts == np.bincount(want[:, 2], minlength=len(c.kws)).astype(np.uint64)).all()
    assert st["pieces"] >= n // p and st["n_records"] == len(want), st


# ---- 2. replace -----------------------------------------------------------------------------------------------------------------
def check_replace(auto, c, repls, want, n_pieces):
    got, st = auto.replace_host(c.hay, repls)
    assert got.shape == want.shape and (got == want).all(), "host"
    assert st["n_records"] == len(c.recs) and st["units_out"] == want.size and st["pieces"] >= n_pieces, st
    got, rc, n_out, st = replace_device(auto, c.hay, repls, need=int(want.size))  # (asserts its canary behind cap)
    assert rc == N.OK and n_out == want.size and (got == want).all(), "device"
    assert st["n_records"] == len(c.recs) and st["units_out"] == want.size and st["pieces"] >= n_pieces, st


@pytest.mark.parametrize("p", PIECES)
@pytest.mark.parametrize("cs", [True, False])
@pytest.mark.parametrize("mode", REPLACING)
def test_replace(mode, cs, p):
    c = family_case(mode, cs)
    regime(mode, c)
    auto = automaton(mode, cs, c)
    pieces(p)
    for label, repls in c.repls.items():
        check_replace(auto, c, repls, splice(c.hay, c.recs, repls), c.hay.size // p)
    N.set_tunable("replace_slab_units", 8)
    check_replace(auto, c, c.repls["one of 300"], splice(c.hay, c.recs, c.repls["one of 300"]), c.hay.size // p)


# ---- 3. batch replace -----------------------------------------------------------------------------------------------------------
def check_batch(auto, c, repls, n_pieces):
    want, off, n_rec = batch_expected(c.hays, c.hay_recs, repls)
    got, got_off, st = auto.replace_batch(c.hays, repls)
    assert got_off.tolist() == off.tolist()
    assert got.shape == want.shape and (got == want).all()
    assert st["n_records"] == n_rec and st["units_out"] == want.size and st["pieces"] >= n_pieces, st


@pytest.mark.parametrize("p", PIECES)
@pytest.mark.parametrize("cs", [True, False])
@pytest.mark.parametrize("mode", REPLACING)
def test_batch_replace(mode, cs, p):
    c = family_case(mode, cs)
    regime(mode, c)
    assert sum(len(r) for r in c.hay_recs) >= 20 and sum(len(h) for h in c.hays) == c.hay.size
    auto = automaton(mode, cs, c)
    pieces(p)
    for label, repls in c.repls.items():
        check_batch(auto, c, repls, (c.hay.size + len(c.hays)) // p)


# ---- 4. pieces that the reservoir shrinks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_pieces_shrunk_by_a_reservoir_of_16_records(mode):
    """default piece sizes, a reservoir budget of 16 Map records, a pool made after that: the text does not fit as one piece and
    on_overflow cuts it by its density -- how a dense text in a small reservoir comes to pieces of a few units"""
    c = family_case(mode, True)
    regime(mode, c)
    assert len(c.recs) > 3 * 16
    want = c.recs
    N.set_tunable("cursor_reservoir_bytes", 16 * N.REC_MAP)
    auto = automaton(mode, True, c)
    got, st = drain(auto, c.hay, True, page_cap(len(want)))
    assert got.shape == want.shape and (got == want).all()
    assert st["rescans"] > 0, st
    counts, st = automaton(mode, True, c).count_host(c.hay)
    assert (counts == np.bincount(want[:, 2], minlength=len(c.kws)).astype(np.uint64)).all() and st["rescans"] > 0, st
    if mode == N.MODE_ALL:
        return
    repls = c.repls["cycle"]
    spliced = splice(c.hay, want, repls)
    auto = automaton(mode, True, c)
    got, st = auto.replace_host(c.hay, repls)
    assert got.shape == spliced.shape and (got == spliced).all() and st["rescans"] > 0 and st["n_records"] == len(want), st
    auto = automaton(mode, True, c)
    got, rc, n_out, st = replace_device(auto, c.hay, repls, need=int(spliced.size))
    assert rc == N.OK and n_out == spliced.size and (got == spliced).all() and st["rescans"] > 0, st
    auto = automaton(mode, True, c)
    b_want, b_off, n_rec = batch_expected(c.hays, c.hay_recs, repls)
    got, got_off, st = auto.replace_batch(c.hays, repls)
    assert got_off.tolist() == b_off.tolist() and got.shape == b_want.shape and (got == b_want).all()
    assert st["n_records"] == n_rec and st["rescans"] > 0, st
