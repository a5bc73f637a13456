"""GPU tests of WholeWordLongestMatchSet/Map at the edges of its own kernels (csrc/acgpu_wwlongest.hip, driven by run_wwlongest in
csrc/acgpu_hostrun.hip), every record against the CPU oracle, bit for bit:

  1. k_wwl_walk's first-word table (`T.ww_fat && ws + 16 <= n`, `r >= 1 && r <= kWwInlineUnits`) on both sides of 12 units;
  2. k_wwl_walk's last 15 units of the buffer (`have < 8`, `at_end`), a text cut at every distance from its last walk start;
  3. k_wwl_starts' seams: 8 units per lane, 2048 per workgroup step, the left neighbour `pu`, the scalar tail `v + 8 > n`;
  4. k_wwl_emit's tile of 2048 walk starts in 8 passes of 256, and its capacity check `dst < cap`;
  5. mark_chain's jump bound (`t.max_len / 2 + 2` in run_wwlongest, trusted as Cn.max_len by the one-pass marking);
  6. k_wwl_select's ownership and chain exit with a shard cut on every unit across a phrase.

That each text reaches what its test is about is asserted from the text, the dictionary and the oracle's records alone (tests/wwl_edges.py)."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, utf16
from tests import wwl_edges as E
from tests.helpers import LOWER, WORD

pytestmark = pytest.mark.gpu

MARK_DOUBLING, MARK_ONE_PASS_EARLY = 2097152, 4194304  # tile_debug: always pointer doubling / the one pass from 64 walk starts on


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k in ("tile_debug", "ww_first_seed", "ww_no_bloom", "region_units", "force_kernel"):
        N.set_tunable(k, 0)


def automaton(kws, cs, **tunables):
    """the automaton, built under `tunables` (set around the constructor only)"""
    for k, v in tunables.items():
        N.set_tunable(k, v)
    try:
        return Automaton(N.MODE_WWLONGEST, kws, cs, word_chars=WORD)
    finally:
        for k in tunables:
            N.set_tunable(k, 0)


def upload(hay):
    import torch
    return torch.from_numpy(np.array(hay, dtype=np.uint16).view(np.int16)).cuda()  # (a copy: the shared texts are read-only)


def device_call(a, d_hay, n, ids, cap, **kw):
    """acgpu_match_device -> (the records written, n_out, rc, profile, chain_exit); a canary row behind `cap` must survive"""
    import torch
    cols = 3 if ids else 2
    d_out = torch.full((cap + 1, cols), -7, dtype=torch.int32, device="cuda")
    n_out, rc, prof, ex = a.match_device(d_hay.data_ptr(), n, ids, d_out.data_ptr(), cap, **kw)
    out = d_out.cpu().numpy()
    assert (out[cap] == -7).all(), "a record was written behind the capacity"
    return out[:min(n_out, cap)], n_out, rc, prof, ex


def check_all_entries(a, hay, want, where, d_hay=None, n=None):
    """Set and Map records of the host entry, Map records of the device entry (which names its scan kernel): all the oracle's"""
    n = len(hay) if n is None else n
    for ids in (True, False):
        ref = want if ids else want[:, :2]
        got = a.match_host(hay[:n], ids, cap=16)  # (a capacity that overflows once: the call is made twice)
        assert got.shape == ref.shape and (got == ref).all(), (where, "host", ids)
    got, n_out, rc, prof, _ = device_call(a, upload(hay) if d_hay is None else d_hay, n, True, len(want) + 4, profile=True)
    assert rc == N.OK and n_out == len(want) and (got == want).all(), (where, "device")
    assert prof["scan_kernel"] == "k_wwl_walk", prof


def same(got, want):
    return got.shape == want.shape and bool((got == want).all())


# ---- 1. the first-word table on both sides of 12 units ---------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [True, False])
def test_first_word_table_on_both_sides_of_12_units(cs):
    """k_wwl_walk: a first word of 1 .. 12 units is settled by ONE probe of the two-choice table behind the Bloom filter (payload:
    a keyword id, or bit 31 and the node the walk goes on from), 13 units and more walk unit by unit.  First words of 11, 12, 13
    and 14 units that share all but their last unit, prefixes of each other, near misses at units 12 to 14, first words that are
    keywords only inside phrases, duplicates.  Built with the default hash seed, from seeds 3 and 7, and with the smallest Bloom
    filter (ww_no_bloom: 1 Kbit, nearly every probe goes to memory).  WholeWordLongest has one pipeline and reads no
    force_kernel (run_wwlongest never looks at it, and the family has no one-launch form), so there is no such run."""
    c = E.edge_case(cs)
    E.regime(c)
    d_hay = upload(c.hay)
    seeds = set()
    for tun in ({}, {"ww_first_seed": 3}, {"ww_first_seed": 7}, {"ww_no_bloom": 1}):
        a = automaton(c.kws, cs, **tun)
        seed = ctypes.c_uint32(0)
        N.check(N.lib().acgpu_debug_wordhash(a.handle, None, None, None, None, None, None, None, ctypes.byref(seed)), "seed")
        seeds.add(seed.value)
        check_all_entries(a, c.hay, c.recs, tun, d_hay=d_hay)
    assert len(seeds) == 3


# ---- 2. every distance from the end of the buffer --------------------------------------------------------------------------------
def end_case(c):
    """A prefix of the edge text of 4100 to 5000 units that ends one unit behind a phrase record whose first word has 16, 17 or 24
    units and is a keyword of its own, and whose second word has 2 .. 10: the 40 lengths up to there cut the text inside that
    first word, right behind it, on the inner space and inside the second word, and leave its start -- the last walk start -- at
    every distance from 1 to 17 from the end.
    -> (prefix length, the lengths to test, that record)"""
    w = WORD[c.hay].astype(bool)
    paths = c.trie.word_paths()
    for s, e, _ in c.recs.tolist():
        inner = np.flatnonzero(~w[s:e])
        if e < 4140 or e + 1 > c.hay.size or len(inner) != 1 or int(inner[0]) not in (16, 17, 24) or not 2 <= e - s - int(inner[0]) - 1 <= 10:
            continue
        if not paths[tuple(E.fold_units(c.hay[s:s + int(inner[0])], c.cs).tolist())][1]:  # (the first word alone is no keyword)
            continue
        end = e + 1
        assert end - 40 <= s and end <= 5000, (s, e)
        lengths = sorted(set(range(end - 39, end + 1)) | {2047, 2048, 2049, 4095, 4096, 4097})
        return end, lengths, (s, e, int(inner[0]))
    raise AssertionError("no such record")


@pytest.mark.parametrize("cs", [True, False])
def test_text_cut_at_every_distance_from_its_last_walk_start(cs):
    """k_wwl_walk near the end of the buffer: `ws + 16 <= n` fails, the walk goes unit by unit, its last load is the `have < 8` tail,
    and a walk that reaches the end reports through `at_end` -- the whole path if it is a keyword, else the carried fail match.
    The device call is given the whole prefix and n units of it: nothing behind n may be looked at."""
    c = E.edge_case(cs)
    end, lengths, (s, e, r) = end_case(c)
    starts = E.walk_starts(c.hay[:end])
    tail = [n for n in lengths if n > end - 40]
    assert {n % 8 for n in tail} == set(range(8))
    assert {n - int(starts[starts < n][-1]) for n in tail} >= set(range(1, 18))  # the last walk start: 1 .. 17 units from the end
    assert any(s < n < s + r for n in tail) and s + r in tail and s + r + 1 in tail and any(s + r + 1 < n < e for n in tail)
    a = automaton(c.kws, cs)
    d_hay = upload(c.hay[:end])
    at_end = carried_at_end = 0
    for n in lengths:
        want = c.oracle.match(c.hay[:n], cap=n)
        check_all_entries(a, c.hay, want, n, d_hay=d_hay, n=n)
        if len(want) and want[-1, 1] == n:
            at_end += 1
        if len(want) and want[-1, 1] < n and c.trie.walk_stop(E.fold_units(c.hay[:n], cs).tolist(), int(want[-1, 0])) == n:
            carried_at_end += 1
    assert at_end >= 2 and carried_at_end >= 2, (at_end, carried_at_end)  # a whole path and a carried fail match reported at the end


# ---- 3. walk starts on the seams of k_wwl_starts ---------------------------------------------------------------------------------
SEAM_UNITS = 3 * 2048 + 5
SEAM_KS = (1, 2, 37, 255, 256, 257, 511, 512, 513, 767, 768)


def seam_case(cs, shift, word_neighbour):
    """A text of 3 * 2048 + 5 units of short words with the word "a" at every 8 k + shift (k in SEAM_KS: 2048 + shift, 4096 + shift
    and the scalar tail among them) behind a space -- a walk start -- or behind "b": then it is none, and 8 k + shift - 1 is.  One
    aligned vector of the text is all word characters, one all spaces."""
    rng = np.random.default_rng(4300 + 8 * shift + word_neighbour)
    letters = utf16("abx" if cs else "abxAB")
    parts = []
    while sum(len(p) for p in parts) < SEAM_UNITS:
        parts += [letters[rng.integers(0, len(letters), int(rng.integers(1, 4)))], E.SP if rng.integers(2) else E.cat(E.SP, E.SP)]
    hay = E.cat(*parts)[:SEAM_UNITS].copy()
    long_word = E.ALPHA[rng.integers(0, len(E.ALPHA), 24)]
    hay[998:1025] = E.cat(E.SP, E.SP, long_word, E.SP)  # (two spaces: no walk reaches it from the left)
    hay[1199:1217] = 32
    targets = [8 * k + shift for k in SEAM_KS]
    for p in targets:
        hay[p - 2:p + 2] = [32, ord("b") if word_neighbour else 32, ord("a"), 32][:len(hay[p - 2:p + 2])]
    kws = [utf16(k) for k in ("a", "b", "ab", "ba", "a a", "a b", "x a", "ba x")] + [long_word, E.cat(long_word, E.SP, utf16("a"))]
    return hay, kws, targets


@pytest.mark.parametrize("cs", [True, False])
def test_walk_starts_on_the_seams_of_the_start_scan(cs):
    """k_wwl_starts: a walk start is a word character whose left neighbour is none; a lane has 8 units and takes the left neighbour
    of unit 0 from memory (`pu`), a workgroup step has 2048, the last lanes take the scalar tail (`v + 8 > n`).  Word starts at
    8 k - 1, 8 k and 8 k + 1 -- 2047 .. 2049 and 4095 .. 4097 among them -- with a space and with a word character in front."""
    from oracle.oracle import FAM_WWLONGEST, Oracle
    for shift in (-1, 0, 1):
        for word_neighbour in (0, 1):
            hay, kws, targets = seam_case(cs, shift, word_neighbour)
            starts = set(E.walk_starts(hay).tolist())
            assert hay.size == SEAM_UNITS and {2048 + shift, 4096 + shift, 6144 + shift} <= set(targets)
            for p in targets:
                assert (p in starts) != bool(word_neighbour) and (p - 1 in starts) == bool(word_neighbour), p
            w = WORD[hay].astype(bool)
            assert w[1008:1016].all() and not w[1208:1216].any()  # a lane's vector of word characters only, one of none
            want = E.oracle_for(kws, cs).match(hay, cap=hay.size)
            at = set(want[:, 0].tolist())
            # (a target is no record start where the walk of the word in front of it runs into it)
            assert len(want) > 300 and sum((p - word_neighbour) in at for p in targets) >= len(targets) // 2 and 1000 in at
            check_all_entries(automaton(kws, cs), hay, want, (shift, word_neighbour))
    if cs:
        return
    # position 0 of the TEXT is a walk start whatever stands there: the root has a transition on the space, and in " éa, b" the
    # walk that begins on it swallows the space and the word behind it is skipped -- "éa" is not reported; in ".éa, b" it is
    kws = [utf16(k) for k in (" ", "Éa", "b", ", ", "b a")]
    a = automaton(kws, False)
    for text, reported in ((" éa, b", False), (".éa, b", True)):
        hay = utf16(text)
        want = Oracle(FAM_WWLONGEST, kws, case_sensitive=False, lower=LOWER, word_chars=WORD).match(hay)
        assert ([1, 3, 1] in want.tolist()) == reported
        check_all_entries(a, hay, want, text)


# ---- 4. M at the edges of k_wwl_emit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097])
def test_number_of_walk_starts_at_the_edges_of_the_emit_tile(M):
    """k_wwl_emit ranks one tile of 2048 walk starts per workgroup in 8 passes of 256 (k = base + j * 256 + thread, `k < M`): texts
    of exactly M one-letter words.  "a b" jumps over the start of its "b", "c" reports nothing: the selected starts are a strict
    subset.  With half the capacity the call overflows with the exact count and the records that fit are the first ones."""
    for cs in (True, False):
        rng = np.random.default_rng(4400 + M)
        words = utf16("abcA")[rng.integers(0, 4, M)]
        words[:2] = utf16("ab")[:M]
        hay = np.full(2 * M - 1, 32, np.uint16)
        hay[0::2] = words
        kws = [utf16(k) for k in ("a", "b", "a b")]
        assert len(E.walk_starts(hay)) == M
        want = E.oracle_for(kws, cs).match(hay, cap=hay.size)
        assert 1 <= len(want) and (len(want) < M or M == 1) and (M == 1 or (want[:, 1] - want[:, 0] == 3).any())
        a = automaton(kws, cs)
        check_all_entries(a, hay, want, (M, cs))
        cap = len(want) // 2
        d_hay = upload(hay)
        for ids in (True, False):
            got, n_out, rc, _, _ = device_call(a, d_hay, hay.size, ids, cap)
            assert rc == N.E_OVERFLOW and n_out == len(want), (M, cs, ids, rc, n_out)
            assert (got == (want if ids else want[:, :2])[:cap]).all(), (M, cs, ids)


# ---- 5. jumps at the bound -------------------------------------------------------------------------------------------------------
PHRASE_WORDS = 300
PREFIX_WORDS = (2, 4, 37, 150)
BREAKS = (3, 38, 151, 299, 149)  # the word that differs -> the longest prefix keyword in front of it is the carried fail match


def other_folded(rng, u):
    """a unit of the alphabet that differs from u under either case rule"""
    while True:
        c = E.other_unit(rng, u)
        if LOWER[c] != LOWER[int(u)]:
            return c


def jump_case(cs, offset):
    """-> (keywords, text, [(word index of a plant, words of the record expected there)]): a stream of one-letter words with the
    phrase of 300 one-letter words planted whole at word `offset` and once more later, and broken at each word of BREAKS."""
    rng = np.random.default_rng(4500 + cs)  # (one phrase per case rule; the stream differs with the offset)
    phrase = E.ALPHA[rng.integers(0, len(E.ALPHA), PHRASE_WORDS)]

    def spaced(words):
        out = np.full(2 * len(words) - 1, 32, np.uint16)
        out[0::2] = words
        return out

    kws = [spaced(phrase)] + [spaced(phrase[:k]) for k in PREFIX_WORDS] + [np.array([u], np.uint16) for u in E.ALPHA]
    rng = np.random.default_rng(4600 + 2 * offset + cs)

    def filler(k):  # (ends on a word that does not begin the phrase)
        f = E.ALPHA[rng.integers(0, len(E.ALPHA), k)]
        f[-1] = other_folded(rng, phrase[0])
        return f

    words, plants = [filler(offset)], [(offset, PHRASE_WORDS)]
    words.append(phrase)
    for b in BREAKS + (PHRASE_WORDS + 1,):
        words.append(filler(int(rng.integers(5, 40))))
        broken = phrase.copy()
        if b <= PHRASE_WORDS:
            broken[b - 1] = other_folded(rng, phrase[b - 1])
        plants.append((sum(len(x) for x in words), max([k for k in PREFIX_WORDS + (1, PHRASE_WORDS) if k < b])))
        words.append(broken)
    words.append(filler(30))
    return kws, spaced(np.concatenate(words)), plants


@pytest.mark.parametrize("offset", [1, 63, 64, 511, 512])
def test_jumps_at_the_bound_of_the_one_pass_marking(offset):
    """run_wwlongest tells mark_chain that no walk jumps over more than max_len / 2 + 2 walk starts, and the one-pass marking
    (64-index groups, 512-index tiles) looks back no further: a phrase of 300 one-letter words, max_len 599, jumps over 300 --
    the bound is 301.  Planted `offset` walk starts behind the text's first, once more later, and broken at words 3, 38, 149,
    151 and 299, where the carried fail match (2, 37, 37, 150, 150 words) ends up to 149 words in front of the stop.  Pointer
    doubling, the one pass from 64 walk starts on and the default choice all give the oracle's records."""
    for cs in (True, False):
        kws, hay, plants = jump_case(cs, offset)
        want = E.oracle_for(kws, cs).match(hay, cap=hay.size)
        starts = E.walk_starts(hay)
        assert (starts == np.arange(0, hay.size, 2)).all() and len(starts) >= 64
        covered = np.searchsorted(starts, want[:, 1]) - np.searchsorted(starts, want[:, 0])
        assert covered.max() == PHRASE_WORDS and len(kws[0]) == 2 * PHRASE_WORDS - 1
        rows = {(s, e) for s, e, _ in want.tolist()}
        for at, n_words in plants:
            assert (2 * at, 2 * at + 2 * n_words - 1) in rows, (cs, at, n_words)
        a = automaton(kws, cs)
        assert a.info()["max_keyword_len"] == 2 * PHRASE_WORDS - 1
        for bits in (0, MARK_DOUBLING, MARK_ONE_PASS_EARLY):
            N.set_tunable("tile_debug", bits)
            check_all_entries(a, hay, want, (cs, bits))
        N.set_tunable("tile_debug", 0)


# ---- 6. a shard cut at every unit across a phrase --------------------------------------------------------------------------------
def cut_case(c):
    """the first 3000 units of the edge text with one three-word phrase of the dictionary planted between two of its tokens
    -> (text, the phrase's first unit, its stop unit)"""
    w = WORD[c.hay].astype(bool)
    phrase = next(k for k in c.kws if (k == 44).any() and int(np.flatnonzero(~WORD[k].astype(bool))[0]) == 13)
    at = next(p for p in range(1500, 3000) if not w[p] and w[p + 1])  # the space in front of a token
    hay = E.cat(c.hay[:at + 1], phrase, c.hay[at:3000 - len(phrase) - 1])
    assert hay.size == 3000 and hay[at] == 32 and hay[at + 1 + len(phrase)] == 32
    return hay, at + 1, at + 1 + len(phrase)


@pytest.mark.parametrize("cs", [True, False])
def test_shard_cut_at_every_unit_across_a_phrase(cs):
    """k_wwl_walk's `mark` of the first walk start at or after the entry, k_wwl_select's `mine` and chain exit (`stop[k] + 1`): two
    shards of one buffer cut at every unit from two in front of a three-word phrase (first word: 13 units) to two behind its stop
    unit -- inside the first word, on the inner space, inside the second word, on the comma, on the stop unit -- chained through
    chain_exit and chain_entry.  Every fourth cut once more as a rank sees its share: a buffer that begins at most 8 units in
    front of it and ends EXACTLY max_keyword_len + 1 units behind own_end."""
    c = E.edge_case(cs)
    hay, first, stop = cut_case(c)
    n = hay.size
    want = c.oracle.match(hay, cap=n)
    assert [first, stop] in want[:, :2].tolist()  # the planted phrase is reported whole
    inner = first + 13
    assert not WORD[hay[inner]] and hay[stop - 1] != 32
    a = automaton(c.kws, cs)
    ml = a.info()["max_keyword_len"]
    own_end = 2600
    assert stop + 2 < own_end and own_end + ml + 1 < n
    d_hay = upload(hay)
    cap = len(want) + 4
    cuts = list(range(first - 2, stop + 3))
    assert {first + 5, inner, inner + 2, stop - 1, stop, stop + 1} <= set(cuts)
    for i, cut in enumerate(cuts):
        left, n_left, rc, prof, ex = device_call(a, d_hay, n, True, cap, own=(0, cut), chain_entry=0, profile=True)
        assert rc == N.OK and prof["scan_kernel"] == "k_wwl_walk" and ex >= 0
        right, n_right, rc, _, ex2 = device_call(a, d_hay, n, True, cap, own=(cut, n), chain_entry=ex)
        assert rc == N.OK and ex2 >= ex
        assert same(np.concatenate([left, right]), want), cut
        assert (left[:, 0] < cut).all() and (right[:, 0] >= cut).all()
        if cut <= stop and cut > first:  # the phrase's walk belongs to the left shard and ends behind the cut
            assert ex == stop + 1, (cut, ex)
        if i % 4:
            continue
        base = (cut - 1) // 8 * 8
        sub = d_hay[base:own_end + ml + 1].clone()
        got, n_out, rc, _, _ = device_call(a, sub, sub.numel(), True, cap, own=(cut - base, own_end - base), text_begin=False,
                                           text_end=False, chain_entry=ex - base)
        assert rc == N.OK, (cut, rc)
        got[:, :2] += base
        assert same(got, want[(want[:, 0] >= cut) & (want[:, 0] < own_end)]), cut
        # one unit less of right halo is refused
        assert a.match_device(sub.data_ptr(), sub.numel() - 1, True, 0, 0, own=(cut - base, own_end - base), text_begin=False,
                              text_end=False, chain_entry=ex - base)[1] == N.E_INVALID
