"""The inputs of tests/test_gpu_selection_edges.py, checked without a device.  For every case of tests/selection_edges.py: the model's
chain over Oracle(FAM_AC)'s list IS the selection -- it equals Oracle(FAM_SHORTEST) / Oracle(FAM_LONGEST) record for record -- and
the input has the property its GPU test names: the number of records M, the chain's length, the head's index, the largest jump
on the stated side of 512 and of 60000, the records per end (the builders assert the rest as they run).  The numpy model itself is
pinned to its two-loop twin on every list short enough.  An edit of an input that takes it off its edge fails here."""
import numpy as np
import pytest

from tests import selection_edges as E


def is_the_selection(c):
    """the model's chain equals the oracle's records of the family"""
    assert c.sel.recs.shape == c.want.shape and (c.sel.recs == c.want).all(), c
    if c.family == "shortest":  # matching restarts at the end of the last reported match
        assert c.sel.exit == (int(c.want[-1, 1]) if len(c.want) else c.entry)


def same_as_the_loops(sel, family, limit=None):
    plain = E.shortest_next_plain(sel.all) if family == "shortest" else E.longest_next_plain(sel.all, limit)
    assert (plain == sel.nxt).all()


def test_the_model_equals_its_two_loop_twin_on_random_lists():
    """records drawn at random (end ascending, longest first): ties in start and in end, records without a successor, every limit"""
    rng = np.random.default_rng(6100)
    for it in range(60):
        n = int(rng.integers(1, 40))
        rows = sorted({(int(s), int(s + ln)) for s, ln in zip(rng.integers(0, 30, n), rng.integers(1, 9, n))}, key=lambda r: (r[1], r[0]))
        recs = np.array([(s, e, 0) for s, e in rows], dtype=np.int32)
        assert (E.shortest_next(recs) == E.shortest_next_plain(recs)).all(), it
        for limit in (0, 7, 15, 40):
            assert (E.longest_next(recs, limit) == E.longest_next_plain(recs, limit)).all(), (it, limit)
            for entry in (0, 5, 29, 38):
                want = [k for k, (s, e) in enumerate(rows) if entry <= s < limit]
                want = min(want, key=lambda k: (rows[k][0], -rows[k][1])) if want else len(rows)
                assert E.longest_head(recs, entry, limit) == want
        for entry in (0, 5, 29, 38):
            assert E.shortest_head(recs, entry) == next((k for k, (s, e) in enumerate(rows) if s >= entry), len(rows))


@pytest.mark.parametrize("M", E.SEAM_M)
def test_seam_cases_have_exactly_m_records(M):
    """case 1: M on both sides of 8^t (the doubling's launches), of 256 (the grids of M + 1 threads), of 512 and 2048"""
    for c in E.case_seams(M):
        assert c.sel.M == M
        is_the_selection(c)
        if M <= 513:
            same_as_the_loops(c.sel, "shortest")
    launches = lambda m: len([r for r in (8 ** t for t in range(8)) if r <= m])  # `for (reach = 1; reach <= M; reach <<= 3)`
    assert [launches(m) for m in (7, 8, 9, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 32767, 32768, 32769)] == [1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5, 6, 6]
    assert E.MARKS_PER_LAUNCH == 8 and {E.BLOCK - 1, E.BLOCK, E.BLOCK + 1, E.SCAN_TILE - 1, E.SCAN_TILE, E.SCAN_TILE + 1} <= set(E.SEAM_M)


@pytest.mark.parametrize("cs", [True, False])
def test_group_search_case(cs):
    """case 2 (its reach assertions run in the builder): first, middle and last of an end group, several groups on, no successor"""
    c = E.case_groups(cs)
    is_the_selection(c)
    assert c.sel.M >= 50000 and len(c.want) >= 500


@pytest.mark.parametrize("with_never", [False, True])
@pytest.mark.parametrize("cs", [True, False])
def test_long_rules_case(cs, with_never):
    """case 3: the leftmost-longest successor on the planted text, the two-loop twin on the whole list, and the dictionary's
    suffix filter is selective (the one statement here that asks the library: it decides who answers the call)"""
    from ahocorasick_amd import _native as N
    from ahocorasick_amd.strings import Automaton
    c = E.case_long_rules(cs, with_never)
    is_the_selection(c)
    same_as_the_loops(c.sel, "longest", c.hay.size)
    info = Automaton(N.MODE_LONGEST, c.d.kws, cs).info()
    assert info["tile_kernel"] == 1 and info["max_keyword_len"] == c.d.max_len
    # an entry behind every record's start, in front of the text's end
    entry = int(c.sel.all[:, 0].max()) + 1
    assert entry < c.hay.size and E.longest_head(c.sel.all, entry, c.hay.size) == c.sel.M


@pytest.mark.parametrize("family,cs", [("shortest", True), ("longest", True), ("longest", False)])
def test_cut_cases_chain_to_the_whole_text(family, cs):
    """case 4: for every cut the model's two shards, chained through exit and entry, are the oracle's records of the whole text;
    both lists have the 64 records the early one pass asks for; cuts fall inside selected records and on their ends"""
    d, hay, cuts, full, want = E.case_cut(family, cs)
    assert len(cuts) >= E.CUT_UNITS
    exits = set()
    for cut in cuts:
        left, right = E.two_shards(d, family, hay, full, cut)
        got = np.concatenate([left.recs, right.recs])
        assert got.shape == want.shape and (got == want).all(), cut
        assert left.M >= E.ONE_PASS_EARLY_FROM and right.M >= E.ONE_PASS_EARLY_FROM, (cut, left.M, right.M)
        assert (left.exit >= cut) if family == "longest" else (left.exit == left.recs[-1, 1] <= cut)
        exits.add(left.exit - cut)
        if cut == cuts[0]:
            for s in (left, right):
                same_as_the_loops(s, family, s.own[1])
    if family == "longest":
        assert 0 in exits and max(exits) >= 8  # the chain leaves a shard on the cut, and up to a keyword behind it
        assert len(full) >= 150
    else:
        assert 0 in exits and min(exits) <= -2  # the restart position lies on the cut, and in front of it
    # an entry behind every record
    entry = int(full[:, 0].max()) + 1
    empty = E.Selection(d, family, hay, all_recs=full, entry=entry)
    assert empty.M >= E.ONE_PASS_EARLY_FROM and empty.head == empty.M and len(empty.recs) == 0 and entry < hay.size


@pytest.mark.parametrize("family", ["shortest", "longest"])
def test_capacity_cases(family):
    c = E.case_capacity(family)
    is_the_selection(c)


@pytest.mark.parametrize("entry", E.HEAD_ENTRIES)
def test_head_cases(entry):
    """case 6: the head's index is the entry"""
    for c in E.case_head(entry):
        is_the_selection(c)
        assert c.sel.head == entry
    covered = {E.HEAD_UNITS - e for e in E.HEAD_ENTRIES}
    assert {1, 511, 512, 513, 1023, 1024, 1025} <= covered and any(c < E.JUMP_BLOCK and c > 1 for c in covered)
    assert {e % E.JUMP_BLOCK for e in E.HEAD_ENTRIES} >= {0, 5, E.JUMP_BLOCK - 1}


def test_far_jump_over_a_crowd_case():
    """case 7, the look-back: a jump of 1101 indices on the chain over 1100 records that land one index further (asserted in the builder)"""
    c = E.case_far_jump_over_a_crowd()
    is_the_selection(c)
    assert c.sel.max_jump > 2 * E.MARK_TILE and c.sel.M >= E.ONE_PASS_EARLY_FROM


@pytest.mark.parametrize("L", E.JUMP_BRUTE_L + E.JUMP_TILE_L + E.JUMP_LIMIT_L)
def test_jump_cases(L):
    """cases 7 and 8: the largest jump is L^2 + 2 L -- by the two loops for L = 3, 5, 8, by the model beyond; on the stated side of
    a tile and of 60000; the tiles without a synchronisation point"""
    c = E.case_jumps(L)
    is_the_selection(c)
    assert c.sel.max_jump == L * L + 2 * L
    if L in E.JUMP_BRUTE_L:
        same_as_the_loops(c.sel, "shortest")
        assert int(E.jumps(E.shortest_next_plain(c.sel.all)).max()) == {3: 15, 5: 35, 8: 80}[L]
    if L in E.JUMP_TILE_L:
        assert c.sel.max_jump > {30: 1, 100: 19}[L] * E.MARK_TILE
        landings = E.landings_into_tiles(c.sel)
        crowded = [x > E.SYNC_SET for x in landings]
        run = max(len(r) for r in "".join("x" if x else " " for x in crowded).split(" "))
        assert run >= {30: 3, 100: 40}[L], (landings, run)  # so many tiles in a row without a synchronisation point
        assert c.sel.M >= {30: 2000, 100: 25000}[L]
        for entry in E.JUMP_ENTRIES[1:]:  # the same list entered a little later: the head is not index 0, the chain meets other records
            other = E.case_jumps(L, entry)
            is_the_selection(other)
            # (both chains end on the second run's first record)
            assert other.sel.head > 0 and not set(other.sel.chain[:-1].tolist()) & set(c.sel.chain[:-1].tolist())
    if L in E.JUMP_LIMIT_L:
        assert (c.sel.max_jump > E.ONE_PASS_MAX_JUMP) == (L == E.JUMP_LIMIT_L[1])
        assert 59000 < c.sel.max_jump < 61000 and c.sel.M > 140000 and c.d.max_len == 2 * L
