"""GPU tests of ShortestMatchSet/Map and of LongestMatchSet/Map over a dictionary with a selective suffix filter at the edges of the
selection they share (run_selection and mark_chain, csrc/acgpu_hostrun.hip; k_short_next, k_long_next, k_short_round, k_short_emit,
csrc/acgpu_shortest.hip; k_wwl_jumps, k_wwl_bits_to_mark, csrc/acgpu_wwlongest.hip; k_longest_sync, k_longest_chain_lds,
csrc/acgpu_longest.hip), every record against the CPU oracle, bit for bit, Set and Map:

  1. M records at the seams of the launches -- 8^t (the doubling's `reach <= M`), 256 (grids of M + 1 threads, the sentinel thread
     `k == M`), 512 (the one pass's tile), 2048 (the prefix-sum tile) -- with every record on the chain, one, and every other one;
  2. k_short_next's group search: up to 98 records per end, a successor that is the first, a middle and the last record of its
     group, several groups on, none at all, duplicate keywords, both case rules;
  3. k_long_next's rules: the longest of the records at the smallest start, `e > cur_s + max_len`, `s < limit`, `s >= pos`;
  4. two shards cut on every unit of a stretch of overlapping matches, chained through chain_exit and chain_entry; an entry behind
     every record (mark_chain's `head >= M`);
  5. k_short_emit's `dst >= cap` and its chain exit, with a canary row;
  6. the one pass with its head at an index other than 0 (`Cn.n_tiles` from `M - head`);
  7. the one pass over jumps of 960 and 10 200 indices and runs of tiles without a synchronisation point;
  8. largest jumps of 59 535 and 60 024: `if (max_jump > 60000) one_pass = false` after k_wwl_jumps has run.

The inputs, the model of the selection and the proof that each input reaches its edge are tests/selection_edges.py (checked without
a device by tests/test_selection_inputs_cpu.py).  Every call goes through acgpu_match_device, which never takes the one-launch
form; texts of more than 4096 units also through the host entry.  The marking runs under tile_debug 0, 2097152 (always the
doubling) and 4194304 (the one pass from 64 records on)."""
import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton
from tests import selection_edges as E

pytestmark = pytest.mark.gpu

MODE = {"shortest": N.MODE_SHORTEST, "longest": N.MODE_LONGEST}


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k in ("tile_debug", "force_kernel"):
        N.set_tunable(k, 0)


_automata = {}


def automaton(d, family):
    """one automaton per dictionary and family; a Longest one has to be the sparse form's"""
    key = (id(d), family)
    if key not in _automata:
        a = Automaton(MODE[family], d.kws, d.cs)
        info = a.info()
        assert info["max_keyword_len"] == d.max_len
        if family == "longest":
            assert info["tile_kernel"] == 1, info
        _automata[key] = (a, d)  # (the dictionary is kept: its id is the key)
    return _automata[key][0]


def upload(hay):
    import torch
    return torch.from_numpy(np.array(hay, dtype=np.uint16).view(np.int16)).cuda()  # (a copy: the shared texts are read-only)


def device_call(a, d_hay, n, ids, cap, **kw):
    """acgpu_match_device -> (the records written, n_out, rc, profile, chain_exit); a canary row behind `cap` must survive"""
    import torch
    cols = 3 if ids else 2
    d_out = torch.full((cap + 1, cols), -7, dtype=torch.int32, device="cuda")
    n_out, rc, prof, ex = a.match_device(d_hay.data_ptr(), n, ids, d_out.data_ptr(), cap, profile=True, **kw)
    out = d_out.cpu().numpy()
    assert (out[cap:] == -7).all(), "a record was written behind the capacity"
    return out[:min(n_out, cap)], n_out, rc, prof, ex


def same(got, want):
    return got.shape == want.shape and bool((got == want).all())


def ran_the_selection(family, prof):
    """the profile names the ALL pipeline's scan kernel: the records came through run_selection, not from the Longest walk"""
    name = prof["scan_kernel"]
    assert name.startswith("k_ac_tile") if family == "longest" else name.startswith("k_ac_"), (family, name)


def check_case(c, d_hay=None):
    """Set and Map records and the chain exit of the device entry under each of the case's markers; the host entry too where the
    text is long enough to reach the selection there"""
    a = automaton(c.d, c.family)
    n = c.hay.size
    d_hay = upload(c.hay) if d_hay is None else d_hay
    for bits in c.markers:
        N.set_tunable("tile_debug", bits)
        for ids in (True, False):
            want = c.want if ids else c.want[:, :2]
            got, n_out, rc, prof, ex = device_call(a, d_hay, n, ids, len(want) + 2, chain_entry=c.entry)
            assert rc == N.OK and n_out == len(want) and same(got, want), (c, bits, ids, rc, n_out)
            assert ex == c.sel.exit, (c, bits, ids, ex, c.sel.exit)
            if c.sel.M:
                ran_the_selection(c.family, prof)
            if n > E.SHORT_TEXT and c.entry == 0:
                assert same(a.match_host(c.hay, ids, cap=16), want), (c, bits, ids, "host")  # (overflows once: the call is made twice)
    N.set_tunable("tile_debug", 0)


# ---- 1. record counts at the kernels' seams --------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", E.SEAM_M)
def test_record_counts_at_the_seams_of_the_launches(M):
    """k_short_next / k_short_round run M + 1 threads in blocks of 256, the thread k == M doing the head's work; launch_chain_mark
    launches while `reach <= M`, 8 marks per marked record and launch; the one pass works in tiles of 512 indices, the prefix sum
    under k_short_emit in tiles of 2048.  `a` on a^M: M records, all on the chain -- the doubling's worst case.  {a, b} on
    b^(M-1) a entered at its last unit: the chain is the last record alone, and the head is index M - 1.  {ab, b} on (ab)^(M/2):
    every other record."""
    for c in E.case_seams(M):
        assert c.sel.M == M
        check_case(c)


# ---- 2. k_short_next's group search ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [True, False])
def test_group_search_of_the_shortest_successor(cs):
    """first_starting_at: the end groups are found by binary searches on the ends, a group's first record that starts late enough
    by one on its starts, and `j = gl + 1` goes on to the next group.  a^3 .. a^100 and a few keywords with a b: up to 98 records
    per end; successors that are the first, a middle and the last record of their group, up to several groups on; records without
    a successor a block and more in front of the list's end; two duplicate keywords (the Map reports the first one)."""
    check_case(E.case_groups(cs))


# ---- 3. k_long_next's rules ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_never", [False, True])
@pytest.mark.parametrize("cs", [True, False])
def test_rules_of_the_leftmost_longest_successor(cs, with_never):
    """leftmost_longest_from: the smallest start >= pos wins; at the same start the record later in the list (the longer one); the
    scan stops at `e > cur_s + max_len`.  Three prefix-nested keywords at one start, the longest EXACTLY max_len units -- and
    four units short of it, with a 16-unit keyword in the dictionary that no text holds; a keyword that starts later and ends
    earlier; one that starts inside the previous match and ends with the next one; matches touching end to start, at unit 0 and
    on the last unit.  And the same list entered behind its last start: no record, and the chain leaves at the end of the text."""
    c = E.case_long_rules(cs, with_never)
    d_hay = upload(c.hay)
    check_case(c, d_hay)
    a = automaton(c.d, "longest")
    entry = int(c.sel.all[:, 0].max()) + 1
    for bits in E.ALL_MARKERS:
        N.set_tunable("tile_debug", bits)
        got, n_out, rc, prof, ex = device_call(a, d_hay, c.hay.size, True, 4, chain_entry=entry)
        assert rc == N.OK and n_out == 0 and ex == c.hay.size, (bits, rc, n_out, ex)
        ran_the_selection("longest", prof)


# ---- 4. shards: a cut on every unit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,cs", [("shortest", True), ("longest", True), ("longest", False)])
def test_two_shards_cut_on_every_unit_of_a_stretch(family, cs):
    """Shortest: k_short_next's head from `entry` (upper_end(recs, 0, M, entry), then the first start at or after it) over the
    records whose last unit the shard owns; the exit is the end of the shard's last record, else its entry.  Longest: `s < limit`
    with limit = own_end over the records of the shard and of the max_len - 1 units behind it; the exit is at or behind own_end.
    A cut on every unit of 40 units of overlapping and nested matches, the second shard entered where the first one left: the two
    together are the oracle's records.  And the whole text entered behind its last record's start: nothing, exit == entry."""
    d, hay, cuts, full, want = E.case_cut(family, cs)
    a = automaton(d, family)
    n = hay.size
    d_hay = upload(hay)
    cap = len(want) + 2
    models = {cut: E.two_shards(d, family, hay, full, cut) for cut in cuts}
    for bits in E.ALL_MARKERS:
        N.set_tunable("tile_debug", bits)
        for cut in cuts:
            m_left, m_right = models[cut]
            for ids in ((True, False) if bits == E.MARK_ONE_PASS_EARLY else (True,)):
                left, n_left, rc, prof, ex = device_call(a, d_hay, n, ids, cap, own=(0, cut), chain_entry=0)
                assert rc == N.OK and ex == m_left.exit, (bits, cut, ids, rc, ex, m_left.exit)
                ran_the_selection(family, prof)
                entry = ex if family == "shortest" else max(ex, cut)
                right, n_right, rc, prof, ex2 = device_call(a, d_hay, n, ids, cap, own=(cut, n), chain_entry=entry)
                assert rc == N.OK and ex2 == m_right.exit, (bits, cut, ids, rc, ex2, m_right.exit)
                ran_the_selection(family, prof)
                cols = 3 if ids else 2
                assert same(left, m_left.recs[:, :cols]) and same(right, m_right.recs[:, :cols]), (bits, cut, ids)
                assert same(np.concatenate([left, right]), want[:, :cols]), (bits, cut, ids)
        entry = int(full[:, 0].max()) + 1
        got, n_out, rc, prof, ex = device_call(a, d_hay, n, True, 4, chain_entry=entry)
        assert rc == N.OK and n_out == 0 and ex == (entry if family == "shortest" else n), (bits, rc, n_out, ex)
        ran_the_selection(family, prof)


# ---- 5. capacity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["shortest", "longest"])
def test_capacity_of_the_emit(family):
    """k_short_emit writes `dst < cap` only and sets the chain exit before it looks at the capacity: with room for 0, 1, all but one
    and all records the count is exact, the call overflows exactly when a record is missing, the records that fit are the
    oracle's first, the row behind them is untouched, and the exit is the end of the last SELECTED record."""
    c = E.case_capacity(family)
    a = automaton(c.d, family)
    d_hay = upload(c.hay)
    total = len(c.want)
    for bits in E.ALL_MARKERS:
        N.set_tunable("tile_debug", bits)
        for ids in (True, False):
            want = c.want if ids else c.want[:, :2]
            for cap in (0, 1, total - 1, total):
                got, n_out, rc, prof, ex = device_call(a, d_hay, c.hay.size, ids, cap)
                assert n_out == total and rc == (N.E_OVERFLOW if cap < total else N.OK), (bits, ids, cap, rc, n_out)
                assert same(got, want[:cap]) and ex == c.sel.exit, (bits, ids, cap, ex)
                ran_the_selection(family, prof)


# ---- 6. one pass, the head not at index 0 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", E.HEAD_ENTRIES)
def test_one_pass_from_a_head_that_is_not_index_0(entry):
    """mark_chain's one pass begins at the head k_wwl_jumps reports: Cn.entry = head, Cn.n_tiles from M - head, and k_longest_sync
    reads blockmax[], one word per 64 indices, from the head's block on.  `a` on a^1100 entered at unit c: the head is index c and
    M - head is 1, 511 .. 513 or 1023 .. 1025; a head in the list's last 64 indices; a head on the first, a middle and the last
    index of its block.  {ab, b} on the same units: jumps of 1 and 2 from the same heads."""
    for c in E.case_head(entry):
        assert c.sel.head == entry
        check_case(c)


# ---- 7. one pass, jumps longer than a tile ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", E.JUMP_TILE_L)
def test_one_pass_over_jumps_longer_than_a_tile(L):
    """Shortest over a^L .. a^2L on a^(4L+1) b a^(L+3): the first record of an end group jumps over L^2 + 2L indices -- 960 and
    10 200, two and twenty tiles of 512 -- and the L + 1 records of a group land on one index, so a tile is entered from some L
    distinct landings, more than k_longest_sync follows: tile after tile without a synchronisation point (3 and 45 in a row, by
    the model), the chain carried across them by the one lane that has one.  Entered at unit 0, 1 and 17: three chains over the
    same list that share no record but the last."""
    d_hay = None
    for entry in E.JUMP_ENTRIES:
        c = E.case_jumps(L, entry)
        assert c.sel.max_jump == L * L + 2 * L > E.MARK_TILE and c.sel.M >= E.ONE_PASS_EARLY_FROM
        d_hay = upload(c.hay) if d_hay is None else d_hay
        check_case(c, d_hay)


def test_one_pass_looks_back_over_the_whole_of_the_largest_jump():
    """k_longest_sync collects the landings of the `Cn.max_len` = largest-jump indices in front of a tile.  a, cd, d and a^i c
    (i = 1 .. 1100) on a^1100 c d a^700: the chain jumps from the last a in front of the c over 1101 indices onto cd, the 1100
    records under the jump all land on d, one index further and not on the chain, and the tile at index 2048 begins among them,
    949 indices behind the jumping record.  A look-back shorter than the jump would see d alone and report it."""
    c = E.case_far_jump_over_a_crowd()
    assert c.sel.max_jump == E.CROWD + 1 > 2 * E.MARK_TILE
    check_case(c)


# ---- 8. both sides of 60000 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", E.JUMP_LIMIT_L)
def test_largest_jump_on_both_sides_of_the_one_pass_limit(L):
    """L = 243: the largest jump is 59 535 and the one pass marks the chain; L = 244: 60 024, and mark_chain falls back to the
    doubling AFTER k_wwl_jumps has run and the head has been read back.  Some 150 000 records on 1225 units, keywords of up to
    488 units.  First the list itself: AhoCorasick over the same keywords and text gives the oracle's records, so a failure
    behind it is the selection's."""
    c = E.case_jumps(L)
    assert (c.sel.max_jump > E.ONE_PASS_MAX_JUMP) == (L == E.JUMP_LIMIT_L[1]) and c.sel.M >= E.ONE_PASS_EARLY_FROM
    d_hay = upload(c.hay)
    ac = Automaton(N.MODE_ALL, c.d.kws, True)
    got, n_out, rc, _, _ = device_call(ac, d_hay, c.hay.size, True, c.sel.M + 2)
    assert rc == N.OK and n_out == c.sel.M and same(got, c.sel.all), (L, rc, n_out)
    check_case(c, d_hay)
