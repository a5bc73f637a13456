"""GPU parity tests of the edges of the tile kernel (csrc/acgpu_tile.hip, k_ac_tile): the start-up and the hand-over of the first
tile group, the classes a lane takes from its left neighbour (lane, tile, tile-group and region boundaries), the number of
verification batches a drain runs, and consecutive calls on one scratch pool.  Every case goes through the C ABI
(acgpu_match_device) and is compared with the CPU oracle (oracle/ac_oracle.c) record for record, in the reference's order.

Dictionaries: a few hundred lower-case keywords of 4..12 letters from the benchmark dictionary's generator (the packed filter
with the second level, `k_ac_tile<4, true, false, false, false, true, true>`); a mixed-case, case-sensitive dictionary (merged
range classes, verification by units); and a case-insensitive one over a..k (folded range classes: a tile that holds a unit
with a bit of DevTables::fr_himask -- U+0130, U+212A, any CJK unit -- takes its classes from the table instead).

Regions: the tunable region_units at its minimum, one tile group (2048 units), puts a region seam every 2048 units; 0 leaves
the library's own choice (16384 here).  The launcher sizes the grid to the waves that own a region, so the last workgroup may
hold waves without one, but a workgroup made of such waves only is never launched."""
import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd import synth
from ahocorasick_amd.strings import Automaton
from oracle.oracle import FAM_AC, Oracle
from tests.helpers import LOWER, rand_case

pytestmark = pytest.mark.gpu

KNOBS = [("force_kernel", 0), ("region_units", 0), ("tile_debug", 0), ("all_form", 0), ("tile_form", 0)]
GROUP = 2048  # units of a tile group = the smallest region; the L2 form's tile is as long
SPACE = ord(" ")


@pytest.fixture(autouse=True)
def _tile_kernel():
    N.set_tunable("force_kernel", 2)
    yield
    for k, v in KNOBS:
        N.set_tunable(k, v)


def _dev(a, d_hay, n, want, own=None):
    """one acgpu_match_device call; the records, and the name of the kernel that scanned"""
    import torch
    cap = len(want) + 16
    d_out = torch.full((cap, 3), -7, dtype=torch.int32, device="cuda")
    n_out, rc, prof, _ = a.match_device(d_hay.data_ptr(), n, True, d_out.data_ptr(), cap, own=own,
                                        stream=torch.cuda.current_stream().cuda_stream, profile=True)
    assert rc == N.OK, rc
    assert prof["scan_kernel"].startswith("k_ac_tile"), prof["scan_kernel"]
    assert n_out <= cap and (d_out[n_out:].cpu().numpy() == -7).all()  # nothing behind the last record was touched
    return d_out[:n_out].cpu().numpy(), prof["scan_kernel"]


def _check(a, orc, hay, own=None, what=None):
    import torch
    want = orc.match(hay, cap=max(4096, hay.size))
    if own is not None:  # a shard reports the occurrences whose last unit it owns
        want = want[(want[:, 1] - 1 >= own[0]) & (want[:, 1] - 1 < own[1])]
    d_hay = torch.from_numpy(np.ascontiguousarray(hay).view(np.int16)).cuda()
    got, kernel = _dev(a, d_hay, hay.size, want, own)
    assert got.shape == want.shape and (got == want).all(), (what, own, got.shape, want.shape)
    return want, kernel


class Case:
    def __init__(self, kws, case_sensitive, alphabet):
        self.kws = kws
        self.a = Automaton(N.MODE_ALL, kws, case_sensitive)
        self.orc = Oracle(FAM_AC, kws, case_sensitive=case_sensitive, lower=None if case_sensitive else LOWER)
        self.alphabet = np.asarray(alphabet, dtype=np.uint16)
        # keywords inside which no other keyword occurs: one occurrence of them is one record
        self.lone = [k for k in kws if len(self.orc.match(np.asarray(k, dtype=np.uint16), cap=64)) == 1]
        assert len(self.lone) >= 8


NESTED = [np.array([ord(c) for c in s], dtype=np.uint16) for s in ("qzjxkvbw", "jxkvbw", "kvbw")]  # three keywords, one end


@pytest.fixture(scope="module")
def lower():
    """config 2's generator, 300 keywords of 4..12 letters: the packed filter with the second level"""
    kws = synth.random_keywords(synth.CONFIGS["C2"]["dict_seed"], 300, 4, 12) + NESTED
    return Case(kws, True, synth.ALPHA_LOWER)


@pytest.fixture(scope="module")
def mixed():
    """mixed-case keywords, case-sensitive: two stretches of letters merged into one set of classes"""
    rng = np.random.default_rng(77)
    low = list(range(ord("b"), ord("z") + 1))
    _, kws = rand_case(rng, low[:12], 200, 11, 16, min_len=4)
    kws = [np.where((rng.integers(0, 2, k.size) == 1) & (k - 32 <= ord("X")), k - 32, k).astype(np.uint16) for k in kws]
    kws = list({k.tobytes(): k for k in kws}.values())
    alphabet = low[:12] + [c - 32 for c in low[:12]] + [SPACE, 0x00E9, 0x4E2D, 0xFFFF]
    return Case(kws, True, alphabet)


@pytest.fixture(scope="module")
def folded():
    """case-insensitive over a..k: folded range classes, and the class table for tiles with a unit beyond the low zone"""
    rng = np.random.default_rng(78)
    low = list(range(ord("a"), ord("k") + 1))
    _, kws = rand_case(rng, low, 60, 10, 16, min_len=4)
    kws = list({k.tobytes(): k for k in kws}.values())
    return Case(kws, False, low + [c - 32 for c in low])


def test_the_lower_case_dictionary_takes_the_packed_filter_with_the_second_level(lower):
    hay = synth.haystack(11, 3 * GROUP + 5)
    _, kernel = _check(lower.a, lower.orc, hay)
    args = kernel.split("<")[1].rstrip(">").split(", ")
    assert args[:2] == ["4", "true"] and args[5:7] == ["true", "true"], kernel


# ---- start-up and hand-over ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("region_units", [GROUP, 0])
def test_short_shards_at_every_start(lower, region_units):
    """shards of 1 .. 2 tile groups + 1 units that begin at units 0, 3, 8 and 11 of the buffer (no carry before unit 8; regions
    laid out from the start rounded down to 8 units), in a text whose first units are keyword occurrences back to back"""
    import torch
    N.set_tunable("region_units", region_units)
    hay = synth.haystack(12, 3 * GROUP).copy()
    k4 = next(k for k in lower.lone if k.size == 4)
    for p in range(0, 32, 4):
        hay[p:p + 4] = k4  # last units 3, 7, 11, ...
    for p in (GROUP - 2, GROUP + 5, 2 * GROUP - 1):
        hay[p:p + 4] = k4
    want = lower.orc.match(hay, cap=hay.size)
    d_hay = torch.from_numpy(hay.view(np.int16)).cuda()
    for begin in (0, 3, 8, 11):
        for length in (1, 7, 8, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP - 1, 2 * GROUP, 2 * GROUP + 1):
            own = (begin, begin + length)
            w = want[(want[:, 1] - 1 >= own[0]) & (want[:, 1] - 1 < own[1])]
            got, _ = _dev(lower.a, d_hay, hay.size, w, own)
            assert got.shape == w.shape and (got == w).all(), own
            # the same units as a buffer of their own (the text begins and ends with the shard)
            sub = hay[begin:begin + length]
            _check(lower.a, lower.orc, sub, what=("sub", own))


@pytest.mark.parametrize("region_units,n_units", [(GROUP, 40 * GROUP + 3), (GROUP, 16 * GROUP), (GROUP, 17 * GROUP - 9), (0, 100_003)])
def test_a_last_workgroup_with_waves_that_own_no_region(lower, region_units, n_units):
    """40 regions: two whole workgroups and one with eight of its sixteen waves idle; 16 and 17 regions: none and all but one"""
    N.set_tunable("region_units", region_units)
    rng = np.random.default_rng(n_units)
    hay = synth.haystack(13, n_units).copy()
    for p in rng.integers(0, n_units - 16, n_units // 200).tolist():
        k = lower.kws[int(rng.integers(0, len(lower.kws)))]
        hay[p:p + k.size] = k
    for own in (None, (11, n_units - 5)):
        want, _ = _check(lower.a, lower.orc, hay, own)
        assert len(want) >= n_units // 400


# ---- the classes of the units in front of a lane's first ------------------------------------------------------------------------

BOUNDARIES = [160, 1024, GROUP - 32, GROUP, 2 * GROUP, 3 * GROUP, 16384]  # lanes, tiles, tile groups, region seams (2048-unit and default regions)


def _boundary_text(case, d, shift, rng, through=None):
    """random text with keyword occurrences that END d units behind every boundary (shifted by `shift`); the text and the
    occurrences' (start, end)"""
    hay = case.alphabet[rng.integers(0, len(case.alphabet), 16384 + 3 * GROUP + 7)].copy()
    by_len = sorted(case.lone, key=lambda k: k.size)
    picks = [by_len[0], by_len[len(by_len) // 2], by_len[-1]]  # the shortest, a middle one, the longest
    spans = []
    for i, b in enumerate(BOUNDARIES):
        k = np.array(picks[(i + d) % 3], dtype=np.uint16)
        if through is not None:
            k = through(k, i + d)
        e = b + shift + d
        hay[e - k.size:e] = k
        spans.append((e - k.size, e))
    return hay, spans


# template arguments <K, RANGE, WIDE, SPLIT, HASHK, PK, L2, ...> of the kernel each dictionary has to select
FORMS = {
    "lower": lambda a: a[1] == "true" and a[5:7] == ["true", "true"],                # range classes, packed filter, second level
    "mixed": lambda a: a[1] == "false" and a[4] == "true" and a[5] == "true",        # merged classes, verification by units, packed
    "folded": lambda a: a[1] == "false" and a[4] == "false" and a[5] == "true",      # folded range classes, packed
}


@pytest.mark.parametrize("which", ["lower", "mixed", "folded"])
@pytest.mark.parametrize("region_units", [GROUP, 0])
def test_occurrences_ending_around_every_boundary(request, which, region_units):
    case = request.getfixturevalue(which)
    N.set_tunable("region_units", region_units)
    rng = np.random.default_rng(5)
    for begin in (0, 8):  # (regions and tiles are laid out from the shard's start rounded down to 8 units)
        for d in range(-1, 13):
            hay, _ = _boundary_text(case, d, begin, rng)
            want, kernel = _check(case.a, case.orc, hay, None if begin == 0 else (begin + 3, hay.size), (which, d))
            args = kernel.split("<")[1].rstrip(">").split(", ")
            assert FORMS[which](args), (which, kernel)
            ends = set(want[:, 1].tolist())
            assert all(b + begin + d in ends for b in BOUNDARIES), (which, d)


@pytest.mark.parametrize("region_units", [GROUP, 0])
def test_units_beyond_the_low_zone_next_to_a_boundary(folded, region_units):
    """the folded form: occurrences spelt through U+0130 (folds to i) and U+212A (folds to k) around the boundaries, and a unit
    that is no keyword unit but has a bit of fr_himask just before and just behind them -- the tile on one side of a boundary
    takes its classes from the table, the one on the other side from the ranges"""
    N.set_tunable("region_units", region_units)
    rng = np.random.default_rng(6)

    def through(k, j):
        k = k.copy()
        k[(k | 32) == ord("i")] = 0x0130 if j % 2 else ord("I")
        k[(k | 32) == ord("k")] = 0x212A if j % 3 else ord("K")
        return k

    assert any(((k | 32) == ord("i")).any() or ((k | 32) == ord("k")).any() for k in folded.lone)
    for d in range(-1, 13):
        hay, spans = _boundary_text(folded, d, 0, rng, through)
        for i, (s, e) in enumerate(spans):  # such a unit right behind the occurrence, or right in front of it
            hay[e if (i + d) % 2 else s - 1] = 0x4E2D
        want, kernel = _check(folded.a, folded.orc, hay, what=d)
        args = kernel.split("<")[1].rstrip(">").split(", ")
        assert args[1] == "false" and args[5] == "true", kernel  # folded range classes, packed filter
        ends = set(want[:, 1].tolist())
        assert all(e in ends for _, e in spans), d


# ---- one verification batch, or two ---------------------------------------------------------------------------------------------

def _region_with(case, k, count, nested_at=None):
    """three 2048-unit regions of spaces; the middle one holds `count` candidates: occurrences of k, one unit apart -- the one
    at index nested_at (if any) is the position where the three NESTED keywords end instead"""
    hay = np.full(3 * GROUP, SPACE, dtype=np.uint16)
    p = GROUP + 3
    for i in range(count):
        w = NESTED[0] if i == nested_at else k
        hay[p:p + w.size] = w
        p += w.size + 1
    assert p < 2 * GROUP
    return hay


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 127, 128, 129])
def test_a_region_with_exactly_that_many_matches(lower, count):
    N.set_tunable("region_units", GROUP)
    k = next(k for k in lower.lone if k.size == 5)
    hay = _region_with(lower, k, count)
    want, _ = _check(lower.a, lower.orc, hay, what=count)
    assert len(want) == count and (count == 0 or ((want[:, 1] > GROUP) & (want[:, 1] <= 2 * GROUP)).all())


@pytest.mark.parametrize("count,nested_at", [(64, 63), (65, 63), (65, 64), (128, 127), (129, 128), (1, 0)])
def test_three_nested_keywords_end_in_the_last_lane_of_a_batch(lower, count, nested_at):
    """the 64th candidate of a region (lane 63 of batch 0) is a position where three keywords end: longest first, and the
    records behind it keep their places -- also as the first candidate of the second batch and of a second drain"""
    N.set_tunable("region_units", GROUP)
    k = next(k for k in lower.lone if k.size == 5)
    hay = _region_with(lower, k, count, nested_at)
    want, _ = _check(lower.a, lower.orc, hay, what=(count, nested_at))
    assert len(want) == count + 2
    three = want[want[:, 1] == want[nested_at, 1]]
    assert len(three) == 3 and (three[:, 1] - three[:, 0]).tolist() == [8, 6, 4]


# ---- consecutive calls on one pool ----------------------------------------------------------------------------------------------

def test_consecutive_calls_on_one_pool(lower):
    """the fused tail of a call zeroes the counters of the next one -- the workgroup numbers among them: a large call, a small
    one, the large one again, and the small one twice more, all on one stream and one scratch pool"""
    import torch
    N.set_tunable("region_units", GROUP)
    rng = np.random.default_rng(9)
    big = synth.haystack(14, 300 * GROUP + 11).copy()
    for p in rng.integers(0, big.size - 16, 4000).tolist():
        k = lower.kws[int(rng.integers(0, len(lower.kws)))]
        big[p:p + k.size] = k
    small = big[:GROUP + 77].copy()
    wants = {id(big): lower.orc.match(big, cap=big.size), id(small): lower.orc.match(small, cap=small.size)}
    devs = {id(h): torch.from_numpy(h.view(np.int16)).cuda() for h in (big, small)}
    for h in (big, small, big, small, small, big):
        got, _ = _dev(lower.a, devs[id(h)], h.size, wants[id(h)])
        assert got.shape == wants[id(h)].shape and (got == wants[id(h)]).all(), h.size
