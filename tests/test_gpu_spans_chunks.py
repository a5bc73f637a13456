"""GPU tests of the spans merge (csrc/acgpu_spans.hip) and of the cover entries behind it (csrc/acgpu_cover.hip) where the SECOND
level of their two-level scans does real work, and where the reservoir is full:

 * k_span_scan_mins, k_span_offsets and k_cover_plan_offsets are ONE workgroup each over the tiles' values, N.SPAN_BLOCK = 256 of them
   per step with a running carry.  Up to 64 tiles only wave 0 of that workgroup holds a value; from 65 on block_suffix_min /
   block_prefix_sum / plan_block_scan combine waves; from 257 on -- N.SPAN_CHUNK + 1 = 524 289 intervals in one piece -- the step
   loop runs twice and its carry is read.
 * a reservoir of 512 Set records: the piece driver (csrc/acgpu_pieces.hip) cuts the text by its density, and `own_hi` of pieces
   whose size no tunable chose decides `bound`, the final / carry split and the settled position.

Every expected value is tests/spans_ref.merge -- a coverage bitmap -- or tests/cover_ref.cover_ref over the CPU oracle's records;
host and device entry in every case (the helpers of tests/test_gpu_spans.py and tests/test_gpu_cover.py, with their canaries behind
cap); every case asserts from the oracle's records and the returned stats that it is in the regime it names."""
import functools

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.spans import spans_utf8
from ahocorasick_amd.strings import Automaton, utf16
from tests import test_gpu_cover as V
from tests import test_gpu_cover_utf8 as V8
from tests import test_gpu_spans as S
from tests.spans_ref import merge
from tests.test_gpu_tiny_pieces import family_case
from tests.test_gpu_utf8 import expected, keywords_from, mixed_text
from tests.test_gpu_utf8 import pair as pair_utf8

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20),
            ("replace_slab_units", 1 << 25), ("cover_lds_segments", N.COVER_LDS_SEGMENTS)]
T = N.SPAN_TILE
C = N.SPAN_CHUNK  # the intervals of 256 tiles: interval C is the first of tile 256, the first tile of the level-2 scans' second step
COUNTS = (64 * T, 64 * T + 1, C - 1, C, C + 1, C + T + 1)  # 64 | 65 tiles; 256 | 257 | 258 tiles
SMALL_RESERVOIR = 4096  # bytes: 512 Set records, a twenty-fifth of the random text's
TINY_RESERVOIR = 64  # bytes: 8 Set records, for the texts that 512 records hold whole or nearly
# The families whose only kernel is sequential over the whole text (shard_rule, csrc/acgpu_call.hip).  None of family_case(mode,
# True) is: tests/test_gpu_spans.py::test_tiny_pieces_every_family asserts pieces for all five.
ONE_PIECE = ()


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def one_large_piece():
    """the texts of the largest counts have more than 1 << 20 units: a first piece that takes them whole"""
    N.set_tunable("cursor_first_piece", 1 << 21)
    N.set_tunable("cursor_max_piece", 1 << 21)


def match(orc, hay, per_unit=1):
    hay = utf16(hay)
    return orc.match(hay, cap=per_unit * hay.size + 1024)


# ---- A. the level-2 scans: 64 to 65 tiles, and past one chunk -------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
def test_as_many_spans_as_records_past_a_wave_and_a_chunk_of_tiles(count):
    """The first to reach: block_prefix_sum's `if (i < w) base += wsum[i]` inside k_span_offsets (65 tiles: wave 1 holds a count),
    and k_span_offsets' `tcnt[b] = (uint32_t)carry + ex` with carry != 0 (257 tiles).  Every record closes a span, so tile t's
    offset is t * T: without the cross-wave sum span 64 T would land at index 0, without the carry span C at index 0 -- either way
    a span list of the right length with wrong entries, which the comparison with the bitmap's spans shows."""
    one_large_piece()
    a, orc = S.pair(N.MODE_ALL, ["a"])
    hay = utf16("a." * count)
    want, st = S.check_both(a, orc, hay, match(orc, hay))
    assert st.n_records == count == len(want)
    assert st.pieces - st.rescans == 1, (st.pieces, st.rescans)  # one merge saw all of it


def one_span_text(count):
    """tests/test_gpu_spans.py::test_one_span_of_all_records_at_the_tile_seams: "a" * k under {a, aa} has 2 k - 1 records; an even
    count takes a "b" behind them and the keyword "ab", one record more"""
    k = (count + 1) // 2
    return "a" * k + ("b" if count % 2 == 0 else "")


@pytest.mark.parametrize("count", COUNTS)
def test_one_span_of_all_records_past_a_wave_and_a_chunk_of_tiles(count):
    """The first to reach: block_suffix_min's `if (i > w) ex = std::min(ex, wmin[i])` inside k_span_scan_mins (65 tiles), and
    k_span_scan_mins' `tmin[b] = std::min(carry, ex)` with carry != kNoStart (257 tiles: the step over tiles 0 .. 255 runs second
    and takes the minimum of tile 256 from `carry`).  The starts ascend, so X_i of tile 255's last interval is the first start of
    tile 256: without the carry it is +infinity, the interval closes, and the answer is two spans instead of one."""
    one_large_piece()
    a, orc = S.pair(N.MODE_ALL, ["a", "aa", "ab"])
    hay = utf16(one_span_text(count))
    want, st = S.check_both(a, orc, hay, match(orc, hay, 2))
    assert want.tolist() == [[0, hay.size]] and st.n_records == count
    # no density is known before the first scan, so its room is a record per unit; the text has two, and the scan is repeated
    assert st.rescans >= 1 and st.pieces - st.rescans == 1, (st.pieces, st.rescans)


@functools.lru_cache(maxsize=None)
def dense(n_units):
    """tests/test_gpu_spans.py's random text (seed 4306, 20 keywords over "ab.") at n_units, its records and its spans"""
    a, orc, hay, recs = S.random_dense(n_units)
    assert (np.diff(recs[:, 1].astype(np.int64)) >= 0).all()  # the ends ascend
    return a, orc, hay, recs, merge(recs[:, :2], hay.size)


def heads_of(recs, want):
    """the first record that ends inside span k (the records' ends ascend): the interval that is span k's head"""
    return np.searchsorted(recs[:, 1].astype(np.int64), want[:, 0], side="right")


def test_random_dense_text_of_one_and_a_quarter_chunks():
    """600 000 units: 654 008 records in 320 tiles, 63 564 spans.  The first to reach, on a text that is not periodic: both carries
    above at once, with heads and closing intervals on either side of interval C and inside tile 256, whose span indices are
    toff[256] + ... = carry + ex of k_span_offsets' second step."""
    a, orc, hay, recs, want = dense(600_000)
    assert C < len(recs) < 2 * C, len(recs)
    heads = heads_of(recs, want)
    tiles = {int(h) // T for h in heads}
    assert min(tiles) < 255 and max(tiles) > 257 and 255 in tiles and 256 in tiles and 257 in tiles, (min(tiles), max(tiles))
    assert len(recs) > 257 * T and len(want) > 1000
    got, st = S.check_both(a, orc, hay, recs)
    assert st.pieces - st.rescans == 1, (st.pieces, st.rescans)


CUT = 600_000  # the first piece of the next test owns the units in front of it


def test_random_dense_text_whose_first_merge_is_not_the_last():
    """640 000 units in two pieces, the first of 600 000: a merge of more than C intervals that is NOT the last.  The first to
    reach: k_span_offsets' `fin += total_f` over two steps with final_below() a real bound -- slot[0] = fin and slot[1] = carry -
    fin split the spans behind tile 256 -- and k_span_scatter's span_slot() sending span n_final, whose index is toff[319] + ...
    from the second step, to the carry buffer."""
    a, orc, hay, recs, want = dense(640_000)
    ends = recs[:, 1].astype(np.int64)
    max_len = 6
    # the regime, from the records: AhoCorasick's piece owns the records that END in it; more than C of them end in the first, a
    # span straddles the cut, and a record of the first piece ends at or behind bound = CUT + 1 - max_len: its span is carried
    assert C < int((ends <= CUT).sum()) < len(recs)
    assert ((want[:, 0] < CUT) & (want[:, 1] > CUT)).any(), "no span straddles the cut"
    assert ((ends >= CUT + 1 - max_len) & (ends <= CUT)).any(), "no record of the first piece ends behind the bound"
    N.set_tunable("cursor_first_piece", CUT)
    N.set_tunable("cursor_max_piece", 1 << 26)
    got, st = S.check_both(a, orc, hay, recs)
    assert st.pieces - st.rescans == 2 and st.max_carry >= 1, (st.pieces, st.rescans, st.max_carry)


@pytest.mark.parametrize("body,open,close", [("drop", "#", ""), ("drop", "##", ""), ("keep", "(", ")")])
def test_cover_of_one_more_span_than_a_chunk(body, open, close):
    """C + 1 spans of one unit in one piece.  DROP reaches k_cover_plan_offsets' second step, `bsum[b] = carry + ex` for plan
    block 256, and plan_block_scan's `if (i < w) base += wsum[i]`.  The plan sums what an item adds, len(open) minus the span's one
    unit: nothing under "#", where pos[C] = 2 C must come out of sums that are all zero, and one unit per span under "##", where
    pos[C] = 3 C only with the carry of the first step, 262 144.  KEEP is pos_at()'s closed form `i * (ol + cl)` with i past 2^19.
    A position too small sends the emit's segment searches to the wrong span: the text is wrong from output unit pos[C] on."""
    one_large_piece()
    a, orc = S.pair(N.MODE_ALL, ["a"])
    count = C + 1
    hay = utf16("a." * count)
    recs = match(orc, hay)
    assert len(recs) == count > 256 * N.PLAN_TILE
    want, st = V.check_both(a, hay, recs, open, close, body)  # (asserts n_records, n_spans and units_out of both entries)
    assert st.n_spans == count and st.units_out == len(want) == count * (1 + len(open) + len(close) + (body == "keep"))
    assert st.pieces - st.rescans == 1, (st.pieces, st.rescans)


def test_cover_drop_of_the_random_dense_text():
    """The 63 564 spans of the 600 000-unit text under DROP: the plan's grid is sized by m = 654 008 intervals, 320 blocks of which
    all but 32 lie wholly beyond n = slot[0].  The first to reach k_cover_sums' and k_cover_plan's `first + k < n` false for whole
    blocks, and k_cover_plan_offsets' second step over sums that are all zero."""
    a, orc, hay, recs, spans_want = dense(600_000)
    assert (len(recs) + N.PLAN_TILE - 1) // N.PLAN_TILE > N.SPAN_BLOCK and (len(spans_want) + N.PLAN_TILE - 1) // N.PLAN_TILE < 64
    want, st = V.check_both(a, hay, recs, "***", "", "drop")
    assert st.n_spans == len(spans_want) and st.pieces - st.rescans == 1, (st.n_spans, st.pieces, st.rescans)


# ---- C. a full reservoir ------------------------------------------------------------------------------------------------------
def shrunk(mode, st, n_records, reservoir):
    """what the stats of a call in a reservoir of `reservoir` bytes must say"""
    budget = reservoir // N.REC_SET
    if mode in ONE_PIECE:  # the one sequential scan takes the exact count past the budget: one repeat, one piece
        assert st.pieces - st.rescans == 1, (st.pieces, st.rescans)
    elif n_records > 6 * budget:  # a scan that is not repeated holds the budget at most, and the ramp aims at half of it
        assert st.rescans >= 1 and st.pieces > 10, (st.pieces, st.rescans)
    else:  # the first scan has room for the whole budget, min(budget, max(units, 4096)) records: it is repeated iff they do not fit
        assert (st.rescans >= 1) == (n_records > budget), (st.pieces, st.rescans, n_records)


def family_in(mode, reservoir):
    """family_case(mode, True) and an automaton whose pool is made under the reservoir (a reservoir never shrinks).  The texts
    have 49 .. 538 records in 774 .. 834 units: of the five only AhoCorasick's overflows 512 records, and that by 26.  8 records
    is a reservoir all five texts fill more than 6 times."""
    c = family_case(mode, True)
    assert len(c.recs) > 6 * (TINY_RESERVOIR // N.REC_SET)
    N.set_tunable("cursor_reservoir_bytes", reservoir)
    return c, Automaton(mode, c.kws, True, word_chars=c.wc)


def test_spans_of_the_random_text_in_a_full_reservoir():
    """The first spans call whose pieces the ramp cuts (PieceRamp::on_overflow, next_size): spans_bound(own_hi) and the final /
    carry split at positions no tunable chose."""
    N.set_tunable("cursor_reservoir_bytes", SMALL_RESERVOIR)
    a, orc, hay, recs = S.random_dense(12000)  # (a pool made after the tunable: a reservoir never shrinks)
    assert len(recs) > 20 * (SMALL_RESERVOIR // N.REC_SET)
    want, st = S.check_both(a, orc, hay, recs)
    shrunk(N.MODE_ALL, st, len(recs), SMALL_RESERVOIR)
    assert st.max_carry >= 1


@pytest.mark.parametrize("reservoir", [SMALL_RESERVOIR, TINY_RESERVOIR])
@pytest.mark.parametrize("mode", sorted(S.MODES))
def test_spans_of_every_family_in_a_full_reservoir(mode, reservoir):
    """... for the first-unit families too, whose B is max(bound, the end of the list's last interval)"""
    c, a = family_in(mode, reservoir)
    want, st = S.check_both(a, c.oracle, c.hay, c.recs)
    shrunk(mode, st, len(c.recs), reservoir)


@pytest.mark.parametrize("body,open,close", V.USES)
def test_cover_of_the_random_text_in_a_full_reservoir(body, open, close):
    """The first cover call whose `done` and L (k_span_settled, cover_piece) come from pieces the ramp cut, each emitted through
    slabs of 1000 units."""
    N.set_tunable("cursor_reservoir_bytes", SMALL_RESERVOIR)
    N.set_tunable("replace_slab_units", 1000)
    a, orc, hay, recs = S.random_dense(12000)
    want, st = V.check_both(a, hay, recs, open, close, body)
    shrunk(N.MODE_ALL, st, len(recs), SMALL_RESERVOIR)
    assert st.units_out == len(want) and st.max_carry >= 1


@pytest.mark.parametrize("body,open,close", V.USES)
@pytest.mark.parametrize("reservoir", [SMALL_RESERVOIR, TINY_RESERVOIR])
@pytest.mark.parametrize("mode", sorted(S.MODES))
def test_cover_of_every_family_in_a_full_reservoir(mode, reservoir, body, open, close):
    c, a = family_in(mode, reservoir)
    N.set_tunable("replace_slab_units", 1000)
    want, st = V.check_both(a, c.hay, c.recs, open, close, body)
    shrunk(mode, st, len(c.recs), reservoir)
    assert st.units_out == len(want)


@functools.lru_cache(maxsize=None)
def mixed_utf8(mode):
    """tests/test_gpu_spans_utf8.py's text of 1- to 4-byte sequences and its dictionary -> (bytes, keywords, records in bytes)"""
    text = mixed_text(np.random.default_rng(77), 1500)
    data = text.encode()
    assert 2000 < len(data) < 6000 and {len(ch.encode()) for ch in text} == {1, 2, 3, 4}
    kws = keywords_from(np.random.default_rng(78 + mode), text, mode, True)
    return data, kws, expected(pair_utf8(mode, kws)[1], data)[1]


@pytest.mark.parametrize("reservoir", [SMALL_RESERVOIR, TINY_RESERVOIR])
@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_LONGEST])
def test_utf8_spans_and_cover_in_a_full_reservoir(mode, reservoir):
    """The first to send the bound of a piece the ramp cut through utf8_map_position (spans_piece: `Bd.d_bound = slot + 2`): a
    position in units that no fixed piece size chooses, rounded down to a byte offset that may lie inside a span.  The text has 90
    (AhoCorasick) and 300 (LongestMatch) records: 512 of them hold it whole, 8 do not."""
    data, kws, recs_b = mixed_utf8(mode)
    want = merge(recs_b[:, :2], len(data))
    assert len(recs_b) > 6 * (TINY_RESERVOIR // N.REC_SET) and len(want) >= 10
    N.set_tunable("cursor_reservoir_bytes", reservoir)
    N.set_tunable("replace_slab_units", 1000)
    a = pair_utf8(mode, kws)[0]
    st = N.SpansStats()
    got = spans_utf8(a, data, stats=st)
    assert got.dtype == np.int32 and got.shape == want.shape and (got == want).all()
    assert (st.n_records, st.n_spans) == (len(recs_b), len(want)), (st.n_records, st.n_spans)
    shrunk(mode, st, len(recs_b), reservoir)
    for body, open, close in V8.USES8:
        out, cst = V8.check(a, data, recs_b, open, close, body)
        shrunk(mode, cst, len(recs_b), reservoir)
        assert cst.units_out == len(out)
