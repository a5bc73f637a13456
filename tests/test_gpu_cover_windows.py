"""GPU tests of the cover host entries (include/acgpu.h: acgpu_cover_u16, acgpu_cover_utf8) where the result leaves through MORE
THAN ONE slab: emit_through_slabs (csrc/acgpu_emit.h) calls k_cover_emit (csrc/acgpu_cover.hip) once per window [w0, w1) of
"replace_slab_units" elements, and every other cover test emits one window with w0 == 0.  A window here begins inside an open, a
body, a close and uncovered text, on a span whose output position lies in front of w0, anywhere in a DROP plan's `pos`; the two
slabs and their event pairs are used again by every piece of a call.  The device entry has no slabs: host entries only.

Every expected value is tests/cover_ref.cover_ref over the CPU oracle's records, and the same call under the default slab -- one
window -- must give it too.  The helpers, with their sentinels behind cap, are those of tests/test_gpu_cover.py and
tests/test_gpu_cover_utf8.py."""
import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, utf16
from tests import test_gpu_cover as V
from tests import test_gpu_cover_utf8 as V8
from tests.cover_ref import cover_ref
from tests.spans_ref import merge
from tests.test_gpu_spans_chunks import mixed_utf8
from tests.test_gpu_tiny_pieces import family_case
from tests.test_gpu_utf8 import expected
from tests.test_gpu_utf8 import pair as pair_utf8

pytestmark = pytest.mark.gpu

DEFAULT_SLAB = 1 << 25
DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20),
            ("replace_slab_units", DEFAULT_SLAB), ("cover_lds_segments", N.COVER_LDS_SEGMENTS)]
T = N.COVER_TILE_UNITS
TB = N.COVER_TILE_BYTES


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def slabs(units):
    N.set_tunable("replace_slab_units", units)


def through(entry, a, hay, want, n_spans, slab, open, close, body, fill):
    """the host entry `entry` (V.host_raw or V8.host_raw) with exactly the capacity the result needs, under the default slab and
    under `slab`, against the reference -> the stats of the call under `slab`"""
    for units in (DEFAULT_SLAB, slab):
        slabs(units)
        got, rc, n_out, st = entry(a, hay, len(want), open, close, body, fill)
        assert rc == N.OK and n_out == len(want), (units, rc, n_out, len(want))
        bad = np.flatnonzero(got != want)
        assert not len(bad), (units, bad[:5], got[bad[:5]], want[bad[:5]])
        assert (st.n_spans, st.units_out) == (n_spans, len(want)), (units, st.n_spans, st.units_out)
    return st


def check_u16(a, hay, recs, slab, open="", close="", body="keep", fill="*"):
    hay = utf16(hay)
    want = cover_ref(hay, recs[:, :2], utf16(open), utf16(close), body, int(utf16(fill)[0]))
    assert len(want) > slab, "one window"
    return want, through(V.host_raw, a, hay, want, len(merge(recs[:, :2], hay.size)), slab, open, close, body, fill)


def check_u8(a, data, recs_b, slab, open=b"", close=b"", body="keep", fill=b"*"):
    want = cover_ref(V8.u8(data), recs_b[:, :2], V8.u8(open), V8.u8(close), body, fill[0])
    assert len(want) > (slab + 15) // 16 * 16, "one window"
    return want, through(V8.host_raw, a, data, want, len(merge(recs_b[:, :2], len(data))), slab, open, close, body, fill)


def window_starts_inside(n_text, spans, ol, cl, body, slab):
    """From the reference's layout alone: the sources -- "open", "body", "close", "text" -- that hold a multiple of `slab` STRICTLY
    inside one of their stretches of the output (behind its first element and in front of its end)."""
    kinds, o, last = set(), 0, 0

    def stretch(kind, length):
        nonlocal o
        first = (o // slab + 1) * slab  # the first multiple behind o
        if first < o + length:
            kinds.add(kind)
        o += length

    for s, e in spans.tolist():
        stretch("text", s - last)
        stretch("open", ol)
        stretch("body", 0 if body == "drop" else e - s)
        stretch("close", cl)
        last = e
    stretch("text", n_text - last)
    return kinds, o


# ---- B1. an ordinary text ---------------------------------------------------------------------------------------------------------
ORDINARY = "ab.bcd..b.abab..bcdb.b..ab.b.bcdd.dd...." * 130  # tests/test_gpu_cover.py::test_the_global_memory_view_on_an_ordinary_text


@pytest.mark.parametrize("lds_cap", [None, 0])
@pytest.mark.parametrize("slab", [8, 1000])
@pytest.mark.parametrize("body,open,close", V.USES)
def test_an_ordinary_text_through_slabs(body, open, close, slab, lds_cap):
    """The first to reach k_cover_emit with A.w0 != 0: `t0 = A.w0 - mis + blockIdx.x * kEmitTile` and `bounds[0] =
    last_at_or_before(A, ov0)` with ov0 = w0 > 0, so that segment i0 is a span in the middle of the list whose position lies in
    front of the window (make_seg: P < 0, rel = -1).  Slab 8: every window is one vector of one lane; slab 1000: a window is half
    a tile and ends inside a vector's worth of elements."""
    a, orc = V.pair(N.MODE_ALL, ["ab", "b", "bcd", "dd"])
    recs = V.match(orc, ORDINARY)
    if lds_cap is not None:
        N.set_tunable("cover_lds_segments", lds_cap)
    want, st = check_u16(a, ORDINARY, recs, slab, open, close, body)
    assert len(want) > 2 * T


# ---- B2. windows that start inside each source ------------------------------------------------------------------------------------
LONG_OPEN = "".join(chr(0x100 + i % 997) for i in range(5000))  # tests/test_gpu_cover.py::test_whole_tiles_inside_one_open_and_one_close
LONG_CLOSE = "".join(chr(0x2000 + i % 991) for i in range(4500))
# (family, keywords, text, open, close, bodies): that test's text; the 5200-unit body of test_a_body_that_crosses_three_tiles; and
# the first text with an uncovered run of more than two slabs in it
INSIDE = {"long open and close": (N.MODE_LONGEST, ["ab", "c"], ".ab...c" + "." * 37 + "ab", LONG_OPEN, LONG_CLOSE, ("keep", "fill", "drop")),
          "long body": (N.MODE_ALL, ["ab", "ba", "zz"], "..zz." + "ab" * 2600 + ".x.zz", "<i>", "</i>", ("keep", "fill")),
          "long uncovered run": (N.MODE_LONGEST, ["ab", "c"], ".ab...c" + "." * 2037 + "ab", LONG_OPEN, LONG_CLOSE, ("keep", "fill", "drop"))}
INSIDE_WANT = {"long open and close": {"open", "close"}, "long body": {"body"}, "long uncovered run": {"open", "close", "text"}}


def inside_case(name):
    mode, kws, hay, open, close, bodies = INSIDE[name]
    a, orc = V.pair(mode, kws)
    recs = V.match(orc, hay)
    return a, hay, recs, merge(recs[:, :2], len(hay)), open, close, bodies


def inside_regime(name, spans, body):
    mode, kws, hay, open, close, bodies = INSIDE[name]
    kinds, n = window_starts_inside(len(hay), spans, len(open), len(close), body, 1000)
    assert kinds >= INSIDE_WANT[name], (name, body, kinds)
    return kinds, n


@pytest.mark.parametrize("name,body", [(name, body) for name in sorted(INSIDE) for body in INSIDE[name][5]])  # (DROP has no body to start inside)
def test_windows_that_start_inside_each_source(name, body):
    """The first to reach emit_tile with a window's first lane inside an open (`u < s.a_end`, s.osrc = -P with P < 0 by thousands
    of units), inside a KEEP / FILL body (`u < s.b_end`, s.bsrc), inside a close (`u < s.c_end`, s.csrc) and inside uncovered text
    (`s.tsrc`), each at an output offset that is no multiple of a tile -- the sources are addressed modulo 2^32 from a negative
    P, which one window from 0 never has for its first tile."""
    a, hay, recs, spans, open, close, bodies = inside_case(name)
    kinds, n = inside_regime(name, spans, body)
    want, st = check_u16(a, hay, recs, 1000, open, close, body, fill="#")
    assert len(want) == n


def test_the_windows_of_the_cases_above_start_inside_all_four_sources():
    """the regime of the test above, from the reference's layout alone"""
    seen = set()
    for name in sorted(INSIDE):
        a, hay, recs, spans, open, close, bodies = inside_case(name)
        for body in bodies:
            seen |= inside_regime(name, spans, body)[0]
    assert seen == {"open", "body", "close", "text"}, seen


# ---- B3. the densest DROP plan across windows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_cap", [None, 0])
@pytest.mark.parametrize("open", ["", "|"])
def test_one_unit_spans_alternating_with_one_uncovered_unit_through_slabs(open, lds_cap):
    """The first to reach last_at_or_before over a DROP source -- a search of A.pos -- for a window that begins in the middle of the plan: with
    no open a window of 1000 units holds 1000 spans (its first is span w0, pos[w0] == w0), with "|" 500."""
    a, orc = V.pair(N.MODE_ALL, ["a"])
    hay = "a." * (3 * T + 5) + "a"
    recs = V.match(orc, hay)
    if lds_cap is not None:
        N.set_tunable("cover_lds_segments", lds_cap)
    want, st = check_u16(a, hay, recs, 1000, open, "", "drop")
    assert st.n_spans == 3 * T + 6 and len(want) == (3 * T + 5) * (1 + len(open)) + len(open) >= 3 * T


# ---- B4. slabs times pieces -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body,open,close", V.USES)
@pytest.mark.parametrize("mode", sorted(V.MODES))
def test_slabs_of_8_units_in_pieces_of_16_every_family(mode, body, open, close):
    """The first to reach emit_through_slabs' `if (copied[b]) hipStreamWaitEvent(stream, d.replace_ev[2 + b])` under cover, and the
    same two slabs and four events used again by the next piece: a piece of 16 units leaves in two or more windows, whose
    destinations continue at c.h_out + c.out_pos behind the piece before."""
    c = family_case(mode, True)
    a = Automaton(mode, c.kws, True, word_chars=c.wc)
    want = cover_ref(c.hay, c.recs[:, :2], utf16(open), utf16(close), body, ord("*"))
    n_spans = len(merge(c.recs[:, :2], c.hay.size))
    got, rc, n_out, st = V.host_raw(a, c.hay, len(want), open, close, body)  # the default sizes: one piece, one window
    assert rc == N.OK and (got == want).all()
    V.pieces(16)
    slabs(8)
    got, rc, n_out, st = V.host_raw(a, c.hay, len(want), open, close, body)
    assert rc == N.OK and n_out == len(want), (rc, n_out, len(want))
    V.same(got, want, "host")
    assert (st.n_records, st.n_spans, st.units_out) == (len(c.recs), n_spans, len(want))
    assert st.pieces >= c.hay.size // 16, st.pieces


# ---- B5. capacity inside a later slab -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body,open,close", V.USES)
def test_capacity_that_ends_inside_a_later_slab(body, open, close):
    """The first to reach emit_piece's `emit_total = std::min(total, room)` from a cover call as the end of a window that is not the first: the last
    window [w0, cap) is shorter than a slab, or one element long (cap = 1001)."""
    a, orc = V.pair(N.MODE_ALL, ["ab", "b", "bcd", "dd"])
    hay = utf16(ORDINARY)
    want = cover_ref(hay, V.match(orc, hay)[:, :2], utf16(open), utf16(close), body, ord("*"))
    n = len(want)
    assert n > 2002
    slabs(1000)
    for cap in (999, 1000, 1001, n // 2, n - 1):
        got, rc, n_out, st = V.host_raw(a, hay, cap, open, close, body)  # (asserts the sentinel behind cap)
        assert rc == N.E_OVERFLOW and n_out == n == st.units_out, (cap, rc, n_out, n)
        V.same(got, want[:cap], "cap %d" % cap)


# ---- B6. the UTF-8 twins ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_cap", [None, 0])
@pytest.mark.parametrize("slab", [8, 1000])  # (in bytes a slab is a whole number of 16: 16 and 1008)
@pytest.mark.parametrize("body,open,close", [("keep", "«".encode(), "»".encode()), ("fill", b"", b""), ("drop", "[…]".encode(), b"")])
def test_utf8_mixed_text_through_slabs(body, open, close, slab, lds_cap):
    """k_cover_emit<uint8_t> with A.w0 != 0, on the text of 1- to 4-byte sequences"""
    data, kws, recs_b = mixed_utf8(N.MODE_ALL)
    a = pair_utf8(N.MODE_ALL, kws)[0]
    if lds_cap is not None:
        N.set_tunable("cover_lds_segments", lds_cap)
    want, st = check_u8(a, data, recs_b, slab, open, close, body)
    want.tobytes().decode()  # the result is well-formed


@pytest.mark.parametrize("body", ["keep", "fill", "drop"])
def test_utf8_windows_that_start_inside_each_source(body):
    """tests/test_gpu_cover_utf8.py::test_whole_tiles_inside_one_open_and_a_body_over_three_tiles in windows of 1008 bytes"""
    a, orc = pair_utf8(N.MODE_ALL, ["ab", "ba", "é"])
    open = bytes(33 + i % 89 for i in range(5000))
    close = bytes(40 + i % 83 for i in range(4700))
    run = "ab" * 4400
    data = (".é.." + run + ".x.é").encode()
    recs_b = expected(orc, data)[1]
    spans = merge(recs_b[:, :2], len(data))
    kinds, n = window_starts_inside(len(data), spans, len(open), len(close), body, 1008)
    assert kinds == ({"open", "close"} if body == "drop" else {"open", "body", "close"}), kinds
    want, st = check_u8(a, data, recs_b, 1000, open, close, body, fill=b"#")
    assert len(want) == n


@pytest.mark.parametrize("open", [b"", b"|"])
def test_utf8_one_byte_spans_alternating_with_one_uncovered_byte_through_slabs(open):
    a, orc = pair_utf8(N.MODE_ALL, ["a"])
    data = b"a." * (3 * TB + 5) + b"a"
    recs_b = expected(orc, data)[1]
    want, st = check_u8(a, data, recs_b, 1000, open, b"", "drop")
    assert st.n_spans == 3 * TB + 6 and len(want) >= 3 * TB
