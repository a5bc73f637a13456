"""GPU tests of the cover entries in UTF-16 units (include/acgpu.h: acgpu_cover_u16 / acgpu_cover_device; csrc/acgpu_cover.hip: the
settled position behind every piece, the plan of a DROP call and k_cover_emit).  Every expected value is tests/cover_ref.py's
splice over tests/spans_ref.py's merge of the CPU oracle's records; host and device entry in every case, element for element, both
with a sentinel behind cap."""
import ctypes
import importlib

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, LongestMatchSet, utf16
from oracle.oracle import FAM_AC, FAM_LONGEST, FAM_SHORTEST, FAM_WHOLEWORD, FAM_WWLONGEST, Oracle
from tests.cover_ref import cover_ref
from tests.helpers import LOWER, WORD, fixture_inputs
from tests.spans_ref import merge
from tests.test_gpu_tiny_pieces import PIECES, family_case

C = importlib.import_module("ahocorasick_amd.cover")  # (the package's name `cover` is the function)

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20),
            ("replace_slab_units", 1 << 25), ("cover_lds_segments", N.COVER_LDS_SEGMENTS)]
MODES = {N.MODE_ALL: FAM_AC, N.MODE_LONGEST: FAM_LONGEST, N.MODE_WHOLEWORD: FAM_WHOLEWORD, N.MODE_SHORTEST: FAM_SHORTEST,
         N.MODE_WWLONGEST: FAM_WWLONGEST}
WORDY = (N.MODE_WHOLEWORD, N.MODE_WWLONGEST)
T = N.COVER_TILE_UNITS  # the output units one workgroup of k_cover_emit<uint16_t> writes
SENTINEL = 0x5A5A
# the three uses: highlight, mask, redaction -- (body, open, close)
USES = [("keep", "<b>", "</b>"), ("fill", "", ""), ("drop", "***", "")]
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def pieces(p):
    if p:
        N.set_tunable("cursor_first_piece", p)
        N.set_tunable("cursor_max_piece", p)


def pair(mode, kws, cs=True, wc=None):
    if wc is None and mode in WORDY:
        wc = WORD
    return Automaton(mode, kws, cs, word_chars=wc), Oracle(MODES[mode], kws, case_sensitive=cs, lower=None if cs else LOWER, word_chars=wc)


def host_raw(a, hay, cap, open="", close="", body="keep", fill="*"):
    """acgpu_cover_u16 into a buffer with a sentinel behind cap -> (the units written, rc, n_out, stats)"""
    hay = utf16(hay)
    spec, keep = C._spec(utf16(open), utf16(close), C.BODIES[body], int(utf16(fill)[0]))
    out = np.full(cap + 64, SENTINEL, np.uint16)
    n_out, st = ctypes.c_uint64(0), N.CoverStats()
    rc = N.lib().acgpu_cover_u16(a.handle, vp(hay if hay.size else np.zeros(1, np.uint16)), int(hay.size), ctypes.byref(spec), vp(out), cap,
                                 ctypes.byref(n_out), ctypes.byref(st))
    assert (out[cap:] == SENTINEL).all(), "host: written at or beyond cap"
    return out[:min(cap, n_out.value)], rc, int(n_out.value), st


def device_raw(a, hay, cap, open="", close="", body="keep", fill="*", off=0):
    """acgpu_cover_device on the current torch stream, d_out `off` units behind a 16-byte boundary, a sentinel in front of it and
    behind cap -> (units, rc, n_out, stats dict)"""
    import torch
    hay = utf16(hay)
    d_hay = torch.from_numpy(np.ascontiguousarray(hay if hay.size else np.zeros(8, np.uint16)).view(np.int16)).cuda()
    d_out = torch.full((cap + off + 64,), SENTINEL, dtype=torch.int16, device="cuda")
    assert d_out.data_ptr() % 16 == 0 and d_hay.data_ptr() % 16 == 0
    n_out, rc, st = C.cover_device(a, d_hay.data_ptr(), int(hay.size), d_out.data_ptr() + 2 * off, cap, open=open, close=close, body=body, fill=fill,
                                   stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint16)
    assert (got[:off] == SENTINEL).all() and (got[off + cap:] == SENTINEL).all(), "device: written outside [d_out, d_out + cap)"
    return got[off:off + min(cap, n_out)], rc, n_out, st


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert not len(bad), (what, bad[:5], got[bad[:5]], want[bad[:5]])


def check_both(a, hay, recs, open="", close="", body="keep", fill="*", off=0):
    """host and device entry, with exactly the capacity the result needs, against the reference -> (the result, the host's stats)"""
    hay = utf16(hay)
    want = cover_ref(hay, recs[:, :2], utf16(open), utf16(close), body, int(utf16(fill)[0]))
    n_spans = len(merge(recs[:, :2], hay.size))
    got, rc, n_out, st = host_raw(a, hay, len(want), open, close, body, fill)
    assert rc == N.OK and n_out == len(want), ("host", rc, n_out, len(want))
    same(got, want, "host")
    assert (st.n_records, st.n_spans, st.units_out) == (len(recs), n_spans, len(want)), (st.n_records, st.n_spans, st.units_out)
    got, rc, n_out, dst = device_raw(a, hay, len(want), open, close, body, fill, off)
    assert rc == N.OK and n_out == len(want), ("device", rc, n_out, len(want))
    same(got, want, "device")
    assert (dst["n_records"], dst["n_spans"], dst["units_out"]) == (len(recs), n_spans, len(want)), dst
    return want, st


def match(orc, hay):
    hay = utf16(hay)
    return orc.match(hay, cap=max(1024, hay.size * 8))


# ---- 1. fixtures ------------------------------------------------------------------------------------------------------------
FIXTURES = [("literal", N.MODE_LONGEST), ("literal", N.MODE_WHOLEWORD), ("literal", N.MODE_ALL), ("overlap2", N.MODE_LONGEST),
            ("overlap2", N.MODE_ALL), ("wwl4", N.MODE_WWLONGEST), ("shortest2", N.MODE_SHORTEST), ("readmeWholeWord", N.MODE_WHOLEWORD)]


@pytest.mark.parametrize("body,open,close", USES)
@pytest.mark.parametrize("name,mode", FIXTURES)
def test_fixtures(fixtures, name, mode, body, open, close):
    fx = [f for f in fixtures if f["name"] == name][0]
    hay, kws = fixture_inputs(fx)
    kws = fx.get({N.MODE_SHORTEST: "S_keywords", N.MODE_WWLONGEST: "WWL_keywords"}.get(mode, "keywords"), kws)
    a, orc = pair(mode, kws)
    check_both(a, hay, match(orc, hay), open, close, body)


# ---- 2. edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", ["keep", "fill", "drop"])
@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_LONGEST])
def test_edges(mode, body):
    a, orc = pair(mode, ["ab", "abc", "c"])
    base = "abzcabczzab"
    for n in (0, 1, 2, 7, 8, 9, len(base)):  # (length 2: the text is one span; 7: a span ends at n; all: one at unit 0 and one at the last)
        check_both(a, base[:n], match(orc, base[:n]), "<", ">", body)
    hay = "zzzz zzzz zzzz zzzz z"  # no match: the output is the input
    want, st = check_both(a, hay, match(orc, hay), "<", ">", body)
    assert st.n_spans == 0 and (want == utf16(hay)).all()
    for open, close in (("", ""), ("<<", ""), ("", ">>")):
        check_both(a, base, match(orc, base), open, close, body)
    want, _ = check_both(a, "abc", match(orc, "abc"), "[", "]", body)  # the text is one span
    assert want.tobytes().decode("utf-16-le") == {"keep": "[abc]", "fill": "[***]", "drop": "[]"}[body]


def test_everything_empty_with_drop_is_deletion():
    a, orc = pair(N.MODE_ALL, ["ab", "b", "bcd"])
    hay = "ab.bcd..b.abab..bcdb.b..ab.b.bcd" * 5
    want, _ = check_both(a, hay, match(orc, hay), "", "", "drop")
    assert set(want.tobytes().decode("utf-16-le")) == {"."}
    want, _ = check_both(a, "abbcd", match(orc, "abbcd"), "", "", "drop")  # ... of the whole text
    assert len(want) == 0


# ---- 3. the emit's tiles ----------------------------------------------------------------------------------------------------
def text_with_output_of(orc, target, open, close, body):
    """a text over "ab.", ".c.." whose result has exactly `target` units: a periodic head, then uncovered units one by one"""
    head = ("ab..c.abab." * (target // 8))[:max(target - 400, 0)]
    while True:
        n = len(cover_ref(utf16(head), match(orc, head)[:, :2], utf16(open), utf16(close), body))
        if n <= target:
            return head + "." * (target - n)
        head = head[:-50]


@pytest.mark.parametrize("body,open,close", USES)
@pytest.mark.parametrize("target", [T - 1, T, T + 1, 3 * T - 1, 3 * T, 3 * T + 1])
def test_output_ends_around_a_tile_boundary(target, body, open, close):
    a, orc = pair(N.MODE_ALL, ["ab", "b", "c"])
    hay = text_with_output_of(orc, target, open, close, body)
    want, _ = check_both(a, hay, match(orc, hay), open, close, body)
    assert len(want) == target


@pytest.mark.parametrize("body", ["keep", "fill", "drop"])
def test_whole_tiles_inside_one_open_and_one_close(body):
    a, orc = pair(N.MODE_LONGEST, ["ab", "c"])
    open = "".join(chr(0x100 + i % 997) for i in range(5000))  # (no period of 8 units: a misplaced vector shows)
    close = "".join(chr(0x2000 + i % 991) for i in range(4500))
    hay = ".ab...c" + "." * 37 + "ab"
    want, _ = check_both(a, hay, match(orc, hay), open, close, body)
    assert len(want) > 3 * 9500 > 13 * T


@pytest.mark.parametrize("body", ["keep", "fill"])
def test_a_body_that_crosses_three_tiles(body):
    a, orc = pair(N.MODE_ALL, ["ab", "ba", "zz"])
    run = "ab" * 2600  # one span of 5200 units under {ab, ba}
    hay = "..zz." + run + ".x.zz"
    recs = match(orc, hay)
    assert [5, 5 + len(run)] in merge(recs[:, :2], len(hay)).tolist() and len(run) > 2 * T + 1000
    check_both(a, hay, recs, "<i>", "</i>", body, fill="#")
    check_both(a, hay, recs, "", "", body, fill="#", off=3)


# ---- 4. the densest segments ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_cap", [None, 0])
@pytest.mark.parametrize("open", ["", "|"])
def test_one_unit_spans_alternating_with_one_uncovered_unit(open, lds_cap):
    a, orc = pair(N.MODE_ALL, ["a"])
    hay = "a." * (3 * T + 5) + "a"
    recs = match(orc, hay)
    # a segment -- open and the uncovered unit behind the span -- has 1 + len(open) units of output: a tile holds T of them, more
    # than LDS stages, or T / 2, which fit
    per_tile = T // (1 + len(open))
    assert (per_tile > N.COVER_LDS_SEGMENTS) == (open == "") and T // 2 <= N.COVER_LDS_SEGMENTS
    if lds_cap is not None:  # ... and with nothing staged the global-memory view serves every tile
        assert N.set_tunable("cover_lds_segments", lds_cap) == N.COVER_LDS_SEGMENTS
    want, st = check_both(a, hay, recs, open, "", "drop")
    assert st.n_spans == 3 * T + 6 and len(want) == (3 * T + 5) * (1 + len(open)) + len(open) >= 3 * T


@pytest.mark.parametrize("body,open,close", USES)
def test_the_global_memory_view_on_an_ordinary_text(body, open, close):
    a, orc = pair(N.MODE_ALL, ["ab", "b", "bcd", "dd"])
    hay = "ab.bcd..b.abab..bcdb.b..ab.b.bcdd.dd...." * 130
    recs = match(orc, hay)
    want, _ = check_both(a, hay, recs, open, close, body)
    N.set_tunable("cover_lds_segments", 0)
    again, _ = check_both(a, hay, recs, open, close, body, off=5)
    assert len(want) > 2 * T and (want == again).all()


# ---- 5. the tiles of the merge and of the plan ------------------------------------------------------------------------------
@pytest.mark.parametrize("body,open,close", [("drop", "#", ""), ("keep", "(", ")")])
@pytest.mark.parametrize("count", [N.SPAN_TILE - 1, N.SPAN_TILE, N.SPAN_TILE + 1])
def test_final_spans_of_one_piece_at_the_span_tile(count, body, open, close):
    a, orc = pair(N.MODE_ALL, ["a", "bb"])
    hay = "a.bb." * (count // 2) + ("a." if count % 2 else "")
    want, st = check_both(a, hay, match(orc, hay), open, close, body)
    assert st.n_spans == count and st.pieces == 1


# ---- 6. pieces and the carry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body,open,close", USES)
@pytest.mark.parametrize("p", PIECES)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_tiny_pieces_every_family(mode, p, body, open, close):
    c = family_case(mode, True)
    a = Automaton(mode, c.kws, True, word_chars=c.wc)
    pieces(p)
    want, st = check_both(a, c.hay, c.recs, open, close, body)
    assert st.pieces >= c.hay.size // p and st.max_carry <= 41 // 2 + 2, (st.pieces, st.max_carry)


@pytest.mark.parametrize("p", [1, 7, 16])
def test_one_span_carried_through_every_piece(p):
    a, orc = pair(N.MODE_ALL, ["aa"])
    hay = "a" * 200
    pieces(p)
    want, st = check_both(a, hay, match(orc, hay), "<", ">", "keep")
    assert want.tobytes().decode("utf-16-le") == "<" + hay + ">" and st.n_spans == 1 and st.max_carry == 1 and st.pieces >= 200 // p
    hay = ".." + "a" * 200 + ".a.aa"
    check_both(a, hay, match(orc, hay), "<", ">", "keep")
    check_both(a, hay, match(orc, hay), "<", ">", "drop")


@pytest.mark.parametrize("body", ["drop", "keep"])
def test_pieces_that_merge_intervals_and_finalise_none(body):
    """Every piece but the last carries its one span: it merges m > 0 intervals and finalises none.  A DROP call that is no batch
    then runs the plan with grids sized by m while the count it reads from the merge's head is 0 (k_cover_sums, k_cover_plan:
    `first + k < n` false for every item; k_cover_plan_offsets: dropped = 0), and emits a piece without output."""
    a, orc = pair(N.MODE_ALL, ["aa"])
    hay = "a" * 600 + "b"
    try:
        N.set_tunable("cursor_first_piece", 64)
        N.set_tunable("cursor_max_piece", 64)
        want, st = check_both(a, hay, match(orc, hay), "[", "]", body)
    finally:
        for k, v in DEFAULTS:
            N.set_tunable(k, v)
    assert want.tobytes().decode("utf-16-le") == {"drop": "[]b", "keep": "[" + "a" * 600 + "]b"}[body]
    assert st.pieces > 1 and st.n_spans == 1 and st.max_carry == 1, (st.pieces, st.n_spans, st.max_carry)


# ---- 7. alignment -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body,open,close", USES)
def test_device_output_at_every_unit_offset_of_a_vector(body, open, close):
    a, orc = pair(N.MODE_ALL, ["ab", "b", "c"])
    hay = "ab..c.abab.x" * 400
    recs = match(orc, hay)
    for off in range(8):  # byte offsets 0, 2 .. 14 of a 16-byte vector, the odd unit offsets among them
        check_both(a, hay, recs, open, close, body, off=off)


def test_device_output_at_an_odd_byte_address_is_refused():
    import torch
    a, _ = pair(N.MODE_ALL, ["ab"])
    d_hay = torch.zeros(64, dtype=torch.int16, device="cuda")
    d_out = torch.full((128,), SENTINEL, dtype=torch.int16, device="cuda")
    for byte in range(1, 16, 2):
        n_out, rc, _ = C.cover_device(a, d_hay.data_ptr(), 64, d_out.data_ptr() + byte, 100)
        assert rc == N.E_INVALID
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy().view(np.uint16) == SENTINEL).all()


# ---- 8. capacity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body,open,close", USES)
@pytest.mark.parametrize("p", [None, 16])
def test_capacity(p, body, open, close):
    a, orc = pair(N.MODE_ALL, ["ab", "b", "bcd"])
    hay = utf16("ab.bcd..b.abab..bcdb.b..ab.b.bcd" * 3)
    want = cover_ref(hay, match(orc, hay)[:, :2], utf16(open), utf16(close), body, ord("*"))
    n = len(want)
    pieces(p)
    for cap in (0, 1, n // 2, n - 1):
        for entry in (host_raw, device_raw):
            got, rc, n_out, st = entry(a, hay, cap, open, close, body)
            assert rc == N.E_OVERFLOW and n_out == n, (entry.__name__, cap, rc, n_out)
            same(got, want[:cap], entry.__name__)
    for entry in (host_raw, device_raw):
        got, rc, n_out, st = entry(a, hay, n, open, close, body)
        assert rc == N.OK and n_out == n
        same(got, want, entry.__name__)


# ---- 9. FILL ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_fill_preserves_the_length_and_changes_the_spans_only(mode):
    c = family_case(mode, True)
    a = Automaton(mode, c.kws, True, word_chars=c.wc)
    assert 0x2588 not in c.hay
    got, rc, n_out, st = host_raw(a, c.hay, c.hay.size, body="fill", fill="█")
    assert rc == N.OK and n_out == c.hay.size
    covered = np.zeros(c.hay.size, bool)
    for s, e in merge(c.recs[:, :2], c.hay.size).tolist():
        covered[s:e] = True
    assert ((got != c.hay) == covered).all() and (got[covered] == 0x2588).all()
    pair_text = "x😀y"  # a surrogate pair becomes two
    a2, orc2 = pair(N.MODE_ALL, ["😀"])
    assert C.mask(a2, pair_text) == "x**y"


# ---- 10. the Python functions -----------------------------------------------------------------------------------------------
def test_python_functions_agree_with_cover_and_redact_with_replace():
    s = LongestMatchSet(["ab", "abc", "dd"], True)
    text = "xab.abc..dd.ab." * 50  # (no two matches touch)
    recs = s.find_all(text)
    assert (recs[1:, 0] > recs[:-1, 1]).all()
    assert C.mask(s, text, fill="#") == C.cover(s, text, body="fill", fill="#") == text.replace("abc", "###").replace("ab", "##").replace("dd", "##")
    assert C.highlight(s, text, "<b>", "</b>") == C.cover(s, text, open="<b>", close="</b>")
    assert C.redact(s, text, "[r]") == C.cover(s, text, open="[r]", body="drop") == s.replace(text, "[r]")
    st = N.CoverStats()
    out = C.cover(s.automaton, utf16(text), open="<", close=">", stats=st)
    assert out == C.highlight(s, text, "<", ">") and st.n_spans == len(recs) and st.units_out == len(text) + 2 * len(recs)
    touching = LongestMatchSet(["ab"], True)
    assert C.redact(touching, "zababz", "R") == "zRz" and touching.replace("zababz", "R") == "zRRz"
