"""GPU tests of acgpu_cover_utf8 / acgpu_cover_utf8_lossy (include/acgpu.h; csrc/acgpu_cover.hip: k_cover_emit<uint8_t>): a UTF-8 text
rewritten in bytes.  Every expected value is tests/cover_ref.py's splice over the byte records that the tests of find_all_utf8
expect (tests/test_gpu_utf8.py, tests/test_gpu_utf8_lossy.py: the CPU oracle on the decoded text, mapped to bytes)."""
import ctypes
import importlib

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickSet, Automaton, LongestMatchSet, Utf8Error
from tests.cover_ref import cover_ref
from tests.helpers import fixture_inputs
from tests.spans_ref import merge
from tests.test_gpu_cover import FIXTURES, MODES, USES
from tests.test_gpu_tiny_pieces import PIECES, family_case
from tests.test_gpu_utf8 import expected, keywords_from, mixed_text, pair
from tests.test_gpu_utf8_lossy import every_unit
from tests.test_gpu_utf8_lossy import expected as expected_lossy

C = importlib.import_module("ahocorasick_amd.cover")  # (the package's name `cover` is the function)

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20),
            ("replace_slab_units", 1 << 25), ("cover_lds_segments", N.COVER_LDS_SEGMENTS)]
TB = N.COVER_TILE_BYTES  # the output bytes one workgroup of k_cover_emit<uint8_t> writes
SENTINEL = 0x5A
USES8 = [(body, open.encode(), close.encode()) for body, open, close in USES]
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
u8 = lambda b: np.frombuffer(bytes(b), np.uint8)


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def pieces(p):
    if p:
        N.set_tunable("cursor_first_piece", p)
        N.set_tunable("cursor_max_piece", p)


def host_raw(a, data, cap, open=b"", close=b"", body="keep", fill=b"*", errors="strict"):
    """acgpu_cover_utf8[_lossy] into a buffer with a sentinel behind cap -> (the bytes written, rc, n_out, stats)"""
    data = u8(data)
    spec, keep = C._spec(u8(open), u8(close), C.BODIES[body], fill[0])
    out = np.full(cap + 64, SENTINEL, np.uint8)
    n_out, st = ctypes.c_uint64(0), N.CoverStats()
    name = "acgpu_cover_utf8" + ("_lossy" if errors == "replace" else "")
    rc = getattr(N.lib(), name)(a.handle, vp(data if data.size else np.zeros(1, np.uint8)), int(data.size), ctypes.byref(spec), vp(out), cap,
                                ctypes.byref(n_out), ctypes.byref(st), None)
    assert (out[cap:] == SENTINEL).all(), "written at or beyond cap"
    return out[:min(cap, n_out.value)], rc, int(n_out.value), st


def check(a, data, recs_b, open=b"", close=b"", body="keep", fill=b"*", errors="strict"):
    """the entry with exactly the capacity the result needs, and the Python function with its guess, against the reference"""
    want = cover_ref(u8(data), recs_b[:, :2], u8(open), u8(close), body, fill[0])
    got, rc, n_out, st = host_raw(a, data, len(want), open, close, body, fill, errors)
    assert rc == N.OK and n_out == len(want), (rc, n_out, len(want))
    bad = np.flatnonzero(got != want)
    assert not len(bad), (bad[:5], got[bad[:5]], want[bad[:5]])
    assert (st.n_records, st.n_spans, st.units_out) == (len(recs_b), len(merge(recs_b[:, :2], len(data))), len(want))
    assert C.cover_utf8(a, data, open=open, close=close, body=body, fill=fill, errors=errors) == want.tobytes()
    return want, st


# ---- 1. fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body,open,close", USES8)
@pytest.mark.parametrize("name,mode", FIXTURES)
def test_fixtures(fixtures, name, mode, body, open, close):
    fx = [f for f in fixtures if f["name"] == name][0]
    hay, kws = fixture_inputs(fx)
    kws = fx.get({N.MODE_SHORTEST: "S_keywords", N.MODE_WWLONGEST: "WWL_keywords"}.get(mode, "keywords"), kws)
    data = hay.tobytes().decode("utf-16-le").encode()
    a, orc = pair(mode, kws)
    check(a, data, expected(orc, data)[1], open, close, body)


# ---- 2. sequences of 1 to 4 bytes inside, at the edges of and between spans, every family, in pieces ---------------------------
@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(77)
    text = mixed_text(rng, 1500)
    data = text.encode()
    assert 2000 < len(data) < 6000 and {len(ch.encode()) for ch in text} == {1, 2, 3, 4}
    cases = {}
    for mode in sorted(MODES):
        kws = keywords_from(np.random.default_rng(78 + mode), text, mode, True)
        a, orc = pair(mode, kws)
        recs_b = expected(orc, data)[1]
        sp = merge(recs_b[:, :2], len(data))
        inside = {len(ch.encode()) for s, e in sp.tolist() for ch in data[s:e].decode()}
        before = {len(data[:s].decode()[-1:].encode()) for s, e in sp.tolist()}
        assert len(sp) >= 10 and inside >= {1, 2, 3} and before >= {1, 2, 3}, (mode, len(sp), inside, before)
        cases[mode] = (a, recs_b)
    return data, cases


@pytest.mark.parametrize("body,open,close", [("keep", "«".encode(), "»".encode()), ("fill", b"", b""), ("drop", "[…]".encode(), b"")])
@pytest.mark.parametrize("p", [None, 3, 16])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_strict_mixed_text(mixed, mode, p, body, open, close):
    data, cases = mixed
    a, recs_b = cases[mode]
    pieces(p)
    want, st = check(a, data, recs_b, open, close, body)
    want.tobytes().decode()  # the result is well-formed
    if p:
        assert st.pieces >= len(data.decode()) // p
    if body == "fill":
        assert len(want) == len(data)


def test_four_byte_sequences_inside_and_around_spans():
    a, orc = pair(N.MODE_ALL, ["😀", "b😀", "ab", "𝒜b"])
    data = ("a😀b😀😀 ab😀.𝒜b é€ " * 60).encode()
    recs_b = expected(orc, data)[1]
    for body, open, close in USES8:
        check(a, data, recs_b, open, close, body)


@pytest.mark.parametrize("p", PIECES)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_tiny_pieces_every_family(mode, p):
    c = family_case(mode, True)  # (an ASCII text: a unit is a byte)
    a = Automaton(mode, c.kws, True, word_chars=c.wc)
    data = c.hay.astype(np.uint8).tobytes()
    pieces(p)
    for body, open, close in USES8:
        want, st = check(a, data, c.recs, open, close, body)
        assert st.pieces >= c.hay.size // p


# ---- 3. the emit's tiles and the densest segments -----------------------------------------------------------------------------
@pytest.mark.parametrize("body,open,close", USES8)
@pytest.mark.parametrize("target", [TB - 1, TB, TB + 1])
def test_output_ends_around_a_tile_boundary(target, body, open, close):
    a, orc = pair(N.MODE_ALL, ["ab", "b", "é"])
    head = ("ab..é.abab." * (target // 8))[:target - 600]  # a periodic head, then uncovered bytes one by one up to the target
    while True:
        n = len(cover_ref(u8(head.encode()), expected(orc, head.encode())[1][:, :2], u8(open), u8(close), body))
        if n <= target:
            break
        head = head[:-50]
    data = (head + "." * (target - n)).encode()
    want, _ = check(a, data, expected(orc, data)[1], open, close, body)
    assert len(want) == target


@pytest.mark.parametrize("body", ["keep", "fill", "drop"])
def test_whole_tiles_inside_one_open_and_a_body_over_three_tiles(body):
    a, orc = pair(N.MODE_ALL, ["ab", "ba", "é"])
    open = bytes(33 + i % 89 for i in range(5000))  # (no period of 16 bytes: a misplaced vector shows)
    close = bytes(40 + i % 83 for i in range(4700))
    run = "ab" * 4400  # one span of 8800 bytes
    data = (".é.." + run + ".x.é").encode()
    recs_b = expected(orc, data)[1]
    assert [5, 5 + len(run)] in merge(recs_b[:, :2], len(data)).tolist() and len(run) > 2 * TB
    check(a, data, recs_b, open, close, body, fill=b"#")


@pytest.mark.parametrize("open", [b"", b"|"])
def test_one_byte_spans_alternating_with_one_uncovered_byte(open):
    a, orc = pair(N.MODE_ALL, ["a"])
    data = b"a." * (3 * TB + 5) + b"a"
    # a segment has 1 + len(open) bytes of output, a tile holds TB or TB / 2 of them: either way more than LDS stages, so the
    # global-memory view of the segments serves every full tile
    assert TB // (1 + len(open)) > N.COVER_LDS_SEGMENTS
    recs_b = expected(orc, data)[1]
    want, st = check(a, data, recs_b, open, b"", "drop")
    assert st.n_spans == 3 * TB + 6 and len(want) >= 3 * TB
    N.set_tunable("cover_lds_segments", 0)  # ... and with nothing staged at all it serves the rest too
    check(a, data, recs_b, open, b"", "drop")


# ---- 4. capacity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body,open,close", USES8)
@pytest.mark.parametrize("p", [None, 16])
def test_capacity(p, body, open, close):
    a, orc = pair(N.MODE_ALL, ["ab", "b", "bcé"])
    data = ("ab.bcé..b.abab..bcéb.b..ab.b.bcé€" * 3).encode()
    want = cover_ref(u8(data), expected(orc, data)[1][:, :2], u8(open), u8(close), body, ord("*"))
    n = len(want)
    pieces(p)
    for cap in (0, 1, n // 2, n - 1):
        got, rc, n_out, st = host_raw(a, data, cap, open, close, body)
        assert rc == N.E_OVERFLOW and n_out == n == st.units_out, (cap, rc, n_out)
        assert (got == want[:cap]).all()
    got, rc, n_out, st = host_raw(a, data, n, open, close, body)
    assert rc == N.OK and n_out == n and (got == want).all()


# ---- 5. an unpaired surrogate, ill-formed input, lossy ------------------------------------------------------------------------
@pytest.mark.parametrize("p", [None, 3, 16])
def test_a_lone_surrogate_keyword_on_supplementary_characters(p):
    s = AhoCorasickSet(["\ud83d", "\ude00", "ab", "b😀"], True)
    data = ("a😀b😀😀 ab😀.𝒜b " * 120).encode()
    recs_b = s.find_all_utf8(data)  # (the widened records, which the spans entries merge)
    assert len(recs_b) > 500
    pieces(p)
    for body, open, close in USES8:
        check(s.automaton, data, recs_b, open, close, body)


def test_ill_formed_text_raises_where_find_all_utf8_does(mixed):
    data, cases = mixed
    a, recs_b = cases[N.MODE_ALL]
    for bad in (data[:1000] + b"\xff" + data[1000:], data + b"\xe2\x82", b"\x80" + data):
        with pytest.raises(Utf8Error) as want:
            a.match_utf8(bad, with_ids=False)
        with pytest.raises(Utf8Error) as got:
            C.cover_utf8(a, bad, open=b"<", close=b">")
        assert (got.value.start, got.value.haystack) == (want.value.start, want.value.haystack)
    check(a, data, recs_b, b"<", b">")  # the pool is as usable as before


@pytest.mark.parametrize("p", [None, 3])
def test_lossy_stray_bytes_and_a_replacement_keyword(p):
    text = "aé€😀kw".encode()
    data = (b"\x80" + text + b"\xbf\xbf" + text * 3 + b"\xc3(" + b"\xe2\x82" + b"x" + b"\xf0\x9f\x98" + text) * 40 + b"ab" + b"\xf0\x9f\x98"
    a, orc = pair(N.MODE_ALL, ["k\ufffdw", "k", "\ufffd\ufffd", "é😀"])  # U+FFFD in a keyword matches a replaced subpart
    recs_b = expected_lossy(orc, data)[0]
    sp = merge(recs_b[:, :2], len(data))
    stray = np.flatnonzero(u8(data) == 0x80)  # (the stray byte in front of every block, and the last byte of every U+1F600)
    covered = np.zeros(len(data), bool)
    for s, e in sp.tolist():
        covered[s:e] = True
    assert len(sp) >= 10 and b"\xbf\xbf" in {data[s:e] for s, e in sp.tolist()} and not covered[stray].any()
    pieces(p)
    for body, open, close in USES8:
        want, _ = check(a, data, recs_b, open, close, body, errors="replace")
    masked = C.mask_utf8(a, data, fill=b"#", errors="replace")
    got = u8(masked)
    assert len(masked) == len(data) and ((got != u8(data)) == covered).all() and (got[covered] == ord("#")).all()  # stray bytes inside a span are filled, outside copied
    with pytest.raises(Utf8Error):
        C.cover_utf8(a, data)


def test_lossy_every_unit_of_a_text_with_stray_bytes():
    data = (b"\x80" + "aé€😀kw".encode() + b"\xbf\xbf" + b"\xc3(" + b"\xe2\x82" + b"x" + b"\xf0\x9f\x98") * 20
    a, orc = every_unit([data])
    recs_b = expected_lossy(orc, data)[0]
    want, st = check(a, data, recs_b, b"<", b">", "keep", errors="replace")
    assert st.n_spans == 1 and want.tobytes() == b"<" + data + b">"  # every byte is covered: one span, the text as it is inside


# ---- 6. the Python functions ------------------------------------------------------------------------------------------------
def test_python_functions_agree_with_cover_utf8_and_redact_with_replace():
    s = LongestMatchSet(["ab", "abé", "dd"], True)
    data = ("xab.abé..dd.ab.€" * 50).encode()  # (no two matches touch)
    recs = s.find_all_utf8(data)
    assert (recs[1:, 0] > recs[:-1, 1]).all()
    assert C.mask_utf8(s, data, fill=b"#") == C.cover_utf8(s, data, body="fill", fill=b"#")
    assert C.mask_utf8(s, data, fill="#").decode() == data.decode().replace("abé", "####").replace("ab", "##").replace("dd", "##")
    assert C.highlight_utf8(s, data, "«", b"</b>") == C.cover_utf8(s, data, open="«".encode(), close=b"</b>")
    assert C.redact_utf8(s, data, "[r]") == C.cover_utf8(s, data, open=b"[r]", body="drop") == s.replace_utf8(data, "[r]")
    assert C.redact_utf8(s, data, b"", errors="replace") == data.decode().replace("abé", "").replace("ab", "").replace("dd", "").encode()
