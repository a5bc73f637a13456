"""GPU tests of stream cover (include/acgpu.h: acgpu_stream_cover_u16 / _utf8 / _utf8_lossy; csrc/acgpu_stream.hip, cover_feed in
csrc/acgpu_cover.hip with the HEADLESS and TAILLESS items of k_cover_emit, the ranged piece loop of csrc/acgpu_spans.hip).  Every
expected value is tests/cover_ref.cover_ref over the CPU oracle's records of the WHOLE text, whatever the chunking, and the
concatenated feeds must also equal the whole-text cover / cover_utf8 call; the span counts are tests/spans_ref.merge's."""
import ctypes
import importlib

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd import synth
from ahocorasick_amd.strings import Automaton, Utf8Error, utf16
from tests.cover_ref import cover_ref
from tests.spans_ref import merge
from tests.test_gpu_utf8 import MODES, expected, pair
from tests.test_gpu_utf8_lossy import expected as expected_lossy

C = importlib.import_module("ahocorasick_amd.cover")  # (the package's name `cover` is the function)

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20),
            ("replace_slab_units", 1 << 25), ("cover_lds_segments", N.COVER_LDS_SEGMENTS)]
BODIES = ("keep", "fill", "drop")
SENTINEL = 0x5A
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
u8 = lambda b: np.frombuffer(bytes(b), np.uint8)


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def split(hay, cuts):
    edges = [0] + [int(c) for c in cuts] + [len(hay)]
    return [hay[edges[i]:edges[i + 1]] for i in range(len(edges) - 1)]


def chunkings(n, rng, k_random=12):
    """one cut at every position, chunks of 1, 2, 3 and 7, and k_random seeded random chunkings -> lists of cuts"""
    out = [[c] for c in range(n + 1)] + [list(range(k, n, k)) for k in (1, 2, 3, 7)]
    for _ in range(k_random):
        out.append(sorted(rng.choice(n + 1, size=int(rng.integers(1, 6)), replace=True).tolist()))
    return out


def feed_units(a, chunks, open, close, body, fill="*", final_in_last=False):
    """the chunks through one CoverStream -> (the whole output, [(n_out, n_spans) per feed])"""
    st, parts, log = N.CoverStats(), [], []
    feeds = [(c, final_in_last and i == len(chunks) - 1) for i, c in enumerate(chunks)]
    if not final_in_last:
        feeds.append((np.zeros(0, np.uint16), True))
    with C.CoverStream(a, open, close, body, fill) as s:
        for c, final in feeds:
            parts.append(s.feed(c, final=final, stats=st))
            assert st.units_out == parts[-1].size
            log.append((parts[-1].size, int(st.n_spans)))
    return np.concatenate(parts), log


def feed_bytes(a, chunks, open, close, body, fill=b"*", errors="strict"):
    cst, parts, log = N.CoverStats(), [], []
    with C.CoverStream(a, open, close, body, fill) as s:
        for c, final in [(c, False) for c in chunks] + [(b"", True)]:
            parts.append(s.feed_utf8(c, final=final, errors=errors, cover_stats=cst))
            assert cst.units_out == len(parts[-1])
            log.append((len(parts[-1]), int(cst.n_spans)))
    return b"".join(parts), log


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape, got[:40], want[:40])
    bad = np.flatnonzero(got != want)
    assert not len(bad), (what, bad[:5], got[bad[:5]], want[bad[:5]])


# ---- 1. every cut ------------------------------------------------------------------------------------------------------------
KWS = ["ab", "bc", "abcd", "d", "xx"]
TEXT = "abcd abbc d xx bcd.ab xx"  # overlapping, nested and touching matches, whole words among them; 24 units


@pytest.mark.parametrize("body", BODIES)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_cut_every_family_every_body(mode, body):
    a, orc = pair(mode, KWS)
    hay = utf16(TEXT)
    assert hay.size <= 24
    recs = orc.match(hay, cap=1024)
    want = cover_ref(hay, recs[:, :2], utf16("<<"), utf16(">"), body, ord("*"))
    n_spans = len(merge(recs[:, :2], hay.size))
    assert n_spans >= 2
    same(utf16(C.cover(a, hay, "<<", ">", body)), want, "the whole-text call")
    rng = np.random.default_rng(2600 + mode)
    for cuts in chunkings(hay.size, rng):
        got, log = feed_units(a, split(hay, cuts), "<<", ">", body)
        same(got, want, (mode, body, cuts))
        assert sum(n for _, n in log) == n_spans, (cuts, log)


# ---- 2. a span through many feeds --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", BODIES)
@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_SHORTEST])
def test_one_span_through_many_feeds_is_delivered_as_it_arrives(mode, body):
    a, orc = pair(mode, ["aa"])
    hay = utf16("xyz " + "a" * 200 + " zyx")
    recs = orc.match(hay, cap=1024)
    want = cover_ref(hay, recs[:, :2], utf16("["), utf16("]"), body, ord("*"))
    assert len(merge(recs[:, :2], hay.size)) == 1
    chunks = [hay[i:i + 16] for i in range(0, hay.size, 16)]
    got, log = feed_units(a, chunks, "[", "]", body)
    same(got, want, (mode, body))
    assert (got == ord("[")).sum() == 1 and (got == ord("]")).sum() == 1
    assert [n for _, n in log].count(1) == 1 and sum(n for _, n in log) == 1
    # The bound: a feed that is not final withholds at most max_keyword_len + 1 units of text, however long the span is, so the
    # rewrite of all that was fed but 3 units has been delivered behind every feed -- the open by the FIRST feed, where a design
    # that withholds an open span delivers "xyz " and then nothing until the span ends.
    assert len(chunks) == 13 and log[0][1] == 1
    delivered = 0
    for i, (n_out, _) in enumerate(log[:len(chunks)]):
        delivered += n_out
        settled = 16 * (i + 1) - 3                                   # text positions that must be out by now, at least
        # (the whole text's records clipped there: under Shortest the record that covers position settled - 1 ends behind it)
        clipped = np.minimum(recs[recs[:, 0] < settled][:, :2], settled)
        floor = len(cover_ref(hay[:settled], clipped, utf16("["), utf16(""), body, ord("*")))
        assert delivered >= floor, (i, delivered, floor, log)
        if body != "drop" and i >= 1:  # ... which for a body that has elements is 16 - (max_keyword_len + 1) per feed
            assert n_out >= 16 - (2 + 1), (i, log)


# ---- 3. seams ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", BODIES)
@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_LONGEST])
def test_seams(mode, body):
    a, orc = pair(mode, ["ab", "cd"])

    def run(text, cuts):
        hay = utf16(text)
        recs = orc.match(hay, cap=64)
        want = cover_ref(hay, recs[:, :2], utf16("<"), utf16(">"), body, ord("*"))
        got, log = feed_units(a, split(hay, cuts), "<", ">", body)
        same(got, want, (text, cuts))
        return got, log, len(merge(recs[:, :2], hay.size))
    # two matches that touch exactly at a feed boundary: one span, one open
    got, log, n = run("..abcd..", [4])
    assert n == 1 and (got == ord("<")).sum() == 1 and sum(k for _, k in log) == 1
    # a span that ends at a feed's end and is not continued: its close is delivered later, before anything else
    got, log, n = run("..ab..", [4])
    assert n == 1
    # ... with single-unit keywords B is the owned end: the span "ab" ends exactly at done_after, and is cut there all the same
    a1, orc1 = pair(N.MODE_ALL, ["a", "b"])
    inner = {"keep": "ab", "fill": "**", "drop": ""}[body]
    with C.CoverStream(a1, "<", ">", body) as s:
        st = N.CoverStats()
        assert C._to_str(s.feed("..ab", stats=st)) == "..<" + inner and st.n_spans == 1
        assert C._to_str(s.feed("..", stats=st)) == ">.." and st.n_spans == 0  # not continued: close first
        assert s.feed("", final=True).size == 0
    with C.CoverStream(a1, "<", ">", body) as s:
        assert C._to_str(s.feed("..ab")) == "..<" + inner
        assert C._to_str(s.feed("a.", stats=st)) == {"keep": "a", "fill": "*", "drop": ""}[body] + ">." and st.n_spans == 0  # continued: no second open
        assert s.feed("", final=True).size == 0
    # a final empty feed that only delivers close: the text ends with the span
    with C.CoverStream(a1, "<", ">", body) as s:
        assert C._to_str(s.feed("..ab")) == "..<" + inner
        assert s.feed("").size == 0
        assert C._to_str(s.feed("", final=True, stats=st)) == ">" and (st.n_spans, st.units_out) == (0, 1)
    hay = utf16("..ab")
    with C.CoverStream(a, "<", ">", body) as s:
        parts = [s.feed(hay), s.feed(np.zeros(0, np.uint16)), s.feed(np.zeros(0, np.uint16), final=True)]
    want = cover_ref(hay, orc.match(hay, cap=64)[:, :2], utf16("<"), utf16(">"), body, ord("*"))
    same(np.concatenate(parts), want, "the text ends with the span")
    assert parts[1].size == 0 and parts[2][-1] == ord(">")
    # a feed shorter than the halo delivers nothing
    a2, orc2 = pair(mode, ["abcdefgh"])
    with C.CoverStream(a2, "<", ">", body) as s:
        assert s.feed("ab").size == 0
        tail = s.feed("cdefgh..", final=True)
    same(tail, cover_ref(utf16("abcdefgh.."), np.array([[0, 8]]), utf16("<"), utf16(">"), body, ord("*")), "short feed")


# ---- 4. pieces and windows inside a feed ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds", [N.COVER_LDS_SEGMENTS, 1])
@pytest.mark.parametrize("body", BODIES)
@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_LONGEST, N.MODE_WHOLEWORD])
def test_small_pieces_small_slabs_and_segments_from_global_memory(mode, body, lds):
    a, orc = pair(mode, ["aa", "ab", "bc"])
    rng = np.random.default_rng(2640 + mode)
    words = ["aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa", "ab", "bc", "xy", " ", "aa", "q"]
    hay = utf16(" ".join(words[int(i)] for i in rng.integers(0, len(words), 160)))
    recs = orc.match(hay, cap=4 * hay.size)
    want = cover_ref(hay, recs[:, :2], utf16("<<<"), utf16(">>"), body, ord("*"))
    for k, v in (("cursor_first_piece", 16), ("cursor_max_piece", 16), ("replace_slab_units", 8), ("cover_lds_segments", lds)):
        N.set_tunable(k, v)
    for size in (97, 100, 103):
        chunks = [hay[i:i + size] for i in range(0, hay.size, size)]
        st = N.CoverStats()
        got, log = feed_units(a, chunks, "<<<", ">>", body)
        same(got, want, (mode, body, size))
        assert sum(n for _, n in log) == len(merge(recs[:, :2], hay.size))


# ---- 5. bytes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", BODIES)
@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_LONGEST])
def test_bytes_cut_inside_sequences_inside_spans(mode, body):
    a, orc = pair(mode, ["é€", "€😀", "a😀b", "😀", "zz"])
    data = "xé€😀a😀b.zzé€ 😀😀 é€".encode()
    recs_u, recs_b = expected(orc, data)
    want = cover_ref(u8(data), recs_b[:, :2], u8(b"<"), u8(b">"), body, ord("#"))
    assert C.cover_utf8(a, data, b"<", b">", body, b"#") == want.tobytes()
    n_spans = len(merge(recs_b[:, :2], len(data)))
    for cut in range(len(data) + 1):  # (inside 2-, 3- and 4-byte sequences, at a span's first byte and behind its last)
        got, log = feed_bytes(a, [data[:cut], data[cut:]], b"<", b">", body, b"#")
        assert got == want.tobytes(), (cut, got, want.tobytes())
        assert sum(n for _, n in log) == n_spans
    for k in (1, 2, 3, 5):
        got, log = feed_bytes(a, [data[i:i + k] for i in range(0, len(data), k)], b"<", b">", body, b"#")
        assert got == want.tobytes(), (k, got, want.tobytes())
    if body == "fill":  # FILL keeps every byte offset
        assert len(want) == len(data) + n_spans * 2


def test_bytes_a_covered_supplementary_character_and_a_lone_surrogate_keyword():
    # B = owned end + 1 - max_keyword_len falls between the two units of a covered U+1F600 for some cut
    a = Automaton(N.MODE_ALL, ["😀😀", "\ud83d", "ab"], True)
    data = "ab😀😀😀😀ab 😀 x".encode()
    recs_b = a.match_utf8(data, with_ids=False)  # (the widened records of the lone surrogate, which the spans entries merge)
    for body in BODIES:
        want = cover_ref(u8(data), recs_b[:, :2], u8(b"<"), u8(b">"), body, ord("#")).tobytes()
        assert C.cover_utf8(a, data, b"<", b">", body, b"#") == want
        for cut in range(len(data) + 1):
            got, _ = feed_bytes(a, [data[:cut], data[cut:]], b"<", b">", body, b"#")
            assert got == want, (body, cut, got, want)
        got, _ = feed_bytes(a, [data[i:i + 3] for i in range(0, len(data), 3)], b"<", b">", body, b"#")
        assert got == want, body


def test_bytes_strict_an_ill_formed_byte_in_the_third_feed():
    a, orc = pair(N.MODE_ALL, ["ab", "bc"])
    chunks = [b"xxabcab", b"cab\xe2\x82", b"\xacab\xffab", b"abab"]
    good = b"".join(chunks)[:b"".join(chunks).index(b"\xff")]
    want = cover_ref(u8(good), expected(orc, good)[1][:, :2], u8(b"<"), u8(b">"), "keep").tobytes()
    ust = N.Utf8StreamStats()
    with C.CoverStream(a, b"<", b">") as s:
        so_far = s.feed_utf8(chunks[0]) + s.feed_utf8(chunks[1])
        with pytest.raises(Utf8Error) as e:
            s.feed_utf8(chunks[2], stats=ust)
        assert e.value.start == len(good) == ust.first_bad
        with pytest.raises(N.AcgpuError):  # the stream is finished
            s.feed_utf8(b"", final=True)
    assert len(so_far) > 0 and want.startswith(so_far)


# ---- 6. lossy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", BODIES)
def test_lossy_stray_bytes_inside_and_outside_spans(body):
    a, orc = pair(N.MODE_ALL, ["k�w", "��", "é😀", "ab"])
    data = b"\x80ab" + "aé😀k".encode() + b"\xf0\x9f\x98w" + b"\xbf\xbf." + b"\xe2\x82" + b"xab\xc3(" + "é😀".encode() + b"k\xffw\xf0\x9f"
    recs_b = expected_lossy(orc, data)[0]
    want = cover_ref(u8(data), recs_b[:, :2], u8(b"<"), u8(b">"), body, ord("#")).tobytes()
    assert C.cover_utf8(a, data, b"<", b">", body, b"#", errors="replace") == want
    rng = np.random.default_rng(2660)
    for cuts in chunkings(len(data), rng):  # (cuts inside ill-formed subparts included)
        got, log = feed_bytes(a, split(data, cuts), b"<", b">", body, b"#", errors="replace")
        assert got == want, (cuts, got, want)
        assert sum(n for _, n in log) == len(merge(recs_b[:, :2], len(data)))
    if body == "fill":  # stray bytes inside a span are filled, outside copied
        plain = feed_bytes(a, [data], b"", b"", "fill", b"#", errors="replace")[0]
        covered = np.zeros(len(data), bool)
        for s, e in merge(recs_b[:, :2], len(data)).tolist():
            covered[s:e] = True
        assert len(plain) == len(data) and ((u8(plain) != u8(data)) == covered).all() and (u8(plain)[covered] == ord("#")).all()
        assert covered[u8(data) >= 0x80].any() and not covered[0]


# ---- 7. overflow -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", BODIES)
def test_overflow_commits_nothing(body):
    a, orc = pair(N.MODE_ALL, ["aa", "bc"])
    hay = utf16("x" + "a" * 30 + ".bc.bc." + "a" * 20)
    recs = orc.match(hay, cap=1024)
    want = cover_ref(hay, recs[:, :2], utf16("<"), utf16(">"), body, ord("*"))
    spec, keep = C._spec(utf16("<"), utf16(">"), C.BODIES[body], ord("*"))
    h = ctypes.c_void_p()
    assert N.lib().acgpu_stream_open(a.handle, ctypes.byref(h)) == N.OK
    parts = []
    try:
        for lo, final in ((0, 0), (20, 0), (40, 1)):
            chunk = np.ascontiguousarray(hay[lo:lo + 20] if not final else hay[lo:])
            n_out, st = ctypes.c_uint64(0), N.CoverStats()
            call = lambda out, cap: N.lib().acgpu_stream_cover_u16(h, vp(chunk), chunk.size, final, ctypes.byref(spec), vp(out), cap,
                                                                   ctypes.byref(n_out), ctypes.byref(st))
            big = np.full(256, SENTINEL, np.uint16)
            assert call(big, 0) == N.E_OVERFLOW  # (every feed here delivers something)
            need = int(n_out.value)
            assert need > 0 and st.units_out == need and (big == SENTINEL).all()
            assert call(big, need - 1) == N.E_OVERFLOW and n_out.value == need and (big[need - 1:] == SENTINEL).all()
            assert call(big, need) == N.OK and n_out.value == need and (big[need:] == SENTINEL).all()
            parts.append(big[:need].copy())
    finally:
        N.lib().acgpu_stream_close(h)
    same(np.concatenate(parts), want, body)


# ---- 8. interleaving -----------------------------------------------------------------------------------------------------------
def test_other_streams_and_whole_text_calls_between_the_feeds():
    a, orc = pair(N.MODE_ALL, ["aa", "bc"])
    hay = utf16("x" + "a" * 40 + ".bc.bc." + "a" * 30 + "..")
    recs = orc.match(hay, cap=1024)[:, :2]
    want = {body: cover_ref(hay, recs, utf16(o), utf16(c), body, ord("*")) for body, o, c in (("keep", "<", ">"), ("fill", "", ""), ("drop", "#", ""))}
    s1, s2, s3 = C.CoverStream(a, "<", ">", "keep"), C.CoverStream(a, "", "", "fill"), C.CoverStream(a, "#", "", "drop")
    got = {"keep": [], "fill": [], "drop": []}
    try:
        for i in range(0, hay.size, 16):
            final = i + 16 >= hay.size
            got["keep"].append(s1.feed(hay[i:i + 16], final=final))
            got["fill"].append(s2.feed(hay[i:i + 16], final=final))
            same(utf16(C.cover(a, hay, "[", "]", "keep")), cover_ref(hay, recs, utf16("["), utf16("]"), "keep"), "whole text in between")
            got["drop"].append(s3.feed(hay[i:i + 16], final=final))
    finally:
        for s in (s1, s2, s3):
            s.close()
    for body in got:
        same(np.concatenate(got[body]), want[body], body)


# ---- 9. one larger text --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [4096, 4099])
def test_the_readme_paragraph_in_units_and_as_mixed_bytes(size):
    kws = synth.readme_dictionary()
    a, orc = pair(N.MODE_ALL, kws, cs=True)
    para = synth.README_PARAGRAPH + " "
    text = (para + "é€😀 ") * (50000 // (len(para) + 4))
    hay = utf16(text)
    assert 40000 <= hay.size <= 60000
    recs = orc.match(hay, cap=4 * hay.size)
    for body, o, c in (("keep", "<b>", "</b>"), ("fill", "", ""), ("drop", "***", "")):
        want = cover_ref(hay, recs[:, :2], utf16(o), utf16(c), body, ord("*"))
        got, log = feed_units(a, [hay[i:i + size] for i in range(0, hay.size, size)], o, c, body)
        same(got, want, (body, size))
        assert sum(n for _, n in log) == len(merge(recs[:, :2], hay.size))
        # (uint16 chunks, which end inside surrogate pairs: no str piece may)
        pieces = list(C.cover_readable(a, [hay[i:i + size] for i in range(0, hay.size, size)], o, c, body))
        assert all(not p or not 0xD800 <= ord(p[-1]) < 0xDC00 for p in pieces) and "".join(pieces) == C.cover(a, hay, o, c, body)
    data = text.encode()
    recs_b = expected(orc, data)[1]
    for body, o, c in (("keep", b"<b>", b"</b>"), ("fill", b"", b""), ("drop", b"***", b"")):
        want = cover_ref(u8(data), recs_b[:, :2], u8(o), u8(c), body, ord("*")).tobytes()
        got, log = feed_bytes(a, [data[i:i + size] for i in range(0, len(data), size)], o, c, body)
        assert got == want, (body, size)
        assert b"".join(C.cover_utf8_readable(a, [data[i:i + size] for i in range(0, len(data), size)], o, c, body)) == want
