"""GPU tests of acgpu_cover_batch_utf8 / acgpu_cover_batch_utf8_lossy (include/acgpu.h; csrc/acgpu_cover.hip: the batch plan over
virtual coordinates, k_cover_emit<uint8_t, BODY, true>; csrc/acgpu_utf8.hip: k_utf8_batch_vmap, k_utf8_batch_vpos, k_utf8_batch_voff).
Every expected value is the reference of DESIGN.md 4.25's tests: for every haystack ON ITS OWN the CPU oracle's records on the
decoded text (lossy: decoded with "replace"), mapped to bytes by tests/test_gpu_utf8.expected / tests/test_gpu_utf8_lossy.expected,
then tests/spans_ref.merge and tests/cover_ref.cover_ref on the haystack's bytes, back to back -- never the code under test.  As a
second assertion only, a haystack's part of the result equals acgpu_cover_utf8 on it alone.  Every call has a sentinel behind cap and
offsets[0] != 0.  The cases are shared with tests/test_gpu_spans_batch_utf8.py."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickSet, Utf8Error, utf16, utf8_line_offsets
from ahocorasick_amd.unicode_tables import word_chars_from_list
from tests import test_gpu_cover as V
from tests import test_gpu_cover_batch as CB
from tests import test_gpu_cover_utf8 as V8
from tests.cover_batch_ref import layout
from tests.cover_ref import cover_ref
from tests.spans_ref import merge
from tests.test_gpu_utf8 import expected, keywords_from, mixed_text, pair
from tests.test_gpu_utf8_lossy import expected as expected_lossy

C = importlib.import_module("ahocorasick_amd.cover")  # (the package's name `cover` is the function)

pytestmark = pytest.mark.gpu

DEFAULTS = V8.DEFAULTS
MODES = sorted(V.MODES)
TB = N.COVER_TILE_BYTES
SENTINEL = 0x5A
LEAD = b"\xff\x80\xfe"  # in front of offsets[0]: never read, or the strict entries would refuse it
USES8 = V8.USES8
EMPTY = np.zeros((0, 2), np.int32)
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
u8 = V8.u8


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def pieces(p):
    if p:
        N.set_tunable("cursor_first_piece", p)
        N.set_tunable("cursor_max_piece", p)


# ---- the reference ------------------------------------------------------------------------------------------------------------
def records(orc, datas, errors="strict"):
    """-> per haystack the (k, 2) records in BYTES of the haystack decoded alone"""
    out = []
    for d in datas:
        d = bytes(d)
        if not d:
            out.append(EMPTY)
        elif errors == "replace":
            out.append(expected_lossy(orc, d)[0][:, :2])
        else:
            out.append(expected(orc, d)[1][:, :2])
    return out


def cover_batch_ref8(datas, recs, open=b"", close=b"", body="keep", fill=b"*"):
    """-> (bytes, out_offsets): every haystack's cover_ref on its own bytes, back to back"""
    parts = [cover_ref(u8(d), r, u8(open), u8(close), body, fill[0]) for d, r in zip(datas, recs)]
    off = np.zeros(len(parts) + 1, np.uint64)
    if parts:
        off[1:] = np.cumsum([p.size for p in parts], dtype=np.uint64)
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)).astype(np.uint8), off


def spans_batch_ref8(datas, recs):
    rows = [np.concatenate([np.full((len(sp), 1), i, np.int32), sp], axis=1) for i, (d, r) in enumerate(zip(datas, recs)) for sp in [merge(r, len(d))]]
    return np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 3), np.int32)


def n_spans_of(datas, recs):
    return sum(len(merge(r, len(d))) for d, r in zip(datas, recs))


# ---- the entries called raw ---------------------------------------------------------------------------------------------------
def packed(datas):
    """one buffer with LEAD in front of the first haystack -> (uint8 buffer, uint64 offsets, offsets[0] != 0)"""
    buf = u8(LEAD + b"".join(bytes(d) for d in datas))
    off = len(LEAD) + np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.uint64)
    return buf, off.astype(np.uint64)


def cover_raw(a, datas, cap, open=b"", close=b"", body="keep", fill=b"*", errors="strict"):
    """acgpu_cover_batch_utf8[_lossy] into a buffer with a sentinel behind cap -> (the bytes written, out_offsets, rc, n_out, stats, utf8 stats)"""
    buf, off = packed(datas)
    spec, keep = C._spec(u8(open), u8(close), C.BODIES[body], fill[0])
    out = np.full(cap + 64, SENTINEL, np.uint8)
    oo = np.full(len(datas) + 1, 99, np.uint64)
    name = "acgpu_cover_batch_utf8" + ("_lossy" if errors == "replace" else "")
    n_out, st, ust = ctypes.c_uint64(77), N.CoverStats(), N.UTF8_STATS[name]()
    rc = getattr(N.lib(), name)(a.handle, vp(buf), vp(off), len(datas), ctypes.byref(spec), vp(out), cap, vp(oo), ctypes.byref(n_out), ctypes.byref(st),
                                ctypes.byref(ust))
    assert (out[cap:] == SENTINEL).all(), "written at or beyond cap"
    return out[:min(cap, n_out.value)], oo, rc, int(n_out.value), st, ust


def check(a, datas, recs, open=b"", close=b"", body="keep", fill=b"*", errors="strict", singles=8):
    """the entry with exactly the capacity the result needs against the reference, then up to `singles` haystacks against
    acgpu_cover_utf8 -> (the expected bytes, offsets, the call's stats)"""
    want, off = cover_batch_ref8(datas, recs, open, close, body, fill)
    got, oo, rc, n_out, st, ust = cover_raw(a, datas, len(want), open, close, body, fill, errors)
    assert rc == N.OK and n_out == len(want), (rc, n_out, len(want))
    assert oo.tolist() == off.tolist(), np.flatnonzero(oo != off)[:5]
    V.same(got, want, "batch")
    assert (st.n_records, st.n_spans, st.units_out) == (sum(len(r) for r in recs), n_spans_of(datas, recs), len(want)), (st.n_records, st.n_spans)
    for i in range(0, len(datas), max(1, len(datas) // singles)):
        part = want[int(off[i]):int(off[i + 1])]
        alone, rc, n_out, _ = V8.host_raw(a, datas[i], len(part), open, close, body, fill, errors)
        assert rc == N.OK and n_out == len(part)
        V.same(alone, part, "haystack %d alone" % i)
    return want, off, st


def as_bytes(hays):
    """the ASCII haystacks of tests/test_gpu_cover_batch.py (uint16 arrays) as bytes: a unit is a byte, and so are the records"""
    assert all(int(h.max(initial=0)) < 0x80 for h in hays)
    return [h.astype(np.uint8).tobytes() for h in hays]


def set_recs(recs):
    return [np.asarray(r, np.int32)[:, :2] for r in recs]


# ---- 1. the seam --------------------------------------------------------------------------------------------------------------
SEAMS = [(["ab"], ["xab", "abx"]), (["é"], ["xé", "éx"]), (["ab", "é"], ["ab", "ab", "é", "éé", "abé"])]


@pytest.mark.parametrize("kws,texts", SEAMS)
def test_a_span_never_reaches_across_two_haystacks(kws, texts):
    a, orc = pair(N.MODE_ALL, kws)
    datas = [t.encode() for t in texts]
    recs = records(orc, datas)
    assert CB.seam_with_two_spans(datas, recs)
    for body, open, close in (("drop", b"", b""), ("keep", b"<", b">"), ("keep", "«".encode(), b""), ("fill", b"", b"]")):
        check(a, datas, recs, open, close, body, singles=len(datas))
    if len(texts) == 2:
        kw = kws[0].encode()
        assert C.redact_batch_utf8(a, datas, b"R") == [b"xR", b"Rx"] and C.redact_utf8(a, b"".join(datas), b"R") == b"xRx"
        assert C.cover_batch_utf8(a, datas, open=b"<", close=b">") == [b"x<" + kw + b">", b"<" + kw + b">x"]
    else:  # consecutive haystacks that are each wholly covered: every result is empty, every offset 0
        out, oo, rc, n_out, st, _ = cover_raw(a, datas, 0, b"", b"", "drop")
        assert rc == N.OK and n_out == 0 and not oo.any() and st.n_spans == len(datas)


@pytest.mark.parametrize("p", [None, 1, 16])
def test_a_lone_low_surrogate_against_four_byte_characters_at_the_seams(p):
    lo = utf16("😀")[1:]
    s = AhoCorasickSet([lo, "ab"], True)
    a, orc = pair(N.MODE_ALL, [lo, "ab"])
    datas = [t.encode() for t in ("a😀", "😀a", "😀", "😀", "", "😀😀", "ab😀", "😀ab", "x")]
    recs = records(orc, datas)  # (the widened records: the whole character, which touch only in bytes)
    assert recs[0].tolist() == [[1, 5]] and recs[1].tolist() == [[0, 4]] and CB.seam_with_two_spans(datas, recs)
    pieces(p)
    for body, open, close in USES8 + [("drop", b"", b"")]:
        check(s.automaton, datas, recs, open, close, body, singles=len(datas))
    assert C.cover_batch_utf8(s, datas[:2], open=b"<", close=b">", body="fill", fill=b"#") == [b"a<####>", b"<####>a"]


# ---- 2. empty haystacks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [None, 16])
def test_empty_haystacks(p):
    a, orc = pair(N.MODE_ALL, ["ab", "b", "é€"])
    some = [t.encode() for t in ("xab", "é€b", "..", "abé€", "b")]
    E = [b""]
    batches = [E + some, some + E, some[:2] + E + some[2:], some[:1] + E * 2 + some[1:3] + E * 300 + some[3:] + E * 2, E * 2 + some + E * 300,
               E * 5, E, some[:1], some[1:2]]
    pieces(p)
    for datas in batches:
        recs = records(orc, datas)
        for body, open, close in USES8 + [("drop", b"", b"")]:
            check(a, datas, recs, open, close, body, singles=4)


# ---- 3. sequences of 1 to 4 bytes at the edges of haystacks and spans, every family -------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_case(mode):
    """a mixed text cut into haystacks at character boundaries -> (kws, datas, records in bytes)"""
    rng = np.random.default_rng(500 + mode)
    text = mixed_text(rng, 1500)
    kws = keywords_from(np.random.default_rng(78 + mode), text, mode, True)
    picks = rng.integers(0, len(text) + 1, 90)
    cuts = np.sort(np.concatenate([[0, 0, len(text), len(text)], picks, picks[:3]]))  # (an empty haystack first, last and at three cuts)
    datas = [text[int(s):int(e)].encode() for s, e in zip(cuts[:-1], cuts[1:])]
    a, orc = pair(mode, kws)
    recs = records(orc, datas)
    nb = lambda ch: len(ch.encode())
    assert {nb(d.decode()[0]) for d in datas if d} == {1, 2, 3, 4} == {nb(d.decode()[-1]) for d in datas if d}
    sp = [(d, s, e) for d, r in zip(datas, recs) for s, e in merge(r, len(d)).tolist()]
    # (every pair of lengths as a span's first and last character: test_every_sequence_length_first_and_last_in_haystacks_and_spans)
    assert len(sp) >= 10 and len({nb(d[s:e].decode()[0]) for d, s, e in sp}) >= 3 and any(not d for d in datas), mode
    return kws, datas, recs


@pytest.mark.parametrize("body,open,close", [("keep", "«".encode(), "»".encode()), ("fill", b"", b""), ("drop", "[…]".encode(), b"")])
@pytest.mark.parametrize("p", [None, 16])
@pytest.mark.parametrize("mode", MODES)
def test_mixed_batch_every_family(mode, p, body, open, close):
    kws, datas, recs = mixed_case(mode)
    a, orc = pair(mode, kws)
    pieces(p)
    want, off, st = check(a, datas, recs, open, close, body)
    want.tobytes().decode()  # the result is well-formed
    if p:
        assert st.pieces >= 50
    if body == "fill":
        assert off.tolist() == np.concatenate([[0], np.cumsum([len(d) for d in datas])]).tolist()


@pytest.mark.parametrize("body,open,close", USES8)
@pytest.mark.parametrize("p", [None, 16])
@pytest.mark.parametrize("mode", MODES)
def test_ascii_batch_every_family(mode, p, body, open, close):
    """the branch without checkpoints: a unit of the scan's text is its virtual coordinate"""
    kws, hays, recs = CB.seam_case(mode) if p is None else CB.small_piece_case(mode)
    a = CB.automaton(mode, kws)
    pieces(p)
    check(a, as_bytes(hays), set_recs(recs), open, close, body)


def test_every_sequence_length_first_and_last_in_haystacks_and_spans():
    chars = ["a", "é", "€", "😀"]
    kws = [x + y for x in chars for y in chars] + chars[1:]  # every pair of lengths as a span's first and last character
    a, orc = pair(N.MODE_ALL, kws)
    rng = np.random.default_rng(8)
    alpha = chars + [".", "ő", "。", "𝒜"]
    texts = [x + "." + y for x in alpha for y in alpha] + [x + y for x in chars for y in chars] + chars
    texts += ["".join(alpha[int(i)] for i in rng.integers(0, len(alpha), int(n))) for n in rng.integers(0, 30, 60)]
    datas = [t.encode() for t in texts]
    recs = records(orc, datas)
    nb = lambda ch: len(ch.encode())
    sp = [(d, s, e) for d, r in zip(datas, recs) for s, e in merge(r, len(d)).tolist()]
    assert {(nb(d[s:e].decode()[0]), nb(d[s:e].decode()[-1])) for d, s, e in sp} >= {(i, j) for i in (1, 2, 3, 4) for j in (1, 2, 3, 4)}
    assert {(nb(t[0]), nb(t[-1])) for t in texts if t} >= {(i, j) for i in (1, 2, 3, 4) for j in (1, 2, 3, 4)}
    for p in (None, 16):
        pieces(p)
        for body, open, close in USES8:
            check(a, datas, recs, open, close, body)


# ---- 4. pieces ----------------------------------------------------------------------------------------------------------------
PIECE_KWS = ["ab", "b", "bé", "é€", "a😀", "😀", "€.a"]


@functools.lru_cache(maxsize=None)
def boundary_case(p):
    """Pieces of p units: a piece boundary falls ON a separator, BETWEEN the two units of a surrogate pair and INSIDE a run of empty
    haystacks (asserted on the scan's text: the haystacks' units with a separator behind each)"""
    rng = np.random.default_rng(900 + p)
    bmp = ["a", "b", ".", "é", "€", "a", "b"]
    fill = lambda n: "".join(bmp[int(i)] for i in rng.integers(0, len(bmp), n))
    texts = [fill(p), fill(p - 2) + "😀" + fill(p - 3), "", "", "", ""]
    texts += [fill(int(n)) + ("😀" if n % 3 == 0 else "") for n in rng.integers(0, 2 * p // 3 + 2, 12)]
    units = [utf16(t) for t in texts]
    starts = np.concatenate([[0], np.cumsum([len(u) + 1 for u in units])])
    seps = set((starts[1:] - 1).tolist())
    cat = np.concatenate([np.concatenate([u, [0]]) for u in units])
    assert p in seps and 0xDC00 <= cat[2 * p] < 0xE000 and {3 * p - 1, 3 * p, 3 * p + 1} <= seps and len(cat) > 5 * p
    a, orc = pair(N.MODE_ALL, PIECE_KWS)
    datas = [t.encode() for t in texts]
    return datas, records(orc, datas)


@pytest.mark.parametrize("body,open,close", USES8 + [("drop", b"", b"")])
@pytest.mark.parametrize("p", [16, 1000])
def test_piece_boundaries_on_a_separator_inside_a_pair_and_among_empty_haystacks(p, body, open, close):
    datas, recs = boundary_case(p)
    a, orc = pair(N.MODE_ALL, PIECE_KWS)
    pieces(p)
    want, off, st = check(a, datas, recs, open, close, body)
    assert st.pieces >= 5, st.pieces


@pytest.mark.parametrize("mode", [N.MODE_LONGEST, N.MODE_SHORTEST])
def test_piece_boundaries_first_unit_and_last_unit_families(mode):
    datas, _ = boundary_case(16)
    a, orc = pair(mode, PIECE_KWS)
    recs = records(orc, datas)
    pieces(16)
    for body, open, close in USES8:
        check(a, datas, recs, open, close, body)


@pytest.mark.parametrize("reservoir", [8 * N.REC_SET, 512 * N.REC_SET])
def test_a_full_reservoir(reservoir):
    rng = np.random.default_rng(55)
    kws = ["ab", "b", "bcd", "dd", "a", "abcd", "é", "dé"]
    alpha = list("abcd") + ["é"]
    datas = ["".join(alpha[int(i)] for i in rng.integers(0, len(alpha), int(n))).encode() for n in rng.integers(0, 60, 250)]
    N.set_tunable("cursor_reservoir_bytes", reservoir)
    a, orc = pair(N.MODE_ALL, kws)  # (a pool made under the tunable: a reservoir never shrinks)
    recs = records(orc, datas)
    assert sum(len(r) for r in recs) > 6 * 512
    for body, open, close in USES8:
        want, off, st = check(a, datas, recs, open, close, body, singles=4)
        assert st.rescans > 0, (st.pieces, st.rescans)


@functools.lru_cache(maxsize=None)
def long_span_case():
    """keyword aa: a haystack of 10 000 a is ONE span carried through the pieces of 1000 units; a non-ASCII batch"""
    rng = np.random.default_rng(5)
    alpha = ["a", ".", "a", "é"]
    short = lambda k: ["".join(alpha[int(i)] for i in rng.integers(0, len(alpha), int(n))) for n in rng.integers(0, 30, k)]
    texts = short(40) + ["a" * 10000, "", "aa", "a", "é" + "a" * 5000 + "😀", "a" * 3000 + ".aa", ".." + "a" * 4000] + short(40)
    a, orc = pair(N.MODE_ALL, ["aa"])
    datas = [t.encode() for t in texts]
    return datas, records(orc, datas)


@pytest.mark.parametrize("body,open,close", USES8)
def test_one_span_carried_through_several_pieces(body, open, close):
    datas, recs = long_span_case()
    a, orc = pair(N.MODE_ALL, ["aa"])
    pieces(1000)
    want, off, st = check(a, datas, recs, open, close, body)
    assert st.pieces >= 20 and st.max_carry >= 1, (st.pieces, st.max_carry)


# ---- 5. windows of the slabs --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def window_case():
    rng = np.random.default_rng(66)
    alpha = list("abcd....") + ["é", "€"]
    datas = ["".join(alpha[int(i)] for i in rng.integers(0, len(alpha), int(n))).encode() for n in rng.integers(0, 16, 3000)]
    a, orc = pair(N.MODE_ALL, ["ab", "b", "bcd", "dd", "é"])
    return datas, records(orc, datas)


@pytest.mark.parametrize("slab", [8, 1000])
def test_windows_of_the_slabs(slab):
    datas, recs = window_case()
    a, orc = pair(N.MODE_ALL, ["ab", "b", "bcd", "dd", "é"])
    window = (max(slab, 8) + 15) & ~15  # a slab is a whole number of 16-byte vectors
    found, total = CB.windows_begin_inside(datas, recs, 5, 4, "keep", window)
    assert found == {"open", "body", "close", "text", "seam"} and total > 4 * TB, (found, total)
    N.set_tunable("replace_slab_units", slab)
    check(a, datas, recs, b"<<b>>", b"<e/>", "keep", singles=4)
    found, total = CB.windows_begin_inside(datas, recs, 5, 0, "drop", window)
    assert found == {"open", "text", "seam"} and total > 4 * TB, (found, total)
    check(a, datas, recs, b"[...]", b"", "drop", singles=4)
    pieces(16)
    N.set_tunable("replace_slab_units", slab)
    check(a, datas[:200], recs[:200], b"<<b>>", b"<e/>", "keep", singles=4)  # ... and in every piece of a call in pieces of 16 units


# ---- 6. segments --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_cap", [None, 0, 5])
@pytest.mark.parametrize("body,open", [("drop", b""), ("keep", b"<")])
def test_more_items_in_an_emit_tile_than_lds_holds(body, open, lds_cap):
    rng = np.random.default_rng(21)
    a, orc = pair(N.MODE_ALL, ["a", "b"])
    datas = [bytes(b"abz"[int(i)] for i in rng.integers(0, 3, int(n))) for n in rng.integers(0, 2, 5000)]  # one-byte and empty haystacks
    recs = records(orc, datas)
    kinds, stretch, item_at = layout(datas, recs, len(open), 0, body)
    first_tile = int(((item_at >= 0) & (item_at < TB)).sum())
    assert first_tile > N.COVER_LDS_SEGMENTS, first_tile
    if lds_cap is not None:
        assert N.set_tunable("cover_lds_segments", lds_cap) == N.COVER_LDS_SEGMENTS
    want, off, st = check(a, datas, recs, open, b"", body)
    if body == "drop":
        assert 0 < want.size < TB and (want == ord("z")).all()


@functools.lru_cache(maxsize=None)
def tile_edge_case():
    rng = np.random.default_rng(31)
    alpha = list("abc.") + ["é", "."]
    datas = ["".join(alpha[int(i)] for i in rng.integers(0, len(alpha), int(n))).encode() for n in rng.integers(0, 40, 4000)]
    a, orc = pair(N.MODE_ALL, ["ab", "bc", "é", "cab"])
    return datas, records(orc, datas)


@pytest.mark.parametrize("lds_cap", [None, 7])
def test_every_kind_of_unit_at_a_tile_s_first_and_last_byte(lds_cap):
    datas, recs = tile_edge_case()
    a, orc = pair(N.MODE_ALL, ["ab", "bc", "é", "cab"])
    kinds, stretch, item_at = layout(datas, recs, 3, 2, "keep")
    assert len(kinds) > 20 * TB
    every = {"open", "body", "close", "text"}
    assert {kinds[o] for o in range(TB, len(kinds), TB)} == every == {kinds[o - 1] for o in range(TB, len(kinds), TB)}
    assert set(range(TB, len(kinds), TB)) & set(item_at.tolist())  # an item -- a span's open or a phantom -- begins a tile
    if lds_cap is not None:
        N.set_tunable("cover_lds_segments", lds_cap)
    check(a, datas, recs, b"<i>", b"</", "keep")  # (one piece, one window: the tiles are those of the whole result)


# ---- 7. capacity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body,open,close", USES8)
@pytest.mark.parametrize("p", [None, 16])
def test_capacity_keeps_every_offset_exact_and_the_sentinel(p, body, open, close):
    kws, datas, recs = mixed_case(N.MODE_ALL)
    a, orc = pair(N.MODE_ALL, kws)
    want, off = cover_batch_ref8(datas, recs, open, close, body)
    total = len(want)
    pieces(p)
    for cap in (total, total - 1, total // 2, 0):
        got, oo, rc, n_out, st, _ = cover_raw(a, datas, cap, open, close, body)
        assert rc == (N.OK if cap == total else N.E_OVERFLOW) and n_out == total == st.units_out, (cap, rc, n_out)
        assert oo.tolist() == off.tolist(), cap
        V.same(got, want[:cap], "cap %d" % cap)


# ---- 8. encoding --------------------------------------------------------------------------------------------------------------
def ill_formed_batches():
    good = [t.encode() for t in ("xab", "é€ab", "", "ab😀", "b.é")]
    out = []
    for at in (0, 2, len(good) - 1):  # the first, a middle (behind an empty one) and the last haystack
        at = 3 if at == 2 else at
        stray = list(good)
        stray[at] = good[at][:2] + b"\xbf" + good[at][2:] if at else b"\x80" + good[at]
        out.append(stray)
    for at in (0, 1, 3):  # a sequence cut by the boundary behind haystack `at`: each half is ill-formed on its own
        cut = list(good) + ["€x".encode()]
        whole = cut[at] + "€".encode() + cut[at + 1]
        cut[at], cut[at + 1] = whole[:len(cut[at]) + 2], whole[len(cut[at]) + 2:]
        out.append(cut)
    out.append(list(good[:-1]) + [good[-1] + b"\xf0\x9f\x98"])  # ... and cut by the batch's end
    return out


def match_batch_stats(a, datas, lossy=False):
    """what acgpu_match_batch_utf8[_lossy] reports for the same buffer -> (rc, the stats' fields)"""
    buf, off = packed(datas)
    name = "acgpu_match_batch_utf8" + ("_lossy" if lossy else "")
    out, n_out, ust = np.zeros((4096, 3), np.int32), ctypes.c_uint64(0), N.UTF8_STATS[name]()
    rc = getattr(N.lib(), name)(a.handle, vp(buf), vp(off), len(datas), N.REC_SET, vp(out), 4096, ctypes.byref(n_out), ctypes.byref(ust))
    return rc, [int(getattr(ust, f)) for f, _ in ust._fields_]


@pytest.mark.parametrize("i", range(7))
def test_strict_refuses_what_match_batch_utf8_refuses_and_touches_nothing(i):
    datas = ill_formed_batches()[i]
    a, orc = pair(N.MODE_ALL, ["ab", "b", "é"])
    rc, want = match_batch_stats(a, datas)
    assert rc == N.E_ENCODING
    buf, off = packed(datas)
    spec, keep = C._spec(u8(b"<"), u8(b">"), C.BODIES["keep"], ord("*"))
    out, oo = np.full(256, SENTINEL, np.uint8), np.full(len(datas) + 1, 99, np.uint64)
    n_out, st, ust = ctypes.c_uint64(77), N.CoverStats(), N.Utf8BatchStats()
    rc = N.lib().acgpu_cover_batch_utf8(a.handle, vp(buf), vp(off), len(datas), ctypes.byref(spec), vp(out), 192, vp(oo), ctypes.byref(n_out), ctypes.byref(st),
                                        ctypes.byref(ust))
    assert rc == N.E_ENCODING and n_out.value == 0
    assert [int(getattr(ust, f)) for f, _ in ust._fields_] == want
    assert (out == SENTINEL).all() and oo[0] == 0 and (oo[1:] == 99).all()
    with pytest.raises(Utf8Error) as e:
        C.mask_batch_utf8(a, datas)
    assert (e.value.haystack, e.value.start) == (ust.bad_haystack, ust.first_bad)
    good = [t.encode() for t in ("xab", "é€ab")]
    check(a, good, records(orc, good), b"<", b">")  # the pool is as usable as before


@pytest.mark.parametrize("p", [None, 3])
@pytest.mark.parametrize("i", range(7))
def test_lossy_decodes_every_haystack_on_its_own(i, p):
    datas = ill_formed_batches()[i]
    a, orc = pair(N.MODE_ALL, ["ab", "b", "é", "\ufffd\ufffd", "b\ufffd", "x\ufffd"])  # U+FFFD in a keyword matches a replaced subpart
    recs = records(orc, datas, "replace")
    pieces(p)
    for body, open, close in USES8:
        want, off, st = check(a, datas, recs, open, close, body, errors="replace", singles=len(datas))
    rc, want_st = match_batch_stats(a, datas, lossy=True)
    got, oo, rc2, n_out, st, ust = cover_raw(a, datas, 0, errors="replace")
    assert rc == N.OK and rc2 == N.E_OVERFLOW and [int(getattr(ust, f)) for f, _ in ust._fields_] == want_st


def test_lossy_stray_bytes_are_copied_outside_the_spans_and_filled_inside():
    text = "aé€😀kw".encode()
    block = b"\x80" + text + b"\xbf\xbf" + text + b"\xc3(" + b"\xe2\x82" + b"x" + b"\xf0\x9f\x98" + text
    datas = [block, b"", block[:9], block[9:], b"\xbf\xbf", b"k\xffw", block * 3, b"\xf0\x9f\x98"]
    a, orc = pair(N.MODE_ALL, ["k\ufffdw", "k", "\ufffd\ufffd", "é😀"])
    recs = records(orc, datas, "replace")
    for body, open, close in USES8:
        check(a, datas, recs, open, close, body, errors="replace", singles=len(datas))
    masked = C.mask_batch_utf8(a, datas, fill=b"#", errors="replace")
    n_filled_stray = 0
    for d, r, m in zip(datas, recs, masked):
        covered = np.zeros(len(d), bool)
        for s, e in merge(r, len(d)).tolist():
            covered[s:e] = True
        got = u8(m)
        assert len(m) == len(d) and ((got != u8(d)) == covered).all() and (got[covered] == ord("#")).all()
        n_filled_stray += int((covered & (u8(d) >= 0x80) & (u8(d) < 0xC0) if len(d) else covered).sum())
    assert n_filled_stray and masked[4] == b"##" and masked[5] == b"###"
    with pytest.raises(Utf8Error):
        C.mask_batch_utf8(a, datas)


# ---- 9. where the library makes one call per haystack -------------------------------------------------------------------------
def unit_records(orc, datas):
    """the reference for an oracle of tests/test_gpu_cover.pair (Set records in units): mapped to bytes as expected() maps them"""
    from tests.test_gpu_utf8 import to_bytes
    out = []
    for d in datas:
        text = bytes(d).decode()
        out.append(to_bytes(orc.match(utf16(text), cap=max(64, 8 * len(text)))[:, :2], text) if text else EMPTY)
    return out


@pytest.mark.parametrize("mode", V.WORDY)
def test_fallback_word_table_that_is_not_fold_consistent(mode):
    rng = np.random.default_rng(9)
    alpha = np.array([ord(ch) for ch in "abxyABXY ,"], dtype=np.uint16)
    wc = word_chars_from_list("abcdxyABCD")  # X, Y are not word characters although x, y are
    kws = [alpha[rng.integers(0, 4, int(rng.integers(1, 5)))] for _ in range(12)]
    kws += [kws[2].copy()]
    a, orc = V.pair(mode, kws, cs=False, wc=wc)
    assert a.info()["fold_consistent"] == 0
    texts = ["".join(chr(int(u)) for u in alpha[rng.integers(0, len(alpha), int(n))]) for n in (0, 1, 40, 300, 7, 0, 120, 3, 12, 60, 0, 25)]
    datas = [(t[:len(t) // 2] + "é€" + t[len(t) // 2:] if len(t) > 20 else t).encode() for t in texts]  # (é and € are no word characters)
    recs = unit_records(orc, datas)
    assert sum(len(r) for r in recs) > 5
    for body, open, close in USES8:
        want, off, st = check(a, datas, recs, open, close, body, singles=len(datas))
        assert st.pieces == sum(1 for d in datas if len(d))  # a text per haystack
    want, off = cover_batch_ref8(datas, recs, b"<", b">", "keep")
    got, oo, rc, n_out, st, _ = cover_raw(a, datas, int(off[3]) + 1, b"<", b">", "keep")  # overflow through the calls per haystack
    assert rc == N.E_OVERFLOW and n_out == len(want) and oo.tolist() == off.tolist()
    V.same(got, want[:int(off[3]) + 1], "overflow")
    # an ill-formed batch on this route: refused as on the other, before any haystack is rewritten
    bad = datas[:5] + [b"ab\xe2\x82"] + datas[5:]
    rc, want_st = match_batch_stats(a, bad)
    got, oo, rc2, n_out, st, ust = cover_raw(a, bad, 4096, b"<", b">", "keep")
    assert rc == rc2 == N.E_ENCODING and n_out == 0 and got.size == 0 and (oo[1:] == 99).all()
    assert [int(getattr(ust, f)) for f, _ in ust._fields_] == want_st and ust.bad_haystack == 5
    check(a, datas, unit_records(orc, datas), b"<", b">", "keep", errors="replace", singles=2)  # the lossy entry takes the same route


def test_fallback_dictionary_without_a_free_unit():
    kws = [np.array([i], dtype=np.uint16) for i in range(65536)]
    a, orc = V.pair(N.MODE_ALL, kws)
    texts = ["\x05\x06", "\x07", "", "\uffff\x00\x01", "\u012c" * 9, "", "\x00", "é€", "\x01\x02\x03\x04", "\t" * 70, "", "😀a"]
    datas = [t.encode() for t in texts]
    recs = unit_records(orc, datas)
    assert sum(len(r) for r in recs) == sum(len(utf16(t)) for t in texts)
    for body, open, close in USES8:
        want, off, st = check(a, datas, recs, open, close, body, singles=len(datas))
        assert st.pieces == sum(1 for d in datas if len(d)) and st.n_spans == sum(1 for d in datas if len(d))
    got, oo, rc, n_out, st, ust = cover_raw(a, datas[:3] + [b"\xc3"] + datas[3:], 4096)
    assert rc == N.E_ENCODING and (ust.bad_haystack, ust.first_bad) == (3, 0) and got.size == 0


# ---- 10. the Python surface ---------------------------------------------------------------------------------------------------
def test_python_functions():
    kws, datas, recs = mixed_case(N.MODE_ALL)
    a, orc = pair(N.MODE_ALL, kws)
    to_list = lambda out, off: [out[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(off) - 1)]
    uses = ((lambda **k: C.mask_batch_utf8(a, fill="#", **k), (b"", b"", "fill")), (lambda **k: C.highlight_batch_utf8(a, open="«", close=b"</b>", **k), ("«".encode(), b"</b>", "keep")),
            (lambda **k: C.redact_batch_utf8(a, replacement="[…]", **k), ("[…]".encode(), b"", "drop")))
    buf = np.frombuffer(b"".join(datas), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.uint64)
    for fn, (open, close, body) in uses:
        want = to_list(*cover_batch_ref8(datas, recs, open, close, body, b"#"))
        assert fn(datas=datas) == want                                             # a list of bytes
        assert fn(datas=[bytearray(d) for d in datas]) == want
        assert fn(datas=buf, offsets=off) == want                                  # one buffer in place
        assert fn(datas=buf, offsets=off[3:]) == want[3:]                          # (offsets[0] != 0)
    log = "ab\nxé\n\néx😀ab".encode()
    lines = log.splitlines(keepends=True)
    s = AhoCorasickSet(["ab", "é"], True)
    assert C.redact_batch_utf8(s, log, "R", offsets=utf8_line_offsets(log)) == [C.redact_utf8(s, ln, "R") for ln in lines] == [b"R\n", b"xR\n", b"\n", "Rx😀R".encode()]
    out, out_off, st = C.cover_batch_bytes(a, datas, open=b"<<<<", close=">>>>", cap=16)  # the wrapper's one retry
    want, woff = cover_batch_ref8(datas, recs, b"<<<<", b">>>>", "keep")
    assert (out == want).all() and out_off.tolist() == woff.tolist() and st["n_spans"] == n_spans_of(datas, recs)
    bad = list(datas[:7]) + [b"a\xffb"] + list(datas[7:])
    with pytest.raises(Utf8Error) as e:
        C.cover_batch_utf8(a, bad)
    assert (e.value.haystack, e.value.start) == (7, 1)
    lossy_recs = records(orc, bad, "replace")
    assert C.cover_batch_utf8(a, bad, open=b"<", close=b">", errors="replace") == to_list(*cover_batch_ref8(bad, lossy_recs, b"<", b">", "keep"))
