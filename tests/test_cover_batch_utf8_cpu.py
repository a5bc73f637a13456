"""The UTF-8 batch spans and batch cover entries without a GPU (include/acgpu.h: acgpu_spans_batch_utf8, acgpu_cover_batch_utf8 and
their _lossy twins; ahocorasick_amd/spans.py, cover.py):
 * a Python restatement of the VIRTUAL-COORDINATE plan of DESIGN.md 4.25 -- records -> v, the merge with its carry, the item list
   of spans and phantoms, deltas, positions, the per-segment source shift of the emit, the offsets read at the phantoms -- driven
   in pieces of 1, 2, 3, 7 and 16 units over random batches, against tests/spans_ref.merge and tests/cover_ref.cover_ref on every
   haystack's own bytes;
 * the symbols, every argument decision made before a device is looked for, the batch without a byte;
 * the wrappers' argument errors and capacity rule against the stub of tests/test_binding_calls_cpu.py."""
import bisect
import ctypes
import importlib

import numpy as np
import pytest

import ahocorasick_amd
from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickSet, Automaton, Utf8Error, utf16, utf8_line_offsets
from tests.cover_ref import cover_ref
from tests.spans_ref import merge
from tests.test_binding_calls_cpu import BAD_HAYSTACK, FIRST_BAD, OVF, automaton, stub  # noqa: F401 (stub: the fixture)
from tests.test_cover_cpu import spec_of
from tests.test_gpu_utf8 import to_bytes, unit_map

C = importlib.import_module("ahocorasick_amd.cover")  # (the package's names `cover` and `spans` are the functions)
S = importlib.import_module("ahocorasick_amd.spans")
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
u8 = lambda b: np.frombuffer(bytes(b), np.uint8)
INF = 1 << 62
TILE = 5  # the model's emit tile: small, so that segments begin in front of, inside and behind a tile


# ---- the dictionary of the model: naive matching on UTF-16 units --------------------------------------------------------------
def occurrences(units, kws):
    """every occurrence of every keyword (arrays of units) -> records (start, end), AhoCorasick's order: end ascending, longest first"""
    out = []
    for k in kws:
        for s in range(len(units) - len(k) + 1):
            if (units[s:s + len(k)] == k).all():
                out.append((s, s + len(k)))
    return sorted(out, key=lambda r: (r[1], r[0]))


def leftmost_longest(units, kws):
    """LongestMatch: at every position the longest keyword, matches do not overlap -> records in position order"""
    out, p = [], 0
    while p < len(units):
        best = max((len(k) for k in kws if p + len(k) <= len(units) and (units[p:p + len(k)] == k).all()), default=0)
        if best:
            out.append((p, p + best))
        p += max(best, 1)
    return out


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def haystack_of(off, n_hay, pos):
    """csrc/acgpu_device.h: the last haystack that begins at or before pos"""
    lo, hi = 0, n_hay
    while hi - lo > 1:
        mid = lo + ((hi - lo) >> 1)
        if off[mid] <= pos:
            lo = mid
        else:
            hi = mid
    return lo


def merge_piece(carry, recs, B):
    """the head rule and the carry rule (csrc/acgpu_spans.hip) -> (final spans, carried spans)"""
    lst = list(carry) + list(recs)
    m = len(lst)
    X, run = [INF] * m, INF
    for i in range(m - 1, -1, -1):
        X[i] = run
        run = min(run, lst[i][0])
    spans, start = [], None
    for i, (s, e) in enumerate(lst):
        M = min(s, X[i])
        if i == 0 or M > lst[i - 1][1]:
            start = M
        if i == m - 1 or X[i] > e:
            spans.append((start, e))
    return [sp for sp in spans if sp[1] < B], [sp for sp in spans if sp[1] >= B]


def make_seg(items, pos, i, t0, done, voff, n_hay, ol, cl, drop):
    """CoverArgs<uint8_t, BODY, true>::make_seg (csrc/acgpu_cover.hip): {rel, a_end, b_end, c_end, osrc, bsrc, csrc, tsrc}; the
    sources carry the haystack's index, which is constant within a segment"""
    if i < 0:
        return (-1, 0, 0, 0, 0, 0, 0, done + t0 - haystack_of(voff, n_hay, done))
    s, e = items[i]
    P = pos[i] - t0
    sep = s == e
    h = haystack_of(voff, n_hay, s)
    a = P + (0 if sep else ol)
    b = a + (0 if drop else e - s)
    c = b + (0 if sep else cl)
    clamp = lambda x: min(max(x, 0), TILE)
    return (max(P, -1), clamp(a), clamp(b), clamp(c), -P, s - h - a, -b, e - h - c)


def element(seg, u, buf, open, close, fill):
    rel, a_end, b_end, c_end, osrc, bsrc, csrc, tsrc = seg
    if u < a_end:
        return open[osrc + u]
    if u < b_end:
        return fill if fill is not None else buf[bsrc + u]
    if u < c_end:
        return close[csrc + u]
    return buf[tsrc + u]


def run_model(texts, kws, first_unit, piece, open, close, body, fill):
    """-> (triples, out bytes, out_offsets) as the device computes them, the scan replaced by the records of every piece"""
    n_hay = len(texts)
    units = [utf16(t) for t in texts]
    buf = u8("".join(texts).encode())
    boff = np.concatenate([[0], np.cumsum([len(t.encode()) for t in texts])]).astype(np.int64)
    cat_off = np.concatenate([[0], np.cumsum([len(u) + 1 for u in units])]).astype(np.int64)
    voff = boff + np.arange(n_hay + 1)
    n_v, cat = int(voff[-1]), int(cat_off[-1])
    off_all, len_all = unit_map("".join(texts))  # the buffer read as one text, WITHOUT separators
    max_len = max(len(k) for k in kws)
    recs = []  # in units of the concatenation
    for h, u in enumerate(units):
        found = leftmost_longest(u, kws) if first_unit else occurrences(u, kws)
        recs += [(s + int(cat_off[h]), e + int(cat_off[h])) for s, e in found]

    def to_v(s, e):  # k_utf8_batch_vmap
        h = haystack_of(cat_off, n_hay, s)
        return int(off_all[s - h]) + h, int(off_all[e - 1 - h] + len_all[e - 1 - h]) + h

    def vpos(x):  # k_utf8_batch_vpos
        if x >= cat:
            return n_v
        h = haystack_of(cat_off, n_hay, x)
        if x + 1 == cat_off[h + 1]:
            return int(boff[h + 1]) + h  # the separator's own phantom
        return int(off_all[x - h]) + h

    w = len(open) + len(close)
    drop = body == "drop"
    triples, out, out_off = [], [], [0] * (n_hay + 1)
    carry, done, out_pos, lo = [], 0, 0, 0
    while lo < cat:
        hi = min(lo + piece, cat)
        last = hi >= cat
        own = [r for r in recs if (lo <= r[0] < hi if first_unit else lo <= r[1] - 1 < hi)]
        own_v = [to_v(s, e) for s, e in own]
        assert own_v == sorted(own_v, key=lambda r: r[1])  # the map is monotone: the order by end survives
        bound = hi if first_unit else max(hi - (max_len - 1), 0)
        lst = carry + own_v
        if last:
            B = INF
        else:
            B = vpos(bound)
            if first_unit and lst:
                B = max(B, lst[-1][1])
        final, carry = merge_piece(carry, own_v, B)
        L = n_v if last else min([B] + [sp[0] for sp in carry[:1]])
        assert done <= L <= n_v and all(done <= s and e <= L for s, e in final)
        for s, e in final:  # k_span_tag over voff
            h = haystack_of(voff, n_hay, s)
            assert e <= voff[h + 1] - 1  # no span covers a phantom
            triples.append((h, s - int(voff[h]), e - int(voff[h])))
        # the item list: the final spans and, as {p, p}, the phantoms in [done, L)
        i0 = bisect.bisect_right(voff[1:].tolist(), done)  # separators_in: the first phantom at or behind done
        i1 = max(i0, bisect.bisect_right(voff[1:].tolist(), L))
        phantoms = [int(voff[j + 1]) - 1 for j in range(i0, i1)]
        assert n_hay - i0 >= len(phantoms)  # the bound the grids are sized by
        items = sorted(final + [(p, p) for p in phantoms])
        delta = [-1 if s == e else w - ((e - s) if drop else 0) for s, e in items]
        pos, run = [], 0
        for (s, e), d in zip(items, delta):
            pos.append(s - done + run)
            run += d
        total = (L - done) + run
        for j, p in enumerate(phantoms):  # k_cover_batch_offsets: a result's first byte is read off the plan at its phantom
            out_off[i0 + j + 1] = out_pos + pos[items.index((p, p))]
        for o in range(total):  # the emit, an element at a time
            t0 = o - o % TILE
            i = bisect.bisect_right(pos, o) - 1  # the LAST of equal positions
            seg = make_seg(items, pos, i, t0, done, voff, n_hay, len(open), len(close), drop)
            out.append(int(element(seg, o - t0, buf, open, close, fill if body == "fill" else None)))
        done, out_pos, lo = L, out_pos + total, hi
    assert not carry and done == n_v and out_off[n_hay] == out_pos
    return triples, np.array(out, np.uint8), out_off


def reference(texts, kws, first_unit, open, close, body, fill):
    """every haystack on its own: its records in bytes, tests/spans_ref.merge and tests/cover_ref.cover_ref, back to back"""
    triples, parts = [], []
    for h, t in enumerate(texts):
        u = utf16(t)
        found = np.array(leftmost_longest(u, kws) if first_unit else occurrences(u, kws), np.int32).reshape(-1, 2)
        recs_b = to_bytes(found, t)
        data = u8(t.encode())
        triples += [(h, s, e) for s, e in merge(recs_b, len(data)).tolist()]
        parts.append(cover_ref(data, recs_b, open, close, body, fill))
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    return triples, np.concatenate(parts) if parts else np.zeros(0, np.uint8), off.tolist()


ALPHABET = ["a", "b", "a", "b", ".", "é", "€", "😀"]
KWS = [utf16("ab"), utf16("b"), utf16("é"), utf16("a😀"), utf16("😀")[:1], utf16("😀")[1:], utf16("bé€")]
USES = [("keep", b"<", b"</>"), ("fill", b"", b""), ("drop", b"", b""), ("drop", b"[r]", b"")]


def random_batch(rng, n):
    lens = rng.choice([0, 0, 1, 2, 3, 5, 9, 14], n)
    return ["".join(ALPHABET[int(i)] for i in rng.integers(0, len(ALPHABET), int(ln))) for ln in lens]


@pytest.mark.parametrize("piece", [1, 2, 3, 7, 16])
@pytest.mark.parametrize("first_unit", [False, True])
def test_the_plan_in_virtual_coordinates_reproduces_the_reference(piece, first_unit):
    rng = np.random.default_rng(40 + piece)
    batches = [random_batch(rng, int(n)) for n in (1, 2, 5, 12, 12, 20)]
    batches += [["xab", "abx"], ["xé", "éx"], ["ab", "ab", "abab"], ["", "", "ab", "", ""], [""] * 4, ["😀", "😀a😀", "😀"], ["b"], ["", "😀"],
                ["a😀b", "", "", "😀😀", "é"]]
    for texts in batches:
        for body, open, close in USES:
            want = reference(texts, KWS, first_unit, u8(open), u8(close), body, ord("*"))
            got = run_model(texts, KWS, first_unit, piece, u8(open), u8(close), body, ord("*"))
            assert got[0] == want[0], (texts, body)
            assert got[1].tolist() == want[1].tolist(), (texts, body, bytes(got[1]), bytes(want[1]))
            assert got[2] == want[2], (texts, body)


def test_the_model_keeps_two_spans_at_a_seam_where_the_joined_text_has_one():
    for texts, kw in ((["xab", "abx"], "ab"), (["xé", "éx"], "é")):
        kws = [utf16(kw)]
        n = len(kw.encode())
        for piece in (1, 3, 16):
            triples, out, off = run_model(texts, kws, False, piece, u8(b""), u8(b""), "drop", 0)
            assert triples == [(0, 1, 1 + n), (1, 0, n)] and bytes(out) == b"xx" and off == [0, 1, 2]
            triples, out, off = run_model(texts, kws, False, piece, u8(b"<"), u8(b">"), "keep", 0)
            assert bytes(out) == ("x<%s><%s>x" % (kw, kw)).encode() and off == [0, 3 + n, 6 + 2 * n]
        joined = "".join(texts)
        assert len(run_model([joined], kws, False, 3, u8(b""), u8(b""), "drop", 0)[0]) == 1
    # a lone low surrogate against haystacks that end and begin with a 4-byte character: the widened records touch only in bytes
    triples, out, off = run_model(["a😀", "😀a"], [utf16("😀")[1:]], False, 2, u8(b"<"), u8(b">"), "fill", ord("#"))
    assert triples == [(0, 1, 5), (1, 0, 4)] and bytes(out) == b"a<####><####>a" and off == [0, 7, 14]


# ---- symbols ------------------------------------------------------------------------------------------------------------------
NAMES = ("acgpu_spans_batch_utf8", "acgpu_spans_batch_utf8_lossy", "acgpu_cover_batch_utf8", "acgpu_cover_batch_utf8_lossy")


def test_the_four_symbols_are_declared_and_exported():
    L = ctypes.CDLL(N.LIB_PATH)
    for name in NAMES:
        assert name in N.SYMBOLS and hasattr(L, name), name
    assert N.lib().acgpu_abi_version() == N.ABI_VERSION == 5
    u64, u32, vp_, P = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER
    assert N.SIGNATURES["acgpu_spans_batch_utf8"][1] == [vp_, vp_, vp_, u32, vp_, u64, P(u64), P(N.SpansStats), P(N.Utf8BatchStats)]
    assert N.SIGNATURES["acgpu_spans_batch_utf8_lossy"][1][-1] == P(N.Utf8LossyStats)
    assert N.SIGNATURES["acgpu_cover_batch_utf8"][1] == [vp_, vp_, vp_, u32, P(N.CoverSpec), vp_, u64, vp_, P(u64), P(N.CoverStats), P(N.Utf8BatchStats)]
    assert N.SIGNATURES["acgpu_cover_batch_utf8_lossy"][1][-1] == P(N.Utf8LossyStats)
    for name in ("spans_batch_utf8", "cover_batch_utf8", "cover_batch_bytes", "mask_batch_utf8", "highlight_batch_utf8", "redact_batch_utf8"):
        assert name in ahocorasick_amd.__all__ and callable(getattr(ahocorasick_amd, name)), name


# ---- decisions made before a device is looked for -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def auto():
    return Automaton(N.MODE_ALL, ["ab", "b"], True)


def _cover(name, auto, data, off, n, spec, out, cap, out_off, n_out=True, stats=True):
    no, st = ctypes.c_uint64(77), N.CoverStats()
    ust = N.UTF8_STATS[name]()
    rc = getattr(N.lib(), name)(auto.handle if auto is not None else None, data, off, n, ctypes.byref(spec) if spec is not None else None, out, cap,
                                out_off, ctypes.byref(no) if n_out else None, ctypes.byref(st) if stats else None, ctypes.byref(ust) if stats else None)
    return rc, no.value


def _spans(name, auto, data, off, n, out, cap, n_out=True, stats=True):
    no, st = ctypes.c_uint64(77), N.SpansStats()
    ust = N.UTF8_STATS[name]()
    rc = getattr(N.lib(), name)(auto.handle if auto is not None else None, data, off, n, out, cap, ctypes.byref(no) if n_out else None,
                                ctypes.byref(st) if stats else None, ctypes.byref(ust) if stats else None)
    return rc, no.value


@pytest.mark.parametrize("name", ["acgpu_cover_batch_utf8", "acgpu_cover_batch_utf8_lossy"])
def test_cover_batch_utf8_refuses_bad_arguments_without_a_device(auto, name):
    data, out = np.zeros(16, np.uint8), np.zeros(64, np.uint8)
    off, oo = np.array([0, 4, 4, 16], np.uint64), np.zeros(4, np.uint64)
    ok = spec_of(np.uint8, b"<", b">")
    E = N.E_INVALID
    cover = lambda *args, **kw: _cover(name, *args, **kw)[0]
    assert cover(None, vp(data), vp(off), 3, ok, vp(out), 64, vp(oo)) == E                    # no automaton
    assert cover(auto, vp(data), None, 3, ok, vp(out), 64, vp(oo)) == E                       # no offsets
    assert cover(auto, vp(data), vp(off), 3, ok, vp(out), 64, vp(oo), n_out=False) == E       # no n_out
    assert cover(auto, vp(data), vp(off), 3, None, vp(out), 64, vp(oo)) == E                  # no spec
    assert cover(auto, vp(data), vp(off), 3, ok, vp(out), 64, None) == E                      # no out_offsets
    assert cover(auto, vp(data), vp(off), 3, ok, None, 64, vp(oo)) == E                       # a capacity without a buffer
    assert cover(auto, None, vp(off), 3, ok, vp(out), 64, vp(oo)) == E                        # bytes without a pointer
    assert cover(auto, vp(data), vp(np.array([0, 5, 4, 16], np.uint64)), 3, ok, vp(out), 64, vp(oo)) == E  # descending offsets
    assert cover(auto, vp(data), vp(np.array([0, (1 << 31) - 1], np.uint64)), 1, ok, vp(out), 64, vp(oo)) == E  # 2^31 with the phantom
    assert cover(auto, vp(data), vp(np.array([0, 1 << 40], np.uint64)), 1, ok, vp(out), 64, vp(oo)) == E
    # everything check_spec refuses of a byte spec, before the offsets are looked at
    bad_off = vp(np.array([0, 5, 4, 16], np.uint64))
    assert cover(auto, vp(data), bad_off, 3, spec_of(np.uint8, body=3), vp(out), 64, vp(oo)) == E
    assert cover(auto, vp(data), vp(off), 3, spec_of(np.uint8, open_len=2), vp(out), 64, vp(oo)) == E
    assert cover(auto, vp(data), vp(off), 3, spec_of(np.uint8, close_len=1), vp(out), 64, vp(oo)) == E
    assert cover(auto, vp(data), vp(off), 3, spec_of(np.uint8, b"<", open_len=1 << 31), vp(out), 64, vp(oo)) == E
    assert cover(auto, vp(data), vp(off), 3, spec_of(np.uint8, body=N.COVER_FILL, fill=0x80), vp(out), 64, vp(oo)) == E  # fill is one ASCII byte
    assert cover(auto, vp(data), vp(off), 0, spec_of(np.uint8, body=3), vp(out), 64, vp(oo)) == E  # ... also for no haystacks


@pytest.mark.parametrize("name", ["acgpu_spans_batch_utf8", "acgpu_spans_batch_utf8_lossy"])
def test_spans_batch_utf8_refuses_bad_arguments_without_a_device(auto, name):
    data, out = np.zeros(16, np.uint8), np.zeros((64, 3), np.int32)
    off = np.array([0, 4, 4, 16], np.uint64)
    E = N.E_INVALID
    spans = lambda *args, **kw: _spans(name, *args, **kw)[0]
    assert spans(None, vp(data), vp(off), 3, vp(out), 64) == E
    assert spans(auto, vp(data), None, 3, vp(out), 64) == E
    assert spans(auto, vp(data), vp(off), 3, vp(out), 64, n_out=False) == E
    assert spans(auto, vp(data), vp(off), 3, None, 64) == E
    assert spans(auto, None, vp(off), 3, vp(out), 64) == E
    assert spans(auto, vp(data), vp(np.array([0, 5, 4, 16], np.uint64)), 3, vp(out), 64) == E
    assert spans(auto, vp(data), vp(np.array([0, (1 << 31) - 1], np.uint64)), 1, vp(out), 64) == E


@pytest.mark.parametrize("lossy", ["", "_lossy"])
def test_a_batch_without_a_byte_needs_no_device(auto, lossy):
    ok = spec_of(np.uint8, b"<", b">")
    for off in ([7], [7, 7], [3, 3, 3, 3, 3]):  # no haystack, one empty haystack, four (offsets[0] != 0)
        off = np.array(off, np.uint64)
        oo = np.full(len(off), 99, np.uint64)
        for stats in (True, False):  # the stats pointers may be NULL
            assert _cover("acgpu_cover_batch_utf8" + lossy, auto, None, vp(off), len(off) - 1, ok, None, 0, vp(oo), stats=stats) == (N.OK, 0)
            assert not oo.any()
            assert _spans("acgpu_spans_batch_utf8" + lossy, auto, None, vp(off), len(off) - 1, None, 0, stats=stats) == (N.OK, 0)
    errors = "replace" if lossy else "strict"
    assert S.spans_batch_utf8(auto, [], errors=errors).shape == (0, 3) and S.spans_batch_utf8(auto, [b"", b""], errors=errors).shape == (0, 3)
    assert C.cover_batch_utf8(auto, [], open="<", errors=errors) == [] and C.mask_batch_utf8(auto, [b"", bytearray()], errors=errors) == [b"", b""]
    out, out_off, st = C.cover_batch_bytes(auto, [b""], errors=errors)
    assert out.size == 0 and out.dtype == np.uint8 and out_off.tolist() == [0, 0] and st["units_out"] == 0
    assert C.redact_batch_utf8(auto, b"", "x", offsets=[0, 0, 0], errors=errors) == [b"", b""]


# ---- the wrappers, against the stub -------------------------------------------------------------------------------------------
def test_wrappers_refuse_bad_arguments_before_a_native_call(stub):
    a = automaton(stub)
    for call in (lambda: C.cover_batch_utf8(a, [b"xabx"], body="mask"), lambda: C.cover_batch_bytes(a, [b"xabx"], body=None),
                 lambda: C.mask_batch_utf8(a, [b"xabx"], fill=b"**"), lambda: C.mask_batch_utf8(a, [b"xabx"], fill=b""),
                 lambda: C.mask_batch_utf8(a, [b"xabx"], fill="é"), lambda: C.mask_batch_utf8(a, [b"xabx"], fill=b"\x80"),
                 lambda: C.cover_batch_utf8(a, [b"x"], errors="ignore"), lambda: S.spans_batch_utf8(a, [b"x"], errors="ignore"),
                 lambda: C.cover_batch_utf8(a, b"xabx", offsets=[]), lambda: S.spans_batch_utf8(a, b"xabx", offsets=[0, 9])):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: C.cover_batch_utf8(a, [b"x", None]), lambda: S.spans_batch_utf8(a, [None]), lambda: C.cover_batch_utf8(a, [b"x"], open=None),
                 lambda: C.cover_batch_utf8(a, [b"x"], close=None), lambda: C.mask_batch_utf8(a, [b"x"], fill=None),
                 lambda: C.redact_batch_utf8(a, [b"x"], None), lambda: C.highlight_batch_utf8(a, [b"x"], b"<", None)):
        with pytest.raises(TypeError):
            call()
    assert not [n for n, _ in stub.calls if "cover" in n or "spans" in n]


def _caps(stub, name, at):
    return [args[at] for n, args in stub.calls if n == name]


def test_cover_batch_bytes_retries_once_with_the_exact_size(stub):
    a = automaton(stub)
    name = "acgpu_cover_batch_utf8"
    datas = [bytes(range(1, 61)), b"", bytearray(range(1, 41))]
    stub.plan[name] = iter([(OVF, 9001), (N.OK, 9001)])
    out, out_off, st = C.cover_batch_bytes(a, datas, open="<b>", close=b"</b>")
    assert len(out) == 9001 and out.dtype == np.uint8 and len(out_off) == 4 and set(st) == {f for f, _ in N.CoverStats._fields_}
    assert _caps(stub, name, 6) == [100 + 25 + 3 + 4, 9001]  # the batch's bytes n: n + n // 4 + len(open) + len(close), then the reported size
    args = [args for n, args in stub.calls if n == name][0]
    assert args[0] == a.handle and args[3] == 3 and (args[4]._obj.open_len, args[4]._obj.close_len, args[4]._obj.body) == (3, 4, N.COVER_KEEP)
    assert isinstance(args[10]._obj, N.Utf8BatchStats)
    stub.calls.clear()
    stub.plan[name] = iter([(OVF, 5000), (OVF, 5001), (N.OK, 5001)])
    with pytest.raises(N.AcgpuError) as e:
        C.cover_batch_bytes(a, datas)
    assert e.value.code == OVF and _caps(stub, name, 6) == [125, 5000]  # a second overflow is an error, not a third call
    stub.calls.clear()
    stub.plan[name + "_lossy"] = iter([(OVF, 700), (N.OK, 700)])
    assert len(C.cover_batch_bytes(a, datas, cap=16, errors="replace")[0]) == 700 and _caps(stub, name + "_lossy", 6) == [16, 700]
    assert isinstance([args for n, args in stub.calls if n == name + "_lossy"][0][10]._obj, N.Utf8LossyStats)


def test_spans_batch_utf8_retries_once_and_takes_one_buffer_in_place(stub):
    a = automaton(stub)
    name = "acgpu_spans_batch_utf8"
    stub.plan[name] = iter([(OVF, 9001), (N.OK, 9001)])
    got = S.spans_batch_utf8(a, [b"xab", b"", memoryview(b"cd")])
    assert got.shape == (9001, 3) and got.dtype == np.int32 and _caps(stub, name, 5) == [4096, 9001]
    stub.calls.clear()
    stub.plan[name] = iter([(OVF, 5000), (OVF, 5001)])
    with pytest.raises(N.AcgpuError) as e:
        S.spans_batch_utf8(a, [b"xab"])
    assert e.value.code == OVF and _caps(stub, name, 5) == [4096, 5000]
    stub.calls.clear()
    buf = np.frombuffer(b"one\ntwo\n\nlast", np.uint8)
    S.spans_batch_utf8(a, buf, offsets=utf8_line_offsets(buf))
    args = [args for n, args in stub.calls if n == name][0]
    assert args[1].value == buf.ctypes.data and args[3] == 4  # the buffer in place, a haystack per line


def test_an_ill_formed_haystack_raises_utf8_error_with_its_place(stub):
    a = automaton(stub)
    for name, call in (("acgpu_cover_batch_utf8", lambda: C.cover_batch_utf8(a, [b"x", b"\xff"])), ("acgpu_spans_batch_utf8", lambda: S.spans_batch_utf8(a, [b"x", b"\xff"])),
                       ("acgpu_cover_batch_utf8", lambda: C.mask_batch_utf8(a, [b"x", b"\xff"]))):
        stub.plan[name] = iter([(N.E_ENCODING, 0)])
        with pytest.raises(Utf8Error) as e:
            call()
        assert (e.value.haystack, e.value.start) == (BAD_HAYSTACK, FIRST_BAD)


def test_thin_wrappers_pass_the_spec_of_their_use(stub):
    s = AhoCorasickSet(["ab", "b"], True)
    stub.objects.append(s.automaton)

    def last_spec(name="acgpu_cover_batch_utf8"):
        args = [args for n, args in stub.calls if n == name][-1]
        assert args[0] == s.automaton.handle and args[3] == 2
        sp = args[4]._obj
        return sp.open_len, sp.close_len, sp.body, sp.fill

    assert C.mask_batch_utf8(s, [b"xabx", b""], fill="#") == [b"", b""]  # (the stub writes nothing: every result is empty)
    assert last_spec() == (0, 0, N.COVER_FILL, ord("#"))
    C.highlight_batch_utf8(s, [b"xabx", b""], "<b>", b"</b>")
    assert last_spec()[:3] == (3, 4, N.COVER_KEEP)
    C.redact_batch_utf8(s, b"xabx", "é😀", offsets=[0, 4, 4], errors="replace")
    assert last_spec("acgpu_cover_batch_utf8_lossy")[:3] == (6, 0, N.COVER_DROP)  # a str is encoded as UTF-8: in bytes
