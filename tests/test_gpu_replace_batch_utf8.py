"""GPU tests of the UTF-8 batch replace entry (include/acgpu.h: acgpu_replace_batch_utf8; csrc/acgpu_replace.hip:
k_replace_span_offsets behind the unchanged plan and byte emit, csrc/acgpu_utf8.hip: k_utf8_batch_map over a piece's records and
k_utf8_batch_pos for its boundary).  The expected result of haystack i is never the library's own output: it is the Python splice,
over the haystack's BYTES, of the CPU oracle's Map records on the haystack decoded alone, mapped to byte offsets by the header's
rule restated over the code points (records / splice_bytes of tests/test_gpu_replace_utf8.py).  Equality is exact: the bytes,
every entry of out_offsets, *n_out and st.n_records.  Every call writes into a buffer with a canary behind its capacity."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import (Automaton, LongestMatchMap, LongestMatchSet, ShortestMatchSet, Utf8Error, WholeWordLongestMatchSet,
                                     WholeWordMatchSet, utf8_line_offsets)
from ahocorasick_amd.unicode_tables import word_chars_from_list
from oracle.oracle import Oracle
from tests.helpers import LOWER
from tests.test_gpu_replace_utf8 import MODES, WORDY, mixed_replacements, mixed_text, pair, records, splice_bytes
from tests.test_gpu_utf8_batch import cpython_first, cut_up, keywords

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20),
            ("replace_slab_units", 1 << 25)]
SETS = {N.MODE_LONGEST: LongestMatchSet, N.MODE_SHORTEST: ShortestMatchSet, N.MODE_WHOLEWORD: WholeWordMatchSet,
        N.MODE_WWLONGEST: WholeWordLongestMatchSet}
CANARY = 0xA5
OFF_CANARY = 0x7777777777777777
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


# ---- the expectation: per haystack, the oracle's records in bytes spliced over the haystack's bytes ---------------------------------
def expected(orc, datas, repls, cache=None):
    """-> (the expected result of every haystack, the records of all of them).  cache: {(haystack bytes) -> byte records}, for
    batches that repeat a few haystacks"""
    per, n_recs = [], 0
    for d in datas:
        d = bytes(d)
        if not d:
            per.append(b"")
            continue
        brecs = cache.get(d) if cache is not None else None
        if brecs is None:
            brecs = records(orc, d.decode("utf-8"))[1]
            if cache is not None:
                cache[d] = brecs
        per.append(splice_bytes(d, brecs, repls))
        n_recs += len(brecs)
    return per, n_recs


def raw(a, datas, repls, cap, room=None, null_out=False):
    """one acgpu_replace_batch_utf8 call into a canary-filled buffer -> (rc, n_out, the buffer, out_offsets, stats dict, Utf8BatchStats)"""
    buf = np.frombuffer(b"".join(bytes(d) for d in datas) or b"\0", np.uint8)
    off = np.cumsum([0] + [len(d) for d in datas], dtype=np.uint64)
    r_bytes, r_off, n_repl = a._replacements_utf8(repls)
    out = np.full((cap if room is None else room) + 64, CANARY, np.uint8)
    oo = np.full(len(datas) + 1, OFF_CANARY, np.uint64)
    n_out = ctypes.c_uint64(12345)
    st, ust = N.ReplaceStats(), N.Utf8BatchStats(7, 7, 7, 7)
    rc = N.lib().acgpu_replace_batch_utf8(a.handle, vp(buf), vp(off), len(datas), vp(r_bytes), vp(r_off), n_repl, None if null_out else vp(out), cap,
                                          vp(oo), ctypes.byref(n_out), ctypes.byref(st), ctypes.byref(ust))
    return rc, int(n_out.value), out, oo, {f: int(getattr(st, f)) for f, _ in N.ReplaceStats._fields_}, ust


def offsets_of(per):
    return np.cumsum([0] + [len(p) for p in per]).astype(np.uint64)


def check(a, orc, datas, repls, cache=None):
    """the entry, at exactly the capacity the result needs, against the splices -> (per-haystack results, stats dict, Utf8BatchStats)"""
    per, n_recs = expected(orc, datas, repls, cache)
    whole, woff = b"".join(per), offsets_of(per)
    rc, n_out, out, oo, st, ust = raw(a, datas, repls, len(whole))
    assert rc == N.OK and n_out == len(whole), (rc, n_out, len(whole))
    bad = np.flatnonzero(oo != woff)
    assert not len(bad), ("out_offsets", bad[:5], oo[bad[:5]], woff[bad[:5]])
    got = out[:n_out].tobytes()
    if got != whole:
        i = next(j for j in range(len(whole)) if got[j] != whole[j])
        h = int(np.searchsorted(woff, i, side="right")) - 1
        raise AssertionError("byte %d of %d (haystack %d) differs: %r, want %r" % (i, len(whole), h, got[max(0, i - 8):i + 24], whole[max(0, i - 8):i + 24]))
    assert (out[n_out:] == CANARY).all(), "written at or beyond cap"
    assert st["n_records"] == n_recs and st["units_out"] == len(whole), (st, n_recs)
    n_bytes = sum(len(d) for d in datas)
    n_units = sum(len(bytes(d).decode("utf-8").encode("utf-16-le")) // 2 for d in datas)
    assert (ust.n_units, ust.first_bad, ust.bad_haystack, ust.ascii) == (n_units, -1, 0, int(n_units == n_bytes)), (n_units, n_bytes)
    return per, st, ust


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [True, False])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_parity_with_every_haystack_rewritten_alone(mode, cs):
    rng = np.random.default_rng(8000 + 10 * mode + cs)
    text = mixed_text(rng, 12000)
    kws = keywords(rng, text, mode, cs)
    a, orc = pair(mode, kws, cs)
    datas = cut_up(rng, text, 20, 100, 8)
    k = max((w for w in kws if len(w) >= 2 and " " not in w), key=len)
    # empty haystacks at the start, in the middle and at the end; a keyword at a haystack's first and last bytes; a keyword cut in
    # two by a haystack boundary, which would match only if the two haystacks were joined
    mid = len(datas) // 2
    datas = [b"", b""] + datas[:mid] + [b"", (k + " · " + k).encode(), k[:1].encode(), k[1:].encode(), b"", b""] + datas[mid:] + [k.encode(), b"", b""]
    assert 150 <= len(datas) <= 400 and sum(1 for d in datas if not d) >= 10
    assert {1, 2, 3, 4} <= {len(c.encode()) for c in text}
    cache = {}
    repls = mixed_replacements(kws)
    per, st, ust = check(a, orc, datas, repls, cache)
    assert ust.ascii == 0 and st["n_records"] >= 100
    firsts = [i for i, d in enumerate(datas) if d and len(cache[bytes(d)]) and cache[bytes(d)][0, 0] == 0]
    lasts = [i for i, d in enumerate(datas) if d and len(cache[bytes(d)]) and cache[bytes(d)][-1, 1] == len(d)]
    assert firsts and lasts  # matches at a haystack's first and at its last byte
    joined = records(orc, k)[1]
    assert len(joined) and joined[0, 1] - joined[0, 0] > len(k[:1].encode())  # the cut keyword matches across the cut when joined
    check(a, orc, datas, "[redacted]", cache)
    check(a, orc, datas, ["" for _ in kws], cache)
    # the facade, against one replace_utf8 call per haystack
    x = SETS[mode](kws, cs)
    for r in ("«*»", b""):
        assert x.replace_batch_utf8(datas, r) == [x.replace_utf8(h, r) for h in datas]
    buf = b"".join(datas)
    off = np.cumsum([0] + [len(d) for d in datas], dtype=np.uint64)
    assert x.replace_batch_utf8(buf, "«*»", offsets=off) == x.replace_batch_utf8(datas, "«*»")


# ---- 2. an all-ASCII batch: no checkpoints, but the records still stand h separators behind their bytes ---------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_ascii_batch_with_matches_behind_the_first_haystack(mode):
    rng = np.random.default_rng(21)
    kws = ["ab", "abc", "q", "dd", "cab"]
    a, orc = pair(mode, kws)
    datas = ["".join(" abcdq,"[int(i)] for i in rng.integers(0, 7, int(ln))).encode() for ln in rng.integers(0, 50, 300)]
    datas = [b"zzz", b"ab", b"", b"q"] + datas
    for repls in (["<1>", "", "QQQQQQQQQQQQQQQQQ", "é", "x"], "#"):
        per, st, ust = check(a, orc, datas, repls)
        assert ust.ascii == 1 and st["n_records"] > 100
    assert per[1] == b"#" and per[3] == b"#"
    N.set_tunable("cursor_first_piece", 64)
    N.set_tunable("cursor_max_piece", 256)
    per, st, ust = check(a, orc, datas, ["<1>", "", "QQQQQQQQQQQQQQQQQ", "é", "x"])
    assert ust.ascii == 1 and st["pieces"] > 8


# ---- 3. many pieces: a boundary at every phase of a period of 21 units ----------------------------------------------------------------
GROUP = ["😀é 😀kw", "", "", "", "kw😀kw", "é"]  # 8 + 0 + 0 + 0 + 6 + 1 units, and a separator behind each: 21 units of the scan's text
N_GROUPS = 149
MANY = {N.MODE_LONGEST: ["kw", "😀é", "é 😀k"], N.MODE_SHORTEST: ["kw", "😀é", "é 😀k", "w😀kw"], N.MODE_WHOLEWORD: ["kw", "é"],
        N.MODE_WWLONGEST: ["kw", "é", "kw😀kw"]}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_many_pieces_with_a_boundary_at_every_phase(mode):
    """Pieces of 64, then 256 units: the boundaries stand at units 64 + 256 k of the scan's text.  A first haystack of p ASCII
    bytes, p = 0 .. 20, moves the period of 21 units under them, so that a boundary falls on every unit of the period: on a
    separator, between the two units of a surrogate pair, inside a match, inside the run of three empty haystacks -- and for
    p = 7 on the batch's last separator (7 + 1 + 21 * 149 - 1 = 64 + 256 * 12).  SHORTEST: its boundary stands max_len - 1 units
    earlier, and max_len (5 units) is longer than some haystacks."""
    N.set_tunable("cursor_first_piece", 64)
    N.set_tunable("cursor_max_piece", 256)
    a, orc = pair(mode, MANY[mode])
    group = [g.encode() for g in GROUP]
    repls = [["<kw>", "", "€€€", "r"][i % 4] for i in range(len(MANY[mode]))]
    cache = {}
    for p in range(21):
        datas = [b"a" * p] + group * N_GROUPS
        total = p + 1 + 21 * N_GROUPS  # units of the scan's text
        per, st, _ = check(a, orc, datas, repls, cache)
        assert st["pieces"] > 8 and st["n_records"] >= 3 * N_GROUPS, st
        assert st["pieces"] == 1 + -(-(total - 64) // 256) and st["rescans"] == 0, (p, st)
    assert (7 + 1 + 21 * N_GROUPS - 1 - 64) % 256 == 0
    check(a, orc, [b"a" * 7] + group * N_GROUPS, "", cache)


# ---- 4. runs of empty haystacks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_len", [1, 63, 64, 65, 5000])
def test_runs_of_empty_haystacks(run_len):
    a, orc = pair(N.MODE_LONGEST, ["kw", "é€"])
    datas = ["xkwé€".encode()] + [b""] * run_len + ["kwyé€kw".encode()] + [b""] * run_len
    repls = ["<keyword>", ""]
    for pieces in (False, True):
        if pieces:
            N.set_tunable("cursor_first_piece", 64)
            N.set_tunable("cursor_max_piece", 256)
        rc, n_out, out, oo, st, _ = raw(a, datas, repls, 64)
        assert rc == N.OK and out[:n_out].tobytes() == b"x<keyword><keyword>y<keyword>" and st["n_records"] == 5
        assert oo[0] == 0 and (oo[1:run_len + 2] == 10).all() and (oo[run_len + 2:] == n_out).all()  # every offset of a run equals its neighbours
        check(a, orc, datas, repls)
        check(a, orc, [b""] * run_len + datas, repls)


# ---- 5. alignment: a haystack boundary at every offset of the 16-byte grid, results across slab seams -----------------------------------
def sized_haystack(n_bytes, phase):
    """well-formed text of exactly n_bytes bytes with matches of "kw" and "é€" in it, sequences of every length"""
    unit = ["kw", "é€", "😀", "ab", "kw", "€"]
    s, i = b"", phase
    while True:
        nxt = unit[i % len(unit)].encode()
        if len(s) + len(nxt) > n_bytes:
            break
        s += nxt
        i += 1
    return s + b"x" * (n_bytes - len(s))


def test_every_alignment_of_source_and_destination():
    N.set_tunable("replace_slab_units", 1000)
    a, orc = pair(N.MODE_LONGEST, ["kw", "é€"])
    lengths = list(range(41))
    orders = [lengths, lengths[::-1], lengths[20:] + lengths[:20], lengths[::2] + lengths[1::2], lengths[::3] + lengths[1::3] + lengths[2::3]]
    base = [sized_haystack(ln, k) for k, order in enumerate(orders) for ln in order]
    cache = {}
    starts = set()
    for shift in range(16):
        datas = [b"x" * shift] + base
        starts |= {int(o) % 16 for o in np.cumsum([len(d) for d in datas])}
        for repls in (["<keyword>", ""], ["", "ß"], ["0123456789abcdefg", "€"]):
            per, st, _ = check(a, orc, datas, repls, cache)
        assert len(b"".join(per)) >= 3000  # several slabs of 1000 bytes (1008: whole vectors)
    assert starts == set(range(16))


# ---- 6. more records than the emit's LDS holds for one tile ------------------------------------------------------------------------------
def test_thousands_of_deleted_one_byte_matches_over_many_haystacks():
    a, orc = pair(N.MODE_LONGEST, ["q", "é"])
    datas = [b"q" * (i % 41) for i in range(200)] + [b"x"] + [b"q" * (40 - i % 41) for i in range(200)] + [b"yq"]
    assert sum(len(d) for d in datas) > 7000
    cache = {}
    per, st, ust = check(a, orc, datas, "", cache)
    assert b"".join(per) == b"xy" and st["n_records"] > 7000 and ust.ascii == 1
    per, st, _ = check(a, orc, datas, ["", "e"], cache)
    assert b"".join(per) == b"xy"
    mixed = [d + "é".encode() * (i % 3) for i, d in enumerate(datas)]  # the same through the checkpoints
    per, st, ust = check(a, orc, mixed, "", cache)
    assert b"".join(per) == b"xy" and ust.ascii == 0
    check(a, orc, mixed, ["", "e"], cache)


# ---- 7. ill-formed input -----------------------------------------------------------------------------------------------------------------
def refused(a, datas):
    """the raw call on an ill-formed batch -> (bad_haystack, first_bad); out and out_offsets[1..] keep their canary"""
    rc, n_out, out, oo, st, ust = raw(a, datas, "#", 64, room=sum(len(d) for d in datas) + 64)
    assert rc == N.E_ENCODING and n_out == 0 and (out == CANARY).all() and (oo[1:] == OFF_CANARY).all()
    assert (ust.n_units, ust.ascii) == (0, 0) and st["n_records"] == 0
    return ust.bad_haystack, ust.first_bad


GOOD = ["kw😀 é€".encode(), b"", "ab€😀kw".encode()]


def test_ill_formed_haystacks_are_refused_where_cpython_fails_and_the_pool_stays_usable():
    a, orc = pair(N.MODE_LONGEST, ["kw", "é€"])
    assert refused(a, [b"a\xc3", b"\xa9b"]) == (0, 1)  # the buffer as a whole is valid
    check(a, orc, GOOD, ["<kw>", ""])
    check(a, orc, [b"a", b"\xc3\xa9b"], "#")
    text = mixed_text(np.random.default_rng(66), 3000).encode()
    for seed in range(5):
        rng = np.random.default_rng(700 + seed)
        cuts = np.sort(rng.integers(0, len(text) + 1, 150)).tolist()
        off = [0] + cuts + [len(text)]
        datas = [text[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        want = cpython_first(datas)
        assert want is not None, seed
        assert refused(a, datas) == want, (seed, want)
        check(a, orc, GOOD, ["<kw>", ""])  # the next call on the same automaton is right
    with pytest.raises(Utf8Error) as e:
        a.replace_batch_utf8(datas, "#")
    assert (e.value.haystack, e.value.start) == want
    with pytest.raises(Utf8Error) as e:
        LongestMatchSet(["kw"], True).replace_batch_utf8([b"ok", b"", b"abc\xed\xa0\x80"], "#")
    assert (e.value.haystack, e.value.start) == (2, 3)


# ---- 8. capacity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slab", [None, 1000])
def test_overflow_reports_exact_sizes_and_offsets_and_writes_nothing_beyond_cap(slab):
    if slab:
        N.set_tunable("replace_slab_units", slab)
        N.set_tunable("cursor_first_piece", 64)
        N.set_tunable("cursor_max_piece", 256)
    a, orc = pair(N.MODE_LONGEST, ["kw", "é€"])
    datas = [("aé€😀kw" * (i % 7)).encode() for i in range(150)]
    repls = ["<keyword>", "€"]
    per, st, _ = check(a, orc, datas, repls)  # cap == need: exact
    whole, woff = b"".join(per), offsets_of(per)
    need = len(whole)
    assert need > sum(len(d) for d in datas) > 3000
    for cap in (0, 1, need // 2, need - 1):
        rc, n_out, out, oo, st2, _ = raw(a, datas, repls, cap, room=need + 100)
        assert rc == N.E_OVERFLOW and n_out == need == st2["units_out"] and st2["n_records"] == st["n_records"], (cap, rc, n_out)
        assert (oo == woff).all(), cap
        assert out[:cap].tobytes() == whole[:cap] and (out[cap:] == CANARY).all(), cap
    rc, n_out, out, oo, st2, _ = raw(a, datas, repls, 0, null_out=True)  # no buffer at all: the call counts
    assert rc == N.E_OVERFLOW and n_out == need and (oo == woff).all()
    got, out_off, st3 = a.replace_batch_utf8(datas, repls, cap=1)  # the wrapper's retry
    assert got.tobytes() == whole and (out_off == woff).all() and st3["units_out"] == need


# ---- 9. where the library goes haystack by haystack --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", WORDY)
def test_fallback_word_table_that_is_not_fold_consistent(mode):
    rng = np.random.default_rng(9)
    alpha = "abxyABXY ,éÉ"
    wc = word_chars_from_list("abcdxyABCDéÉ")  # X, Y are not word characters although x, y are
    kws = ["".join(alpha[int(i)] for i in rng.integers(0, 4, int(rng.integers(1, 5)))) for _ in range(24)] + ["é", "aé"]
    kws += [kws[2]]
    a, orc = Automaton(mode, kws, False, word_chars=wc), Oracle(MODES[mode], kws, False, LOWER, wc, map_flavour=True)
    assert a.info()["fold_consistent"] == 0
    datas = ["".join(alpha[int(i)] for i in rng.integers(0, len(alpha), int(ln))).encode() for ln in (0, 1, 40, 300, 7, 0, 120, 3, 12, 60, 0, 25)]
    cache = {}
    per, st, _ = check(a, orc, datas, mixed_replacements(kws), cache)
    assert st["n_records"] > 5 and per != [bytes(d) for d in datas]
    check(a, orc, datas, "#", cache)
    # an ill-formed haystack late in the batch: the whole batch is refused before anything is written
    assert refused(a, datas + [b"ab", "é".encode()[:1], "é".encode()[1:]]) == (len(datas) + 1, 0)
    check(a, orc, datas, "", cache)


def test_fallback_dictionary_without_a_free_unit_and_without_a_lone_surrogate():
    """every BMP unit that is no surrogate as a keyword of its own, and 1024 pairs that use every surrogate once: all 65536 units
    stand in a keyword, so no unit is free to separate haystacks, and no keyword holds an unpaired surrogate"""
    kws = [np.array([u], dtype=np.uint16) for u in range(65536) if not 0xD800 <= u < 0xE000]
    kws += [np.array([0xD800 + k, 0xDC00 + k], dtype=np.uint16) for k in range(1024)]
    a, orc = pair(N.MODE_LONGEST, kws)
    pairs = "".join(chr(0x10000 + (k << 10) + k) for k in (0, 1, 700, 1023))
    datas = [t.encode() for t in ["ab", "é", "", "zéa", pairs, "ü" * 9, "", "a", "ÿ€", "abcd" + pairs[:1], "ñ" * 70, "", "éé"]]
    cache = {}
    per, st, ust = check(a, orc, datas, "#", cache)
    n_cp = sum(len(d.decode()) for d in datas)
    assert st["n_records"] == n_cp and b"".join(per) == b"#" * n_cp
    assert st["pieces"] == sum(1 for d in datas if d)  # a text per haystack
    per, st, ust = check(a, orc, [b"ab", b"", b"xyz"], "é", cache)
    assert ust.ascii == 1 and per == ["éé".encode(), b"", "ééé".encode()]
    assert refused(a, datas + [b"ab", b"", b"a\xc3", b"\xa9b"]) == (len(datas) + 2, 1)
    check(a, orc, datas, "", cache)


# ---- 10. the stream rule -------------------------------------------------------------------------------------------------------------------
def test_tickets_in_flight_refuse_the_call():
    import torch
    from ahocorasick_amd.strings import utf16
    a, orc = pair(N.MODE_WHOLEWORD, ["kw", "aé"])  # (a family whose ticket is enqueued, not run to its end inside _begin)
    text = "aé € 😀 kw " * 2000
    hay = utf16(text)
    d_hay = torch.from_numpy(hay.view(np.int16)).cuda()
    d_recs = torch.empty((hay.size, 3), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    tk, rc = a.match_device_begin(d_hay.data_ptr(), hay.size, True, d_recs.data_ptr(), hay.size, stream=stream.cuda_stream)
    assert rc == N.OK
    datas = ["aé € 😀 kw ".encode()] * 50
    rc, n_out, out, oo, st, ust = raw(a, datas, "#", 64)
    assert rc == N.E_INVALID and n_out == 0 and (out == CANARY).all() and (oo[1:] == OFF_CANARY).all()
    assert ust.first_bad == -1 and st["n_records"] == 0
    m, rc, _ = a.match_device_end(tk)
    assert rc == N.OK and m == 2 * 2000
    check(a, orc, datas, ["<kw>", ""])


# ---- 11. the facade -------------------------------------------------------------------------------------------------------------------------
def test_the_facade_rewrites_a_buffer_line_by_line():
    buf = "Grüße aus Köln\n\ngrüße, KÖLN\nnichts\nköln".encode()
    s = WholeWordMatchSet(["grüße", "köln"], False)
    lines = buf.splitlines(keepends=True)
    got = s.replace_batch_utf8(buf, "***", offsets=utf8_line_offsets(buf))
    assert got == [b"*** aus ***\n", b"\n", b"***, ***\n", b"nichts\n", b"***"] and b"".join(got) == s.replace_utf8(buf, "***")
    assert s.replace_batch_utf8(lines, b"\xe2\x82\xac") == [s.replace_utf8(ln, "€") for ln in lines]
    assert s.replace_batch_utf8([memoryview(buf), bytearray(b""), np.frombuffer(lines[2], np.uint8)], "") == [b" aus \n\n, \nnichts\n", b"", b", \n"]
    m = LongestMatchMap(["grüße", "köln"], ["<G>", "<K>"], False)
    assert m.replace_batch_utf8(lines) == [m.replace_utf8(ln) for ln in lines] == [m.replace(ln.decode()).encode() for ln in lines]
    assert m.replace_batch_utf8(lines, ["ö", b""]) == [m.replace_utf8(ln, ["ö", b""]) for ln in lines]
    assert m.replace_batch_utf8(buf, "#", offsets=utf8_line_offsets(buf)) == m.replace_batch_utf8(lines, b"#")
