"""GPU tests of lossy replace (include/acgpu.h: acgpu_replace_utf8_lossy, acgpu_replace_batch_utf8_lossy; csrc/acgpu_replace.hip:
replace_utf8<P>, replace_batch_utf8<P>; csrc/acgpu_utf8.hip: the lossy form of k_utf8_batch_pos).  Every expected result is the
Python splice, over the caller's ORIGINAL bytes, of the CPU oracle's records on the text that tests/utf8_lossy_ref.py decodes, mapped
to bytes through that decoder's per-unit table (lossy_records and splice, checked in tests/test_utf8_lossy_more_cpu.py): outside the
matches the bytes stay as they are, ill-formed ones included.  Equality is exact -- content, n_out, st.n_records, the lossy stats --
and every call writes into a buffer with a canary behind its capacity."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, LongestMatchMap, LongestMatchSet, Utf8Error, WholeWordMatchMap
from ahocorasick_amd.unicode_tables import word_chars_from_list
from oracle.oracle import Oracle
from tests.helpers import LOWER
from tests.test_gpu_replace_utf8 import DEFAULTS, MODES, WORDY, keywords_from, mixed_text, pair
from tests.test_gpu_utf8_lossy import fuzz_keywords
from tests.test_utf8_lossy_more_cpu import lossy_records, splice
from tests.utf8_lossy_ref import TABLE, damaged, decode_replace

pytestmark = pytest.mark.gpu

BLOCK = 4096  # bytes per workgroup of the transcoder (16 per lane, 1024 per wave), and output bytes per workgroup of the emit
CANARY = 0xA5
ROWS = [row for row, _ in TABLE]
ASTRAL = "😀".encode()
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def small_pieces():
    """the pieces of the replace driver at 64 .. 256 units: a text of a few KB has dozens of piece boundaries"""
    N.set_tunable("cursor_first_piece", 64)
    N.set_tunable("cursor_max_piece", 256)


def min_pieces(*datas):
    """under small_pieces() no piece owns more than 256 units of the scan's text"""
    return sum(len(decode_replace(d)[1]) for d in datas) // 256


def as_bytes(r):
    return r.encode("utf-8") if isinstance(r, str) else bytes(r)


def table_of(repls):
    return [as_bytes(r) for r in repls] if isinstance(repls, list) else as_bytes(repls)


def want_stats(datas):
    """the lossy stats of the haystacks decoded alone: (n_units, n_replaced, first_replaced, first_haystack, ascii)"""
    tabs = [decode_replace(d) for d in datas]
    hit = [i for i, t in enumerate(tabs) if t[3].any()]
    first = int(tabs[hit[0]][1][tabs[hit[0]][3]][0]) if hit else -1
    return (sum(len(t[1]) for t in tabs), sum(int(t[3].sum()) for t in tabs), first, hit[0] if hit else 0,
            int(all(max(bytes(d), default=0) < 0x80 for d in datas)))


def fields(ust):
    return (ust.n_units, ust.n_replaced, ust.first_replaced, ust.first_haystack, ust.ascii)


def raw(a, data, repls, cap, room=None, null_out=False):
    """one acgpu_replace_utf8_lossy call into a canary-filled buffer -> (rc, n_out, the buffer, replace stats dict, lossy stats)"""
    arr = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
    r_bytes, off, n_repl = a._replacements_utf8(repls)
    out = np.full((cap if room is None else room) + 64, CANARY, np.uint8)
    n_out = ctypes.c_uint64(12345)
    st, ust = N.ReplaceStats(), N.Utf8LossyStats(7, 7, 7, 7, 7)
    rc = N.lib().acgpu_replace_utf8_lossy(a.handle, vp(arr), len(data), vp(r_bytes), vp(off), n_repl, None if null_out else vp(out), cap,
                                          ctypes.byref(n_out), ctypes.byref(st), ctypes.byref(ust))
    return rc, int(n_out.value), out, {f: int(getattr(st, f)) for f, _ in N.ReplaceStats._fields_}, ust


def raw_batch(a, datas, repls, cap, room=None, null_out=False):
    """one acgpu_replace_batch_utf8_lossy call -> (rc, n_out, the buffer, out_offsets, replace stats dict, lossy stats)"""
    buf = b"".join(datas)
    arr = np.frombuffer(buf, np.uint8) if buf else np.zeros(1, np.uint8)
    off = np.cumsum([0] + [len(d) for d in datas], dtype=np.uint64)
    r_bytes, r_off, n_repl = a._replacements_utf8(repls)
    out = np.full((cap if room is None else room) + 64, CANARY, np.uint8)
    out_off = np.full(len(datas) + 1, 77, np.uint64)
    n_out = ctypes.c_uint64(12345)
    st, ust = N.ReplaceStats(), N.Utf8LossyStats(7, 7, 7, 7, 7)
    rc = N.lib().acgpu_replace_batch_utf8_lossy(a.handle, vp(arr), vp(off), len(datas), vp(r_bytes), vp(r_off), n_repl, None if null_out else vp(out),
                                                cap, vp(out_off), ctypes.byref(n_out), ctypes.byref(st), ctypes.byref(ust))
    return rc, int(n_out.value), out, out_off, {f: int(getattr(st, f)) for f, _ in N.ReplaceStats._fields_}, ust


def differ(got, want):
    i = next((j for j in range(min(len(got), len(want))) if got[j] != want[j]), min(len(got), len(want)))
    return "byte %d of %d / %d differs: %r, want %r" % (i, len(got), len(want), got[max(0, i - 8):i + 24], want[max(0, i - 8):i + 24])


def check(a, orc, data, repls):
    """the text entry at exactly the capacity the result needs, against the splice -> (expected bytes, byte records, replace stats)"""
    brecs = lossy_records(orc, data)
    want = splice(data, brecs, table_of(repls))
    rc, n_out, out, st, ust = raw(a, data, repls, len(want))
    assert rc == N.OK and n_out == len(want), (rc, n_out, len(want))
    got = out[:n_out].tobytes()
    assert got == want, differ(got, want)
    assert (out[n_out:] == CANARY).all(), "written at or beyond cap"
    assert st["n_records"] == len(brecs) and st["units_out"] == len(want), st
    assert fields(ust) == (want_stats([data]) if len(data) else (0, 0, -1, 0, 1))
    return want, brecs, st


def check_batch(a, orc, datas, repls):
    """the batch entry against every haystack spliced alone -> (the expected results, replace stats)"""
    per_recs = [lossy_records(orc, d) for d in datas]
    per = [splice(d, r, table_of(repls)) for d, r in zip(datas, per_recs)]
    whole = b"".join(per)
    woff = np.cumsum([0] + [len(p) for p in per], dtype=np.uint64)
    rc, n_out, out, out_off, st, ust = raw_batch(a, datas, repls, len(whole))
    assert rc == N.OK and n_out == len(whole), (rc, n_out, len(whole))
    assert (out_off == woff).all(), (out_off[:8], woff[:8])
    got = out[:n_out].tobytes()
    assert got == whole, differ(got, whole)
    assert (out[n_out:] == CANARY).all(), "written at or beyond cap"
    assert st["n_records"] == sum(len(r) for r in per_recs) and st["units_out"] == len(whole), st
    assert fields(ust) == (want_stats(datas) if any(len(d) for d in datas) else (0, 0, -1, 0, 1))
    return per, st


def touching(data, brecs):
    """the records that cover or abut a replaced subpart"""
    _, off, length, replaced = decode_replace(data)
    edge = np.zeros(len(data) + 2, bool)
    for o, n in zip(off[replaced].tolist(), length[replaced].tolist()):
        edge[o + 1:o + n + 1] = True
    return sum(1 for s, e, _ in brecs.tolist() if edge[s:e + 2].any())


def family(mode, cs=True):
    """(automaton, oracle, keywords) of one of the four families, with keywords that hold U+FFFD where a family can match them"""
    valid = mixed_text(np.random.default_rng(77), 1500)
    kws = fuzz_keywords(mode, cs, valid)
    a, orc = pair(mode, kws, cs)
    return a, orc, kws, valid


def mixed_replacements(kws):
    """one replacement per keyword: str and bytes, longer and shorter than the keyword, empty ones, ill-formed bytes"""
    pool = ["", "#", "<<é>>", b"\xff", b"", "😀!", b"[\xe2\x82]", "long replacement, longer than any keyword"]
    return [pool[i % len(pool)] for i in range(len(kws))]


# ---- 1. the table, in a text and in a batch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_row_of_the_table_in_a_text_and_in_a_batch(mode):
    a, orc, kws, valid = family(mode)
    head, mid = valid[:300].encode(), valid[300:420].encode()
    cases = [c for row in ROWS for c in (row, b"A" + row + b"A(", head + row + mid, ASTRAL + row + ASTRAL, head + b" A" + row)]
    n_touch = n_recs = 0
    for repls in (mixed_replacements(kws), "#", b"\xc0\x80", ""):
        for data in cases:
            want, brecs, st = check(a, orc, data, repls)
            n_touch += touching(data, brecs)
            n_recs += len(brecs)
        check_batch(a, orc, cases, repls)
    assert n_recs > 100 and (n_touch >= 20 or mode in WORDY)
    if mode in WORDY:  # "A" between replaced bytes is a whole word: the bytes around it stay
        assert check(a, orc, b"\xe2\x82A\xf5 AA\x80", "<w>")[0] == b"\xe2\x82<w>\xf5 <w>\x80"


def test_keywords_with_the_replacement_character():
    kws = ["�", "a�", "�b", "q��"]
    a, orc = pair(N.MODE_LONGEST, kws)
    repls = ["?", "<a?>", "<?b>", "<q??>"]
    # a subpart's bytes are what is removed, a genuine EF BF BD likewise; everything else stays
    assert check(a, orc, b"a\xef\xbf\xbdb a\xf0\x9fb \xe2\x82 q\xc0\x80 \xf0\x9f\x98\x80", repls)[0] == "<a?>b <a?>b ? <q??> 😀".encode()
    f, forc = pair(N.MODE_LONGEST, ["�"])
    for row, spans in TABLE:  # alone, the records are the table's spans, and deleting them leaves what the table leaves
        want, brecs, _ = check(f, forc, b"z" + row + b"z", "")
        assert [r[:2] for r in brecs.tolist()] == [[b + 1, e + 1] for b, e in spans] and len(want) == 2 + len(row) - sum(e - b for b, e in spans)
    sh, sorc = pair(N.MODE_SHORTEST, kws)
    assert check(sh, sorc, b"a\xe2\x82b q\x80\x80", repls)[0] == b"<a?>b q??"


# ---- 2. seams: the transcoder's lanes, waves and workgroups, and forced piece boundaries ----------------------------------------------
def seam_text(row, j, three):
    """about 10 KB: `row` placed so that its byte j is the first byte of a lane (2064), of a wave (1024, 3072) and of a workgroup
    (4096, 8192), each followed by "A(" and preceded by "A"; between them ASCII words, or 3-byte characters padded to the byte"""
    buf = bytearray()
    for seam in (1024, 2064, 3072, 4096, 8192):
        gap = seam - j - len(buf) - 1
        buf += ("中" * (gap // 3)).encode() + b"x" * (gap % 3) if three else (b"kw A " * (gap // 5 + 1))[:gap]
        buf += b"A" + row + b"A("
        assert len(buf) == seam - j + len(row) + 2
    buf += "中文".encode() * 300 if three else b"w A" * 600
    return bytes(buf)


@pytest.mark.parametrize("three", [False, True])
def test_subparts_across_lane_wave_and_workgroup_seams_and_at_piece_boundaries(three):
    kws = ["A", "�", "A�", "�(", "�A", "中文", "kw"]
    a, orc = pair(N.MODE_LONGEST, kws)
    sa, sorc = pair(N.MODE_SHORTEST, kws)
    repls = ["<A>", "", "<A?>", b"\xff(", "<?A>", "CJ", "KW!"]
    texts = [seam_text(row, j, three) for row in ROWS for j in range(len(row))]
    assert all(2 * BLOCK + 1000 < len(t) < 3 * BLOCK for t in texts)
    for i, t in enumerate(texts):
        if i % 2:
            small_pieces()
        want, brecs, st = check(a, orc, t, repls)
        assert touching(t, brecs) >= 5 and decode_replace(t)[3].sum() >= 5
        assert st["pieces"] >= (min_pieces(t) if i % 2 else 1) and min_pieces(t) >= 10
        for k, v in DEFAULTS:
            N.set_tunable(k, v)
    small_pieces()
    for t in texts[::7]:
        assert check(sa, sorc, t, repls)[2]["pieces"] >= min_pieces(t)
    check_batch(a, orc, texts[:5], repls)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_piece_boundary_at_every_phase_of_subparts_and_four_byte_sequences(mode):
    """every 80 units or so the text holds a knot of subparts of one, two and three bytes and astral characters: with pieces of 64
    to 256 units, and the text shifted by 0 .. 11 leading units, piece boundaries fall on, before and behind each of them"""
    small_pieces()
    kws = ["A", "AA", "�", "�A", "A�", "😀", "x😀"] if mode not in WORDY else ["A", "AA", "x", "xx"]
    a, orc = pair(mode, kws)
    knot = b"A\xe2\x82A\xf0\x9f\x98" + ASTRAL + b"\x80" + ASTRAL + b"A\xc0 " + ASTRAL + b"\xf0\x9fA " + ASTRAL * 2 + b"\xed\xa0\x80A "
    n_touch = 0
    for shift in range(12):
        data = b"x " * (shift // 2) + b"x" * (shift % 2) + (b"xx A " * 11 + knot) * 24
        want, brecs, st = check(a, orc, data, "#" if shift % 2 else ["<%d>" % i for i in range(len(kws))])
        n_touch += touching(data, brecs)
        assert st["pieces"] >= min_pieces(data) >= 5 and decode_replace(data)[3].sum() >= 120
    assert n_touch >= 100


# ---- 3. batches ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_batch_whose_cuts_split_sequences(mode):
    a, orc, kws, valid = family(mode)
    text = (valid[:900] + " A😀(é€ ").encode() * 5
    repls = mixed_replacements(kws)
    cuts = 0
    for seam in (2064, BLOCK):
        off = [0] + list(range(seam - 6, seam + 7)) + [len(text)]
        datas = [text[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        cuts += sum(1 for d in datas if d and (d[0] & 0xC0) == 0x80)
        check_batch(a, orc, datas, repls)
        for p in range(seam - 4, seam + 5, 2):
            check_batch(a, orc, [text[:p], b"", text[p:]], "#")
    assert cuts >= 4
    small_pieces()
    lines = [l + b"\xe2\x82" if i % 3 == 0 else l for i, l in enumerate(text.split(b" "))]
    per, st = check_batch(a, orc, lines, repls)
    assert st["pieces"] >= min_pieces(*lines) >= 10 and st["n_records"] > 50
    e = [b""]
    for n in (1, 3):
        check_batch(a, orc, [b"A\xf0\x9f"] + e * n + [b"\x98\x80A("] + e * n, "#")
        check_batch(a, orc, e * n + [b"\xe2"] + e * n + [b"\x82\xacA"] + e * n + [b"\xac"], ["<%d>" % i for i in range(len(kws))])


@pytest.mark.parametrize("mode", WORDY)
def test_the_per_haystack_route_word_table_that_is_not_fold_consistent(mode):
    rng = np.random.default_rng(9)
    alpha = "abxyABXY ,éÉ"
    wc = word_chars_from_list("abcdxyABCDéÉ")  # X, Y are not word characters although x, y are
    kws = ["".join(alpha[int(i)] for i in rng.integers(0, 4, int(rng.integers(1, 5)))) for _ in range(24)] + ["é", "aé"]
    a, orc = Automaton(mode, kws, False, word_chars=wc), Oracle(MODES[mode], kws, False, LOWER, wc, map_flavour=True)
    assert a.info()["fold_consistent"] == 0
    bad = [b"\x80", b"\xc3", b"\xe2\x82", b"\xf5"]
    datas = []
    for ln in (0, 1, 40, 300, 7, 0, 120, 3, 12, 60, 0, 25):
        s = "".join(alpha[int(i)] for i in rng.integers(0, len(alpha), int(ln)))
        cut = int(rng.integers(len(s) + 1))
        datas.append(s[:cut].encode() + bad[int(rng.integers(4))] + s[cut:].encode() if ln > 1 else s.encode())
    per, st = check_batch(a, orc, datas, mixed_replacements(kws))
    assert st["n_records"] > 5 and st["pieces"] >= sum(1 for d in datas if d) and per != datas
    check_batch(a, orc, datas, "")
    with pytest.raises(Utf8Error):
        a.replace_batch_utf8(datas, "#")  # the strict entry refuses the same batch


def test_the_per_haystack_route_dictionary_without_a_free_unit():
    kws = [np.array([u], dtype=np.uint16) for u in range(65536) if not 0xD800 <= u < 0xE000]
    kws += [np.array([0xD800 + k, 0xDC00 + k], dtype=np.uint16) for k in range(1024)]
    a, orc = pair(N.MODE_LONGEST, kws)
    datas = [b"ab", "é".encode(), b"", b"z\xc3", b"\xa9a", "ü".encode() * 9 + b"\xe2\x82", b"", b"\xf0\x9f\x98", "ñ".encode() * 70, b"\x80\xbf", b"a\x80b",
             chr(0x10000).encode()[:3] + chr(0x10000).encode()]
    per, st = check_batch(a, orc, datas, "#")
    n_units = want_stats(datas)[0]
    assert st["n_records"] == n_units - 1 and b"".join(per) == b"#" * (n_units - 1)  # a record per code point or subpart
    assert st["pieces"] == sum(1 for d in datas if d)  # a text per haystack
    check_batch(a, orc, datas, "")


# ---- 4. overflow ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slab", [None, 1000])
def test_overflow_reports_the_exact_size_and_writes_nothing_beyond_cap(slab):
    if slab:
        N.set_tunable("replace_slab_units", slab)
        small_pieces()
    a, orc, kws, valid = family(N.MODE_LONGEST)
    rng = np.random.default_rng(5)
    data = b"".join(damaged(rng, valid.encode(), n_buffers=40, max_len=300))
    repls = mixed_replacements(kws)
    want, brecs, _ = check(a, orc, data, repls)
    need = len(want)
    assert len(brecs) > 50 and decode_replace(data)[3].sum() > 50
    for cap in (0, 1, need // 2, need - 1):
        rc, n_out, out, st, ust = raw(a, data, repls, cap, room=need)
        assert rc == N.E_OVERFLOW and n_out == need and st["units_out"] == need, (cap, rc, n_out)
        assert (out[cap:] == CANARY).all(), "written at or beyond cap"
        assert out[:cap].tobytes() == want[:cap]
        rc, n_out, out, st, ust = raw(a, data, repls, n_out)  # then success
        assert rc == N.OK and out[:n_out].tobytes() == want
    rc, n_out, out, st, ust = raw(a, data, repls, 0, null_out=True)  # no buffer at all: the call counts
    assert rc == N.E_OVERFLOW and n_out == need
    got, st2 = a.replace_utf8(data, repls, cap=1, errors="replace")  # the wrapper's retry
    assert got.tobytes() == want
    # the batch: *n_out and every offset exact all the same
    datas = [data[i:i + 97] for i in range(0, len(data), 97)]
    per, _ = check_batch(a, orc, datas, repls)
    whole = b"".join(per)
    woff = np.cumsum([0] + [len(p) for p in per], dtype=np.uint64)
    for cap in (0, len(whole) // 3, len(whole) - 1):
        rc, n_out, out, oo, st, ust = raw_batch(a, datas, repls, cap, room=len(whole))
        assert rc == N.E_OVERFLOW and n_out == len(whole) and (oo == woff).all() and (out[cap:] == CANARY).all()
        assert out[:cap].tobytes() == whole[:cap]
    got, out_off, st3 = a.replace_batch_utf8(datas, repls, cap=1, errors="replace")
    assert got.tobytes() == whole and (out_off == woff).all()


# ---- 5. well-formed input: the strict results ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_well_formed_input_gives_the_strict_results(mode):
    rng = np.random.default_rng(8200 + mode)
    text = mixed_text(np.random.default_rng(1000), 9000)
    a, _ = pair(mode, keywords_from(rng, text[:4000], mode, True), True)
    data = text.encode()
    repls = mixed_replacements(a.keywords)
    small_pieces()
    ust = N.Utf8LossyStats()
    strict, st = a.replace_utf8(data, repls)
    lossy, st2 = a.replace_utf8(data, repls, stats=ust, errors="replace")
    assert st["n_records"] > 10 and lossy.tobytes() == strict.tobytes() and st2 == st
    assert (ust.n_replaced, ust.first_replaced, ust.ascii) == (0, -1, 0)
    lines = data.split(b" ")[:400]
    s_out, s_off, s_st = a.replace_batch_utf8(lines, repls)
    l_out, l_off, l_st = a.replace_batch_utf8(lines, repls, stats=ust, errors="replace")
    assert l_out.tobytes() == s_out.tobytes() and (l_off == s_off).all() and l_st == s_st and ust.n_replaced == 0


# ---- 6. fuzz -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [True, False])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_fuzz_single_texts_and_one_batch(mode, cs):
    rng = np.random.default_rng(31337)
    valid = mixed_text(rng, 3000)
    bufs = damaged(rng, valid.encode(), n_buffers=120)
    bufs[50] = b""
    a, orc = pair(mode, fuzz_keywords(mode, cs, valid), cs)
    repls = mixed_replacements(a.keywords)
    n_replaced = sum(int(decode_replace(b)[3].sum()) for b in bufs)
    n_touch = 0
    for b in bufs[:60]:
        want, brecs, st = check(a, orc, b, repls)
        n_touch += touching(b, brecs)
    assert n_replaced > 300 and n_touch >= 20, (n_replaced, n_touch)
    check_batch(a, orc, bufs, repls)
    check_batch(a, orc, bufs, "")
    small_pieces()
    long = b"".join(bufs)  # one text of about 18 KB: many pieces, their boundaries wherever they fall among the subparts
    want, brecs, st = check(a, orc, long, repls)
    assert st["pieces"] >= min_pieces(long) >= 20 and touching(long, brecs) >= 30


# ---- 7. the facade ---------------------------------------------------------------------------------------------------------------------------
def test_the_facade_redacts_a_damaged_log():
    m = WholeWordMatchMap(["error", "straße", "GPU"], ["E", "S", "G"], False)
    lines = [b"an ERROR \xff here", "Stra\xdfe".encode("latin-1") + b" gpu", b"", "straße ok".encode(), b"\xc3", b"gpu\xe2\x82error"]
    with pytest.raises(Utf8Error):
        m.replace_batch_utf8(lines)
    assert m.replace_batch_utf8(lines, errors="replace") == [b"an E \xff here", b"Stra\xdfe G", b"", b"S ok", b"\xc3", b"G\xe2\x82E"]
    assert m.replace_utf8(lines[5], ["<e>", "<s>", "<g>"], errors="replace") == b"<g>\xe2\x82<e>"
    s = LongestMatchSet(["secret", "�"], True)
    assert s.replace_utf8(b"a secret\x80 \xe2\x82", b"*", errors="replace") == b"a ** *"
    assert s.replace_batch_utf8([b"secret\xc3", b"\xa9secret"], "", errors="replace") == [b"", b""]
    buf = b"secret\xc3\n\xa9x\n"
    assert s.replace_batch_utf8(buf, "#", offsets=np.array([0, 8, 11], np.uint64), errors="replace") == [b"##\n", b"#x\n"]
    assert LongestMatchMap(["k"], ["v"], True).replace_utf8(b"k\xffk", errors="replace") == b"v\xffv"
