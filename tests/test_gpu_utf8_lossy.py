"""GPU tests of the lossy UTF-8 entries (include/acgpu.h: acgpu_match_utf8_lossy, acgpu_match_batch_utf8_lossy,
acgpu_summary_batch_utf8_lossy; csrc/acgpu_utf8.hip: the LOSSY forms of the count, write and map kernels).  Every expected record
comes from the CPU oracle on the text that tests/utf8_lossy_ref.py decodes -- CPython's errors="replace", rebuilt from its strict
decoder (checked in tests/test_utf8_lossy_cpu.py) -- with its positions mapped to bytes by that decoder's per-unit table: a
replaced subpart's U+FFFD maps to the subpart.  Equality is exact.  To check the mapping at EVERY unit, most tests use an
AhoCorasick dictionary of every distinct unit of the decoded text as a keyword of its own, and U+FFFD twice: a record per unit."""
import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickSet, Automaton, Utf8Error, WholeWordMatchMap, utf16
from ahocorasick_amd.unicode_tables import word_chars_from_list
from oracle.oracle import Oracle
from tests.helpers import LOWER, WORD
from tests.test_gpu_utf8 import MODES, WORDY, big_text, filler, keywords_from, mixed_text, pair
from tests.utf8_lossy_ref import TABLE, damaged, decode_replace

pytestmark = pytest.mark.gpu

BLOCK = 4096  # bytes per workgroup of the transcoder (16 per lane, 1024 per wave)
EMPTY = np.zeros((0, 3), np.int32)
ROWS = [row for row, _ in TABLE]
ASTRAL = "😀".encode()


def every_unit(datas):
    """(automaton, oracle) of the AhoCorasick dictionary that reports every unit of the decoded buffers"""
    units = sorted({int(u) for d in datas for u in utf16(decode_replace(d)[0]).tolist()} | {0xFFFD})
    return pair(N.MODE_ALL, [np.array([u], np.uint16) for u in units] + [np.array([0xFFFD, 0xFFFD], np.uint16)])


def expected(orc, data):
    """-> (records in bytes, n_units, n_replaced, first_replaced) of one buffer decoded alone"""
    text, off, length, replaced = decode_replace(data)
    if not text:
        return EMPTY, 0, 0, -1
    recs = orc.match(utf16(text), cap=max(1024, 8 * len(off)))
    want = recs.copy()
    if len(recs):
        want[:, 0] = off[recs[:, 0]]
        want[:, 1] = off[recs[:, 1] - 1] + length[recs[:, 1] - 1]
    return want, len(off), int(replaced.sum()), int(off[replaced][0]) if replaced.any() else -1


def same(got, want):
    assert got.shape == want.shape and got.dtype == np.int32, (got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (bad[:5], got[bad[:5]], want[bad[:5]])


def check(a, orc, data, kinds=(True,)):
    """match_utf8(errors="replace") against the reference -> (records in bytes, stats)"""
    want, n_units, n_replaced, first = expected(orc, data)
    st = N.Utf8LossyStats(7, 7, 7, 7, 7)
    for with_ids in kinds:
        same(a.match_utf8(data, with_ids=with_ids, stats=st, errors="replace"), want if with_ids else want[:, :2])
        ascii_ = int(max(bytes(data), default=0) < 0x80)
        assert (st.n_units, st.n_replaced, st.first_replaced, st.first_haystack, st.ascii) == (n_units, n_replaced, first, 0, ascii_)
    return want, st


def check_batch(a, orc, datas, kinds=(True,), offsets=False):
    """match_batch_utf8 and summary_batch_utf8 (errors="replace") against every haystack decoded alone -> the tagged records"""
    per = [expected(orc, d) for d in datas]
    rows = [np.column_stack([np.full(len(w), i, np.int32), w]) for i, (w, *_) in enumerate(per) if len(w)]
    want = np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 4), np.int32)
    hit = [i for i, p in enumerate(per) if p[3] >= 0]
    stats = (sum(p[1] for p in per), sum(p[2] for p in per), per[hit[0]][3] if hit else -1, hit[0] if hit else 0,
             int(all(max(bytes(d), default=0) < 0x80 for d in datas)))
    arg, kw = datas, {}
    if offsets:
        arg, kw = b"".join(datas), {"offsets": np.cumsum([0] + [len(d) for d in datas], dtype=np.uint64)}
    for with_ids in kinds:
        st = N.Utf8LossyStats(7, 7, 7, 7, 7)
        same(a.match_batch_utf8(arg, with_ids=with_ids, stats=st, errors="replace", **kw), want if with_ids else want[:, :3])
        assert (st.n_units, st.n_replaced, st.first_replaced, st.first_haystack, st.ascii) == stats
    # the summary against the batch's own records: count and first record of every haystack
    ws = np.zeros(len(per), dtype=N.SUMMARY_DTYPE)
    for i, (w, *_) in enumerate(per):
        ws[i] = (len(w),) + (tuple(w[0].tolist()) if len(w) else (-1, -1, -1)) + (0,)
    st = N.Utf8LossyStats(7, 7, 7, 7, 7)
    got, sst = a.summary_batch_utf8(arg, stats=st, errors="replace", **kw)
    bad = [i for i in range(len(ws)) if got[i] != ws[i]]
    assert got.shape == ws.shape and not bad, (bad[:5], got[bad[:5]], ws[bad[:5]])
    assert sst["n_records"] == len(want) and sst["n_matched"] == sum(1 for w, *_ in per if len(w))
    assert (st.n_units, st.n_replaced, st.first_replaced, st.first_haystack, st.ascii) == stats
    return want


# ---- 1. the table, in four surroundings ------------------------------------------------------------------------------------------
def test_hand_cases_alone_between_ascii_between_astral_and_at_the_end():
    cases = [c for row in ROWS for c in (row, b"ab" + row + b"cd", ASTRAL + row + ASTRAL, b"ab" + row, "é€".encode() + row)]
    a, orc = every_unit(cases)
    for (row, spans), data in zip([r for r in TABLE for _ in range(5)], cases):
        want, st = check(a, orc, data, kinds=(True, False))
        assert len(want) >= st.n_units  # a record per unit at least
    # alone, the spans are those of the table: the U+FFFD records of the text
    fffd = AhoCorasickSet(["\ufffd"], True)
    for row, spans in TABLE:
        got = fffd.find_all_utf8(row, errors="replace").tolist()
        assert got == [list(s) for s in spans], (row, got)
    # a keyword with U+FFFD matches the genuine character and a replaced subpart alike
    got = AhoCorasickSet(["a\ufffd", "\ufffdb"], True).find_all_utf8(b"a\xef\xbf\xbdb a\xf0\x9fb \xe2\x82", errors="replace")
    assert sorted(got.tolist()) == [[0, 4], [1, 5], [6, 9], [7, 10]]


# ---- 2. seams of the transcoder: lanes, waves, workgroups ------------------------------------------------------------------------
def seam_text(row, j, three):
    """about 10 KB, more than two workgroups: `row` placed so that its byte j is the first byte of a lane (2064), of a wave
    (1024, 3072) and of a workgroup (4096, 8192); between them ASCII, or 3-byte characters padded with ASCII to the byte"""
    buf = bytearray()
    for seam in (1024, 2064, 3072, 4096, 8192):
        gap = seam - j - len(buf)
        buf += ("中" * (gap // 3)).encode() + b"x" * (gap % 3) if three else b"k" * gap
        assert len(buf) == seam - j
        buf += row
    buf += "中文".encode() * 300 if three else b"w" * 1800
    return bytes(buf)


@pytest.mark.parametrize("three", [False, True])
def test_every_byte_of_every_pattern_on_a_lane_a_wave_and_a_workgroup_seam(three):
    texts = [seam_text(row, j, three) for row in ROWS for j in range(len(row))]
    assert all(2 * BLOCK + 1000 < len(t) < 3 * BLOCK for t in texts) and len(texts) == sum(len(r) for r in ROWS)
    a, orc = every_unit(texts)
    for t in texts:
        want, st = check(a, orc, t)
        assert st.n_replaced >= 5 and len(want) >= st.n_units
    check_batch(a, orc, texts[:6])  # the same seams with haystack boundaries between the texts


# ---- 3. checkpoints ---------------------------------------------------------------------------------------------------------------
def test_replaced_units_and_low_surrogates_at_the_checkpoints():
    cases = []
    for k in (32, 64, 96):
        head = "é" + "a" * (k - 1)                                        # k units, not as many bytes
        cases.append(head.encode() + b"\x80" + b"z")                      # a replaced unit with index k
        cases.append(head.encode() + b"\xf0\x9f\x98" + "😀z".encode())    # ... of three bytes, an astral character behind it
        cases.append(head[:-1].encode() + ASTRAL + b"\xe2\x82" + b"z")    # a low surrogate with index k, a subpart directly behind it
        cases.append(head[:-2].encode() + b"\xe2\x82" + ASTRAL + b"z")    # ... and directly before it
        cases.append(head[:-2].encode() + b"\xc0" + ASTRAL + b"\xbf" * 40 + ASTRAL)
    a, orc = every_unit(cases)
    for i, data in enumerate(cases):
        text, off, length, replaced = decode_replace(data)
        k = (32, 64, 96)[i // 5]
        units = utf16(text)
        assert replaced[k] if i % 5 < 2 else (units[k] & 0xFC00) == 0xDC00 and (replaced[k + 1] or replaced[k - 2]), (i, k)
        check(a, orc, data, kinds=(True, False))
    check_batch(a, orc, cases)


# ---- 4. as many units as bytes: the identity, no checkpoints, no bitmap ---------------------------------------------------------------
def test_the_equality_shortcut():
    for data, n_replaced in ((b"a\x80b", 1), (b"\x80" * 5000, 5000), (b"ab\xc0\xf5(" * 900, 1800)):
        a, orc = every_unit([data])
        want, st = check(a, orc, data, kinds=(True, False))
        assert st.n_units == len(data) and st.n_replaced == n_replaced and st.ascii == 0
        ones = want[want[:, 1] - want[:, 0] == 1]
        assert sorted(ones[:, 0].tolist()) == list(range(len(data)))  # identity offsets: a record [i, i + 1) for every byte
        check_batch(a, orc, [data[:1], data[1:700], b"", data[700:]])
    a, orc = every_unit([b"plain ascii"])
    _, st = check(a, orc, b"plain ascii")
    assert (st.ascii, st.n_replaced) == (1, 0)


# ---- 5. well-formed input: the strict results ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_well_formed_input_gives_the_strict_results(mode):
    rng = np.random.default_rng(8100 + mode)
    big = big_text()
    a, _ = pair(mode, keywords_from(rng, big[:4000], mode, True), True)
    data = big[:20000].encode()
    st = N.Utf8LossyStats()
    strict = a.match_utf8(data, with_ids=True)
    assert len(strict) > 10
    same(a.match_utf8(data, with_ids=True, stats=st, errors="replace"), strict)
    assert (st.n_units, st.n_replaced, st.first_replaced, st.ascii) == (len(utf16(big[:20000])), 0, -1, 0)
    lines = data.split(b" ")[:500]
    same(a.match_batch_utf8(lines, with_ids=True, stats=st, errors="replace"), a.match_batch_utf8(lines, with_ids=True))
    assert (st.n_replaced, st.first_replaced, st.first_haystack) == (0, -1, 0)
    got, want = a.summary_batch_utf8(lines, errors="replace"), a.summary_batch_utf8(lines)
    assert (got[0] == want[0]).all() and got[1] == want[1]


# ---- 6. fuzz ------------------------------------------------------------------------------------------------------------------------
def fuzz_buffers():
    if not _FUZZ:
        rng = np.random.default_rng(31337)
        valid = mixed_text(rng, 3000)
        bufs = damaged(rng, valid.encode())
        bufs[50] = b""
        _FUZZ.append((valid, bufs))
    return _FUZZ[0]


_FUZZ = []


def fuzz_keywords(mode, cs, valid):
    kws = keywords_from(np.random.default_rng(900 + mode), valid, mode, cs)
    if mode in WORDY:  # whole words; "A" stands between replaced bytes, which are no word characters
        return kws + ["A", "AA", "a" if cs else "aa"]
    return kws + ["\ufffd", "A\ufffd", "\ufffd(", "\ufffd\ufffdA", "(", "a" if cs else "\ufffda"]


@pytest.mark.parametrize("cs", [True, False])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_fuzz_single_texts_and_one_batch(mode, cs):
    valid, bufs = fuzz_buffers()
    a, orc = pair(mode, fuzz_keywords(mode, cs, valid), cs)
    # the inputs' own conditions
    tables = [decode_replace(b) for b in bufs]
    lens = np.concatenate([t[2][t[3]] for t in tables])
    assert len(bufs) == 200 and len(lens) >= 500 and set(lens.tolist()) == {1, 2, 3} and any(not b for b in bufs)
    touching = 0
    for b, (_, off, length, replaced) in zip(bufs, tables):
        want, _ = check(a, orc, b, kinds=(True, False) if mode == N.MODE_ALL else (True,))
        edge = np.zeros(len(b) + 2, bool)  # bytes of replaced subparts, shifted by one: a record touches one that it covers or abuts
        for o, n in zip(off[replaced].tolist(), length[replaced].tolist()):
            edge[o + 1:o + n + 1] = True
        touching += sum(1 for s, e, _ in want.tolist() if edge[s:e + 2].any())
    assert touching >= 50, touching
    check_batch(a, orc, bufs, kinds=(True, False))
    check_batch(a, orc, bufs, offsets=True)


def test_the_strict_entries_still_refuse_the_same_buffers():
    valid, bufs = fuzz_buffers()
    a, orc = pair(N.MODE_ALL, ["A", "(", "q"])
    refused = 0
    for b in bufs:
        first = expected(orc, b)[3]
        if first < 0:
            assert len(a.match_utf8(b, with_ids=True)) == len(expected(orc, b)[0])
            continue
        with pytest.raises(Utf8Error) as e:
            a.match_utf8(b, with_ids=True)
        assert (e.value.start, e.value.haystack) == (first, None)
        refused += 1
    assert refused >= 150
    firsts = [(i, expected(orc, b)[3]) for i, b in enumerate(bufs)]
    want = next(f for f in firsts if f[1] >= 0)
    for call in (lambda: a.match_batch_utf8(bufs, with_ids=True), lambda: a.summary_batch_utf8(bufs)):
        with pytest.raises(Utf8Error) as e:
            call()
        assert (e.value.haystack, e.value.start) == want
    check_batch(a, orc, bufs[:20])  # and the lossy call behind a refusal finds the pool as usable as ever


# ---- 7. batches: cuts inside sequences -------------------------------------------------------------------------------------------------
def test_a_valid_text_cut_at_every_byte_around_a_lane_seam_and_a_workgroup_seam():
    text = filler(BLOCK + 200)
    a, orc = every_unit([text, b"\x80"])
    inside = 0
    for seam in (2064, BLOCK):
        for p in range(seam - 5, seam + 6):
            datas = [text[:p], text[p:]]
            want = check_batch(a, orc, datas)
            inside += (text[p] & 0xC0) == 0x80
            assert ((text[p] & 0xC0) == 0x80) == (expected(orc, datas[0])[2] > 0)
        # all those cuts at once: haystacks of one byte, continuation bytes alone among them
        off = [0] + list(range(seam - 5, seam + 6)) + [len(text)]
        datas = [text[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        assert any(len(d) == 1 and (d[0] & 0xC0) == 0x80 for d in datas)
        check_batch(a, orc, datas, kinds=(True, False))
        check_batch(a, orc, datas, offsets=True)
    assert inside >= 8


def test_hand_batches():
    a, orc = every_unit([b"ab\xc3\xa9 \xe2\x82\xac \xf0\x9f\x98\x80kw", b"\x80"])
    want = check_batch(a, orc, [b"a\xc3", b"\xa9b"])
    assert want[:, :3].tolist() == [[0, 0, 1], [0, 1, 2], [1, 0, 1], [1, 1, 2]]  # a, U+FFFD | U+FFFD, b
    e = [b""]
    for n in (1, 2, 5):  # runs of empty haystacks beside a cut sequence
        check_batch(a, orc, [b"a\xf0\x9f"] + e * n + [b"\x98\x80b"] + e * n)
        check_batch(a, orc, e * n + [b"\xe2"] + e * n + [b"\x82\xac"] + e * n + [b"\xac"])
        check_batch(a, orc, [filler(BLOCK - 2) + b"\xe2\x82"] + e * n + [b"\xac" + filler(40)], kinds=(True, False))
    check_batch(a, orc, [b"\x80"])  # a haystack that is one continuation byte
    check_batch(a, orc, [b"kw", b"\xac", b"kw"])
    check_batch(a, orc, ["é".encode(), b"", b"\xa9", b"\xa9\xa9", "€".encode()[:2], "€".encode()[2:]])
    # where the first replaced subpart lies: not in the first haystacks, and not at its haystack's first byte
    st = N.Utf8LossyStats()
    a.match_batch_utf8(["é".encode(), b"", "ab€".encode() + b"\xf0\x9f" + b"b", b"\x80"], with_ids=True, stats=st, errors="replace")
    assert (st.first_haystack, st.first_replaced, st.n_replaced, st.n_units) == (2, 5, 2, 7)


# ---- 8. where the library scans haystack by haystack ---------------------------------------------------------------------------------
DAMAGED = [b"ab", "é".encode(), b"", b"z\xc3", b"\xa9a", "ü".encode() * 9 + b"\xe2\x82", b"", b"\xf0\x9f\x98", "ñ".encode() * 70, b"\x80\xbf", b"a\x80b",
           "😀".encode()[:3] + "😀".encode()]


def test_fallback_dictionary_without_a_free_unit():
    a, orc = pair(N.MODE_ALL, [np.array([i], dtype=np.uint16) for i in range(65536)])
    want = check_batch(a, orc, DAMAGED, kinds=(True, False))
    assert len(want) == sum(expected(orc, d)[1] for d in DAMAGED)  # a record per unit
    assert a.summary_batch_utf8(DAMAGED, errors="replace")[1]["pieces"] == sum(1 for d in DAMAGED if d)  # a text per haystack
    check(a, orc, b"".join(DAMAGED))


@pytest.mark.parametrize("mode", WORDY)
def test_fallback_word_table_that_is_not_fold_consistent(mode):
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
    want = check_batch(a, orc, datas)
    assert len(want) > 5 and sum(expected(orc, d)[2] for d in datas) >= 8


# ---- 9. the separator unit is U+FFFD ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [N.MODE_ALL] + list(WORDY))
def test_a_dictionary_whose_separator_unit_is_the_replacement_character(mode):
    """U+FFFF and U+FFFE are keywords, so the builder's separator -- the highest unit that is in no keyword and no word
    character -- is U+FFFD: replaced bytes and separators are the same unit in the text the scan sees"""
    kws = ["\uffff", "\ufffe", "ab", "b", "kw", "é"]
    wc = None
    if mode in WORDY:  # (a word matcher's keywords are word characters: here the two noncharacters are)
        wc = WORD.copy()
        wc[0xFFFE:] = 1
    a, orc = Automaton(mode, kws, True, word_chars=wc), Oracle(MODES[mode], kws, True, None, wc, map_flavour=True)
    datas = [b"ab\x80ab", b"\x80", b"ab", b"", b"\xe2\x82kw", "kw\uffff".encode() + b"\xf0\x9f", b"\xbfb", "é".encode()[:1], "é".encode()[1:] + b"ab",
             "\ufffeab".encode() + b"\xc0kw\xf5", filler(60) + b"\xed\xa0\x80 kw"]
    want = check_batch(a, orc, datas, kinds=(True, False))
    assert len(want) >= 8 and len(set(want[:, 0].tolist())) >= 6  # (the word matchers find fewer than AhoCorasick)
    for d in datas:
        check(a, orc, d)


# ---- 10. the facade -------------------------------------------------------------------------------------------------------------------
def test_facade_keyword_on_a_damaged_log():
    words, values = ["error", "straße", "GPU"], ["E", "S", "G"]
    m = WholeWordMatchMap(words, values, False)
    lines = [b"an ERROR \xff here", "Stra\xdfe".encode("latin-1") + b" gpu", b"", "straße ok".encode(), b"\xc3", b"gpu\xe2\x82error"]
    with pytest.raises(Utf8Error):
        m.contains_batch_utf8(lines)
    assert m.contains_batch_utf8(lines, errors="replace").tolist() == [True, True, False, True, False, True]
    assert m.count_matches_batch_utf8(lines, errors="replace").tolist() == [1, 1, 0, 1, 0, 2]
    assert m.first_batch_utf8(lines, errors="replace") == [(3, 8, "E"), (7, 10, "G"), None, (0, 7, "S"), None, (0, 3, "G")]
    assert m.find_all_batch_utf8(lines, errors="replace").tolist() == [[0, 3, 8, 0], [1, 7, 10, 2], [3, 0, 7, 1], [5, 0, 3, 2], [5, 5, 10, 0]]
    assert m.find_all_utf8(lines[5], errors="replace").tolist() == [[0, 3, 2], [5, 10, 0]]
    seen = []
    m.match_utf8(lines[0], lambda h, b, e, v: seen.append((bytes(h[b:e]), v)) or True, errors="replace")
    m.match_batch_utf8(lines, lambda h, b, e, v: seen.append((bytes(h[b:e]), v)) or True, errors="replace")
    assert seen == [(b"ERROR", "E")] + [(b"ERROR", "E"), (b"gpu", "G"), ("straße".encode(), "S"), (b"gpu", "G"), (b"error", "E")]
