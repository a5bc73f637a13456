"""GPU tests of the chunked UTF-8 feed (include/acgpu.h: acgpu_stream_feed_utf8; csrc/acgpu_stream.hip, and in csrc/acgpu_utf8.hip
the open form of the validator, k_utf8_open_count).  Every expected record comes from the CPU oracle on the decoded whole text,
its positions mapped to bytes by the header's rule (the helpers of tests/test_gpu_utf8.py); equality is exact.  What is held
back, which feed fails and where is what CPython's codecs.getincrementaldecoder("utf-8") does with the same chunks."""
import codecs
import ctypes
import io

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickMap, AhoCorasickSet, Automaton, LongestMatchMap, Stream, Utf8Error, utf16
from oracle.oracle import FAM_AC, FAM_LONGEST, FAM_WHOLEWORD, Oracle
from tests.test_gpu_utf8 import MODES, expected, keywords_from, mixed_text, pair, to_bytes

pytestmark = pytest.mark.gpu

vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
SECONDS = [0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0]


def feed_all(a, chunks, with_ids, final_in_last, cap=8):
    """the chunks through one stream -> (records with global byte offsets, [(n_units, ascii, held) per feed])"""
    st = N.Utf8StreamStats()
    s = Stream(a, with_ids=with_ids)
    pages, stats = [], []
    try:
        for i, c in enumerate(chunks):
            pages.append(s.feed_utf8(c, final=final_in_last and i == len(chunks) - 1, cap=cap, stats=st))
            stats.append((st.n_units, st.ascii, st.held))
            assert st.first_bad == -1
        if not final_in_last:
            pages.append(s.feed_utf8(b"", final=True, cap=cap, stats=st))
            stats.append((st.n_units, st.ascii, st.held))
    finally:
        s.close()
    return np.concatenate(pages), stats


def same(got, want, what):
    assert got.dtype == np.int64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (what, bad[:5], got[bad[:5]], want[bad[:5]])


def split(data, cuts):
    edges = [0] + [int(c) for c in cuts] + [len(data)]
    return [data[edges[i]:edges[i + 1]] for i in range(len(edges) - 1)]


def seq_lengths(data):
    return {1 if b < 0x80 else 2 if b < 0xE0 else 3 if b < 0xF0 else 4 for b in data if (b & 0xC0) != 0x80}


def cpython(chunks):
    """[(bytes, final)] through CPython's incremental decoder -> (index of the feed that fails or None, the global offset it
    fails at, [bytes held after every feed that passed])"""
    d = codecs.getincrementaldecoder("utf-8")()
    fed, held = 0, []
    for i, (c, final) in enumerate(chunks):
        pending = len(d.getstate()[0])
        try:
            d.decode(c, final)
        except UnicodeDecodeError as e:
            return i, fed - pending + e.start, held  # (e.start counts from the first held byte)
        held.append(len(d.getstate()[0]))
        fed += len(c)
    return None, -1, held


def ours(a, chunks, with_ids=True):
    """the same through a stream -> (failing feed or None, global offset, [held], records or None)"""
    st = N.Utf8StreamStats()
    s = Stream(a, with_ids=with_ids)
    held, pages = [], []
    try:
        for i, (c, final) in enumerate(chunks):
            try:
                pages.append(s.feed_utf8(c, final=final, stats=st))
            except Utf8Error as e:
                assert e.start == st.first_bad and (st.n_units, st.ascii, st.held) == (0, 0, 0)
                return i, e.start, held, None
            held.append(st.held)
    finally:
        s.close()
    return None, -1, held, np.concatenate(pages)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------
def stream_text():
    """about 60 000 characters (some 110 000 bytes), generated once, and in it a 300-byte stretch with sequences of every length"""
    if not _TEXT:
        text = mixed_text(np.random.default_rng(1700), 60000)
        data = text.encode("utf-8")
        s0 = len(text[:20000].encode("utf-8"))
        assert seq_lengths(data[s0:s0 + 300]) == {1, 2, 3, 4} and 100000 < len(data) < 130000
        _TEXT.append((text, data, s0))
    return _TEXT[0]


_TEXT = []


@pytest.mark.parametrize("cs", [True, False])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_parity_with_the_whole_text(mode, cs):
    rng = np.random.default_rng(1700 + 10 * mode + cs)
    text, data, s0 = stream_text()
    kws = keywords_from(rng, text[:4000], mode, cs)
    a, orc = pair(mode, kws, cs)
    recs, want32 = expected(orc, data)
    want = want32.astype(np.int64)
    assert len(recs) > 300 and (want[:, 0] != recs[:, 0]).any() and max(len(k.encode()) for k in kws) > 2
    same(a.match_utf8(data, with_ids=True).astype(np.int64), want, "match_utf8")
    n = len(data)
    chunkings = [("no cut", [data]), ("one cut", split(data, [n // 2 + 1])),
                 ("twelve cuts", split(data, sorted(set(rng.integers(1, n, 12).tolist())))),
                 ("one-byte chunks", split(data, range(s0, s0 + 301))),
                 ("empty chunks", [b"", data[:s0 + 1], b"", b"", data[s0 + 1:s0 + 2], b"", data[s0 + 2:], b""]),
                 ("chunks shorter than the keywords", split(data, range(s0, s0 + 601, 2)))]
    chunkings += [("cut at %d" % c, split(data, [c])) for c in range(s0, s0 + 300)]  # every sequence at each interior byte
    for i, (what, chunks) in enumerate(chunkings):
        assert b"".join(chunks) == data
        for with_ids in (True, False):
            got, stats = feed_all(a, chunks, with_ids, final_in_last=i % 2 == 0)
            same(got, want if with_ids else want[:, :2], (what, with_ids))
            assert sum(s[0] for s in stats) == len(utf16(text)) and stats[-1][2] == 0


# ---- 2. carry boundaries inside surrogate pairs ----------------------------------------------------------------------------------
def pair_word_chars():
    """the two units of the emoji are word characters, `a` is not: the text's words are runs of emoji"""
    wc = np.zeros(65536, np.uint8)
    wc[utf16("😀")] = 1
    return wc


@pytest.mark.parametrize("family", ["AhoCorasick", "Longest", "WholeWord"])
def test_carry_boundaries_inside_surrogate_pairs(family):
    rng = np.random.default_rng(2)
    text = "".join("a😀"[int(i)] for i in rng.integers(0, 2, 260))
    data = text.encode("utf-8")
    lone = [np.concatenate([utf16("a"), utf16("😀")[:1]]), np.concatenate([utf16("😀a"), utf16("😀")[:1]])]  # a match ends inside a pair
    if family == "WholeWord":
        kws, wc = ["😀", "😀😀", "😀😀😀"], pair_word_chars()
        a = Automaton(N.MODE_WHOLEWORD, kws, True, word_chars=wc)
        orc = Oracle(FAM_WHOLEWORD, kws, True, None, wc, map_flavour=True)
    else:
        kws = ["a😀", "😀a😀", "a", "😀😀a", "aa😀a"] + lone  # 3, 5, 1, 5 and 5 units, and the two that end on a high surrogate
        mode, fam = (N.MODE_ALL, FAM_AC) if family == "AhoCorasick" else (N.MODE_LONGEST, FAM_LONGEST)
        a, orc = Automaton(mode, kws, True), Oracle(fam, kws, True, None, None, map_flavour=True)
    recs, want32 = expected(orc, data)
    want = want32.astype(np.int64)
    assert len(recs) > 50 and len(data) > 400
    if family == "AhoCorasick":  # the lone-surrogate keywords are reported, and end in the middle of a code point
        assert (np.isin(recs[:, 2], [5, 6])).sum() > 10
    same(a.match_utf8(data, with_ids=True).astype(np.int64), want, "match_utf8")
    s0 = 100
    for c in range(s0, s0 + 200):
        got, _ = feed_all(a, split(data, [c]), True, final_in_last=c % 2 == 0)
        same(got, want, ("cut at", c))
    for step in (1, 2, 3, 5):
        got, _ = feed_all(a, split(data, range(step, len(data), step)), False, final_in_last=False)
        same(got, want[:, :2], ("chunks of", step))


# ---- 3. hold or refuse, against CPython -------------------------------------------------------------------------------------------
def hold_pair():
    if not _HOLD:
        _HOLD.append(pair(N.MODE_ALL, ["ab", "b", "é", "€b", "😀", "bé"]))
    return _HOLD[0]


_HOLD = []


def agree(a, chunks):
    """-> what CPython does with the chunks, after checking that the stream does the same"""
    want = cpython(chunks)
    got = ours(a, chunks)
    assert got[:3] == want, ([c.hex() for c, _ in chunks], got[:3], want)
    return want, got[3]


def test_every_lead_and_second_byte_is_held_or_refused_as_cpython_does():
    a, _ = hold_pair()
    outcomes = set()
    for lead in range(0x80, 0x100):
        want, _ = agree(a, [(b"ab" + bytes([lead]), False), (b"", True)])
        outcomes.add((want[0], tuple(want[2])))
        for second in SECONDS:
            want, _ = agree(a, [(b"ab" + bytes([lead, second]), False), (b"", True)])
            outcomes.add((want[0], tuple(want[2])))
    # the cases' own condition: refused at once, held one or two bytes and refused at the end
    assert {(0, ()), (1, (1,)), (1, (2,))} <= outcomes


def test_three_byte_tails_are_held_or_refused_as_cpython_does():
    a, _ = hold_pair()
    held3 = 0
    for lead in range(0xF0, 0xF5):
        for second in SECONDS:
            for third in (0x7F, 0x80, 0xBF, 0xC0):
                want, _ = agree(a, [(b"ab" + bytes([lead, second, third]), False), (b"", True)])
                held3 += want[2] == [3]
    assert held3 >= 10
    # ... and three bytes under a three-byte lead are a whole sequence, or none
    for lead in (0xE0, 0xE1, 0xED, 0xEF):
        for second in SECONDS:
            agree(a, [(b"ab" + bytes([lead, second, 0x80]), False), (b"b", False), (b"", True)])


def test_a_held_prefix_completed_and_not_completed():
    a, orc = hold_pair()
    for ch in ("é", "€", "😀", "ࠀ", "퟿", "\U00010000", "\U0010ffff"):
        enc = ch.encode("utf-8")
        whole = b"ab" + enc + b"b" + enc
        want = expected(orc, whole)[1].astype(np.int64)
        # byte by byte: held grows to the sequence's length less one, then the sequence is decoded
        res, got = agree(a, [(b"ab" + enc[:1], False)] + [(enc[i:i + 1], False) for i in range(1, len(enc))] + [(b"b" + enc, False), (b"", True)])
        assert res[0] is None and res[2][:len(enc)] == list(range(1, len(enc))) + [0]
        same(got, want, (ch, "byte by byte"))
        for k in range(1, len(enc)):
            res, got = agree(a, [(b"ab" + enc[:k], False), (enc[k:] + b"b" + enc, True)])  # completed in the next feed
            assert res == (None, -1, [k, 0])
            same(got, want, (ch, k))
            # not completed: the offset reported is the lead's, which lies in the EARLIER feed
            for nxt in (b"ab", enc, enc[k:-1] + b"ab", enc[k:-1] + enc, b"\x80" * (len(enc) - k + 1)):
                res, _ = agree(a, [(b"ab" + enc[:k], False), (nxt, False), (b"", True)])
                assert res[0] == 1 and res[1] in (2, 2 + len(enc))  # (the last: the sequence is completed, a stray byte follows)
            res, _ = agree(a, [(b"ab" + enc[:k], False), (b"ab", False)])
            assert res[:2] == (1, 2)
            res, _ = agree(a, [(b"ab" + enc[:k], False), (b"", False), (b"", True)])  # held through an empty feed, refused at the end
            assert res[:2] == (2, 2) and res[2] == [k, k]
            res, _ = agree(a, [(b"ab" + enc[:k], True)])  # nothing is held at the end
            assert res[:2] == (0, 2)


def test_held_prefixes_at_lane_and_block_seams():
    """the prefix begins in one lane (16 bytes) or workgroup (4096 bytes) of the validator and the buffer ends in the next"""
    a, orc = hold_pair()
    enc = "😀".encode("utf-8")
    for pad in list(range(10, 36)) + [4096 - 2 + d for d in range(-3, 5)] + [8192 + d for d in range(-3, 3)]:
        body = b"ab" * (pad // 2) + b"x" * (pad % 2)
        whole = body + enc + b"ab"
        want = expected(orc, whole)[1].astype(np.int64)
        for k in (1, 2, 3):
            res, got = agree(a, [(body + enc[:k], False), (enc[k:] + b"ab", False), (b"", True)])
            assert res[0] is None and res[2][0] == k
            same(got, want, (pad, k))
            res, _ = agree(a, [(body + enc[:k], False), (b"ab", False)])
            assert res[:2] == (1, pad)


# ---- 4. after ACGPU_E_ENCODING ------------------------------------------------------------------------------------------------------
def test_after_an_encoding_error_the_stream_is_finished_and_the_pool_usable():
    s = AhoCorasickSet(["ab", "é"], True)
    a = s.automaton
    st = Stream(a, with_ids=False)
    try:
        assert st.feed_utf8("abé ab".encode()).tolist() == [[0, 2], [2, 4], [5, 7]]
        with pytest.raises(Utf8Error) as e:
            st.feed_utf8(b"ab\xffab")
        assert e.value.start == 9 and e.value.haystack is None
        for chunk, final in ((b"ab", False), (b"", False), (b"", True)):
            with pytest.raises(N.AcgpuError) as inv:
                st.feed_utf8(chunk, final=final)
            assert inv.value.code == N.E_INVALID
    finally:
        st.close()
    assert s.find_all_utf8("abé".encode()).tolist() == [[0, 2], [2, 4]]
    st = Stream(a, with_ids=False)
    try:
        got = np.concatenate([st.feed_utf8("ab\xc3".encode("latin-1")), st.feed_utf8(b"\xa9ab", final=True)])
        assert got.tolist() == [[0, 2], [2, 4], [4, 6]]
    finally:
        st.close()


# ---- 5. ASCII -----------------------------------------------------------------------------------------------------------------------
def test_an_ascii_stream_is_not_remapped():
    rng = np.random.default_rng(5)
    data = bytes(rng.choice(np.frombuffer(b"abcq ", np.uint8), 50000).tolist())
    a = Automaton(N.MODE_LONGEST, ["ab", "abc", "q", "cab a", "bb"], True)
    want = a.match_utf8(data, with_ids=True).astype(np.int64)
    assert len(want) > 5000
    for cuts in ([], [25000], sorted(set(rng.integers(1, len(data), 20).tolist())), range(4090, 4110)):
        got, stats = feed_all(a, split(data, cuts), True, final_in_last=False)
        same(got, want, "ascii")
        assert all(s[1:] == (1, 0) for s in stats) and sum(s[0] for s in stats) == len(data)
    # one byte that is none: that feed says so, and the next as long as it carries the byte
    got, stats = feed_all(a, [data[:100], "é".encode(), data[100:200], data[200:]], True, final_in_last=True)
    same(got, a.match_utf8(data[:100] + "é".encode() + data[100:], with_ids=True).astype(np.int64), "one é")
    assert [s[1] for s in stats][:2] == [1, 0] and stats[3][1] == 1


# ---- 6. past 2^31 bytes -------------------------------------------------------------------------------------------------------------
def test_a_stream_runs_past_2_to_the_31_bytes():
    n = 1 << 28
    buf = np.full(n, ord("x"), np.uint8)
    buf[-2:] = np.frombuffer(b"ke", np.uint8)  # "keyw" lies across the buffer's end and its begin
    buf[:2] = np.frombuffer(b"yw", np.uint8)
    buf[1000:1002] = np.frombuffer(b"zq", np.uint8)
    a = Automaton(N.MODE_ALL, ["keyw", "zq"], True)
    L = N.lib()
    h = ctypes.c_void_p()
    assert L.acgpu_stream_open(a.handle, ctypes.byref(h)) == N.OK
    out = np.empty((16, 3), np.int32)
    got, bases = [], []
    try:
        for k in range(9):
            m, base, st = ctypes.c_uint64(0), ctypes.c_int64(-1), N.Utf8StreamStats()
            rc = L.acgpu_stream_feed_utf8(h, vp(buf), n, 1 if k == 8 else 0, N.REC_MAP, vp(out), 16, ctypes.byref(m), ctypes.byref(base), ctypes.byref(st))
            assert rc == N.OK and (st.first_bad, st.ascii, st.held) == (-1, 1, 0) and st.n_units == n
            # the buffer begins with the carried bytes: fewer than a keyword's
            assert k * n - 4 < base.value <= k * n
            bases.append(base.value)
            r = out[:m.value].astype(np.int64)
            assert (r[:, :2] >= 0).all()
            r[:, :2] += base.value
            got += r.tolist()
    finally:
        L.acgpu_stream_close(h)
    want = []
    for k in range(9):
        if k:
            want.append([k * n - 2, k * n + 2, 0])
        want.append([k * n + 1000, k * n + 1002, 1])
    assert got == want
    assert bases[0] == 0 and bases[8] > (1 << 31) - 4 and got[-1][1] > (1 << 31) and got[-2][0] > (1 << 31) - 4


# ---- 7. the facade --------------------------------------------------------------------------------------------------------------------
class CountingReader:
    def __init__(self, data):
        self._f, self.reads = io.BytesIO(data), 0

    def read(self, n):
        self.reads += 1
        return self._f.read(n)


def test_readable_facade_of_a_set_and_a_map():
    text = "she said: ünï €5 and 😀 ushers, ü😀 hers"
    data = text.encode("utf-8")
    kws = ["he", "she", "hers", "ü", "€5", "😀", "ü😀", "s"]
    s = AhoCorasickSet(kws, True)
    m = LongestMatchMap(kws, ["v%d" % i for i in range(len(kws))], True)
    am = AhoCorasickMap(kws, list(range(len(kws))), True)
    want_s = s.find_all_utf8(data).tolist()
    want_m = m.find_all_utf8(data).tolist()
    assert len(want_s) > 12 and len(want_m) > 6
    seen = []
    s.match_utf8_readable(io.BytesIO(data), lambda b, e: seen.append([b, e]) or True, chunk_bytes=7)
    assert seen == want_s
    seen = []
    m.match_utf8_readable(io.BytesIO(data), lambda b, e, v: seen.append([b, e, int(v[1:])]) or True, chunk_bytes=7)
    assert seen == want_m

    class Listener:
        def __init__(self):
            self.seen = []

        def match(self, b, e, v):
            self.seen.append([b, e, v])
            return True

    li = Listener()
    am.match_utf8_readable(io.BytesIO(data), li, chunk_bytes=7)
    assert li.seen == am.find_all_utf8(data).tolist()
    # the iterable-of-chunks form, cut inside sequences, bytes-like objects of every kind
    chunks = [data[:11], bytearray(data[11:12]), memoryview(data[12:20]), np.frombuffer(data[20:], np.uint8)]
    seen = []
    s.match_utf8_readable(iter(chunks), lambda b, e: seen.append([b, e]) or True)
    assert seen == want_s
    got = s.find_all_utf8_readable(io.BytesIO(data), chunk_bytes=5)
    assert got.dtype == np.int64 and got.tolist() == want_s
    got = m.find_all_utf8_readable(chunks)
    assert got.dtype == np.int64 and got.shape[1] == 3 and got.tolist() == want_m
    assert s.find_all_utf8_readable(io.BytesIO(b"")).shape == (0, 2) and m.find_all_utf8_readable([]).shape == (0, 3)
    # a listener that returns False at the third record gets no fourth, and nothing more is read
    for obj, want in ((s, want_s), (am, am.find_all_utf8(data).tolist())):
        r, seen = CountingReader(data), []
        obj.match_utf8_readable(r, lambda *rec: seen.append(list(rec)) or len(seen) < 3, chunk_bytes=7)
        assert seen == want[:3]
        needed = -(-max(x[1] for x in want[:3]) // 7)  # reads that bring the third record's last byte
        assert needed <= r.reads <= needed + 3 < len(data) // 7
        reads = r.reads
        assert r.read(1) and r.reads == reads + 1  # (the reader itself is not at its end)
    # ill-formed input: the global offset
    with pytest.raises(Utf8Error) as e:
        s.find_all_utf8_readable([b"she \xe2\x82", b"\xac ok ", b"\xe2\x82", b"x"])
    assert e.value.start == 11


# ---- 8. the Readable rule ------------------------------------------------------------------------------------------------------------
def test_word_table_that_is_not_fold_consistent_follows_the_unit_stream():
    """`A`, `B` and `x` are word characters, `a` and `b` are not, case-insensitive: the feeds of bytes report what the feeds of units
    report for the decoded text (the Readable loops fold in every lookup; match(String) does not), mapped to bytes"""
    rng = np.random.default_rng(8)
    wc = np.zeros(65536, np.uint8)
    for ch in "ABx":
        wc[ord(ch)] = 1
    alphabet = "aAbB xX.é😀"
    text = "".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), 3000))
    data = text.encode("utf-8")
    for mode in (N.MODE_WHOLEWORD, N.MODE_WWLONGEST):
        a = Automaton(mode, ["A", "AB", "BA", "x"], False, word_chars=wc)
        assert a.info()["fold_consistent"] == 0
        st = Stream(a, with_ids=True)
        try:
            units = st.feed(utf16(text), final=True)
        finally:
            st.close()
        want = to_bytes(units, text)
        assert len(want) > 100 and (want[:, 0] != units[:, 0]).any()
        for cuts in ([], [len(data) // 2], sorted(set(rng.integers(1, len(data), 40).tolist())), range(1000, 1060)):
            got, _ = feed_all(a, split(data, cuts), True, final_in_last=False)
            same(got, want, (mode, len(list(cuts))))
