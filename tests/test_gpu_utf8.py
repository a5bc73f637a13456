"""GPU tests of the UTF-8 entry (include/acgpu.h: acgpu_match_utf8; csrc/acgpu_utf8.hip: k_utf8_count, k_utf8_scan, k_utf8_write,
k_utf8_batch_map around the unchanged scan).  Every expected record comes from the CPU oracle on utf16(data.decode()), its positions
mapped to bytes by the header's rule, restated here over the text's code points (not through the product's own
utf8_unit_offsets); equality is exact.  Expected error positions are CPython's UnicodeDecodeError.start."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickMap, AhoCorasickSet, Automaton, LongestMatchMap, Utf8Error, WholeWordMatchSet, utf16
from oracle.oracle import FAM_AC, FAM_LONGEST, FAM_SHORTEST, FAM_WHOLEWORD, FAM_WWLONGEST, Oracle
from tests.helpers import LOWER, WORD

pytestmark = pytest.mark.gpu

MODES = {N.MODE_ALL: FAM_AC, N.MODE_LONGEST: FAM_LONGEST, N.MODE_WHOLEWORD: FAM_WHOLEWORD, N.MODE_SHORTEST: FAM_SHORTEST,
         N.MODE_WWLONGEST: FAM_WWLONGEST}
WORDY = (N.MODE_WHOLEWORD, N.MODE_WWLONGEST)
BLOCK = 4096  # bytes per workgroup of the transcoder (16 per lane)
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None

POOLS = ["abcdefghq", "éüßñàöÉÜ", "αβγδλΛЖдиФф", "中語文東京日本", "😀𝒜𐍈🙂"]
WEIGHTS = [0.45, 0.15, 0.15, 0.15, 0.10]
SEPS = [" ", ", ", "·", "。", "\n", " "]


def pair(mode, kws, cs=True):
    wc = WORD if mode in WORDY else None
    return Automaton(mode, kws, cs, word_chars=wc), Oracle(MODES[mode], kws, cs, None if cs else LOWER, wc, map_flavour=True)


def unit_map(text):
    """-> (off, length): per UTF-16 unit of `text` the byte offset of the code point that holds it, and that code point's bytes"""
    cps = np.frombuffer(text.encode("utf-32-le"), dtype=np.uint32).astype(np.int64)
    nbytes = 1 + (cps >= 0x80) + (cps >= 0x800) + (cps >= 0x10000)
    units = 1 + (cps >= 0x10000)
    return np.repeat(np.cumsum(nbytes) - nbytes, units), np.repeat(nbytes, units)


def to_bytes(recs, text):
    """the mapping rule: start -> first byte of the code point that holds unit start, end -> one past the last byte of the code
    point that holds unit end - 1"""
    off, length = unit_map(text)
    want = recs.copy()
    if len(recs):
        want[:, 0] = off[recs[:, 0]]
        want[:, 1] = off[recs[:, 1] - 1] + length[recs[:, 1] - 1]
    return want


def expected(orc, data):
    """-> (records in units, records in bytes)"""
    text = bytes(data).decode("utf-8")
    recs = orc.match(utf16(text), cap=max(1024, len(text)))
    return recs, to_bytes(recs, text)


def check(a, orc, data, kinds=(True, False)):
    """match_utf8 against the oracle -> (records in units, stats)"""
    recs, want = expected(orc, data)
    st = N.Utf8Stats()
    for with_ids in kinds:
        got = a.match_utf8(data, with_ids=with_ids, stats=st)
        w = want if with_ids else want[:, :2]
        assert got.shape == w.shape and got.dtype == np.int32, (got.shape, w.shape)
        bad = np.flatnonzero((got != w).any(axis=1))
        assert not len(bad), (bad[:5], got[bad[:5]], w[bad[:5]])
        assert (st.n_units, st.first_bad) == (len(utf16(bytes(data).decode())), -1)
    return recs, st


def mixed_text(rng, n_chars):
    """words of one script each -- ASCII, Latin-1 letters, Greek / Cyrillic, CJK, astral -- with separators between them"""
    parts, n = [], 0
    while n < n_chars:
        pool = POOLS[int(rng.choice(len(POOLS), p=WEIGHTS))]
        word = "".join(pool[int(i)] for i in rng.integers(0, len(pool), int(rng.integers(1, 7))))
        sep = SEPS[int(rng.integers(len(SEPS)))]
        parts += [word, sep]
        n += len(word) + len(sep)
    return "".join(parts)


def big_text():
    """about 300 000 bytes, generated once"""
    if not _BIG:
        _BIG.append(mixed_text(np.random.default_rng(1000), 170000))
    return _BIG[0]


_BIG = []


def keywords_from(rng, text, mode, cs):
    """keywords drawn from the text: slices of its characters -- for the word matchers, whole words of word characters (and for
    WholeWordLongest phrases of two) -- and "q", which the 3-byte text is made of"""
    kws = ["q"]
    if mode in WORDY:
        toks = [t for t in text.replace(",", " ").replace("·", " ").replace("。", " ").split() if all(WORD[u] for u in utf16(t))]
        for _ in range(40):
            i = int(rng.integers(len(toks)))
            kws.append(toks[i])
        if mode == N.MODE_WWLONGEST:
            for _ in range(4):
                i = text.index(" ", int(rng.integers(len(text) // 2)))
                kws.append(text[i + 1:text.index(" ", text.index(" ", i + 1) + 1)])
    else:
        for _ in range(14):
            i, ln = int(rng.integers(len(text) - 6)), int(rng.integers(1, 6))
            kws.append(text[i:i + ln])
    if not cs:  # the other case, where that is a character for a character
        kws = [k.swapcase() if len(k.swapcase()) == len(k) and rng.integers(2) else k for k in kws]
    return [k for k in kws if k.strip()] + [kws[1]]  # (a duplicate)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [True, False])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_parity_with_the_decoded_text(mode, cs):
    rng = np.random.default_rng(1000 + 10 * mode + cs)
    big = big_text()
    kws = keywords_from(rng, big[:4000], mode, cs)
    a, orc = pair(mode, kws, cs)
    texts = ["§q", big[:150], big[:1000], big[:20000], big]
    assert len(texts[0].encode()) == 3 and 280000 < len(big.encode()) < 340000
    for text in texts:
        data = text.encode("utf-8")
        recs, st = check(a, orc, data)
        # the inputs' own condition: records, and one at least whose byte start is not its unit start
        want = to_bytes(recs, text)
        assert len(recs) and (want[:, 0] != recs[:, 0]).any(), (mode, cs, len(data))
        assert st.ascii == 0
    assert len(recs) > 500


# ---- 2. seams of the transcoder -------------------------------------------------------------------------------------------------
def seam_pair():
    if not _SEAM:
        _SEAM.append(pair(N.MODE_ALL, ["é", "€", "😀", "kw", "€😀k", "aaé"]))
    return _SEAM[0]


_SEAM = []


@pytest.mark.parametrize("pads", [range(0, 20), [BLOCK * k + d for k in (1, 2) for d in range(-3, 4)]], ids=["lanes", "blocks"])
def test_sequences_across_lane_and_block_seams(pads):
    a, orc = seam_pair()
    for p in pads:
        recs, _ = check(a, orc, ("a" * p + "é€😀kw").encode())
        assert len(recs) == 5 + (p >= 2)
        check(a, orc, ("a" * p + "😀€ékw" + "é" * 9).encode(), kinds=(True,))


def test_block_sums_scanned_in_more_than_one_round():
    """2^22 bytes and a little: 1025 blocks of 4096 bytes, five rounds of the one-workgroup scan; a non-ASCII character every 1000
    bytes, so that every block's base differs from its byte offset"""
    a, orc = pair(N.MODE_ALL, ["needle", "é", "xén"])
    period = "x" * 992 + "é" + "needle"
    assert len(period.encode()) == 1000
    data = (period * 4196).encode()
    assert (len(data) + BLOCK - 1) // BLOCK > 4 * 256
    recs, st = check(a, orc, data, kinds=(True,))
    assert len(recs) == 3 * 4196 and st.n_units == len(data) - 4196


# ---- 3. checkpoints ---------------------------------------------------------------------------------------------------------------
def test_records_at_and_around_the_checkpoints():
    """A record starts and ends at every unit; unit 32 and unit 64 are low surrogates (their checkpoints name the 4-byte sequence)"""
    text = "é" + "bcdefghijklmnopqrstuvwxyzABCDEF"[:30] + "😀" + "€" + "λ" * 10 + "中" * 10 + "xyzXYZuvw" + "𝒜" + "ß" + "€z"
    units = utf16(text)
    assert units[31] == 0xD83D and units[32] == 0xDE00 and 0xD800 <= units[63] < 0xDC00 <= units[64] < 0xE000
    chars = sorted(set(text))
    kws = chars + [np.array([0xD83D], np.uint16), np.array([0xDE00], np.uint16), utf16("𝒜")[:1], utf16("𝒜")[1:], text[29:33], "😀€", "w𝒜ß", "€z"]
    a, orc = pair(N.MODE_ALL, kws)
    recs, st = check(a, orc, text.encode())
    for u in (0, 1, 31, 32, 33, 63, 64):
        assert (recs[:, 0] == u).any() and (recs[:, 1] - 1 == u).any(), u
    assert (recs[:, 1] == units.size).any() and st.ascii == 0
    # ... and far into a text: checkpoints past the first workgroup, sequences of every length between them
    long_text = ("aé€😀" * 7 + "b") * 700
    check(*pair(N.MODE_LONGEST, ["😀aé", "€😀", "b", "é€😀a"]), long_text.encode())


# ---- 4. the mid-pair rule ---------------------------------------------------------------------------------------------------------
def test_a_match_inside_a_surrogate_pair_covers_the_code_point():
    s = AhoCorasickSet(["\ud83d", "\ude00"], True)
    assert s.find_all_utf8("a😀b".encode()).tolist() == [[1, 5], [1, 5]]
    m = AhoCorasickMap(["\ud83d", "\ude00", "😀b"], ["hi", "lo", "both"], True)
    assert m.find_all_utf8("a😀b".encode()).tolist() == [[1, 5, 0], [1, 5, 1], [1, 6, 2]]


# ---- 5. ASCII -----------------------------------------------------------------------------------------------------------------------
def test_ascii_texts_are_not_remapped():
    rng = np.random.default_rng(5)
    text = "".join(" abcdq,"[int(i)] for i in rng.integers(0, 7, 9000))
    a, orc = pair(N.MODE_LONGEST, ["ab", "abc", "q", "dd", "cab"])
    data = text.encode()
    st = N.Utf8Stats()
    for with_ids in (True, False):
        got = a.match_utf8(data, with_ids=with_ids, stats=st)
        assert len(got) > 500 and (got == a.match_host(utf16(text), with_ids=with_ids)).all()
        assert (st.ascii, st.n_units, st.first_bad) == (1, len(data), -1)
    _, st = check(a, orc, data)
    assert st.ascii == 1
    for other in (text + "é", "é" + text):
        recs, st = check(a, orc, other.encode())
        assert st.ascii == 0 and st.n_units == len(data) + 1 and len(recs) == len(got)


# ---- 6. ill-formed input ------------------------------------------------------------------------------------------------------------
ILL_FORMED = [b"\x80", b"\xbf", b"\xc3\x28", b"\xc3", b"\xe2\x82", b"\xe2\x28\xa1", b"\xf0\x9f\x98", b"\xf0\x9f\x28\x80",  # stray, missing, truncated
              b"\xc0\xaf", b"\xc1\xbf", b"\xe0\x80\xaf", b"\xe0\x9f\xbf", b"\xf0\x80\x80\xaf", b"\xf0\x8f\xbf\xbf",           # overlong
              b"\xed\xa0\x80", b"\xed\xbf\xbf",                                                                              # surrogates
              b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xf8\x88\x80\x80\x80", b"\xfe", b"\xff"]                           # above U+10FFFF


def filler(n_bytes):
    """well-formed text of exactly n_bytes bytes, sequences of every length in it"""
    return ("é€😀ab" * (n_bytes // 11) + "x" * (n_bytes % 11)).encode()


def cpython_start(buf):
    with pytest.raises(UnicodeDecodeError) as e:
        buf.decode("utf-8")
    return e.value.start


def test_ill_formed_input_reports_where_cpython_stops():
    a, orc = seam_pair()
    for bad in ILL_FORMED:
        bufs = [bad + filler(40), filler(50) + bad + filler(50), filler(45) + bad,
                filler(64 + 16 - 1) + bad + filler(30), filler(BLOCK - 1) + bad + filler(20), filler(2 * BLOCK - 2) + bad]
        if len(bad) > 2:
            bufs += [filler(32 - 2) + bad + filler(7), filler(BLOCK - 2) + bad]
        for buf in bufs:
            want = cpython_start(buf)
            with pytest.raises(Utf8Error) as e:
                a.match_utf8(buf, with_ids=True)
            assert e.value.start == want, (bad, len(buf), e.value.start, want)
    # a sequence that only the end of the text truncates, in a lane and a block of its own
    for n in (16, BLOCK):
        buf = filler(n) + "€".encode()[:2]
        with pytest.raises(Utf8Error) as e:
            a.match_utf8(buf, with_ids=False)
        assert e.value.start == cpython_start(buf) == n


def test_the_first_of_two_errors_is_reported_and_the_pool_stays_usable():
    a, orc = seam_pair()
    buf = filler(3 * BLOCK + 5) + b"\xff" + filler(100) + b"\xc0\x80" + filler(9)
    st = N.Utf8Stats()
    out = np.full((8, 3), 77, np.int32)
    n_out = ctypes.c_uint64(5)
    arr = np.frombuffer(buf, np.uint8)
    rc = N.lib().acgpu_match_utf8(a.handle, vp(arr), arr.size, N.REC_MAP, vp(out), 8, ctypes.byref(n_out), ctypes.byref(st))
    assert rc == N.E_ENCODING and n_out.value == 0 and st.first_bad == cpython_start(buf) == 3 * BLOCK + 5 and (out == 77).all()
    buf2 = filler(7) + b"\x80" + filler(5000) + b"\xed\xa0\x80"  # the later one in another workgroup
    with pytest.raises(Utf8Error) as e:
        a.match_utf8(bytearray(buf2), with_ids=False)
    assert e.value.start == 7
    recs, _ = check(a, orc, filler(3 * BLOCK + 5) + "kw €😀k".encode())
    assert len(recs) > 3 * BLOCK // 11


# ---- 7. capacity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [N.REC_SET, N.REC_MAP])
def test_overflow_reports_the_exact_count(kind):
    a, orc = seam_pair()
    data = np.frombuffer(("aé€😀kw" * 300).encode(), np.uint8)
    _, want = expected(orc, data.tobytes())
    want = want[:, :kind // 4]
    n_out = ctypes.c_uint64(0)

    def call(out, cap):
        return N.lib().acgpu_match_utf8(a.handle, vp(data), data.size, kind, vp(out), cap, ctypes.byref(n_out), None)
    assert len(want) == 1500
    out = np.zeros((len(want), kind // 4), np.int32)
    assert call(out, len(want) - 1) == N.E_OVERFLOW and n_out.value == len(want)
    assert call(None, 0) == N.E_OVERFLOW and n_out.value == len(want)  # no buffer at all: the call counts
    assert call(out, len(want)) == N.OK and n_out.value == len(want) and (out == want).all()
    assert (a.match_utf8(data, with_ids=kind == N.REC_MAP, cap=1) == want).all()  # the wrapper's retry


# ---- 8. the smallest texts ------------------------------------------------------------------------------------------------------------
def test_smallest_texts():
    a, orc = seam_pair()
    assert a.match_utf8(b"", with_ids=True).shape == (0, 3)
    recs, st = check(a, orc, "😀".encode())
    assert recs.tolist() == [[0, 2, 2]] and st.n_units == 2
    for text in ("kw" + "a" * 12 + "kw", "aé€😀kw" + "é" * 2, "a" * 12 + "😀"):
        assert len(text.encode()) == 16
        recs, _ = check(a, orc, text.encode())
        assert len(recs)
    assert a.match_utf8(b"zzzz", with_ids=False).shape == (0, 2)  # nothing found


# ---- the facade ------------------------------------------------------------------------------------------------------------------------
def test_listeners_get_the_bytes_and_byte_offsets():
    data = "Grüße aus Köln, grüße".encode()
    seen = []
    LongestMatchMap(["grüße", "köln"], ["G", "K"], False).match_utf8(data, lambda h, s, e, v: seen.append((h is data, bytes(h[s:e]).decode(), v)) or True)
    assert seen == [(True, "Grüße", "G"), (True, "Köln", "K"), (True, "grüße", "G")]
    seen = []
    s = WholeWordMatchSet(["grüße", "köln"], False)
    s.match_utf8(data, lambda h, b, e: seen.append((b, e)) and False)  # False: stops after the first
    assert seen == [(0, 7)] and s.find_all_utf8(memoryview(data)).tolist() == [[0, 7], [12, 17], [19, 26]]
    with pytest.raises(Utf8Error):
        s.find_all_utf8(data[:-1] + b"\xff")


# ---- the stream rule -------------------------------------------------------------------------------------------------------------------
def test_tickets_in_flight_refuse_the_call():
    import torch
    a, orc = seam_pair()
    text = "aé€😀kw" * 2000
    hay = utf16(text)
    d_hay = torch.from_numpy(hay.view(np.int16)).cuda()
    d_recs = torch.empty((hay.size, 3), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    tk, rc = a.match_device_begin(d_hay.data_ptr(), hay.size, True, d_recs.data_ptr(), hay.size, stream=stream.cuda_stream)
    assert rc == N.OK
    data = np.frombuffer(text.encode(), np.uint8)
    out = np.full((16, 3), 77, np.int32)
    n_out = ctypes.c_uint64(5)
    st = N.Utf8Stats(7, 7, 7, 7)
    rc = N.lib().acgpu_match_utf8(a.handle, vp(data), data.size, N.REC_MAP, vp(out), 16, ctypes.byref(n_out), ctypes.byref(st))
    assert rc == N.E_INVALID and n_out.value == 0 and (out == 77).all() and st.first_bad == -1
    m, rc, _ = a.match_device_end(tk)
    assert rc == N.OK and m == 5 * 2000
    check(a, orc, data.tobytes())
