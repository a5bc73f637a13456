"""GPU tests of the UTF-8 replace entry (include/acgpu.h: acgpu_replace_utf8; csrc/acgpu_replace.hip: k_replace_emit<uint8_t> behind
the unchanged plan, csrc/acgpu_utf8.hip: k_utf8_batch_map over a piece's records and k_utf8_batch_pos for its boundary, both without a batch).  Every expected
result is the Python splice, over the BYTES, of the CPU oracle's records on utf16(data.decode()), mapped to byte offsets by the
header's rule restated here over the text's code points; equality is exact: content, n_out and st.n_records.  Every call writes
into a buffer with a canary behind its capacity."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, LongestMatchMap, Utf8Error, WholeWordMatchSet, _to_str, utf16
from oracle.oracle import FAM_LONGEST, FAM_SHORTEST, FAM_WHOLEWORD, FAM_WWLONGEST, Oracle
from tests.helpers import LOWER, WORD

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20),
            ("replace_slab_units", 1 << 25)]
MODES = {N.MODE_LONGEST: FAM_LONGEST, N.MODE_WHOLEWORD: FAM_WHOLEWORD, N.MODE_SHORTEST: FAM_SHORTEST, N.MODE_WWLONGEST: FAM_WWLONGEST}
WORDY = (N.MODE_WHOLEWORD, N.MODE_WWLONGEST)
BLOCK = 4096  # output bytes per workgroup of the emit, and bytes per workgroup of the transcoder
CANARY = 0xA5
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None

POOLS = ["abcdefghq", "éüßñàöÉÜ", "αβγδλΛЖдиФф", "中語文東京日本", "😀𝒜𐍈🙂"]
WEIGHTS = [0.45, 0.15, 0.15, 0.15, 0.10]
SEPS = [" ", ", ", "·", "。", "\n", " "]


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def pair(mode, kws, cs=True):
    wc = WORD if mode in WORDY else None
    return Automaton(mode, kws, cs, word_chars=wc), Oracle(MODES[mode], kws, cs, None if cs else LOWER, wc, map_flavour=True)


# ---- the expectation: the oracle's records, in bytes, spliced over the bytes ------------------------------------------------------
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


def as_bytes(r):
    return r.encode("utf-8") if isinstance(r, str) else bytes(r)


def records(orc, text):
    """-> (records in units, records in bytes)"""
    recs = orc.match(utf16(text), cap=max(1024, 2 * len(text)))
    return recs, to_bytes(recs, text)


def splice_bytes(data, brecs, repls):
    """data[0:s_0] + repl[id_0] + data[e_0:s_1] + ... + data[e_{k-1}:n] over byte records that neither overlap nor go back"""
    if len(brecs):
        assert (brecs[:, 0] < brecs[:, 1]).all() and (brecs[1:, 0] >= brecs[:-1, 1]).all() and brecs[-1, 1] <= len(data)
    one = not isinstance(repls, list)
    parts, last = [], 0
    for s, e, k in brecs.tolist():
        parts += [data[last:s], as_bytes(repls if one else repls[k])]
        last = e
    parts.append(data[last:])
    return b"".join(parts)


def raw(a, data, repls, cap, room=None, null_out=False):
    """one acgpu_replace_utf8 call into a canary-filled buffer of `room` bytes -> (rc, n_out, the buffer, stats dict, Utf8Stats)"""
    arr = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
    r_bytes, off, n_repl = a._replacements_utf8(repls)
    out = np.full((cap if room is None else room) + 64, CANARY, np.uint8)
    n_out = ctypes.c_uint64(12345)
    st, ust = N.ReplaceStats(), N.Utf8Stats()
    rc = N.lib().acgpu_replace_utf8(a.handle, vp(arr), len(data), vp(r_bytes), vp(off), n_repl, None if null_out else vp(out), cap,
                                    ctypes.byref(n_out), ctypes.byref(st), ctypes.byref(ust))
    return rc, int(n_out.value), out, {f: int(getattr(st, f)) for f, _ in N.ReplaceStats._fields_}, ust


def check(a, orc, text, repls, recs=None):
    """the entry, at exactly the capacity the result needs, against the splice -> (the expected bytes, stats dict, Utf8Stats)"""
    data = text.encode("utf-8")
    urecs, brecs = records(orc, text) if recs is None else recs
    want = splice_bytes(data, brecs, repls)
    rc, n_out, out, st, ust = raw(a, data, repls, len(want))
    assert rc == N.OK and n_out == len(want), (rc, n_out, len(want))
    got = out[:n_out].tobytes()
    if got != want:
        i = next(j for j in range(len(want)) if got[j] != want[j])
        raise AssertionError("byte %d of %d differs: %r, want %r" % (i, len(want), got[max(0, i - 8):i + 24], want[max(0, i - 8):i + 24]))
    assert (out[n_out:] == CANARY).all(), "written at or beyond cap"
    assert st["n_records"] == len(brecs) and st["units_out"] == len(want), st
    assert (ust.n_units, ust.first_bad, ust.ascii) == (utf16(text).size, -1, int(len(data) == len(text))) or not len(data)
    return want, st, ust


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


def family_case(mode, cs):
    """the automaton, oracle and keywords of one family and case over the big text, built once"""
    if (mode, cs) not in _FAMILY:
        rng = np.random.default_rng(1000 + 10 * mode + cs)
        kws = keywords_from(rng, big_text()[:4000], mode, cs)
        _FAMILY[(mode, cs)] = pair(mode, kws, cs) + (kws,)
    return _FAMILY[(mode, cs)]


_FAMILY = {}


def mixed_replacements(kws):
    """per keyword: empty, ASCII and short, non-ASCII and longer"""
    return [["", "r", "«%d»" % i][i % 3] for i in range(len(kws))]


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [True, False])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_parity_with_the_spliced_bytes(mode, cs):
    a, orc, kws = family_case(mode, cs)
    big = big_text()
    texts = ["§q", big[:150], big[:1000], big[:20000]]
    assert len(texts[0].encode()) == 3
    for text in texts:
        urecs, brecs = records(orc, text)
        assert len(urecs), (mode, cs, len(text))
        for repls in ("[redacted]", mixed_replacements(kws), ["" for _ in kws]):
            want, st, ust = check(a, orc, text, repls, recs=(urecs, brecs))
            assert ust.ascii == 0
            assert _to_str(a.replace_host(utf16(text), repls)[0]).encode("utf-8") == want  # the UTF-16 entry agrees
    assert len(urecs) >= 100 and (brecs[:, 0] != urecs[:, 0]).any()  # the largest text's own condition


# ---- 2. every source and destination alignment of the byte funnel shift -----------------------------------------------------------
def seam_pair():
    if not _SEAM:
        _SEAM.append(pair(N.MODE_LONGEST, ["kw", "é€"]))
    return _SEAM[0]


_SEAM = []


def seam_text(p):
    return "a" * p + "kw" + "é€😀" * 12 + "kw" + "x" * 40


def sized(n_bytes, filler):
    """a replacement of exactly n_bytes bytes, non-ASCII from 2 bytes on"""
    r = ("ß" + filler * (n_bytes - 2)) if n_bytes >= 2 else filler * n_bytes
    assert len(r.encode()) == n_bytes
    return r


def seam_checks(pads, lengths):
    a, orc = seam_pair()
    for p in pads:
        text = seam_text(p)
        recs = records(orc, text)
        assert len(recs[0]) == 14
        for ln in lengths:  # "kw" -> ln bytes: everything behind it moves by every residue mod 16; "é€" (5 bytes) -> another length
            check(a, orc, text, [sized(ln, "r"), sized((ln + 5) % 18, "s")], recs=recs)


def test_every_alignment_of_source_and_destination():
    assert len(sized(17, "r").encode()) == 17 and len(seam_text(16).encode()) > 16 + 2 + 12 * 9
    seam_checks(range(0, 33), range(0, 18))


# ---- 3. tile and slab seams -------------------------------------------------------------------------------------------------------
SEAM_PADS = [BLOCK * k + d for k in (1, 2) for d in range(-3, 4)]


def test_matches_across_tile_seams():
    seam_checks(SEAM_PADS, range(0, 18))


def test_matches_across_slab_seams():
    N.set_tunable("replace_slab_units", 1000)
    a, orc = seam_pair()
    for p in (BLOCK + 900, 2 * BLOCK - 2):
        want, _, _ = check(a, orc, seam_text(p), [sized(17, "r"), sized(0, "s")])
        assert len(want) >= 5000  # five slabs and more
    seam_checks([999, 1000, 1001, 1990, 2001], (0, 1, 5, 16, 17))


# ---- 4. many pieces -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_many_pieces(mode):
    N.set_tunable("cursor_first_piece", 64)
    N.set_tunable("cursor_max_piece", 256)
    a, orc, kws = family_case(mode, True)
    text = big_text()[:20000]
    recs = records(orc, text)
    for repls in (mixed_replacements(kws), "#"):
        _, st, _ = check(a, orc, text, repls, recs=recs)
        assert st["pieces"] > 10, st


@pytest.mark.parametrize("mode", [N.MODE_LONGEST, N.MODE_SHORTEST])
def test_piece_boundaries_inside_surrogate_pairs_and_matches(mode):
    """11 units per period against pieces of 64 and 256 units: a boundary at every phase of the period (the word matchers take no
    such keyword: a surrogate is no word character)"""
    N.set_tunable("cursor_first_piece", 64)
    N.set_tunable("cursor_max_piece", 256)
    text = ("😀é" * 3 + "kw") * 400
    a, orc = pair(mode, ["kw", "😀é😀"])
    for repls in (["<kw>", ""], ["", "€€€€"]):
        _, st, _ = check(a, orc, text, repls)
        assert st["pieces"] > 10, st


# ---- 5. more segments than a tile's LDS holds ----------------------------------------------------------------------------------------
def test_thousands_of_deleted_matches_in_one_tile():
    a, orc = pair(N.MODE_LONGEST, ["é"])
    text = "é" * 5000 + "x" + "é" * 5000
    recs = records(orc, text)
    want, st, _ = check(a, orc, text, "", recs=recs)
    assert want == b"x" and st["n_records"] == 10000
    want, _, _ = check(a, orc, text, "e", recs=recs)
    assert len(want) == 10001


# ---- 6. ASCII -----------------------------------------------------------------------------------------------------------------------
def test_ascii_texts_are_not_remapped():
    rng = np.random.default_rng(5)
    text = "".join(" abcdq,"[int(i)] for i in rng.integers(0, 7, 9000))
    kws = ["ab", "abc", "q", "dd", "cab"]
    a, orc = pair(N.MODE_LONGEST, kws)
    for repls in (["<1>", "", "QQQQQQQQQQQQQQQQQ", "é", "x"], "#"):
        want, st, ust = check(a, orc, text, repls)
        assert ust.ascii == 1 and ust.n_units == 9000 and st["n_records"] > 500
        if all(len(as_bytes(r)) == len(r) for r in repls):  # (ASCII replacements: the units of the UTF-16 entry ARE the bytes)
            assert a.replace_host(utf16(text), repls)[0].astype(np.uint8).tobytes() == want


# ---- 7. ill-formed input ------------------------------------------------------------------------------------------------------------
def filler(n_bytes):
    """well-formed text of exactly n_bytes bytes, sequences of every length in it"""
    return ("é€😀ab" * (n_bytes // 11) + "x" * (n_bytes % 11)).encode()


def test_ill_formed_input_is_refused_and_the_pool_stays_usable():
    a, orc = seam_pair()
    buf = filler(3 * BLOCK + 5) + b"\xff" + filler(100) + b"\xc0\x80" + filler(9)
    with pytest.raises(UnicodeDecodeError) as e:
        buf.decode("utf-8")
    rc, n_out, out, st, ust = raw(a, buf, "#", len(buf))
    assert rc == N.E_ENCODING and n_out == 0 and ust.first_bad == e.value.start == 3 * BLOCK + 5 and (out == CANARY).all()
    assert (ust.n_units, ust.ascii) == (0, 0)
    with pytest.raises(Utf8Error) as e2:
        a.replace_utf8(bytearray(buf), "#")
    assert e2.value.start == 3 * BLOCK + 5
    with pytest.raises(Utf8Error):
        WholeWordMatchSet(["grüße"], False).replace_utf8(b"gr\xfc\xdfe", "*")
    want, st, _ = check(a, orc, filler(3 * BLOCK + 5).decode() + "kw é€k", ["<kw>", ""])
    assert st["n_records"] > 3 * BLOCK // 11


# ---- 8. capacity ----------------------------------------------------------------------------------------------------------------------
def test_overflow_reports_the_exact_size_and_writes_nothing_beyond_cap():
    a, orc = seam_pair()
    text = "aé€😀kw" * 300
    data = text.encode()
    repls = ["<keyword>", "€"]
    want, _, _ = check(a, orc, text, repls)  # cap == need: exact
    need = len(want)
    assert need > len(data)
    rc, n_out, out, st, _ = raw(a, data, repls, need - 1, room=need + 100)
    assert rc == N.E_OVERFLOW and n_out == need == st["units_out"] and (out[need - 1:] == CANARY).all()
    rc, n_out, out, st, _ = raw(a, data, repls, need // 2, room=need)
    assert rc == N.E_OVERFLOW and n_out == need and (out[need // 2:] == CANARY).all()
    rc, n_out, out, st, _ = raw(a, data, repls, 0, null_out=True)  # no buffer at all: the call counts
    assert rc == N.E_OVERFLOW and n_out == need and st["n_records"] == 600
    got, st = a.replace_utf8(data, repls, cap=1)  # the wrapper's retry
    assert got.tobytes() == want and st["units_out"] == need


# ---- 9. the smallest texts ------------------------------------------------------------------------------------------------------------
def test_smallest_texts():
    a, orc = pair(N.MODE_LONGEST, ["q", "😀", "0123456789abcdef"])
    for repls in (["<Q>", "€", ""], ["", "", "0123456789abcdefg"], "é"):
        for text in ("q", "z", "é", "😀", "0123456789abcdef", "0123456789abcde", "zzzz zzzz zzzz zzzz z"):
            want, st, _ = check(a, orc, text, repls)
            if st["n_records"] == 0:
                assert want == text.encode()  # no match: returned unchanged
    assert check(a, orc, "😀", ["", "", ""])[0] == b"" and check(a, orc, "0123456789abcdef", "")[0] == b""
    assert a.replace_utf8(b"", "x")[0].size == 0


# ---- 10. the facade --------------------------------------------------------------------------------------------------------------------
def test_the_facade_takes_and_returns_bytes():
    data = "Grüße aus Köln, grüße".encode()
    s = WholeWordMatchSet(["grüße", "köln"], False)
    assert s.replace_utf8(data, "***") == b"*** aus ***, ***"
    assert s.replace_utf8(memoryview(data), b"\xe2\x82\xac") == "€ aus €, €".encode()
    assert s.replace_utf8(bytearray(data), "") == b" aus , "
    m = LongestMatchMap(["grüße", "köln"], ["<G>", "<K>"], False)
    assert m.replace_utf8(data) == b"<G> aus <K>, <G>"
    assert m.replace_utf8(np.frombuffer(data, np.uint8), ["ö", b""]) == "ö aus , ö".encode()
    assert m.replace_utf8(data, "#") == b"# aus #, #" and m.replace_utf8(data, b"#") == b"# aus #, #"
    assert m.replace_utf8(data) == m.replace(data.decode()).encode()


# ---- 11. the stream rule ---------------------------------------------------------------------------------------------------------------
def test_tickets_in_flight_refuse_the_call():
    import torch
    a, orc = pair(N.MODE_WHOLEWORD, ["kw", "aé"])  # (a family whose ticket is enqueued, not run to its end inside _begin)
    text = "aé € 😀 kw " * 2000
    hay = utf16(text)
    d_hay = torch.from_numpy(hay.view(np.int16)).cuda()
    d_recs = torch.empty((hay.size, 3), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    tk, rc = a.match_device_begin(d_hay.data_ptr(), hay.size, True, d_recs.data_ptr(), hay.size, stream=stream.cuda_stream)
    assert rc == N.OK
    rc, n_out, out, st, ust = raw(a, text.encode(), "#", 64)
    assert rc == N.E_INVALID and n_out == 0 and (out == CANARY).all() and ust.first_bad == -1 and st["n_records"] == 0
    m, rc, _ = a.match_device_end(tk)
    assert rc == N.OK and m == 2 * 2000
    check(a, orc, text, ["<kw>", ""])
