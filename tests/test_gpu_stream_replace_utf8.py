"""GPU tests of stream replace in UTF-8 bytes (include/acgpu.h: acgpu_stream_replace_utf8; csrc/acgpu_stream.hip).  The expected
bytes are the splice of the CPU oracle's records on the decoded WHOLE text, mapped to bytes by the header's rule (the helpers of
tests/test_gpu_utf8.py), whatever the chunking; equality is exact.  What is held back is what CPython's incremental decoder holds."""
import codecs
import io

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, LongestMatchMap, LongestMatchSet, Stream, Utf8Error, WholeWordMatchSet
from oracle.oracle import FAM_WHOLEWORD, Oracle
from tests.test_gpu_utf8 import MODES, expected, keywords_from, mixed_text, pair
from tests.test_gpu_utf8_stream import pair_word_chars, seq_lengths, split, stream_text

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20),
            ("replace_slab_units", 1 << 25)]
REPLACE_MODES = sorted(m for m in MODES if m != N.MODE_ALL)


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def small_pieces():
    for k, v in (("cursor_first_piece", 64), ("cursor_max_piece", 256), ("cursor_reservoir_bytes", 4096), ("replace_slab_units", 1000)):
        N.set_tunable(k, v)


def as_bytes(r):
    return r.encode("utf-8") if isinstance(r, str) else bytes(r)


def splice_bytes(data, recs, repls):
    """data[:s_0] + repl[id_0] + data[e_0:s_1] + ... over the (n, 3) records in BYTE offsets; repls: one per keyword, or one for all"""
    if len(recs):
        assert (recs[:, 0] < recs[:, 1]).all() and (recs[1:, 0] >= recs[:-1, 1]).all() and recs[-1, 1] <= len(data)
    one = isinstance(repls, (str, bytes))
    parts, last = [], 0
    for s, e, k in recs.tolist():
        parts += [data[last:s], as_bytes(repls if one else repls[k])]
        last = e
    parts.append(data[last:])
    return b"".join(parts)


def feed_all(a, chunks, repls, final_in_last):
    """the chunks through one replace stream -> (the whole output, [(bytes fed, bytes delivered, held, replace stats dict) per feed])"""
    s = Stream(a)
    ust, st = N.Utf8StreamStats(), N.ReplaceStats()
    parts, log, fed = [], [], 0
    feeds = [(c, final_in_last and i == len(chunks) - 1) for i, c in enumerate(chunks)]
    if not final_in_last:
        feeds.append((b"", True))
    try:
        for c, final in feeds:
            parts.append(s.replace_feed_utf8(c, repls, final=final, stats=ust, replace_stats=st))
            fed += len(c)
            assert st.units_out == len(parts[-1]) and ust.first_bad == -1
            log.append((fed, sum(len(p) for p in parts), int(ust.held), {f: int(getattr(st, f)) for f, _ in N.ReplaceStats._fields_}))
    finally:
        s.close()
    return b"".join(parts), log


def same(got, want, what):
    if got != want:
        g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        n = min(g.size, w.size)
        bad = np.flatnonzero(g[:n] != w[:n])
        assert False, (what, len(got), len(want), bad[:3], got[int(bad[0]) - 8:int(bad[0]) + 8] if len(bad) else None,
                       want[int(bad[0]) - 8:int(bad[0]) + 8] if len(bad) else None)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", REPLACE_MODES)
def test_parity_with_the_whole_text(mode):
    cs = mode in (N.MODE_LONGEST, N.MODE_SHORTEST)  # (two families fold, two do not)
    rng = np.random.default_rng(1700 + 10 * mode + cs)
    text, data, s0 = stream_text()
    kws = keywords_from(rng, text[:4000], mode, cs)
    a, orc = pair(mode, kws, cs)
    recs, want_recs = expected(orc, data)
    assert len(recs) > 300 and (want_recs[:, 0] != recs[:, 0]).any() and max(len(k.encode()) for k in kws) > 2
    sets = {"str": ["«%d·é»" % i for i in range(len(kws))], "bytes": [("[%d]" % i).encode() if i % 3 else b"" for i in range(len(kws))],
            "one str": "😀", "one bytes": b"#"}
    wants = {name: splice_bytes(data, want_recs, r) for name, r in sets.items()}
    for name, r in sets.items():
        same(a.replace_utf8(data, r)[0].tobytes(), wants[name], ("replace_utf8", name))
    n = len(data)
    chunkings = [("no cut", [data]), ("one cut", split(data, [n // 2 + 1])),
                 ("twelve cuts", split(data, sorted(set(rng.integers(1, n, 12).tolist())))),
                 ("one-byte chunks", split(data, range(s0, s0 + 301))),
                 ("empty chunks", [b"", data[:s0 + 1], b"", b"", data[s0 + 1:s0 + 2], b"", data[s0 + 2:], b""]),
                 ("chunks shorter than the keywords", split(data, range(s0, s0 + 601, 2)))]
    chunkings += [("cut at %d" % c, split(data, [c])) for c in range(s0, s0 + 300)]  # every sequence at each interior byte
    names = sorted(sets)
    for i, (what, chunks) in enumerate(chunkings):
        assert b"".join(chunks) == data
        for name in (names if i < 3 else [names[i % len(names)]]):
            got, log = feed_all(a, chunks, sets[name], final_in_last=i % 2 == 0)
            same(got, wants[name], (what, name))
            assert sum(st["n_records"] for _, _, _, st in log) == len(recs) and log[-1][2] == 0


# ---- 2. a held prefix ----------------------------------------------------------------------------------------------------------------
def test_a_held_prefix_is_delivered_with_the_bytes_that_complete_it():
    a, orc = pair(N.MODE_LONGEST, ["ab", "é", "😀b"])
    repls = ["<1>", "E", "<😀>"]
    for ch in ("é", "€", "😀", "\U0010ffff"):
        enc = ch.encode("utf-8")
        whole = b"xab" + enc + b"b" + enc + b"ab"
        want = splice_bytes(whole, expected(orc, whole)[1], repls)
        for k in range(1, len(enc)):
            chunks = [b"xab" + enc[:k], enc[k:] + b"b" + enc[:1], enc[1:] + b"ab"]
            dec = codecs.getincrementaldecoder("utf-8")()
            held = []
            for c in chunks:
                dec.decode(c, False)
                held.append(len(dec.getstate()[0]))
            assert held[0] == k and held[1] == 1
            got, log = feed_all(a, chunks, repls, final_in_last=False)
            same(got, want, (ch, k))
            assert [h for _, _, h, _ in log] == held + [0]
            # the first feed: "x" and the rewrite of "ab" at the most, nothing of the cut sequence; a prefix of the result
            out1 = got[:log[0][1]]
            assert log[0][1] <= len(b"x<1>") and want.startswith(out1) and enc[:1] not in out1.replace(b"<1>", b"")
            # ... and the sequence appears, unchanged, once completed ("é" itself is a keyword: rewritten)
            if ch != "é" and ch != "😀":
                assert got.count(enc) == 2
    # held through an empty feed and through a feed that adds one byte of three
    enc = "😀".encode()
    got, log = feed_all(a, [b"ab" + enc[:1], b"", enc[1:2], enc[2:3], enc[3:] + b"b"], repls, final_in_last=True)
    assert got == b"<1><\xf0\x9f\x98\x80>" and [h for _, _, h, _ in log] == [1, 1, 2, 3, 0]


# ---- 3. surrogate pairs at every seam ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["Longest", "WholeWord"])
def test_surrogate_pairs_at_carry_and_piece_seams(family):
    """LONGEST has no left context: the unit the carry begins at, and the unit a piece ends at, may be a low surrogate"""
    rng = np.random.default_rng(3)
    text = "".join("a😀"[int(i)] for i in rng.integers(0, 2, 1200))
    data = text.encode("utf-8")
    if family == "WholeWord":
        kws, wc = ["😀", "😀😀", "😀😀😀"], pair_word_chars()
        a = Automaton(N.MODE_WHOLEWORD, kws, True, word_chars=wc)
        orc = Oracle(FAM_WHOLEWORD, kws, True, None, wc, map_flavour=True)
    else:
        kws = ["a😀", "😀a😀", "aaa", "😀😀a", "aa😀a"]
        a, orc = pair(N.MODE_LONGEST, kws)
    recs, want_recs = expected(orc, data)
    assert len(recs) > 150
    repls = ["«%d»" % i if i % 2 else "🙂" for i in range(len(kws))]
    want = splice_bytes(data, want_recs, repls)
    small_pieces()
    pieces = 0
    for c in range(1000, 1160):
        got, log = feed_all(a, split(data, [c]), repls, final_in_last=c % 2 == 0)
        same(got, want, ("cut at", c))
        pieces = max(pieces, max(st["pieces"] for _, _, _, st in log))
    assert pieces > 3  # (piece boundaries inside the feeds too)
    for step in (1, 2, 3, 5):
        got, log = feed_all(a, split(data, range(800, 1200, step)), repls, final_in_last=False)
        same(got, want, ("chunks of", step))
        # every feed's output is whole code points: the concatenation so far decodes at every seam
        assert got.decode("utf-8") == want.decode("utf-8")
        for _, delivered, _, _ in log:
            got[:delivered].decode("utf-8")


# ---- 4. the boundary at the buffer's end ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [N.MODE_LONGEST, N.MODE_SHORTEST])
def test_a_piece_boundary_at_the_end_of_the_buffer(mode):
    """one-unit keywords: no halo and no left context, a feed that is not final owns its buffer to the last unit"""
    rng = np.random.default_rng(4)
    text = mixed_text(rng, 6000)
    data = text.encode("utf-8")
    a, orc = pair(mode, ["é", "q", "中", "λ"])
    assert a.info()["max_keyword_len"] == 1
    recs, want_recs = expected(orc, data)
    assert len(recs) > 100 and seq_lengths(data) == {1, 2, 3, 4}
    repls = ["E", "", "<中中>", "l"]
    want = splice_bytes(data, want_recs, repls)
    bounds = [len(text[:i].encode()) for i in (500, 1500, 1501, 3000, 4400)]  # feeds that end on a code point's last byte
    for cuts in (bounds, sorted(set(rng.integers(1, len(data), 15).tolist())), range(2000, 2100)):
        got, log = feed_all(a, split(data, cuts), repls, final_in_last=False)
        same(got, want, (mode, list(cuts)[:3]))
        for fed, delivered_so_far, held, _ in log[:-1]:  # nothing but a held prefix is withheld
            assert held <= 3
    small_pieces()
    got, log = feed_all(a, split(data, bounds), repls, final_in_last=True)
    same(got, want, (mode, "small pieces"))


# ---- 5. ill-formed input ---------------------------------------------------------------------------------------------------------------
def test_ill_formed_input_in_the_third_feed():
    s = LongestMatchSet(["ab", "é"], True)
    a = s.automaton
    st = Stream(a)
    try:
        out = st.replace_feed_utf8("xabé ab".encode(), "#") + st.replace_feed_utf8(b" x\xc3", "#")
        assert "x#".encode() == out[:2] and len(out) <= 12
        ust = N.Utf8StreamStats()
        with pytest.raises(Utf8Error) as e:
            st.replace_feed_utf8(b"\xa9 ab\xffab", "#", stats=ust)  # (the held byte is completed; the FF is the 15th byte fed)
        assert e.value.start == 15 and ust.first_bad == 15 and (ust.n_units, ust.held) == (0, 0)
        for chunk, final in ((b"ab", False), (b"", False), (b"", True)):
            with pytest.raises(N.AcgpuError) as inv:
                st.replace_feed_utf8(chunk, "#", final=final)
            assert inv.value.code == N.E_INVALID
    finally:
        st.close()
    assert s.replace_utf8("abé x".encode(), "#") == b"## x"
    # the lead of a held prefix that the next feed fails to complete: the offset lies in the earlier feed
    st = Stream(a)
    try:
        assert st.replace_feed_utf8(b"ab ab\xe2\x82", "#").startswith(b"#")
        st.replace_feed_utf8(b"", "#")
        with pytest.raises(Utf8Error) as e:
            st.replace_feed_utf8(b"ab", "#")
        assert e.value.start == 5
    finally:
        st.close()
    assert s.replace_utf8("é".encode(), b"") == b""


# ---- 6. latency bound in bytes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", REPLACE_MODES)
def test_without_matches_a_feed_withholds_a_bounded_number_of_bytes(mode):
    """at most max_len + 1 units are withheld and one more where a pair is rounded down, of at most 4 bytes each (an upper bound:
    two units of a pair share four bytes), and 3 bytes of a cut sequence"""
    rng = np.random.default_rng(60 + mode)
    text = mixed_text(rng, 4000).replace("q", "a")
    data = text.encode("utf-8")
    kws = ["qq", "qqqqq", "q", "qéqéqéqq"]
    max_len = 8
    a, orc = pair(mode, kws)
    assert len(expected(orc, data)[0]) == 0 and a.info()["max_keyword_len"] == max_len
    cuts = sorted(set(rng.integers(1, len(data), 40).tolist()) | set(range(3000, 3060)))
    got, log = feed_all(a, split(data, cuts), "#", final_in_last=False)
    same(got, data, "no match, no change")
    for fed, delivered, held, _ in log[:-1]:
        assert fed - (4 * (max_len + 2) + 3) <= delivered <= fed - held, (fed, delivered, held)
        assert data.startswith(got[:delivered])
    assert log[-1][1] == len(data)


# ---- 7. the facade -----------------------------------------------------------------------------------------------------------------------
def test_replace_utf8_readable_of_a_set_and_a_map():
    rng = np.random.default_rng(7)
    words = ["he", "she", "hers", "ü", "€5", "😀", "ü😀", "s"]
    values = ["[%d·é]" % i for i in range(len(words))]
    text = "".join(("she said: ünï €5 and 😀 ushers, ü😀 hers. ", "😀😀 x ", "his ")[int(i)] for i in rng.integers(0, 3, 400))
    data = text.encode("utf-8")
    s, m = LongestMatchSet(words, True), LongestMatchMap(words, values, True)
    parts = list(s.replace_utf8_readable(io.BytesIO(data), "***", chunk_bytes=1000))
    assert len(parts) > len(data) // 1000 and all(isinstance(p, bytes) for p in parts) and b"".join(parts) == s.replace_utf8(data, "***")
    assert b"".join(m.replace_utf8_readable(io.BytesIO(data), chunk_bytes=1000)) == m.replace_utf8(data)
    assert b"".join(m.replace_utf8_readable(io.BytesIO(data), b"\xe2\x82\xac", chunk_bytes=7)) == m.replace_utf8(data, b"\xe2\x82\xac")
    chunks = [data[:11], bytearray(data[11:12]), memoryview(data[12:20]), np.frombuffer(data[20:], np.uint8)]
    assert b"".join(s.replace_utf8_readable(iter(chunks), b"")) == s.replace_utf8(data, b"")
    w = WholeWordMatchSet(["she", "hers", "ünï"], False)
    assert b"".join(w.replace_utf8_readable(io.BytesIO(data), "_", chunk_bytes=5)) == w.replace_utf8(data, "_")
    assert list(s.replace_utf8_readable(io.BytesIO(b""), "x")) == [b""]
    with pytest.raises(Utf8Error) as e:
        list(s.replace_utf8_readable([b"she \xe2\x82", b"\xac ok ", b"\xe2\x82", b"x"], "#"))
    assert e.value.start == 11
    g = s.replace_utf8_readable(io.BytesIO(data), "***", chunk_bytes=50)
    assert s.replace_utf8(data, "***").startswith(next(g))
    g.close()
    assert b"".join(s.replace_utf8_readable([data], "***")) == s.replace_utf8(data, "***")
