"""GPU tests of the lossy streams (include/acgpu.h: acgpu_stream_feed_utf8_lossy, acgpu_stream_replace_utf8_lossy;
csrc/acgpu_stream.hip: feed_utf8, stream_replace_utf8, the lossy walk of byte_feed_commit; csrc/acgpu_utf8.hip:
k_utf8_lossy_open_count, the validator that is both lossy and open).  One text T of about 8.5 KB -- every row of the table of
tests/utf8_lossy_ref.py, and 2-, 3- and 4-byte sequences, across the wave seam at 1024 and the workgroup seam at 4096 -- is fed
under many chunkings.  Every expected record comes from the CPU oracle on the text that the reference decodes from T as a whole,
mapped to bytes through the reference's per-unit table; every expected output is the Python splice of those records over T's
original bytes; what a feed holds back is the claim rule of the header, restated over the last three bytes fed (held_ref, checked
against CPython's incremental decoder in tests/test_utf8_lossy_more_cpu.py).  Equality is exact."""
import io

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickMap, AhoCorasickSet, LongestMatchMap, LongestMatchSet, Stream, Utf8Error
from tests.test_gpu_utf8 import MODES, WORDY, mixed_text, pair
from tests.test_gpu_utf8_lossy import fuzz_keywords
from tests.test_utf8_lossy_more_cpu import held_ref, lossy_records, splice
from tests.utf8_lossy_ref import TABLE, decode_replace

pytestmark = pytest.mark.gpu

ROWS = [row for row, _ in TABLE]
WINDOWS = ((1008, 1040), (4080, 4112))
REPLACE_MODES = [m for m in sorted(MODES) if m != N.MODE_ALL]
PREFIXES = [(b"\xc3", 1, 1), (b"\xe2\x82", 2, 1), (b"\xf0\x9f", 2, 1), (b"\xf0\x9f\x98", 3, 1), (b"\xed", 1, 1), (b"\xed\xa0", 0, 2)]


# ---- the text ----------------------------------------------------------------------------------------------------------------------
def the_text():
    """-> (T, the valid text its filler comes from)"""
    if not _TEXT:
        rng = np.random.default_rng(2024)
        valid = mixed_text(rng, 4000)
        vb = valid.encode()
        knot1 = b"A" + ROWS[0] + "é".encode() + ROWS[5] + b"(" + "€".encode() + ROWS[6] + "😀".encode() + ROWS[3] + b"AA" + ROWS[8] + b"A(" + "é😀".encode()
        knot2 = b"A" + ROWS[1] + "😀".encode() + ROWS[2] + b"AA(" + ROWS[7] + b"(" + "€".encode() + ROWS[4] + b"A" + ROWS[9] + b" A" + "é€".encode() + b"\x80("

        def filler(n, seed):
            r = np.random.default_rng(seed)
            buf = bytearray()
            while len(buf) < n:
                i = int(r.integers(len(vb) - 80))
                buf += vb[i:i + int(r.integers(20, 80))]  # cut anywhere, inside sequences too
                buf += [b" A\xe2\x82(", b"A\x80\x80 ", b" \xf0\x9f\x98A", b"\xc0 A(", b" A", b"( "][int(r.integers(6))]
            return bytes(buf[:n - 2]) + b" A"
        t = filler(1007, 1) + knot1
        t += filler(4077 - len(t), 2) + knot2
        t += filler(8500 - len(t), 3) + b"".join(b"A" + row + b"(" for row in ROWS) + b" tail A\xf0\x9f\x98"
        for lo, hi in WINDOWS:  # damaged bytes and sequences of every length begin inside both windows
            _, off, length, replaced = decode_replace(t)
            inside = (off >= lo) & (off < hi)
            assert replaced[inside].sum() >= 8 and {2, 3, 4} <= set(length[inside & ~replaced].tolist()), (lo, hi)
            assert set(length[inside & replaced].tolist()) == {1, 2, 3}
        assert 2 * 4096 + 300 < len(t) < 9000 and all(row in t for row in ROWS)
        _TEXT.append((t, valid))
    return _TEXT[0]


_TEXT = []


def chunkings():
    t, _ = the_text()
    out = [("cut at %d" % c, [t[:c], t[c:]]) for lo, hi in WINDOWS for c in range(lo, hi + 1)]
    out += [("chunks of %d" % k, [t[i:i + k] for i in range(0, len(t), k)]) for k in (1, 2, 3, 5, 17)]
    return out


def family(mode):
    """(automaton, oracle, records of T in bytes, the reference's table of T), once per family"""
    if mode not in _FAMILY:
        t, valid = the_text()
        a, orc = pair(mode, fuzz_keywords(mode, True, valid), True)
        want = lossy_records(orc, t)
        tab = decode_replace(t)
        # the inputs' own conditions: something replaced, records that touch a replaced subpart
        edge = np.zeros(len(t) + 2, bool)
        for o, n in zip(tab[1][tab[3]].tolist(), tab[2][tab[3]].tolist()):
            edge[o + 1:o + n + 1] = True
        assert tab[3].sum() > 100 and sum(1 for s, e, _ in want.tolist() if edge[s:e + 2].any()) >= 20 and len(want) > 150
        _FAMILY[mode] = (a, orc, want.astype(np.int64), tab)
    return _FAMILY[mode]


_FAMILY = {}


def same(got, want, what):
    assert got.dtype == np.int64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (what, bad[:5], got[bad[:5]], want[bad[:5]])


def spanning(want, chunks):
    """the records that span a feed boundary"""
    edges = np.cumsum([len(c) for c in chunks])[:-1]
    return sum(1 for s, e, _ in want.tolist() if ((edges > s) & (edges < e)).any())


def feed_all(a, chunks, with_ids=True, final_in_last=False):
    """-> (records in global byte offsets, [(n_units, n_replaced, ascii, held) per feed])"""
    st = N.Utf8LossyStreamStats()
    s = Stream(a, with_ids=with_ids)
    pages, stats = [], []
    try:
        for i, c in enumerate(chunks):
            pages.append(s.feed_utf8(c, final=final_in_last and i == len(chunks) - 1, stats=st, errors="replace"))
            stats.append((st.n_units, st.n_replaced, st.ascii, st.held))
        if not final_in_last:
            pages.append(s.feed_utf8(b"", final=True, stats=st, errors="replace"))
            stats.append((st.n_units, st.n_replaced, st.ascii, st.held))
    finally:
        s.close()
    return np.concatenate(pages), stats


def replace_all(a, chunks, repls, final_in_last=False):
    """-> (the concatenated output, [(n_units, n_replaced, held) per feed], the parts)"""
    st = N.Utf8LossyStreamStats()
    s = Stream(a)
    parts, stats = [], []
    try:
        for i, c in enumerate(chunks):
            parts.append(s.replace_feed_utf8(c, repls, final=final_in_last and i == len(chunks) - 1, stats=st, errors="replace"))
            stats.append((st.n_units, st.n_replaced, st.held))
        if not final_in_last:
            parts.append(s.replace_feed_utf8(b"", repls, final=True, stats=st, errors="replace"))
            stats.append((st.n_units, st.n_replaced, st.held))
    finally:
        s.close()
    return b"".join(parts), stats, parts


def check_stats(stats, chunks, tab, held_at):
    """the sums over the feeds are the whole text's; every feed that is not final holds what the claim rule says"""
    assert sum(s[0] for s in stats) == len(tab[1]) and sum(s[1] for s in stats) == int(tab[3].sum())
    fed = bytearray()
    for i, c in enumerate(chunks):
        fed += c
        last = i == len(stats) - 1  # (the final feed holds nothing)
        assert stats[i][held_at] == (0 if last else held_ref(fed)), (i, bytes(fed[-4:]), stats[i])
    assert stats[-1][held_at] == 0


def mixed_replacements(kws):
    pool = ["", "#", "<<é>>", b"\xff", b"", "😀!", b"[\xe2\x82]", "long replacement, longer than any keyword"]
    return [pool[i % len(pool)] for i in range(len(kws))]


def table_of(repls):
    return [r.encode() if isinstance(r, str) else bytes(r) for r in repls]


# ---- 1. every chunking: records, stats, held ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["two chunks", "chunks of 1", "chunks of 2", "chunks of 3", "chunks of 5", "chunks of 17"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_the_records_of_every_chunking_are_the_one_shot_records(mode, what):
    a, orc, want, tab = family(mode)
    t, _ = the_text()
    if what == "chunks of 1":  # the one-shot entry itself, once per family
        st = N.Utf8LossyStats()
        same(a.match_utf8(t, with_ids=True, stats=st, errors="replace").astype(np.int64), want, "match_utf8")
        assert (st.n_units, st.n_replaced) == (len(tab[1]), int(tab[3].sum()))
    todo = [c for c in chunkings() if (c[0].startswith("cut at") if what == "two chunks" else c[0] == what)]
    assert len(todo) == (66 if what == "two chunks" else 1)
    n_span = 0
    for i, (name, chunks) in enumerate(todo):
        assert b"".join(chunks) == t
        got, stats = feed_all(a, chunks, final_in_last=i % 2 == 1)
        same(got, want, name)
        check_stats(stats, chunks, tab, 3)
        n_span += spanning(want, chunks)
    assert n_span >= 1, "no record spans a feed boundary"
    if what == "chunks of 17":  # Set records, once per family
        same(feed_all(a, todo[0][1], with_ids=False)[0], want[:, :2], "set records")


@pytest.mark.parametrize("what", ["two chunks", "chunks of 1", "chunks of 2", "chunks of 3", "chunks of 5", "chunks of 17"])
@pytest.mark.parametrize("mode", REPLACE_MODES)
def test_the_output_of_every_chunking_is_the_one_shot_replace(mode, what):
    a, orc, want, tab = family(mode)
    t, _ = the_text()
    repls = mixed_replacements(a.keywords)
    whole = splice(t, want.astype(np.int32), table_of(repls))
    if what == "chunks of 1":  # the one-shot entry itself, once per family
        assert a.replace_utf8(t, repls, errors="replace")[0].tobytes() == whole
    todo = [c for c in chunkings() if (c[0].startswith("cut at") if what == "two chunks" else c[0] == what)]
    for i, (name, chunks) in enumerate(todo):
        got, stats, parts = replace_all(a, chunks, repls, final_in_last=i % 2 == 1)
        assert got == whole, (name, next(j for j in range(len(whole)) if got[j:j + 1] != whole[j:j + 1]))
        check_stats(stats, chunks, tab, 2)
    assert sum(spanning(want, chunks) for _, chunks in todo) >= 1, "no record spans a feed boundary"


# ---- 2. the end of the stream --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix,held,n_fffd", PREFIXES)
def test_a_stream_that_ends_in_a_proper_prefix_flushes_it_as_replacement_characters(prefix, held, n_fffd):
    a, orc = pair(N.MODE_ALL, ["�", "A", "A�"])
    assert int(decode_replace(prefix)[3].sum()) == n_fffd == len(decode_replace(prefix)[0])
    for head in (b"", b"xA", ("é" * 2050).encode() + b"A"):  # (the last: the prefix begins at byte 4101, in the second workgroup)
        data = head + prefix
        want = lossy_records(orc, data).astype(np.int64)
        for chunks in ([data], [head, prefix], [data[:-1], data[-1:]]):
            chunks = [c for c in chunks if c]
            got, stats = feed_all(a, chunks)
            same(got, want, (head[:4], prefix, len(chunks)))
            # the last feed with bytes holds the prefix, but for ED A0, which is two U+FFFD at once; the final feed flushes it
            assert stats[-2][3] == held and stats[-1][:2] == ((n_fffd, n_fffd) if held else (0, 0)) and stats[-1][3] == 0
            assert sum(s[1] for s in stats) == n_fffd
            got, stats = feed_all(a, chunks, final_in_last=True)
            same(got, want, (head[:4], prefix, "final in the last feed"))
            assert stats[-1][3] == 0 and sum(s[1] for s in stats) == n_fffd
        s = LongestMatchSet(["�", "A"], True)
        assert b"".join(s.replace_utf8_readable([head, prefix], "?", errors="replace")) == head.replace(b"A", b"?") + b"?" * n_fffd
        # the prefix is never delivered before the final feed decides it
        st = Stream(s._auto)
        try:
            first = st.replace_feed_utf8(data, "?", errors="replace")
            last = st.replace_feed_utf8(b"", "?", final=True, errors="replace")
        finally:
            st.close()
        assert first + last == head.replace(b"A", b"?") + b"?" * n_fffd and (not held or len(first) <= len(head))


def test_a_keyword_across_a_boundary_whose_left_side_is_a_held_prefix_found_ill_formed():
    m = LongestMatchMap(["�A", "€A"], ["bad", "euro"], True)
    for chunks, want in (([b"xx\xe2\x82", b"Ayy"], [[2, 5, 0]]), ([b"xx\xe2", b"\x82", b"Ayy"], [[2, 5, 0]]), ([b"xx\xe2\x82", b"\xacAyy"], [[2, 6, 1]]),
                         ([b"xx\xf0\x9f\x98", b"Ayy"], [[2, 6, 0]]), ([b"xx\xf0", b"\x9f", b"\x98", b"A"], [[2, 6, 0]]),
                         ([b"xx\xed\xa0", b"A"], [[3, 5, 0]])):
        assert m.find_all_utf8_readable(chunks, errors="replace").tolist() == want, chunks
        assert m.find_all_utf8(b"".join(chunks), errors="replace").tolist() == want, chunks
        got = b"".join(m.replace_utf8_readable(chunks, errors="replace"))
        assert got == splice(b"".join(chunks), np.array(want, np.int32), [b"bad", b"euro"]), chunks
    st, s = N.Utf8LossyStreamStats(), Stream(m._auto)
    try:
        assert s.feed_utf8(b"xx\xe2\x82", stats=st, errors="replace").tolist() == [] and (st.n_units, st.n_replaced, st.held) == (2, 0, 2)
        got = s.feed_utf8(b"Ayy", stats=st, errors="replace").tolist()  # (whichever of the two feeds finds the record decidable)
        assert (st.n_units, st.n_replaced, st.held) == (4, 1, 0)
        got += s.feed_utf8(b"", final=True, stats=st, errors="replace").tolist()
        assert got == [[2, 5, 0]] and (st.n_units, st.n_replaced, st.held) == (0, 0, 0)
    finally:
        s.close()


# ---- 3. the facade -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_LONGEST])
def test_the_readable_methods_over_an_iterable_of_chunks(mode):
    a, orc, want, tab = family(mode)
    t, valid = the_text()
    kws = fuzz_keywords(mode, True, valid)
    chunks = [t[i:i + 1000] for i in range(0, len(t), 1000)]
    f, m = (AhoCorasickSet, AhoCorasickMap) if mode == N.MODE_ALL else (LongestMatchSet, LongestMatchMap)
    s, mp = f(kws, True), m(kws, list(range(len(kws))), True)
    same(s.find_all_utf8_readable(chunks, errors="replace"), want[:, :2], "set, iterable")
    same(mp.find_all_utf8_readable(io.BytesIO(t), chunk_bytes=777, errors="replace"), want, "map, file object")
    seen = []
    mp.match_utf8_readable(iter(chunks), lambda b, e, v: seen.append((b, e, v)) or True, errors="replace")
    assert seen == [tuple(r) for r in want.tolist()]
    seen = []
    s.match_utf8_readable(chunks, lambda b, e: seen.append((b, e)) or len(seen) < 7, errors="replace")
    assert seen == [tuple(r[:2]) for r in want[:7].tolist()]
    if mode == N.MODE_LONGEST:
        assert b"".join(s.replace_utf8_readable(chunks, "#", errors="replace")) == splice(t, want.astype(np.int32), b"#")
        repls = ["<%d>" % i for i in range(len(kws))]
        got = b"".join(mp.replace_utf8_readable(io.BytesIO(t), repls, chunk_bytes=333, errors="replace"))
        assert got == splice(t, want.astype(np.int32), [r.encode() for r in repls])


def test_a_strict_stream_still_raises_at_the_same_global_offset():
    a, orc, want, tab = family(N.MODE_LONGEST)
    t, _ = the_text()
    first = int(tab[1][tab[3]][0])
    with pytest.raises(UnicodeDecodeError) as e:
        t.decode("utf-8")
    assert e.value.start == first > 20
    for k in (17, 1000, len(t)):
        s = Stream(a)
        try:
            with pytest.raises(Utf8Error) as e:
                for i in range(0, len(t), k):
                    s.feed_utf8(t[i:i + k])
            assert e.value.start == first
        finally:
            s.close()
        gen = LongestMatchSet(["A"], True).replace_utf8_readable([t[i:i + k] for i in range(0, len(t), k)], "#")
        with pytest.raises(Utf8Error) as e:
            b"".join(gen)
        assert e.value.start == first
    same(feed_all(a, [t[:4000], t[4000:]])[0], want, "the lossy feed behind the refusals")  # the pool is as usable as ever
