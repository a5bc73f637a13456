"""Development tool: what a caller pays who reads a UTF-8 text in chunks, one box, one process --
  stream : one Stream fed the chunks as bytes (acgpu_stream_feed_utf8: carry + chunk copied, validated + transcoded, scanned,
           remapped on the device, records in global byte offsets); `calls` beside it: the same feeds through the C entry alone,
           records left as they come (int32 relative to *base) -- what Stream.feed_utf8 adds is their conversion to int64 arrays;
  whole  : acgpu_match_utf8 on the whole text in one call (what the chunked form is measured against; needs the text in one piece
           and below 2^31 bytes);
  host   : what the same caller does without the entry: codecs' incremental decoder per chunk -> utf16() -> Stream.feed ->
           the records' unit positions mapped back to bytes on the host (one table for the whole text, built chunk by chunk from
           strings.utf8_unit_offsets -- a caller that cannot keep such a table pays more).
All three on the 19.4 MB mixed text of tools/utf8_rate.py and its automaton (WholeWordMatch over the README word list), Map records,
capacity known (no overflow retry timed), the three results compared.  Chunks are cut at multiples of the chunk size, wherever
that falls in a sequence.
--errors replace: the stream fed through acgpu_stream_feed_utf8_lossy against acgpu_match_utf8_lossy on the whole
text -- beside the strict stream where the text is well-formed, and with --damage on a copy in which about one byte per KB is
overwritten with a random byte from 0x80..0xFF (the strict entries refuse that one).
usage: utf8_stream_rate.py [--log2 24] [--chunks 65536,1048576,4194304] [--reps 3] [--errors strict|replace] [--damage]"""
import argparse, codecs, ctypes, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ahocorasick_amd import _native as N, synth
from ahocorasick_amd.strings import Automaton, Stream, _to_str, utf16, utf8_unit_offsets
from ahocorasick_amd.unicode_tables import default_word_chars

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=24, help="bytes of the text before the non-ASCII tokens go in, about")
ap.add_argument("--chunks", default="65536,1048576,4194304")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--errors", default="strict", choices=["strict", "replace"])
ap.add_argument("--damage", action="store_true", help="with --errors replace: overwrite about one byte per KB")
args = ap.parse_args()

EXTRA = ["Zürich", "naïve", "straße", "λόγος", "Москва", "東京", "데이터", "😀", "𝒜𝓃𝓈"]  # (tools/utf8_rate.py)


def mixed_text(n_bytes):
    words = synth.readme_dictionary()
    toks = _to_str(synth.readme_text(2006, n_bytes, words)).split(" ")
    mixed = " ".join(t if i % 6 else t + " " + EXTRA[(i // 6) % len(EXTRA)] for i, t in enumerate(toks))
    return words, mixed.encode("utf-8")


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, out


def stream_bytes(a, data, chunk, cap, errors="strict"):
    st = Stream(a, with_ids=True)
    try:
        pages = [st.feed_utf8(data[i:i + chunk], final=i + chunk >= len(data), cap=cap, errors=errors) for i in range(0, len(data), chunk)]
    finally:
        st.close()
    return np.concatenate(pages)


def stream_calls(a, data, chunk, cap):
    """the feeds of stream_bytes through acgpu_stream_feed_utf8 itself -> the number of records"""
    L, h = N.lib(), ctypes.c_void_p()
    N.check(L.acgpu_stream_open(a.handle, ctypes.byref(h)), "acgpu_stream_open")
    buf, out = np.frombuffer(data, np.uint8), np.empty((cap, 3), np.int32)
    total, m, base = 0, ctypes.c_uint64(0), ctypes.c_int64(0)
    try:
        for i in range(0, len(data), chunk):
            piece = buf[i:i + chunk]
            N.check(L.acgpu_stream_feed_utf8(h, piece.ctypes.data_as(ctypes.c_void_p), piece.size, 1 if i + chunk >= len(data) else 0, N.REC_MAP,
                                             out.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(m), ctypes.byref(base), None), "acgpu_stream_feed_utf8")
            total += m.value
    finally:
        L.acgpu_stream_close(h)
    return total


def stream_host(a, data, chunk, cap, split):
    """-> records in byte offsets; split: a dict that receives the host steps' seconds"""
    dec = codecs.getincrementaldecoder("utf-8")()
    st = Stream(a, with_ids=True)
    pages, offs, pos = [], [], 0
    t = dict(decode=0.0, utf16=0.0, feed=0.0, remap=0.0)
    try:
        for i in range(0, len(data), chunk):
            piece, final = data[i:i + chunk], i + chunk >= len(data)
            t0 = time.perf_counter()
            pending = len(dec.getstate()[0])
            text = dec.decode(piece, final)
            t1 = time.perf_counter()
            units = utf16(text)
            t2 = time.perf_counter()
            pages.append(st.feed(units, final=final, cap=cap))
            t3 = time.perf_counter()
            consumed = pending + len(piece) - len(dec.getstate()[0])
            offs.append(utf8_unit_offsets(data[pos:pos + consumed]) + pos)
            pos += consumed
            t4 = time.perf_counter()
            t["decode"] += t1 - t0
            t["utf16"] += t2 - t1
            t["feed"] += t3 - t2
            t["remap"] += t4 - t3
    finally:
        st.close()
    t0 = time.perf_counter()
    recs, off, b = np.concatenate(pages), np.concatenate(offs), np.frombuffer(data, np.uint8)
    last = off[recs[:, 1] - 1]
    lead = b[last]
    out = recs.copy()
    out[:, 0] = off[recs[:, 0]]
    out[:, 1] = last + 1 + (lead >= 0xC0) + (lead >= 0xE0) + (lead >= 0xF0)
    t["remap"] += time.perf_counter() - t0
    split.update(t)
    return out


def damage(data, seed=7):
    """a copy with about one byte per KB overwritten by a byte from 0x80..0xFF (tools/utf8_rate.py)"""
    rng = np.random.default_rng(seed)
    b = np.frombuffer(data, np.uint8).copy()
    at = np.arange(0, b.size, 1024) + rng.integers(0, 1024, (b.size + 1023) // 1024)
    at = at[at < b.size]
    b[at] = rng.integers(0x80, 0x100, at.size)
    return b.tobytes()


def lossy_routes(a, data):
    label = "text*" if args.damage else "text"
    ust = N.Utf8LossyStats()
    want = a.match_utf8(data, with_ids=True, stats=ust, errors="replace")
    cap = len(want) + 16
    ms_whole, _ = timed(lambda: a.match_utf8(data, with_ids=True, cap=cap, errors="replace"), args.reps)
    print("%s %d bytes, %d replaced, %d records" % (label, len(data), ust.n_replaced, len(want)))
    print("whole lossy    : %8.3f ms = %6.2f GB/s of bytes (acgpu_match_utf8_lossy, one call)" % (ms_whole, len(data) / ms_whole / 1e6), flush=True)
    for chunk in [int(c) for c in args.chunks.split(",")]:
        feeds = -(-len(data) // chunk)
        ms_lossy, got = timed(lambda: stream_bytes(a, data, chunk, cap, "replace"), args.reps)
        assert got.shape == want.shape and (got == want).all(), "the lossy feeds and the lossy call differ"
        line = "chunk %8d : lossy stream %8.3f ms = %6.2f GB/s (%d feeds, %.3f ms a feed), stream / whole = %.2f" % (
            chunk, ms_lossy, len(data) / ms_lossy / 1e6, feeds, ms_lossy / feeds, ms_lossy / ms_whole)
        if not ust.n_replaced:
            ms_strict, strict = timed(lambda: stream_bytes(a, data, chunk, cap), args.reps)
            assert (strict == want).all(), "lossy and strict differ on well-formed bytes"
            line += " | strict stream %8.3f ms, lossy / strict = %.3f" % (ms_strict, ms_lossy / ms_strict)
        print(line, flush=True)


words, data = mixed_text(1 << args.log2)
a = Automaton(N.MODE_WHOLEWORD, words + EXTRA[:7], True, word_chars=default_word_chars())
if args.errors == "replace":
    lossy_routes(a, damage(data) if args.damage else data)
    sys.exit(0)
n = len(data)
want = a.match_utf8(data, with_ids=True)
cap = len(want) + 16
ms_whole, got = timed(lambda: a.match_utf8(data, with_ids=True, cap=cap), args.reps)
assert (got == want).all()
print("text  %d bytes, %d records" % (n, len(want)))
print("whole          : %8.3f ms = %6.2f GB/s of bytes (acgpu_match_utf8, one call)" % (ms_whole, n / ms_whole / 1e6), flush=True)
result = {"bytes": n, "records": int(len(want)), "whole_ms": round(ms_whole, 3), "chunks": []}
for chunk in [int(c) for c in args.chunks.split(",")]:
    feeds = -(-n // chunk)
    ms_stream, got = timed(lambda: stream_bytes(a, data, chunk, cap), args.reps)
    assert got.shape == want.shape and (got == want).all(), "feed_utf8 and match_utf8 differ"
    ms_calls, total = timed(lambda: stream_calls(a, data, chunk, cap), args.reps)
    assert total == len(want)
    split = {}
    ms_host, got = timed(lambda: stream_host(a, data, chunk, cap, split), args.reps)
    assert got.shape == want.shape and (got == want).all(), "the host route and match_utf8 differ"
    print("chunk %8d : stream %8.3f ms = %6.2f GB/s (%d feeds, %.3f ms a feed; calls alone %.3f ms) | host %8.3f ms = %6.2f GB/s (decode %.1f + utf-16 %.1f "
          "+ remap %.1f ms around %.1f ms of Stream.feed) | host / stream = %.1f, stream / whole = %.2f" % (
              chunk, ms_stream, n / ms_stream / 1e6, feeds, ms_stream / feeds, ms_calls, ms_host, n / ms_host / 1e6, split["decode"] * 1e3,
              split["utf16"] * 1e3, split["remap"] * 1e3, split["feed"] * 1e3, ms_host / ms_stream, ms_stream / ms_whole), flush=True)
    result["chunks"].append({"chunk_bytes": chunk, "feeds": feeds, "stream_ms": round(ms_stream, 3), "calls_ms": round(ms_calls, 3), "host_ms": round(ms_host, 3),
                             "host_split_ms": {k: round(v * 1e3, 3) for k, v in split.items()}})
print(json.dumps(result))
