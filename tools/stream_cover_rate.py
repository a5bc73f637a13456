"""Development tool: what a caller pays who masks or redacts a UTF-8 text that is read in chunks, one box, one process (DESIGN.md
4.26) --
  stream : one CoverStream fed the chunks through CoverStream.feed_utf8 (acgpu_stream_cover_utf8: carry + chunk copied, validated +
           transcoded, the owned range scanned piece by piece, merge, plan, byte emit, the feed's part of the result copied out);
  whole  : acgpu_cover_utf8 on the whole text in one call, same build (what the chunked form is measured against; needs the text in
           one piece and below 2^31 bytes);
  host   : what the same caller does without the entry: codecs' incremental decoder per chunk -> utf16() -> Stream.feed (Set
           records) -> the records' unit positions mapped to bytes and a numpy splice of the whole text at the end (a coverage mask
           from a difference array; redact: the kept bytes placed by a cumulative sum) -- a caller that has to write as it goes pays
           more.
All three on the 19.4 MB mixed text of tools/stream_replace_rate.py with the README word list under AhoCorasick;
the three results are compared.  Chunks are cut at multiples of the chunk size, wherever that falls in a sequence.  Every route is
warmed once and timed --reps times; the median and the spread (min .. max) are printed, the host clock around calls that end in a
device synchronise.
usage: stream_cover_rate.py [--log2 24] [--chunks 4194304,1048576,65536] [--reps 5]"""
import argparse, codecs, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ahocorasick_amd import _native as N, synth
from ahocorasick_amd.cover import CoverStream, cover_utf8
from ahocorasick_amd.strings import Automaton, Stream, _to_str, utf16, utf8_unit_offsets

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=24, help="bytes of the text before the non-ASCII tokens go in, about")
ap.add_argument("--chunks", default="4194304,1048576,65536")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

EXTRA = ["Zürich", "naïve", "straße", "λόγος", "Москва", "東京", "데이터", "😀", "𝒜𝓃𝓈"]  # (tools/utf8_replace_rate.py)
USES = [("mask", dict(body="fill", fill=b"*")), ("redact", dict(open=b"***", body="drop"))]


def mixed_text(n_bytes):
    words = synth.readme_dictionary()
    toks = _to_str(synth.readme_text(2006, n_bytes, words)).split(" ")
    mixed = " ".join(t if i % 6 else t + " " + EXTRA[(i // 6) % len(EXTRA)] for i, t in enumerate(toks))
    return words, mixed.encode("utf-8")


def timed(fn, reps):
    """-> (median ms, min ms, max ms, the last result), after one warm-up call"""
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), min(ts), max(ts), out


def stream_bytes(a, data, chunk, kw):
    with CoverStream(a, **kw) as st:
        return b"".join(st.feed_utf8(data[i:i + chunk], final=i + chunk >= len(data)) for i in range(0, len(data), chunk))


def stream_host(a, data, chunk, cap, kw):
    dec = codecs.getincrementaldecoder("utf-8")()
    st = Stream(a, with_ids=False)
    pages, offs, pos = [], [], 0
    try:
        for i in range(0, len(data), chunk):
            piece, final = data[i:i + chunk], i + chunk >= len(data)
            pending = len(dec.getstate()[0])
            units = utf16(dec.decode(piece, final))
            pages.append(st.feed(units, final=final, cap=cap))
            consumed = pending + len(piece) - len(dec.getstate()[0])
            offs.append(utf8_unit_offsets(data[pos:pos + consumed]) + pos)
            pos += consumed
    finally:
        st.close()
    recs, off, b = np.concatenate(pages), np.concatenate(offs), np.frombuffer(data, np.uint8)
    last = off[recs[:, 1] - 1]
    lead = b[last]
    start, end = off[recs[:, 0]], last + 1 + (lead >= 0xC0) + (lead >= 0xE0) + (lead >= 0xF0)
    diff = np.zeros(b.size + 1, np.int32)
    np.add.at(diff, start, 1)
    np.add.at(diff, end, -1)
    covered = np.cumsum(diff[:-1]) > 0
    if kw["body"] == "fill":
        return np.where(covered, kw["fill"][0], b).astype(np.uint8).tobytes()
    # redact: every span's first byte becomes open, its other bytes go
    o = np.frombuffer(kw["open"], np.uint8)
    first = covered & ~np.concatenate([[False], covered[:-1]])
    length = np.where(first, o.size, np.where(covered, 0, 1))
    at = np.cumsum(length) - length
    out = np.empty(int(length.sum()), np.uint8)
    out[at[~covered]] = b[~covered]
    for j in range(o.size):
        out[at[first] + j] = o[j]
    return out.tobytes()


words, data = mixed_text(1 << args.log2)
a = Automaton(N.MODE_ALL, words + EXTRA[:7], True)
n = len(data)
n_recs = len(a.match_utf8(data, with_ids=False))
result = {"bytes": n, "records": n_recs, "uses": {}}
print("text  %d bytes, %d records (AhoCorasick over the README word list)" % (n, n_recs), flush=True)
for use, kw in USES:
    st = N.CoverStats()
    want = cover_utf8(a, data, stats=st, **kw)
    ms_whole, lo, hi, got = timed(lambda: cover_utf8(a, data, **kw), args.reps)
    assert got == want
    print("%-6s whole          : %8.3f ms (%.3f .. %.3f) = %6.2f GB/s of input bytes (acgpu_cover_utf8, one call; %d spans, %d bytes out)" % (
        use, ms_whole, lo, hi, n / ms_whole / 1e6, st.n_spans, len(want)), flush=True)
    rows = []
    for chunk in [int(c) for c in args.chunks.split(",")]:
        feeds = -(-n // chunk)
        ms_stream, s_lo, s_hi, got = timed(lambda: stream_bytes(a, data, chunk, kw), args.reps)
        assert got == want, "CoverStream.feed_utf8 and cover_utf8 differ"
        ms_host, h_lo, h_hi, got = timed(lambda: stream_host(a, data, chunk, n_recs + 16, kw), max(1, args.reps // 2))
        assert got == want, "the host route and cover_utf8 differ"
        print("%-6s chunk %8d : stream %8.3f ms (%.3f .. %.3f) = %6.2f GB/s (%d feeds, %.3f ms a feed) | host %8.3f ms (%.3f .. %.3f) | "
              "host / stream = %.1f, stream / whole = %.2f" % (use, chunk, ms_stream, s_lo, s_hi, n / ms_stream / 1e6, feeds, ms_stream / feeds,
                                                             ms_host, h_lo, h_hi, ms_host / ms_stream, ms_stream / ms_whole), flush=True)
        rows.append({"chunk_bytes": chunk, "feeds": feeds, "stream_ms": round(ms_stream, 3), "stream_min_max_ms": [round(s_lo, 3), round(s_hi, 3)],
                     "host_ms": round(ms_host, 3)})
    result["uses"][use] = {"whole_ms": round(ms_whole, 3), "whole_min_max_ms": [round(lo, 3), round(hi, 3)], "bytes_out": len(want), "chunks": rows}
print(json.dumps(result))
