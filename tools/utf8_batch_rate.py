"""Development tool: what a caller with many short UTF-8 texts pays, one box, one process -- N lines of mixed text
(synth.readme_text words, every sixth followed by a non-ASCII token, about 12 words a line) through three routes:
  batch    : Automaton.summary_batch_utf8 / match_batch_utf8 on the one buffer and its line offsets (offsets=): one device call each;
  decode   : what the same caller does without them: every line decoded on the host, Automaton.summary_batch / match_batch on the
             str lines, the records' positions mapped back to bytes line by line (the mapping rule over each line's lead bytes);
  per line : one Automaton.match_utf8 call per line (on the first --per-line lines; the figure is scaled to N).
The same automaton (WholeWordMatch over the README word list), Map records, capacity known (no overflow retry timed), the routes'
results compared.  A host clock around each step; the kernels' own share is what rocprofv3 --kernel-trace --stats shows, in a run
of its own.
--errors replace: the lossy entries (acgpu_summary_batch_utf8_lossy / acgpu_match_batch_utf8_lossy) on the same buffer
and offsets, beside the strict ones where the buffer is well-formed (results compared); --damage overwrites about one byte per KB
with a random byte from 0x80..0xFF (never a line feed: the lines stay the lines), which the strict entries refuse.
usage: utf8_batch_rate.py [--lines 20000] [--per-line 2000] [--errors strict|replace] [--damage]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ahocorasick_amd import _native as N, synth
from ahocorasick_amd.strings import Automaton, _to_str, utf8_line_offsets
from ahocorasick_amd.unicode_tables import default_word_chars

ap = argparse.ArgumentParser()
ap.add_argument("--lines", type=int, default=20000)
ap.add_argument("--per-line", type=int, default=2000)
ap.add_argument("--errors", default="strict", choices=["strict", "replace"])
ap.add_argument("--damage", action="store_true", help="with --errors replace: overwrite about one byte per KB")
args = ap.parse_args()

EXTRA = ["Zürich", "naïve", "straße", "λόγος", "Москва", "東京", "데이터", "😀", "𝒜𝓃𝓈"]
WORDS_PER_LINE = 12


def make_lines(n_lines):
    words = synth.readme_dictionary()
    toks = _to_str(synth.readme_text(2006, n_lines * WORDS_PER_LINE * 8, words)).split(" ")
    toks = [t if i % 6 else t + " " + EXTRA[(i // 6) % len(EXTRA)] for i, t in enumerate(toks)]
    lines = [" ".join(toks[i * WORDS_PER_LINE:(i + 1) * WORDS_PER_LINE]) for i in range(n_lines)]
    return words, ("\n".join(lines) + "\n").encode("utf-8")


def timed(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, out


def remap(recs, raw_lines):
    """(haystack, start, end, id) in units of the decoded lines -> in bytes of the lines, line by line"""
    out = recs.copy()
    tables = {}
    for r, (h, s, e, _) in enumerate(recs.tolist()):
        t = tables.get(h)
        if t is None:
            b = np.frombuffer(raw_lines[h], np.uint8)
            leads = np.flatnonzero((b & 0xC0) != 0x80)
            t = tables[h] = (np.repeat(leads, 1 + (b[leads] >= 0xF0)), b)
        off, b = t
        last = int(off[e - 1])
        out[r, 1] = off[s]
        out[r, 2] = last + 1 + (b[last] >= 0xC0) + (b[last] >= 0xE0) + (b[last] >= 0xF0)
    return out


words, buf = make_lines(args.lines)
a = Automaton(N.MODE_WHOLEWORD, words + EXTRA[:7], True, word_chars=default_word_chars())
off = utf8_line_offsets(buf)
n = len(off) - 1
if args.errors == "replace":
    if args.damage:
        rng = np.random.default_rng(7)
        b = np.frombuffer(buf, np.uint8).copy()
        at = np.arange(0, b.size, 1024) + rng.integers(0, 1024, (b.size + 1023) // 1024)
        at = at[at < b.size]
        at = at[b[at] != 0x0A]
        b[at] = rng.integers(0x80, 0x100, at.size)
        buf = b.tobytes()
    st = N.Utf8LossyStats()
    cap = len(a.match_batch_utf8(buf, with_ids=True, offsets=off, stats=st, errors="replace")) + 16
    print("%d lines, %d bytes -> %d units, %d replaced (first in line %d at %d), ascii=%d, %d records" % (
        n, len(buf), st.n_units, st.n_replaced, st.first_haystack, st.first_replaced, st.ascii, cap - 16))
    ms_sum, (sum_l, _) = timed(lambda: a.summary_batch_utf8(buf, offsets=off, errors="replace"))
    ms_rec, rec_l = timed(lambda: a.match_batch_utf8(buf, with_ids=True, cap=cap, offsets=off, errors="replace"))
    print("lossy    : summary %8.3f ms = %6.3f us a line | match %8.3f ms = %6.3f us a line" % (ms_sum, ms_sum * 1e3 / n, ms_rec, ms_rec * 1e3 / n))
    if not st.n_replaced:
        ms_sum8, (sum8, _) = timed(lambda: a.summary_batch_utf8(buf, offsets=off))
        ms_rec8, rec8 = timed(lambda: a.match_batch_utf8(buf, with_ids=True, cap=cap, offsets=off))
        assert (sum8 == sum_l).all() and rec8.shape == rec_l.shape and (rec8 == rec_l).all(), "lossy and strict differ on well-formed bytes"
        print("strict   : summary %8.3f ms | match %8.3f ms | ratios lossy / strict = %.3f, %.3f" % (ms_sum8, ms_rec8, ms_sum / ms_sum8, ms_rec / ms_rec8), flush=True)
    sys.exit(0)
st = N.Utf8BatchStats()
cap = len(a.match_batch_utf8(buf, with_ids=True, offsets=off, stats=st)) + 16
print("%d lines, %d bytes -> %d units, ascii=%d, %d records" % (n, len(buf), st.n_units, st.ascii, cap - 16))

ms_sum8, (sum8, _) = timed(lambda: a.summary_batch_utf8(buf, offsets=off))
ms_rec8, rec8 = timed(lambda: a.match_batch_utf8(buf, with_ids=True, cap=cap, offsets=off))
print("batch    : summary %8.3f ms = %6.3f us a line | match %8.3f ms = %6.3f us a line" % (ms_sum8, ms_sum8 * 1e3 / n, ms_rec8, ms_rec8 * 1e3 / n))

o = off.tolist()
ms_split, raw_lines = timed(lambda: [buf[o[i]:o[i + 1]] for i in range(n)])
ms_dec, lines = timed(lambda: [ln.decode("utf-8") for ln in raw_lines])
ms_sum16, (sum16, _) = timed(lambda: a.summary_batch(lines))
ms_rec16, rec16 = timed(lambda: a.match_batch(lines, with_ids=True, cap=cap))
ms_remap, want = timed(lambda: remap(rec16, raw_lines), reps=2)
assert rec8.shape == want.shape and (rec8 == want).all(), "the routes' records differ"
assert (sum8["n_matches"] == sum16["n_matches"]).all(), "the routes' summaries differ"
host = ms_split + ms_dec
print("decode   : summary %8.3f ms (host: slice %.3f + decode %.3f; summary_batch, its UTF-16 packing included, %.3f)" % (host + ms_sum16, ms_split, ms_dec, ms_sum16))
print("decode   : match   %8.3f ms (host: slice + decode %.3f + remap %.3f; match_batch, its UTF-16 packing included, %.3f)" % (
    host + ms_rec16 + ms_remap, host, ms_remap, ms_rec16))

k = min(n, args.per_line)
t0 = time.perf_counter()
got = [a.match_utf8(ln, with_ids=True) for ln in raw_lines[:k]]
ms_line = (time.perf_counter() - t0) * 1e3
assert sum(len(g) for g in got) == int((rec8[:, 0] < k).sum()), "the per-line route differs"
print("per line : match   %8.3f ms for %d lines = %6.3f us a line, %8.3f ms scaled to %d lines" % (ms_line, k, ms_line * 1e3 / k, ms_line * n / k, n))
print("ratios   : decode / batch = %.2f (summary), %.2f (match); per line / batch = %.2f (match)" % (
    (host + ms_sum16) / ms_sum8, (host + ms_rec16 + ms_remap) / ms_rec8, ms_line * n / k / ms_rec8), flush=True)
