"""Development tool: what masking, highlighting and redacting the covered runs of a text cost, one box, one process --
  cover   : ahocorasick_amd.mask / highlight / redact on a host text (scan, merge, plan and emit on the device; the text comes back);
  today   : what a caller does without it on the same build -- spans() and a splice of the text on the host in numpy (a coverage
            mask from the spans; for highlight and redact a cumulative sum of the added and dropped units places every unit);
  replace : for a non-overlapping family on a text without touching matches, the replace entry with one replacement, which redact
            then equals.
Workloads: the two texts of tools/spans_rate.py -- the README word list on its paragraph repeated to about --units units (dense,
overlapping records; AhoCorasickSet, and LongestMatchSet for the comparison with replace), config 2's dictionary on its synthetic
text (sparse).
usage: cover_rate.py [--units 20000000] [--only readme|c2]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ahocorasick_amd import _native as N, synth
from ahocorasick_amd.cover import cover
from ahocorasick_amd.spans import spans
from ahocorasick_amd.strings import Automaton, utf16

ap = argparse.ArgumentParser()
ap.add_argument("--units", type=int, default=20_000_000)
ap.add_argument("--only", default=None)
args = ap.parse_args()

USES = [("mask", dict(body="fill", fill="*")), ("highlight", dict(open="<b>", close="</b>", body="keep")), ("redact", dict(open="***", body="drop"))]


def splice_on_host(hay, sp, open="", close="", body="keep", fill="*"):
    """the covered text from the spans in numpy: every output unit is placed by a cumulative sum, no Python loop over the spans"""
    o, c = utf16(open), utf16(close)
    covered = np.zeros(hay.size + 1, np.int32)
    np.add.at(covered, sp[:, 0], 1)
    np.add.at(covered, sp[:, 1], -1)
    covered = np.cumsum(covered[:-1]) > 0
    if body == "fill" and not o.size and not c.size:
        return np.where(covered, utf16(fill)[0], hay).astype(np.uint16)
    keep = np.ones(hay.size, bool) if body != "drop" else ~covered
    src = np.where(covered, utf16(fill)[0], hay).astype(np.uint16) if body == "fill" else hay
    # units added in front of text position p: an open per span that starts at or before p, a close per span that ends at or before p
    add = np.zeros(hay.size + 1, np.int64)
    np.add.at(add, sp[:, 0], o.size)
    np.add.at(add, sp[:, 1], c.size)
    shift = np.cumsum(add)
    dst = np.cumsum(keep) - keep + shift[:-1]
    total = int(keep.sum() + shift[-1])
    out = np.empty(total, np.uint16)
    out[dst[keep]] = src[keep]
    at_open = (np.cumsum(keep) - keep)[sp[:, 0]] + shift[sp[:, 0]] - o.size  # in front of the span's first unit
    for j in range(o.size):
        out[at_open + j] = o[j]
    if c.size:
        ends = sp[:, 1]
        at_close = np.cumsum(keep)[ends - 1] + shift[ends] - c.size  # behind the span's last kept unit
        for j in range(c.size):
            out[at_close + j] = c[j]
    return out


def timed(fn, reps=3):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, out


def run(label, a, hay, replace_too=False):
    st = N.CoverStats()
    cover(a, hay, stats=st)  # (warm: the pool's buffers)
    print("%-9s N=%d  R=%d  S=%d  pieces=%d rescans=%d max_carry=%d" % (label, hay.size, st.n_records, st.n_spans, st.pieces, st.rescans, st.max_carry))
    for use, kw in USES:
        ms_cover, got = timed(lambda: utf16(cover(a, hay, **kw)))
        ms_today, want = timed(lambda: splice_on_host(hay, spans(a, hay), **kw))
        assert got.shape == want.shape and (got == want).all(), "cover and the host splice differ: " + use
        line = "%-9s %-9s cover %.1f ms | spans + numpy splice %.1f ms (x%.1f)" % (label, use, ms_cover, ms_today, ms_today / max(ms_cover, 1e-9))
        if replace_too and use == "redact":
            ms_repl, rep = timed(lambda: a.replace_host(hay, kw["open"])[0])
            assert (np.asarray(rep, np.uint16) == got).all(), "redact and replace differ on a text without touching matches"
            line += " | replace %.1f ms" % ms_repl
        print(line, flush=True)


if args.only in (None, "readme"):
    para = utf16(synth.README_PARAGRAPH + " ")
    hay = np.tile(para, max(1, args.units // para.size))
    run("README", Automaton(N.MODE_ALL, synth.readme_dictionary(), True), hay)
    longest = Automaton(N.MODE_LONGEST, synth.readme_dictionary(), True)
    recs = longest.match_host(para, False)
    run("README-L", longest, hay, replace_too=bool((recs[1:, 0] > recs[:-1, 1]).all()))
if args.only in (None, "c2"):
    hay = synth.haystack(synth.CONFIGS["C2"]["hay_seed"], args.units)
    run("C2", Automaton(N.MODE_ALL, synth.config_keywords("C2"), True), hay)
