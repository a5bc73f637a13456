"""Development tool: what masking, redacting and highlighting MANY SHORT texts costs, one box, one process --
  batch   : ahocorasick_amd.mask_batch / redact_batch / highlight_batch on a list of host texts: ONE device call;
  calls   : the same bodies through one cover call per text, what a caller does without the batch entry on the same build;
  replace : on LongestMatch, redact_batch against replace_batch with one replacement (the results differ only where two matches
            touch; the tool says how many texts do).
Workload: --texts README paragraphs or lines (the paragraph of tools/cover_rate.py cut at its sentence ends and repeated), matched
against the README word list -- AhoCorasickSet, and LongestMatchSet for the comparison with replace.
usage: cover_batch_rate.py [--texts 20000] [--lines]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ahocorasick_amd import _native as N, synth
from ahocorasick_amd.cover import cover, cover_batch, cover_batch_units
from ahocorasick_amd.strings import AhoCorasickSet, LongestMatchSet

ap = argparse.ArgumentParser()
ap.add_argument("--texts", type=int, default=20_000)
ap.add_argument("--lines", action="store_true", help="the paragraph's sentences, one text each, instead of whole paragraphs")
args = ap.parse_args()

USES = [("mask", dict(body="fill", fill="*")), ("redact", dict(open="***", body="drop")), ("highlight", dict(open="<b>", close="</b>", body="keep"))]


def timed(fn, reps=3):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, out


def texts_of(n, lines):
    para = synth.README_PARAGRAPH
    parts = [s.strip() + "." for s in para.split(".") if s.strip()] if lines else [para]
    return [parts[i % len(parts)] for i in range(n)]


def run(label, s, texts, replace_too=False):
    units, out_off, st = cover_batch_units(s, texts)  # (warm: the pool's buffers)
    n_units = sum(len(t) for t in texts)
    print("%-9s texts=%d units=%d  R=%d  S=%d  pieces=%d rescans=%d" % (label, len(texts), n_units, st["n_records"], st["n_spans"], st["pieces"], st["rescans"]))
    for use, kw in USES:
        ms_batch, got = timed(lambda: cover_batch(s, texts, **kw))
        ms_calls, want = timed(lambda: [cover(s, t, **kw) for t in texts], reps=1)
        assert got == want, "the batch and the calls per text differ: " + use
        line = "%-9s %-9s batch %.1f ms (%.2f us/text) | one call per text %.1f ms (%.1f us/text, x%.1f)" % (
            label, use, ms_batch, 1e3 * ms_batch / len(texts), ms_calls, 1e3 * ms_calls / len(texts), ms_calls / max(ms_batch, 1e-9))
        if replace_too and use == "redact":
            ms_repl, rep = timed(lambda: s.replace_batch(texts, kw["open"]))
            line += " | replace_batch %.1f ms, %d texts differ (touching matches)" % (ms_repl, sum(1 for x, y in zip(got, rep) if x != y))
        print(line, flush=True)


texts = texts_of(args.texts, args.lines)
words = synth.readme_dictionary()
run("README", AhoCorasickSet(words, True), texts)
run("README-L", LongestMatchSet(words, True), texts, replace_too=True)
