"""Development tool: what masking, redacting and highlighting MANY SHORT texts costs, one box, one process --
  batch   : ahocorasick_amd.mask_batch / redact_batch / highlight_batch on a list of host texts: ONE device call;
  calls   : the same bodies through one cover call per text, what a caller does without the batch entry on the same build;
  replace : on LongestMatch, redact_batch against replace_batch with one replacement (the results differ only where two matches
            touch; the tool says how many texts do).
Workload: --texts README paragraphs or lines (the paragraph of tools/cover_rate.py cut at its sentence ends and repeated), matched
against the README word list -- AhoCorasickSet, and LongestMatchSet for the comparison with replace.
--utf8: the same batch as UTF-8 bytes -- mask_batch_utf8 and redact_batch_utf8 against
  calls   : one cover_utf8 call per text;
  decode  : what a caller does with the UTF-16 batch entry: decode every text, mask_batch / redact_batch, encode every result
            (the byte offsets are lost on the way);
  replace : on LongestMatch, replace_batch_utf8 with one replacement.
  --non-ascii appends " \u2713 \u00e9" to every text, so that the batch takes the branch with checkpoints.
usage: cover_batch_rate.py [--texts 20000] [--lines] [--utf8 [--non-ascii]]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ahocorasick_amd import _native as N, synth
from ahocorasick_amd.cover import (cover, cover_batch, cover_batch_bytes, cover_batch_units, cover_batch_utf8, cover_utf8, mask_batch, redact_batch)
from ahocorasick_amd.strings import AhoCorasickSet, LongestMatchSet

ap = argparse.ArgumentParser()
ap.add_argument("--texts", type=int, default=20_000)
ap.add_argument("--lines", action="store_true", help="the paragraph's sentences, one text each, instead of whole paragraphs")
ap.add_argument("--utf8", action="store_true", help="the batch as UTF-8 bytes: mask_batch_utf8, redact_batch_utf8")
ap.add_argument("--non-ascii", action="store_true", help="with --utf8: a check mark and an e acute behind every text")
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


def run_utf8(label, s, texts, replace_too=False):
    datas = [t.encode() for t in texts]
    out, out_off, st = cover_batch_bytes(s, datas)  # (warm: the pool's buffers)
    print("%-9s texts=%d bytes=%d ascii=%d  R=%d  S=%d  pieces=%d rescans=%d" % (label, len(datas), sum(len(d) for d in datas), all(d.isascii() for d in datas),
                                                                                 st["n_records"], st["n_spans"], st["pieces"], st["rescans"]))
    decoded = {"mask": lambda: [t.encode() for t in mask_batch(s, [d.decode() for d in datas])],
               "redact": lambda: [t.encode() for t in redact_batch(s, [d.decode() for d in datas], "***")]}
    for use, kw in USES[:2]:
        kw8 = {k: v.encode() if isinstance(v, str) and k != "body" else v for k, v in kw.items()}
        ms_batch, got = timed(lambda: cover_batch_utf8(s, datas, **kw8))
        ms_calls, want = timed(lambda: [cover_utf8(s, d, **kw8) for d in datas], reps=1)
        assert got == want, "the batch and the calls per text differ: " + use
        ms_dec, dec = timed(decoded[use])
        assert dec == got, "the batch and decode + batch + encode differ: " + use
        line = "%-9s %-9s batch %.1f ms (%.2f us/text) | one call per text %.1f ms (%.1f us/text, x%.1f) | decode + batch + encode %.1f ms (x%.2f)" % (
            label, use, ms_batch, 1e3 * ms_batch / len(datas), ms_calls, 1e3 * ms_calls / len(datas), ms_calls / max(ms_batch, 1e-9), ms_dec,
            ms_dec / max(ms_batch, 1e-9))
        if replace_too and use == "redact":
            ms_repl, rep = timed(lambda: s.replace_batch_utf8(datas, kw["open"]))
            line += " | replace_batch_utf8 %.1f ms, %d texts differ (touching matches)" % (ms_repl, sum(1 for x, y in zip(got, rep) if x != y))
        print(line, flush=True)


texts = texts_of(args.texts, args.lines)
words = synth.readme_dictionary()
if args.utf8:
    if args.non_ascii:
        texts = [t + " \u2713 \u00e9" for t in texts]
    run_utf8("README", AhoCorasickSet(words, True), texts)
    run_utf8("README-L", LongestMatchSet(words, True), texts, replace_too=True)
else:
    run("README", AhoCorasickSet(words, True), texts)
    run("README-L", LongestMatchSet(words, True), texts, replace_too=True)
