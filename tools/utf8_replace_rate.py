"""Development tool: what a caller who rewrites a UTF-8 buffer pays, one box, one process --
  replace_utf8 : acgpu_replace_utf8 on the buffer (copy, validate + transcode, scan piece by piece, records and boundaries to bytes,
                 plan, byte emit, the result copied out through the slabs);
  match_utf8   : acgpu_match_utf8 on the same input -- the call that replace_utf8 contains, so the difference is what plan, emit and
                 the result's way out cost;
  today        : what the same caller does without it: data.decode() -> utf16() -> Automaton.replace_host -> str -> encode().
All on the mixed text of tools/utf8_rate.py (restated here) and its automaton (WholeWordMatch over the README word list), one
replacement for every keyword, capacity known (no overflow retry timed), the results compared.
usage: utf8_replace_rate.py [--log2 24] [--repl "[redacted]"]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ahocorasick_amd import _native as N, synth
from ahocorasick_amd.strings import Automaton, _to_str, utf16
from ahocorasick_amd.unicode_tables import default_word_chars

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=24, help="bytes of the text, about")
ap.add_argument("--repl", default="[redacted]")
args = ap.parse_args()

EXTRA = ["Zürich", "naïve", "straße", "λόγος", "Москва", "東京", "데이터", "😀", "𝒜𝓃𝓈"]


def mixed_text(n_bytes):
    words = synth.readme_dictionary()
    toks = _to_str(synth.readme_text(2006, n_bytes, words)).split(" ")
    mixed = " ".join(t if i % 6 else t + " " + EXTRA[(i // 6) % len(EXTRA)] for i, t in enumerate(toks))
    return words, mixed.encode("utf-8")


def timed(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, out


words, data = mixed_text(1 << args.log2)
a = Automaton(N.MODE_WHOLEWORD, words + EXTRA[:7], True, word_chars=default_word_chars())
n = len(data)
ust = N.Utf8Stats()
n_recs = len(a.match_utf8(data, with_ids=True))
cap_out = len(a.replace_utf8(data, args.repl)[0]) + 64
ms_repl, (got, st) = timed(lambda: a.replace_utf8(data, args.repl, cap=cap_out, stats=ust))
ms_match, _ = timed(lambda: a.match_utf8(data, with_ids=True, cap=n_recs + 16))
ms_dec, text = timed(lambda: data.decode("utf-8"))
ms_u16, units = timed(lambda: utf16(text))
ms_host, (out_units, _) = timed(lambda: a.replace_host(units, args.repl, cap=cap_out))
ms_enc, want = timed(lambda: _to_str(out_units).encode("utf-8"))
assert got.tobytes() == want and st["n_records"] == n_recs, "the two routes differ"
today = ms_dec + ms_u16 + ms_host + ms_enc
print("mix   %d bytes -> %d units, %d records replaced by %r, %d bytes out, %d pieces" % (n, ust.n_units, n_recs, args.repl, got.size, st["pieces"]))
print("mix   replace_utf8 : %8.3f ms = %6.2f GB/s of input bytes (one call, no host step)" % (ms_repl, n / ms_repl / 1e6))
print("mix   match_utf8   : %8.3f ms = %6.2f GB/s (the call replace_utf8 contains; %d B of records back instead of the text)" % (
    ms_match, n / ms_match / 1e6, n_recs * 12))
print("mix   today        : %8.3f ms = %6.2f GB/s | host: decode %.3f + utf-16 %.3f + str, encode %.3f = %.3f ms | replace_host %.3f ms" % (
    today, n / today / 1e6, ms_dec, ms_u16, ms_enc, ms_dec + ms_u16 + ms_enc, ms_host))
print("mix   ratio today / replace_utf8 = %.2f, replace_utf8 / match_utf8 = %.2f" % (today / ms_repl, ms_repl / ms_match), flush=True)
