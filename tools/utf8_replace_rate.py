"""Development tool: what a caller who rewrites a UTF-8 buffer pays, one box, one process --
  replace_utf8 : acgpu_replace_utf8 on the buffer (copy, validate + transcode, scan piece by piece, records and boundaries to bytes,
                 plan, byte emit, the result copied out through the slabs);
  match_utf8   : acgpu_match_utf8 on the same input -- the call that replace_utf8 contains, so the difference is what plan, emit and
                 the result's way out cost;
  today        : what the same caller does without it: data.decode() -> utf16() -> Automaton.replace_host -> str -> encode().
All on the mixed text of tools/utf8_rate.py (restated here) and its automaton (WholeWordMatch over the README word list), one
replacement for every keyword, capacity known (no overflow retry timed), the results compared.
--batch N: N lines of that text, about 12 words a line, rewritten line by line through three routes instead --
  batch    : acgpu_replace_batch_utf8 on the one buffer and its line offsets (offsets=): one device call;
  per line : one acgpu_replace_utf8 call per line (on the first --per-line lines; the figure is scaled to N);
  decode   : every line decoded on the host, Automaton.replace_batch on the str lines, every result encoded again.
--errors replace: acgpu_replace_utf8_lossy on the same buffer (with --batch: acgpu_replace_batch_utf8_lossy) --
beside the strict call where the buffer is well-formed (the results compared), and with --damage on a copy in which about one byte
per KB is overwritten with a random byte from 0x80..0xFF (the strict call refuses that one).
usage: utf8_replace_rate.py [--log2 24] [--repl "[redacted]"] [--batch 20000 [--per-line 2000]] [--errors strict|replace] [--damage]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ahocorasick_amd import _native as N, synth
from ahocorasick_amd.strings import Automaton, _split_batch, _to_str, utf8_line_offsets, utf16
from ahocorasick_amd.unicode_tables import default_word_chars

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=24, help="bytes of the text, about")
ap.add_argument("--repl", default="[redacted]")
ap.add_argument("--batch", type=int, default=0, help="lines of a batch; 0: the one-text measurement")
ap.add_argument("--per-line", type=int, default=2000)
ap.add_argument("--errors", default="strict", choices=["strict", "replace"])
ap.add_argument("--damage", action="store_true", help="with --errors replace: overwrite about one byte per KB")
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


WORDS_PER_LINE = 12
def damage(data, seed=7):
    """a copy with about one byte per KB overwritten by a byte from 0x80..0xFF (tools/utf8_rate.py)"""
    rng = np.random.default_rng(seed)
    b = np.frombuffer(data, np.uint8).copy()
    at = np.arange(0, b.size, 1024) + rng.integers(0, 1024, (b.size + 1023) // 1024)
    at = at[at < b.size]
    b[at] = rng.integers(0x80, 0x100, at.size)
    return b.tobytes()


def lossy_routes(a, data, batch_off=None):
    """the lossy entry on `data` (a batch: with its line offsets) beside the strict one where that takes the buffer"""
    label = "mix*" if args.damage else "mix"
    ust = N.Utf8LossyStats()
    call = (lambda e, **kw: a.replace_batch_utf8(data, args.repl, offsets=batch_off, errors=e, **kw)) if batch_off is not None else (
        lambda e, **kw: a.replace_utf8(data, args.repl, errors=e, **kw))
    first = call("replace", stats=ust)
    cap_out = first[0].size + 64
    ms_lossy, got = timed(lambda: call("replace", cap=cap_out))
    print("%-4s %d bytes -> %d units, %d replaced (first at %d), %d records replaced by %r, %d bytes out, %d pieces" % (
        label, len(data), ust.n_units, ust.n_replaced, ust.first_replaced, got[-1]["n_records"], args.repl, got[0].size, got[-1]["pieces"]))
    print("%-4s lossy  : %8.3f ms = %6.2f GB/s of input bytes" % (label, ms_lossy, len(data) / ms_lossy / 1e6))
    if not ust.n_replaced:
        ms_strict, want = timed(lambda: call("strict", cap=cap_out))
        assert got[0].tobytes() == want[0].tobytes() and got[-1] == want[-1], "lossy and strict differ on well-formed bytes"
        print("%-4s strict : %8.3f ms = %6.2f GB/s | ratio lossy / strict = %.3f" % (label, ms_strict, len(data) / ms_strict / 1e6, ms_lossy / ms_strict), flush=True)



def make_lines(n_lines):
    words = synth.readme_dictionary()
    toks = _to_str(synth.readme_text(2006, n_lines * WORDS_PER_LINE * 8, words)).split(" ")
    toks = [t if i % 6 else t + " " + EXTRA[(i // 6) % len(EXTRA)] for i, t in enumerate(toks)]
    lines = [" ".join(toks[i * WORDS_PER_LINE:(i + 1) * WORDS_PER_LINE]) for i in range(n_lines)]
    return words, ("\n".join(lines) + "\n").encode("utf-8")


def batch_routes():
    words, buf = make_lines(args.batch)
    a = Automaton(N.MODE_WHOLEWORD, words + EXTRA[:7], True, word_chars=default_word_chars())
    off = utf8_line_offsets(buf)
    n = len(off) - 1
    ust = N.Utf8BatchStats()
    out, out_off, st = a.replace_batch_utf8(buf, args.repl, offsets=off, stats=ust)
    cap_out = out.size + 64
    print("%d lines, %d bytes -> %d units, ascii=%d, %d records replaced by %r, %d bytes out, %d pieces" % (
        n, len(buf), ust.n_units, ust.ascii, st["n_records"], args.repl, out.size, st["pieces"]))
    ms_batch, (got, got_off, _) = timed(lambda: a.replace_batch_utf8(buf, args.repl, cap=cap_out, offsets=off))
    o = off.tolist()
    ms_split, raw_lines = timed(lambda: [buf[o[i]:o[i + 1]] for i in range(n)])
    ms_dec, lines = timed(lambda: [ln.decode("utf-8") for ln in raw_lines])
    ms_u16, (units, u_off, _) = timed(lambda: a.replace_batch(lines, args.repl, cap=cap_out))
    ms_enc, want = timed(lambda: [s.encode("utf-8") for s in _split_batch(units, u_off)])
    go = got_off.tolist()
    assert [got[go[i]:go[i + 1]].tobytes() for i in range(n)] == want, "the routes differ"
    decode = ms_split + ms_dec + ms_u16 + ms_enc
    k = min(n, args.per_line)
    t0 = time.perf_counter()
    per = [a.replace_utf8(ln, args.repl)[0].tobytes() for ln in raw_lines[:k]]
    ms_line = (time.perf_counter() - t0) * 1e3
    assert per == want[:k], "the per-line route differs"
    print("batch    : %8.3f ms = %6.3f us a line = %6.2f GB/s of input bytes (one call, no host step)" % (ms_batch, ms_batch * 1e3 / n, len(buf) / ms_batch / 1e6))
    print("per line : %8.3f ms for %d lines = %6.3f us a line, %8.3f ms scaled to %d lines" % (ms_line, k, ms_line * 1e3 / k, ms_line * n / k, n))
    print("decode   : %8.3f ms (host: slice %.3f + decode %.3f + str, encode %.3f; replace_batch, its UTF-16 packing included, %.3f)" % (
        decode, ms_split, ms_dec, ms_enc, ms_u16))
    print("ratios   : per line / batch = %.2f, decode / batch = %.2f" % (ms_line * n / k / ms_batch, decode / ms_batch), flush=True)


if args.errors == "replace":
    words, data = make_lines(args.batch) if args.batch else mixed_text(1 << args.log2)
    data = damage(data) if args.damage else data
    lossy_routes(Automaton(N.MODE_WHOLEWORD, words + EXTRA[:7], True, word_chars=default_word_chars()), data,
                 utf8_line_offsets(data) if args.batch else None)
    sys.exit(0)
if args.batch:
    batch_routes()
    sys.exit(0)

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
