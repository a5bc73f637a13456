"""Development tool: what a caller with a UTF-8 buffer pays, one box, one process --
  utf8  : acgpu_match_utf8 on the buffer (copy, validate + transcode, scan, remap on the device, records in byte offsets);
  today : what the same caller does without it: data.decode() -> utf16() -> Automaton.match_host -> the records' positions
          mapped back to bytes on the host through strings.utf8_unit_offsets.
Both on the same buffer and automaton (WholeWordMatch over the README word list), Map records, capacity known (no overflow retry
timed), the results compared.  The split host / device: `today` prints its three host steps (decode, UTF-16, remap) beside its
match_host call; `utf8` is one library call with no host step -- its kernels' share is what rocprofv3 --kernel-trace --stats shows
for k_utf8_* and the scan, in a run of its own.  Texts: a natural-language-like mix (synth.readme_text words, every sixth followed
by a non-ASCII token) and the same words as pure ASCII.
--errors replace: acgpu_match_utf8_lossy on the same buffer instead -- beside the strict call where the buffer is
well-formed (the records compared), and with --damage on a copy in which about one byte per KB is overwritten with a random byte
from 0x80..0xFF (the strict call refuses that one); beside both, the host's data.decode("utf-8", "replace") alone.
usage: utf8_rate.py [--log2 24] [--only mix|ascii] [--errors strict|replace] [--damage]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ahocorasick_amd import _native as N, synth
from ahocorasick_amd.strings import Automaton, _to_str, utf16, utf8_unit_offsets
from ahocorasick_amd.unicode_tables import default_word_chars

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=24, help="bytes of the text, about")
ap.add_argument("--only", default=None)
ap.add_argument("--errors", default="strict", choices=["strict", "replace"])
ap.add_argument("--damage", action="store_true", help="with --errors replace: overwrite about one byte per KB")
args = ap.parse_args()

EXTRA = ["Zürich", "naïve", "straße", "λόγος", "Москва", "東京", "데이터", "😀", "𝒜𝓃𝓈"]


def texts(n_bytes):
    words = synth.readme_dictionary()
    base = _to_str(synth.readme_text(2006, n_bytes, words))
    toks = base.split(" ")
    mixed = " ".join(t if i % 6 else t + " " + EXTRA[(i // 6) % len(EXTRA)] for i, t in enumerate(toks))
    return words, {"ascii": base.encode("utf-8")[:n_bytes], "mix": mixed.encode("utf-8")}


def timed(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, out


def run(label, a, data):
    n = len(data)
    st = N.Utf8Stats()
    cap = len(a.match_utf8(data, with_ids=True)) + 16
    ms_utf8, got = timed(lambda: a.match_utf8(data, with_ids=True, cap=cap, stats=st))
    ms_dec, text = timed(lambda: data.decode("utf-8"))
    ms_u16, units = timed(lambda: utf16(text))
    ms_match, recs = timed(lambda: a.match_host(units, with_ids=True, cap=cap))

    def remap():
        off = utf8_unit_offsets(data)
        b = np.frombuffer(data, np.uint8)
        last = off[recs[:, 1] - 1]
        lead = b[last]
        out = recs.copy()
        out[:, 0] = off[recs[:, 0]]
        out[:, 1] = last + 1 + (lead >= 0xC0) + (lead >= 0xE0) + (lead >= 0xF0)
        return out
    ms_remap, want = timed(remap)
    assert got.shape == want.shape and (got == want).all(), "the two routes differ"
    today = ms_dec + ms_u16 + ms_match + ms_remap
    print("%-5s %d bytes -> %d units, ascii=%d, %d records" % (label, n, st.n_units, st.ascii, len(got)))
    print("%-5s utf8  : %8.3f ms = %6.2f GB/s of bytes (one call: copy %d B, transcode, scan, remap, copy %d B back)" % (
        label, ms_utf8, n / ms_utf8 / 1e6, n, len(got) * 12))
    print("%-5s today : %8.3f ms = %6.2f GB/s of bytes | host: decode %.3f + utf-16 %.3f + remap %.3f = %.3f ms | match_host (copy %d B + scan) %.3f ms" % (
        label, today, n / today / 1e6, ms_dec, ms_u16, ms_remap, ms_dec + ms_u16 + ms_remap, 2 * units.size, ms_match))
    print("%-5s ratio today / utf8 = %.2f" % (label, today / ms_utf8), flush=True)


def damage(data, seed=7):
    """a copy with about one byte per KB overwritten by a byte from 0x80..0xFF"""
    rng = np.random.default_rng(seed)
    b = np.frombuffer(data, np.uint8).copy()
    at = np.arange(0, b.size, 1024) + rng.integers(0, 1024, (b.size + 1023) // 1024)
    at = at[at < b.size]
    b[at] = rng.integers(0x80, 0x100, at.size)
    return b.tobytes()


def run_lossy(label, a, data):
    n = len(data)
    st = N.Utf8LossyStats()
    cap = len(a.match_utf8(data, with_ids=True, errors="replace")) + 16
    ms_lossy, got = timed(lambda: a.match_utf8(data, with_ids=True, cap=cap, stats=st, errors="replace"))
    ms_dec, _ = timed(lambda: data.decode("utf-8", "replace"))
    print("%-5s %d bytes -> %d units, %d replaced (first at %d), ascii=%d, %d records" % (
        label, n, st.n_units, st.n_replaced, st.first_replaced, st.ascii, len(got)))
    print("%-5s lossy : %8.3f ms = %6.2f GB/s of bytes | host decode(errors='replace') alone: %.3f ms" % (label, ms_lossy, n / ms_lossy / 1e6, ms_dec))
    if not st.n_replaced:
        ms_strict, want = timed(lambda: a.match_utf8(data, with_ids=True, cap=cap))
        assert got.shape == want.shape and (got == want).all(), "lossy and strict differ on well-formed bytes"
        print("%-5s strict: %8.3f ms = %6.2f GB/s of bytes | ratio lossy / strict = %.3f" % (label, ms_strict, n / ms_strict / 1e6, ms_lossy / ms_strict), flush=True)


words, tx = texts(1 << args.log2)
a = Automaton(N.MODE_WHOLEWORD, words + EXTRA[:7], True, word_chars=default_word_chars())
for label in ("mix", "ascii"):
    if args.only in (None, label):
        if args.errors == "replace":
            run_lossy(label + ("*" if args.damage else ""), a, damage(tx[label]) if args.damage else tx[label])
        else:
            run(label, a, tx[label])
