"""Development tool: what deciding about many short texts costs, one box, one process --
  summary : ONE acgpu_summary_batch_u16 call (24 bytes per haystack leave the device);
  records : ONE acgpu_match_batch_u16 call with Map records, its capacity known from a warm call (no overflow retry is timed),
            followed by the numpy reduction of its records to {count, first record} per haystack -- the only way to the same
            answer without the summary call.
Both per haystack and per GiB of haystack units, median of --reps calls.  Workloads: the README word list (AhoCorasick and
WholeWordMatch) over paragraphs of synth.readme_text (400-600 units each), and a sparse dictionary -- 1000 random keywords of 6-10
lower-case letters over random lower-case text, next to no match.
usage: summary_rate.py [--haystacks 20000] [--reps 5] [--only readme|sparse]"""
import argparse, ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ahocorasick_amd import _native as N, synth
from ahocorasick_amd.strings import Automaton, _pack
from ahocorasick_amd.unicode_tables import default_word_chars

ap = argparse.ArgumentParser()
ap.add_argument("--haystacks", type=int, default=20000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", default=None)
args = ap.parse_args()
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)


def reduce_records(recs, n_hay):
    """(n, 4) records {haystack, start, end, id}, haystacks ascending -> the summaries"""
    out = np.zeros(n_hay, dtype=N.SUMMARY_DTYPE)
    out["start"] = out["end"] = out["keyword_id"] = -1
    if len(recs):
        hs, first, counts = np.unique(recs[:, 0], return_index=True, return_counts=True)
        out["n_matches"][hs] = counts
        out["start"][hs], out["end"][hs], out["keyword_id"][hs] = recs[first, 1], recs[first, 2], recs[first, 3]
    return out


def run(label, a, hays):
    units, off = _pack(hays)
    n_hay, total = len(hays), int(off[-1])
    L = N.lib()
    out = np.zeros(n_hay, dtype=N.SUMMARY_DTYPE)
    st = N.SummaryStats()

    def summary():
        N.check(L.acgpu_summary_batch_u16(a.handle, vp(units), vp(off), n_hay, vp(out), ctypes.byref(st)), "acgpu_summary_batch_u16")
        return out
    cap = len(a.match_batch(hays, with_ids=True)) + 16  # (warm, and the capacity)
    recs = np.empty((cap, 4), dtype=np.int32)
    n_out = ctypes.c_uint64(0)

    def records():
        N.check(L.acgpu_match_batch_u16(a.handle, vp(units), vp(off), n_hay, N.REC_MAP, vp(recs), cap, ctypes.byref(n_out)), "acgpu_match_batch_u16")
        return reduce_records(recs[:n_out.value], n_hay)

    def timed(fn):
        fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), r.copy()
    t_sum, got = timed(summary)
    t_rec, want = timed(records)
    assert (got == want).all(), "summary and reduced records differ"
    gib = total * 2 / 2.0 ** 30
    print("%-16s H=%d units=%d records=%d (%.2f per unit) matched=%d pieces=%d rescans=%d" % (
        label, n_hay, total, st.n_records, st.n_records / max(total, 1), st.n_matched, st.pieces, st.rescans))
    for name, t, moved in (("summary", t_sum, 24 * n_hay), ("records+reduce", t_rec, 16 * int(n_out.value))):
        print("%-16s %-15s %8.3f ms per call = %7.3f us per haystack = %8.1f ms per GiB; %d bytes to the host" % (
            label, name, t * 1e3, t * 1e6 / n_hay, t * 1e3 / gib, moved), flush=True)


rng = np.random.default_rng(12)
n_hay = args.haystacks
if args.only in (None, "readme"):
    words = synth.readme_dictionary()
    text = synth.readme_text(2006, n_hay * 600, words)
    cuts = np.concatenate([[0], np.cumsum(rng.integers(400, 600, n_hay))])
    hays = [text[cuts[i]:cuts[i + 1]] for i in range(n_hay)]
    run("README/AC", Automaton(N.MODE_ALL, words, True), hays)
    run("README/WholeWord", Automaton(N.MODE_WHOLEWORD, words, True, word_chars=default_word_chars()), hays)
if args.only in (None, "sparse"):
    kws = synth.random_keywords(77, 1000, 6, 10)
    text = synth.haystack(78, n_hay * 600)
    cuts = np.concatenate([[0], np.cumsum(rng.integers(400, 600, n_hay))])
    hays = [text[cuts[i]:cuts[i + 1]] for i in range(n_hay)]
    run("sparse/AC", Automaton(N.MODE_ALL, kws, True), hays)
