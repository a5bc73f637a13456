"""Development tool: what the covered runs of a text cost, one box, one process --
  spans : ahocorasick_amd.spans.spans on a host text (scan + merge on the device, the spans alone come back);
  today : what a caller does without it on the same build -- find_all (every record over PCIe) and a merge of the intervals on
          the host in numpy (a running maximum of the ends; the records of every family can be sorted by start);
  match : acgpu_match_u16 alone with Set records (the scan and the records' way to the host inside `today`).
Workloads: the README word list (AhoCorasickSet) on its paragraph repeated to about --units units: dense, overlapping records;
config 2's dictionary on its synthetic text: sparse.
usage: spans_rate.py [--units 20000000] [--only readme|c2]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ahocorasick_amd import _native as N, synth
from ahocorasick_amd.spans import spans
from ahocorasick_amd.strings import Automaton, utf16

ap = argparse.ArgumentParser()
ap.add_argument("--units", type=int, default=20_000_000)
ap.add_argument("--only", default=None)
args = ap.parse_args()


def merge_on_host(recs):
    """the spans of (n, 2) records in numpy: sort by start, a span begins where a start exceeds every end before it"""
    if not len(recs):
        return np.zeros((0, 2), np.int32)
    r = recs[np.argsort(recs[:, 0], kind="stable")]
    reach = np.maximum.accumulate(r[:, 1])
    head = np.concatenate([[True], r[1:, 0] > reach[:-1]])
    first = np.flatnonzero(head)
    return np.stack([r[first, 0], reach[np.concatenate([first[1:] - 1, [len(r) - 1]])]], axis=1).astype(np.int32)


def timed(fn, reps=3):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, out


def run(label, a, hay):
    st = N.SpansStats()
    got = spans(a, hay, stats=st)  # (warm: the pool's buffers)
    ms_spans, got = timed(lambda: spans(a, hay, stats=st))
    cap = int(st.n_records) + 16
    ms_match, recs = timed(lambda: a.match_host(hay, False, cap=cap))
    ms_today, want = timed(lambda: merge_on_host(a.match_host(hay, False, cap=cap)))
    assert got.shape == want.shape and (got == want).all(), "spans and the host merge differ"
    print("%-7s N=%d  R=%d  S=%d  pieces=%d rescans=%d max_carry=%d" % (label, hay.size, len(recs), len(got), st.pieces, st.rescans, st.max_carry))
    print("%-7s spans %.1f ms | find_all + numpy merge %.1f ms (x%.1f) | acgpu_match_u16 alone %.1f ms" % (
        label, ms_spans, ms_today, ms_today / max(ms_spans, 1e-9), ms_match), flush=True)


if args.only in (None, "readme"):
    para = utf16(synth.README_PARAGRAPH + " ")
    hay = np.tile(para, max(1, args.units // para.size))
    run("README", Automaton(N.MODE_ALL, synth.readme_dictionary(), True), hay)
if args.only in (None, "c2"):
    hay = synth.haystack(synth.CONFIGS["C2"]["hay_seed"], args.units)
    run("C2", Automaton(N.MODE_ALL, synth.config_keywords("C2"), True), hay)
