"""Development tool: what the document-term matrix of many short texts costs, one box, one process --
  count_batch : ONE acgpu_count_batch_u16 (--utf8: acgpu_count_batch_utf8) call, its capacity known from a warm call (no overflow
                retry is timed): 12 bytes per entry leave the device, the host finishes them in one pass;
  records     : the route without it -- ONE acgpu_match_batch_u16 (acgpu_match_batch_utf8) call with Map records, capacity known
                likewise, then np.unique(ids, return_counts=True) haystack by haystack on the host: 16 bytes per record leave the
                device and Python loops over the haystacks.
Both per haystack and per GiB of haystack units, median of --reps calls; the two matrices are compared.  Workloads: those of
tools/summary_rate.py -- the README word list (AhoCorasick and WholeWordMatch) over paragraphs of synth.readme_text (400-600 units
each), and a sparse dictionary, 1000 random keywords of 6-10 lower-case letters over random lower-case text.
The per-kernel split (k_terms_block, k_terms_place, k_terms_gather against the scan) comes from a run of its own under the
profiler: tools/kstats.sh count_batch tools/count_batch_rate.py --reps 1 --only readme.
usage: count_batch_rate.py [--haystacks 20000] [--reps 5] [--only readme|sparse] [--utf8]"""
import argparse, ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ahocorasick_amd import _native as N, synth
from ahocorasick_amd.strings import Automaton, _pack, _pack_utf8, _to_str
from ahocorasick_amd.unicode_tables import default_word_chars

ap = argparse.ArgumentParser()
ap.add_argument("--haystacks", type=int, default=20000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", default=None)
ap.add_argument("--utf8", action="store_true")
args = ap.parse_args()
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)


def unique_per_haystack(recs, n_hay):
    """(n, 4) records {haystack, start, end, id}, haystacks ascending -> (indptr, indices, data), a np.unique per haystack"""
    bounds = np.searchsorted(recs[:, 0], np.arange(n_hay + 1))
    indptr, ids, counts = np.zeros(n_hay + 1, np.int64), [], []
    for i in range(n_hay):
        u, c = np.unique(recs[bounds[i]:bounds[i + 1], 3], return_counts=True)
        ids.append(u)
        counts.append(c)
        indptr[i + 1] = indptr[i] + len(u)
    return indptr, np.concatenate(ids).astype(np.int32), np.concatenate(counts).astype(np.uint32)


def run(label, a, hays):
    L = N.lib()
    if args.utf8:
        text, off = _pack_utf8([_to_str(h).encode("utf-8") for h in hays], None)
        count_entry, match_entry, tail = L.acgpu_count_batch_utf8, L.acgpu_match_batch_utf8, (None,)
        warm = a.match_batch_utf8(text, True, offsets=off)
    else:
        text, off = _pack(hays)
        count_entry, match_entry, tail = L.acgpu_count_batch_u16, L.acgpu_match_batch_u16, ()
        warm = a.match_batch(hays, with_ids=True)
    n_hay, total = len(hays), int(off[-1])
    cap = len(warm) + 16  # (the record count always suffices for the entries)
    row_ptr, ids, counts = np.zeros(n_hay + 1, np.uint64), np.empty(cap, np.uint32), np.empty(cap, np.uint32)
    recs = np.empty((cap, 4), dtype=np.int32)
    n_out, st = ctypes.c_uint64(0), N.CountBatchStats()

    def count_batch():
        N.check(count_entry(a.handle, vp(text), vp(off), n_hay, vp(row_ptr), vp(ids), vp(counts), cap, ctypes.byref(n_out), ctypes.byref(st), *tail),
                count_entry.__name__)
        return row_ptr.view(np.int64).copy(), ids[:n_out.value].view(np.int32).copy(), counts[:n_out.value].copy()

    def records():
        N.check(match_entry(a.handle, vp(text), vp(off), n_hay, N.REC_MAP, vp(recs), cap, ctypes.byref(n_out), *tail), match_entry.__name__)
        return unique_per_haystack(recs[:n_out.value], n_hay)

    def timed(fn):
        fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), r
    t_cnt, got = timed(count_batch)
    t_rec, want = timed(records)
    assert all((g == w).all() for g, w in zip(got, want)), "count_batch and the records' np.unique differ"
    gib = total * 2 / 2.0 ** 30
    print("%-16s H=%d units=%d n_records=%d (%.2f per unit) n_entries=%d n_terms=%d rows_cut=%d pieces=%d rescans=%d" % (
        label, n_hay, total, st.n_records, st.n_records / max(total, 1), st.n_entries, st.n_terms, st.rows_cut, st.pieces, st.rescans))
    for name, t, moved in (("count_batch", t_cnt, 12 * st.n_entries), ("records+unique", t_rec, 16 * st.n_records)):
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
