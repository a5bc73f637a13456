"""Development tool: three routes to the same per-keyword counts, one box, one process --
  count  : acgpu_count_device (no records), with the A/B switches of the tunable count_form;
  match  : acgpu_match_device with Map records, then torch.bincount of the keyword_id column on the device;
  cursor : the cursor's pages through host memory, np.bincount of every page (the README text only, and only with --cursor).
Workloads: the README dictionary in synth.readme_text (2^28 units: dense matches, the direct form); config 2's dictionary over
its random text (sparse matches, the records form); a one-letter text (one hot id, one hot state).
usage: count_rate.py [--log2 28] [--cursor] [--only readme|c2|hot]"""
import argparse, ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from ahocorasick_amd import _native as N, synth
from ahocorasick_amd.strings import Automaton

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=28)
ap.add_argument("--cursor", action="store_true")
ap.add_argument("--only", default=None)
args = ap.parse_args()
n = 1 << args.log2
stream = torch.cuda.current_stream().cuda_stream


def timed(fn, reps=3):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, out


def count_route(a, d_hay, d_counts):
    d_counts.zero_()
    rc, st, _ = a.count_device(d_hay.data_ptr(), n, d_counts.data_ptr(), stream=stream)
    assert rc == 0, rc
    return d_counts, st


def match_route(a, d_hay, n_kw, d_out, cap):
    nm, rc, prof, _ = a.match_device(d_hay.data_ptr(), n, True, d_out.data_ptr(), cap, stream=stream, profile=True)
    assert rc == 0, rc
    return torch.bincount(d_out[:nm, 2], minlength=n_kw), prof


def cursor_route(a, hay, n_kw):
    counts = np.zeros(n_kw, np.int64)
    for page in a.pages(hay, True, page_records=1 << 24):
        counts += np.bincount(page[:, 2], minlength=n_kw)
    return counts


def run(label, kws, d_hay, cap, all_forms, hay_host=None):
    n_kw = len(kws)
    a = Automaton(N.MODE_ALL, kws, True)
    d_out = torch.empty((cap, 3), dtype=torch.int32, device="cuda")
    d_counts = torch.zeros(n_kw, dtype=torch.int64, device="cuda")
    ref = None
    for all_form in all_forms:  # (0: what the pool's density decides; 1: never the states form; 2: always)
        N.set_tunable("all_form", all_form)
        ms, (m_counts, prof) = timed(lambda: match_route(a, d_hay, n_kw, d_out, cap))
        ref = m_counts if ref is None else ref
        assert bool((m_counts == ref).all())
        print("%-10s all_form=%d  match + bincount : %9.3f ms wall (scan %.3f + records %.3f ms, %s), %d records" % (
            label, all_form, ms, prof["scan_ms"], prof["finalize_ms"], prof["scan_kernel"][:24], int(ref.sum())), flush=True)
        for cform in (0, 1, 2, 4):
            N.set_tunable("count_form", cform)
            ms, (c_counts, st) = timed(lambda: count_route(a, d_hay, d_counts))
            assert bool((c_counts == ref).all()), (label, all_form, cform)
            print("%-10s all_form=%d  count_form=%d     : %9.3f ms wall, direct %d + records %d units, %d pieces, %d rescans" % (
                label, all_form, cform, ms, st["units_direct"], st["units_records"], st["pieces"], st["rescans"]), flush=True)
        N.set_tunable("count_form", 0)
    N.set_tunable("all_form", 0)
    if hay_host is not None:
        t0 = time.perf_counter()
        c = cursor_route(a, hay_host, n_kw)
        print("%-10s cursor pages + np.bincount : %9.1f ms wall" % (label, (time.perf_counter() - t0) * 1e3), flush=True)
        assert (c == ref.cpu().numpy()).all()
    del a, d_out, d_counts


if args.only in (None, "readme"):
    words = synth.readme_dictionary()
    block = synth.readme_text(2006, min(n, 1 << 25), words)
    d_hay = torch.from_numpy(block.view(np.int16)).cuda().repeat(max(1, n // block.size))
    run("README", words, d_hay, int(n * 1.75), (0, 1), hay_host=np.tile(block, max(1, n // block.size)) if args.cursor else None)
    del d_hay
if args.only in (None, "c2"):
    kws = synth.config_keywords("C2")
    d_hay = torch.empty(n, dtype=torch.int16, device="cuda")
    tab = np.ascontiguousarray(synth.ALPHA_LOWER)
    N.check(N.lib().acgpu_synth_fill(d_hay.data_ptr(), n, 0, synth.CONFIGS["C2"]["hay_seed"], tab.ctypes.data_as(ctypes.c_void_p), len(tab),
                                     ctypes.c_void_p(stream)), "synth_fill")
    run("C2", kws, d_hay, max(1 << 16, n // 64), (0,))
    del d_hay
if args.only in (None, "hot"):
    d_hay = torch.full((n,), ord("a"), dtype=torch.int16, device="cuda")
    run("one letter", ["a"], d_hay, n + 8, (1, 2))
