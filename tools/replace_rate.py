"""Development tool: what a rewrite costs beyond the match call it contains, one box, one process --
  match   : acgpu_match_device with Map records on a device-resident text (the scan inside a rewrite);
  replace : acgpu_replace_device on the same text (scan + plan + emit);
  probe   : acgpu_stream_probe pattern 1 over 2 N + 2 N_out bytes (a pure read of what the emit moves).
Workloads: config 4's dictionary (LongestMatch) over its text; the README word list with WholeWordMatch in synth.readme_text.
--batch N instead: N haystacks of the README paragraph's size (400-600 units of synth.readme_text) rewritten by ONE
acgpu_replace_batch_u16 call and by a loop of acgpu_replace_u16 calls (at most --loop of them) on the same build, per haystack.
usage: replace_rate.py [--log2 28] [--only c4|readme] | --batch N [--loop 2000]"""
import argparse, ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from ahocorasick_amd import _native as N, synth
from ahocorasick_amd.strings import Automaton
from ahocorasick_amd.unicode_tables import default_word_chars

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=28)
ap.add_argument("--only", default=None)
ap.add_argument("--batch", type=int, default=0)
ap.add_argument("--loop", type=int, default=2000)
args = ap.parse_args()


def batch_mode(n_hay, n_loop):
    words = synth.readme_dictionary()
    a = Automaton(N.MODE_WHOLEWORD, words, True, word_chars=default_word_chars())
    rng = np.random.default_rng(5)
    text = synth.readme_text(2006, n_hay * 600, words)
    cuts = np.concatenate([[0], np.cumsum(rng.integers(400, 600, n_hay))])
    hays = [text[cuts[i]:cuts[i + 1]] for i in range(n_hay)]
    units, off, st = a.replace_batch(hays, "***")  # (warm: the pool's buffers, the size)
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        units, off, st = a.replace_batch(hays, "***", cap=int(units.size) + 16)
        times.append(time.perf_counter() - t0)
    dt = float(np.median(times))
    print("batch : %d haystacks of ~500 units, %d keywords, %d records, %d pieces: %.3f ms per call = %.3f us per haystack" % (
        n_hay, len(words), st["n_records"], st["pieces"], dt * 1e3, dt * 1e6 / n_hay))
    some = hays[:min(n_hay, n_loop)]
    for h in some[:20]:
        a.replace_host(h, "***")
    t0 = time.perf_counter()
    got = [a.replace_host(h, "***")[0] for h in some]
    dt = time.perf_counter() - t0
    print("loop  : acgpu_replace_u16 per haystack, %d calls: %.1f us per haystack" % (len(some), dt / len(some) * 1e6), flush=True)
    o = off.tolist()
    assert all((units[o[i]:o[i + 1]] == g).all() for i, g in enumerate(got)), "batch and loop differ"


if args.batch:
    batch_mode(args.batch, args.loop)
    sys.exit(0)
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


def run(label, a, d_hay, rec_cap, repls):
    d_recs = torch.empty((rec_cap, 3), dtype=torch.int32, device="cuda")

    def match():
        nm, rc, _, _ = a.match_device(d_hay.data_ptr(), n, True, d_recs.data_ptr(), rec_cap, stream=stream)
        assert rc == 0, rc
        return nm
    ms_match, n_recs = timed(match)
    need, rc, _ = a.replace_device(d_hay.data_ptr(), n, repls, 0, 0, stream=stream)  # cap 0: the size
    assert rc in (N.OK, N.E_OVERFLOW), rc
    d_out = torch.empty(need + 8, dtype=torch.int16, device="cuda")

    def replace():
        n_out, rc, st = a.replace_device(d_hay.data_ptr(), n, repls, d_out.data_ptr(), need, stream=stream)
        assert rc == 0 and n_out == need, (rc, n_out)
        return st
    ms_repl, st = timed(replace)
    assert st["n_records"] == n_recs, (st, n_recs)
    nbytes = 2 * n + 2 * need
    d_probe = torch.empty(nbytes // 2 + 8, dtype=torch.int16, device="cuda")
    ms_probe = ctypes.c_float(0)
    N.check(N.lib().acgpu_stream_probe(d_probe.data_ptr(), nbytes & ~15, ctypes.c_void_p(stream), 5, 1, ctypes.byref(ms_probe)), "stream_probe")
    print("%-8s N=%d  R=%d  N_out=%d  pieces=%d rescans=%d" % (label, n, n_recs, need, st["pieces"], st["rescans"]))
    print("%-8s match %.3f ms | replace %.3f ms | beyond the match %.3f ms | pure read of 2N+2N_out %.3f ms (x%.1f)" % (
        label, ms_match, ms_repl, ms_repl - ms_match, ms_probe.value, (ms_repl - ms_match) / max(ms_probe.value, 1e-6)), flush=True)


if args.only in (None, "c4"):
    kws = synth.config_keywords("C4")
    d_hay = torch.empty(n, dtype=torch.int16, device="cuda")
    tab = np.ascontiguousarray(synth.ALPHA_LOWER)
    N.check(N.lib().acgpu_synth_fill(d_hay.data_ptr(), n, 0, synth.CONFIGS["C4"]["hay_seed"], tab.ctypes.data_as(ctypes.c_void_p), len(tab),
                                     ctypes.c_void_p(stream)), "synth_fill")
    run("C4", Automaton(N.MODE_LONGEST, kws, True), d_hay, n // 2 + 1024, "#")
    del d_hay
if args.only in (None, "readme"):
    words = synth.readme_dictionary()
    block = synth.readme_text(2006, min(n, 1 << 25), words)
    d_hay = torch.from_numpy(block.view(np.int16)).cuda().repeat(max(1, n // block.size))
    run("README", Automaton(N.MODE_WHOLEWORD, words, True, word_chars=default_word_chars()), d_hay, n // 2 + 1024, "***")
