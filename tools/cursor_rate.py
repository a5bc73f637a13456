#!/usr/bin/env python3
"""Development tool: the match cursor (acgpu_cursor_*) against acgpu_match_u16 on the same host text -- time to the first page,
time to drain every page, and the host memory the records take (the cursor: its page buffer and the page handed out; the
single call: the record array it returns).  C2's dictionary over 2^29 units (AhoCorasickMap), and the README word list over
2^28 units of token text, Set and Map.  One JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ahocorasick_amd import _native as N, synth  # noqa: E402
from ahocorasick_amd.strings import Automaton, Cursor  # noqa: E402


def measure(name, auto, hay, ids, page, reps, skip_single):
    rk = N.REC_MAP if ids else N.REC_SET
    res = dict(case=name, units=int(hay.size), page_records=page)
    if not skip_single:
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = auto.match_host(hay, ids)
            ts.append(time.perf_counter() - t0)
            n_single = len(r)
            del r
        res.update(single_ms=1e3 * float(np.median(ts)), single_records=n_single, single_host_bytes=n_single * rk)
    first, full = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        with Cursor(auto, hay, ids) as c:
            p = c.next(page)
            first.append(time.perf_counter() - t0)
            total = len(p)
            while len(p):
                p = c.next(page)
                total += len(p)
            st = c.stats()
        full.append(time.perf_counter() - t0)
    res.update(first_page_ms=1e3 * float(np.median(first)), drain_ms=1e3 * float(np.median(full)), cursor_records=total,
               cursor_host_bytes=2 * min(page, max(total, 1)) * rk, pieces=st["pieces"], rescans=st["rescans"])
    if not skip_single:
        res["drain_vs_single"] = res["drain_ms"] / res["single_ms"]
        assert total == res["single_records"], (total, res["single_records"])
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--page", type=int, default=1 << 20)
    ap.add_argument("--skip-single", action="store_true", help="cursor only (the single call of a dense text needs GBs)")
    ap.add_argument("--only", choices=["C2", "README"], default=None)
    args = ap.parse_args()
    if args.only in (None, "C2"):
        auto = Automaton(N.MODE_ALL, synth.config_keywords("C2"), True)
        measure("C2 AhoCorasickMap 2^29", auto, synth.haystack(2002, 1 << 29), True, args.page, args.reps, args.skip_single)
    if args.only in (None, "README"):
        words = synth.readme_dictionary()
        block = synth.readme_text(2006, 1 << 25, words)
        hay = np.tile(block, 8)  # 2^28 units
        for ids in (False, True):
            auto = Automaton(N.MODE_ALL, words, True)
            measure("README AhoCorasick%s 2^28" % ("Map" if ids else "Set"), auto, hay, ids, args.page, args.reps, args.skip_single)


if __name__ == "__main__":
    main()
