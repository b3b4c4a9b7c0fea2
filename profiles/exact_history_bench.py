#!/usr/bin/env python3
"""What keeping the history of the exact (forked-hashgraph) path costs (sw_set_exact_history; csrc/exact_history.hip.h).

One process = one build of the library and one setting of the switch: forked hashgraphs at 8, 64 and 256 members, `--laps`
passes each (rewind in between), divide_rounds + decide_fame + find_order timed on the host clock, events/s per lap, one JSON
line per size.  With SWEEP_LIB=<path> the process loads that build instead (as profiles/consensus_export_bench.py does).

The comparison the design asks for: the parent commit's build against this one with the switch off — run in
processes of their own, alternately, the parent first and last — where "off" has to lie inside the spread of the parent's
own laps; then this build with `--history`, whose slowdown and store bytes per entry are reported beside them (no bar).

usage: [SWEEP_LIB=old.so] python profiles/exact_history_bench.py [--history] [--laps 5] [--sizes 8:20000,64:20000,256:8000]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("py-swirld_amd")
if os.environ.get("SWEEP_LIB"):   # another build of the library for this process (the loader reads the path at its first call)
    _l = importlib.import_module("py-swirld_amd._lib")
    _l.LIB_PATH = os.path.abspath(os.environ["SWEEP_LIB"])
    _have = C.CDLL(_l.LIB_PATH)
    for _name in [k for k in _l.SIGNATURES if not hasattr(_have, k)]:   # (an older build: entries it does not export are not bound)
        del _l.SIGNATURES[_name]
from test_exact_host import add_forks  # noqa: E402  (test helper: forked stream generator)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--history", action="store_true")
    ap.add_argument("--laps", type=int, default=5)
    ap.add_argument("--sizes", default="8:20000,64:20000,256:8000")
    args = ap.parse_args()
    for size in args.sizes.split(","):
        n, N = (int(v) for v in size.split(":"))
        stream = add_forks(pkg.synth_hashgraph(n, N, 5), n, 5, 20, start=0)
        K = len(stream[0])
        h = pkg.Hashgraph(n)
        if args.history:
            h.set_exact_history()
        h.append_events(*stream)
        assert h.exact
        rates, ordered = [], 0
        for _ in range(args.laps):
            h.rewind()
            h.synchronize()
            t0 = time.perf_counter()
            h.divide_rounds(0, K)
            ordered = len(h.find_order(h.decide_fame()))
            rates.append(K / (time.perf_counter() - t0))
        out = {"lib": os.environ.get("SWEEP_LIB", "this build"), "history": bool(args.history), "members": n, "events": K, "ordered": ordered,
               "events_per_s": {"median": float(np.median(rates)), "min": float(min(rates)), "max": float(max(rates))}}
        if args.history:
            st = h.vote_store_stats()
            out["store"] = {"entries": st["entries"], "bytes": st["bytes"], "bytes_per_entry": st["bytes"] / max(st["entries"], 1), "grows": st["grows"]}
        print(json.dumps(out), flush=True)
        h.close()


if __name__ == "__main__":
    main()
