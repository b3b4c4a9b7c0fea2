#!/usr/bin/env python3
"""The ordered stream out of the device (sw_export_ordered_device: the gather of csrc/consensus.hip.h) in events/s against the
bytes it moves, and what keeping round received / consensus time costs a find_order call.

  default          one context, `--members` x `--events` (256 x 1 M), one pass (divide_rounds, decide_fame, find_order); then
                   `--laps` export calls over the whole order per set of arrays — every array, every array but the ids, the
                   two values alone — each timed from the call to the completion of the context's stream (host clock).
                   Bytes per event: read 4 (order) + 32 (id) + 4 (creator) + 4 + 8 (the two values), written 4 + 32 + 4 + 4 + 8;
                   without ids 64 less.  Prints a table and one JSON line.
  --order-laps K   K passes on one context (rewind in between), find_order's host time per pass, one JSON line.  With
                   SWEEP_LIB=<path> the process loads that build of the library instead (as profiles/knob_sweep.py does): run
                   the two builds in processes of their own, alternately, the older one first and last.

usage: python profiles/consensus_export_bench.py [--members 256] [--events 1000000] [--laps 10] [--order-laps K]"""
import argparse
import ctypes as C
import hashlib
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("py-swirld_amd")
if os.environ.get("SWEEP_LIB"):   # another build of the library for this process (the loader reads the path at its first call)
    _l = importlib.import_module("py-swirld_amd._lib")
    _l.LIB_PATH = os.path.abspath(os.environ["SWEEP_LIB"])
    _have = C.CDLL(_l.LIB_PATH)
    for _name in [k for k in _l.SIGNATURES if not hasattr(_have, k)]:   # (an older build: entries it does not export are not bound)
        del _l.SIGNATURES[_name]


def stats(x):
    x = np.array(x)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--laps", type=int, default=10)
    ap.add_argument("--order-laps", type=int, default=0)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    n, N = args.members, args.events
    h = pkg.Hashgraph(n)
    h.reserve(N)
    h.append_events(*pkg.synth_hashgraph(n, N, args.seed))

    def one_pass():
        h.rewind()
        h.divide_rounds(0, N)
        nc = h.decide_fame()
        h.synchronize()
        t0 = time.perf_counter()
        tx = h.find_order(nc)
        h.synchronize()      # (what the call left on the context's stream counts as its cost)
        return len(tx), (time.perf_counter() - t0) * 1e3

    if args.order_laps:
        one_pass()           # the first call of a context allocates
        ms = []
        for _ in range(args.order_laps):
            K, dt = one_pass()
            ms.append(dt)
        print(json.dumps({"library": os.environ.get("SWEEP_LIB", "this tree"), "members": n, "events": N, "ordered": K,
                          "find_order_ms": [round(x, 3) for x in ms], "median_ms": round(float(np.median(ms)), 3)}))
        return 0

    K, _ = one_pass()
    ids = np.frombuffer(b"".join(hashlib.blake2b(int(k).to_bytes(8, "little"), digest_size=32).digest() for k in range(N)), np.uint8).reshape(N, 32)
    h.set_event_ids(0, ids)
    hip = C.CDLL(pkg._lib.LIB_PATH)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]

    def dmalloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(nbytes, 16)) == 0
        return p.value
    buf = dict(event=dmalloc(4 * K), ids=dmalloc(32 * K), creator=dmalloc(4 * K), round_received=dmalloc(4 * K), time=dmalloc(8 * K))
    sets = (("every array", ("event", "ids", "creator", "round_received", "time"), 104),
            ("without ids", ("event", "creator", "round_received", "time"), 40),
            ("the two values", ("round_received", "time"), 28))
    result = {"members": n, "events": N, "ordered": K, "laps": args.laps, "lanes_per_position": 4}
    print("== %d members x %d events, %d ordered; %d export calls over the whole order per set of arrays" % (n, N, K, args.laps))
    for name, keys, nbytes in sets:
        kw = {k: buf[k] for k in keys}
        h.export_ordered_device(0, K, **kw)
        h.synchronize()
        ms = []
        for _ in range(args.laps):
            t0 = time.perf_counter()
            h.export_ordered_device(0, K, **kw)
            h.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        s = stats(ms)
        s.update(bytes_per_event=nbytes, events_per_s=K / (s["median"] * 1e-3), gb_per_s=K * nbytes / (s["median"] * 1e-3) / 1e9)
        result[name] = s
        print("   %-16s median %8.3f ms  [%8.3f, %8.3f]   %8.1f M events/s   %3d B/event   %7.1f GB/s"
              % (name, s["median"], s["min"], s["max"], s["events_per_s"] / 1e6, nbytes, s["gb_per_s"]))
    print(json.dumps(result))
    for p in buf.values():
        hip.hipFree(C.c_void_p(p))
    h.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
