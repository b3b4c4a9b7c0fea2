"""sw_append_events (host arrays) against sw_append_events_device (arrays resident on the device), one process, no torch.

Per size: laps alternate  reset + append(host)  and  reset + append_device, each followed by divide_rounds + decide_fame +
read-back of the rounds; the host variant runs first and last, so a drift of the machine shows up as a difference between
its first and last laps.  The host variant is the code path bulk appends have always taken: it is the baseline.

Reported per variant, median and [min, max] over the laps, in ms:
  append   the append call alone
  divide   the sw_divide_rounds call that follows (beyond 256 members it starts with the heights the level sweep is sized by:
           the host variant computes them in ensure_dag_h's sequential loop, the device variant waits for its heights kernel)
  pass     append + divide_rounds + decide_fame + rounds read back
Both variants must end in the same new_c and the same round array, or nothing is printed but the mismatch.

usage: python profiles/ingest_device_bench.py [--laps 7] [--sizes 256x1000000,1024x2000000]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--laps", type=int, default=7)
    ap.add_argument("--sizes", default="256x1000000,1024x2000000")
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    pkg = importlib.import_module("py-swirld_amd")
    hip = C.CDLL(pkg.LIB_PATH)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    for size in args.sizes.split(","):
        n, N = (int(x) for x in size.split("x"))
        stream = pkg.synth_hashgraph(n, N, args.seed)
        dev = []
        for a in stream:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), a.nbytes) == 0
            assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
            dev.append(p)
        h = pkg.Hashgraph(n)
        h.reserve(N)

        def lap(variant):
            h.reset()
            h.synchronize()
            t0 = time.perf_counter()
            if variant == "host":
                h.append_events(*stream)
            else:
                h.append_events_device(*[p.value for p in dev], count=N)
            t1 = time.perf_counter()
            h.divide_rounds(0, N)
            t2 = time.perf_counter()
            nc = list(h.decide_fame())
            rounds = h.rounds()
            t3 = time.perf_counter()
            return {"append": (t1 - t0) * 1e3, "divide": (t2 - t1) * 1e3, "pass": (t3 - t0) * 1e3}, nc, rounds

        for v in ("host", "device"):   # warm-up: allocations, graphs, the first-shot history of the round loop
            lap(v)
        times = {"host": [], "device": []}
        ref = None
        order = ["host" if i % 2 == 0 else "device" for i in range(2 * args.laps + 1)]   # host first and last
        for v in order:
            tm, nc, rounds = lap(v)
            if ref is None:
                ref = (nc, rounds)
            elif nc != ref[0] or not np.array_equal(rounds, ref[1]):
                print("MISMATCH between the variants at %s (%s lap): nothing is reported" % (size, v))
                return 1
            times[v].append(tm)
        st = h.ingest_stats()
        out = {"members": n, "events": N, "seed": args.seed, "laps": {v: len(times[v]) for v in times}, "ingest_stats": st}
        print("== %d members x %d events, seed %d: %d host laps, %d device laps (alternating, host first and last); "
              "same new_c and rounds in every lap" % (n, N, args.seed, len(times["host"]), len(times["device"])))
        print("   device batches %d, fallbacks %d, events whose height the host loop computed %d (the host variant's laps)"
              % (st["device_batches"], st["fallback_batches"], st["host_height_events"]))
        for key in ("append", "divide", "pass"):
            row = {}
            for v in ("host", "device"):
                x = np.array([t[key] for t in times[v]])
                row[v] = {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}
                print("   %-7s %-7s median %8.3f ms   [%8.3f, %8.3f]   first lap %8.3f, last lap %8.3f"
                      % (key, v, row[v]["median"], row[v]["min"], row[v]["max"], x[0], x[-1]))
            out[key] = row
        for v in ("host", "device"):
            out["events_per_s_end_to_end_" + v] = N / (out["pass"][v]["median"] * 1e-3)
        print(json.dumps(out))
        h.close()
        for p in dev:
            hip.hipFree(p)
    return 0


if __name__ == "__main__":
    sys.exit(main())
