#!/usr/bin/env python3
"""Node.votes out of the device in bulk (sw_export_votes[_device], csrc/votes.hip.h) against the per-entry route
(sw_get_vote), at 256 members x 1 M events and at 64 members x 100 k events, each after one pass (divide_rounds, decide_fame).

  default         the driver: per size one untimed process of this build that writes a random sample of the table's entries,
                  then processes of their own, alternately — per-entry route, bulk route, per-entry, bulk, per-entry (the older
                  route first and last).  With --parent-lib <path> the per-entry processes load that build of the library
                  (the parent commit's); without it they load this tree's, whose sw_get_vote is the same code.
  --route bulk    one context, one pass; `--laps` whole calls of export_votes over all rounds (size query + table into numpy
                  arrays), `--laps` calls of export_votes_device on resident arrays (to the completion of the stream), and the
                  phase times of sw_get_votes_stats under profiling.  One JSON line.
  --route entry   one context, one pass; sw_get_vote for the sampled entries, per entry, and EXTRAPOLATED to the whole table
                  (entries x time per entry: the table itself is never read that way — and a reader that does not know which
                  entries exist asks for every earlier witness slot, which costs more).  One JSON line.

usage: python profiles/votes_export_bench.py [--parent-lib PATH] [--laps 5] [--sample 2000]"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import tempfile
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

SIZES = ((256, 1_000_000, 3), (64, 100_000, 2))


def stats(x):
    x = np.array(x)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def one_pass(n, N, seed):
    h = pkg.Hashgraph(n)
    h.reserve(N)
    stream = pkg.synth_hashgraph(n, N, seed)
    h.append_events(*stream)
    h.divide_rounds(0, N)
    h.decide_fame()
    h.synchronize()
    return h, stream


def route_bulk(args):
    n, N = args.members, args.events
    h, stream = one_pass(n, N, args.seed)
    R, nwo = h.max_round + 1, (n + 63) // 64
    table = h.export_votes()           # the first call allocates
    rows = len(table[0])
    entries = int(np.unpackbits(np.ascontiguousarray(table[2]).view(np.uint8)).sum())
    if args.sample_out:                # (voter round, voter member, candidate round, candidate member) of random entries
        cr, rnd = stream[0], h.rounds()
        bits = np.unpackbits(np.ascontiguousarray(table[2]).view(np.uint8).reshape(rows, -1), axis=1, bitorder="little")
        i, mc = np.nonzero(bits)
        pick = np.random.default_rng(1).choice(len(i), min(args.sample, len(i)), replace=False)
        y = table[0][i[pick]]
        np.save(args.sample_out, np.stack([rnd[y], cr[y], table[1][i[pick]], mc[pick]], axis=1).astype(np.int32))
    host_ms = []
    for _ in range(args.laps):
        t0 = time.perf_counter()
        h.export_votes()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    hip = C.CDLL(pkg._lib.LIB_PATH)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    bufs = []
    for nbytes in (4 * rows, 4 * rows, 8 * rows * nwo, 8 * rows * nwo):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(nbytes, 16)) == 0
        bufs.append(p.value)
    h.export_votes_device(1, R, rows, *bufs)
    h.synchronize()
    dev_ms = []
    for _ in range(args.laps):
        t0 = time.perf_counter()
        h.export_votes_device(1, R, rows, *bufs)
        h.synchronize()
        dev_ms.append((time.perf_counter() - t0) * 1e3)
    h.set_profiling(True)
    h.export_votes_device(1, R, rows, *bufs)
    st = h.votes_stats()
    for p in bufs:
        hip.hipFree(C.c_void_p(p))
    print(json.dumps({"route": "bulk", "members": n, "events": N, "rounds": R, "rows": rows, "entries": entries,
                      "table_bytes": rows * (8 + 16 * nwo), "export_votes_ms": stats(host_ms), "export_votes_device_ms": stats(dev_ms),
                      "phase_ms": {"plan_existence_counts": st["phase_ms"][0], "rows_values": st["phase_ms"][1]},
                      "levels_per_call": st["levels"] // st["calls"]}))
    h.close()
    return 0


def route_entry(args):
    n, N = args.members, args.events
    h, _ = one_pass(n, N, args.seed)
    sample = np.load(args.sample_in)
    for rv, mv, rc, mc in sample[:50].tolist():   # warm
        h.vote(rv, mv, rc, mc)
    t0 = time.perf_counter()
    for rv, mv, rc, mc in sample.tolist():
        assert h.vote(rv, mv, rc, mc) >= 0
    dt = time.perf_counter() - t0
    print(json.dumps({"route": "entry", "library": "the parent commit's build" if os.environ.get("SWEEP_LIB") else "this tree", "members": n, "events": N,
                      "sampled_entries": len(sample), "us_per_entry": dt / len(sample) * 1e6, "mean_distance": float((sample[:, 0] - sample[:, 2]).mean())}))
    h.close()
    return 0


def driver(args):
    me = os.path.abspath(__file__)
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for n, N, seed in SIZES:
            common = [sys.executable, me, "--members", str(n), "--events", str(N), "--seed", str(seed), "--laps", str(args.laps), "--sample", str(args.sample)]
            path = os.path.join(tmp, "sample_%d.npy" % n)
            env_entry = dict(os.environ, SWEEP_LIB=args.parent_lib) if args.parent_lib else dict(os.environ)

            def child(extra, env=None):
                r = subprocess.run(common + extra, capture_output=True, text=True, env=env)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr[-3000:])
                    raise SystemExit(r.returncode)
                return json.loads(r.stdout.strip().splitlines()[-1])
            child(["--route", "bulk", "--sample-out", path, "--laps", "1"])
            entry, bulk = [], []
            for lap in range(5):
                if lap % 2 == 0:
                    entry.append(child(["--route", "entry", "--sample-in", path], env_entry))
                else:
                    bulk.append(child(["--route", "bulk"]))
            b = bulk[-1]
            us = [e["us_per_entry"] for e in entry]
            host = [x["export_votes_ms"]["median"] for x in bulk]
            dev = [x["export_votes_device_ms"]["median"] for x in bulk]
            extrap_s = float(np.median(us)) * 1e-6 * b["entries"]
            print("== %d members x %d events: %d rounds, %d rows, %d entries, table %.1f MB; %d levels replayed per call"
                  % (n, N, b["rounds"], b["rows"], b["entries"], b["table_bytes"] / 1e6, b["levels_per_call"]))
            print("   export_votes (size query + table to numpy)   median of process medians %9.3f ms   per process %s"
                  % (float(np.median(host)), ["%.3f" % x for x in host]))
            print("   export_votes_device (resident arrays)        median of process medians %9.3f ms   per process %s"
                  % (float(np.median(dev)), ["%.3f" % x for x in dev]))
            print("   phases of one device call under profiling: plan + existence + counts %.3f ms, rows + values %.3f ms"
                  % (b["phase_ms"]["plan_existence_counts"], b["phase_ms"]["rows_values"]))
            print("   sw_get_vote (%s), %d sampled entries, mean distance %.1f: %s us per entry (median %.1f)"
                  % (entry[0]["library"], entry[0]["sampled_entries"], entry[0]["mean_distance"], ["%.1f" % x for x in us], float(np.median(us))))
            print("   EXTRAPOLATED to the %d entries of the table: %.1f s  (%.0f x export_votes, %.0f x export_votes_device)"
                  % (b["entries"], extrap_s, extrap_s * 1e3 / float(np.median(host)), extrap_s * 1e3 / float(np.median(dev))))
            out.append({"members": n, "events": N, "bulk": bulk, "entry": entry, "extrapolated_entry_route_s": extrap_s})
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("bulk", "entry"))
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--laps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--sample-out")
    ap.add_argument("--sample-in")
    ap.add_argument("--parent-lib")
    args = ap.parse_args()
    if args.route == "bulk":
        return route_bulk(args)
    if args.route == "entry":
        return route_entry(args)
    return driver(args)


if __name__ == "__main__":
    sys.exit(main())
