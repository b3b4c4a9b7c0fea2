#!/usr/bin/env python3
"""Filling a batch: histories generated on the device (sw_synth_batch, csrc/batch_synth.hip.h) against the host route, which
is what the library offered before.

Routes, per shape (members x B x schedule), 600 events per hashgraph, distinct seeds, gossip mode 0:
  (h) host    synth_hashgraph per hashgraph on one host core (gen), then HashgraphBatch.append of the CSR arrays (append:
              slicing the instalment out of the generated arrays, host validation, upload of 88 bytes per event, scatter
              kernel, synchronise).  Timed in three parts: gen, append, total.
  (d) device  synth_begin once, then synth(K) per instalment: one launch and one read-back of 8 bytes per hashgraph per
              call; every call ends synchronised.
Schedules: "one-call" (all 600 events at once) and "of-8" (the roots — max(n, 8) events — then 8 events per hashgraph and
call).  A fresh batch per lap, made outside the windows.  One untimed lap per route first, after which both batches must
hold equal export_events() arrays (creator and height of every event; the bit-for-bit comparison of parents and
signatures is tests/test_gpu_batch_synth.py's).  Then laps alternate (h), (d), ..., (h); medians with min and max.
--device-only runs route (d) alone, once per shape: what a rocprofv3 --kernel-trace --stats run of its own wraps.

usage: python profiles/batch_synth_bench.py [--members 4,16,64] [--B 64,1024,8192] [--events 600] [--laps 2]
       [--schedules one-call,of-8] [--device-only]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
pkg = importlib.import_module("py-swirld_amd")


def med(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def schedule(n, N, chunk):
    """Instalments per hashgraph: the roots first and together."""
    if chunk >= N:
        return [N]
    out = [max(n, chunk)]
    while sum(out) < N:
        out.append(min(chunk, N - sum(out)))
    return out


def host_lap(n, B, N, seeds, sched, cap_rounds):
    hb = pkg.HashgraphBatch(B, n, cap_events=N, cap_rounds=cap_rounds)
    t0 = time.perf_counter()
    streams = [pkg.synth_hashgraph(n, N, int(s)) for s in seeds]
    t1 = time.perf_counter()
    cols = [np.stack([st[k] for st in streams]) for k in range(5)]   # [B][N] per array ([B][N][64] for the signatures)
    at = 0
    for k in sched:
        off = np.arange(B + 1, dtype=np.int64) * k
        part = [np.ascontiguousarray(c[:, at:at + k]).reshape((B * k,) + c.shape[2:]) for c in cols]
        hb.append(off=off, creator=part[0], self_parent=part[1], other_parent=part[2], t=part[3], sig=part[4])   # (ends synchronised)
        at += k
    t2 = time.perf_counter()
    return (t1 - t0, t2 - t1, t2 - t0), hb, streams


def device_lap(n, B, N, seeds, sched, cap_rounds):
    hb = pkg.HashgraphBatch(B, n, cap_events=N, cap_rounds=cap_rounds)
    t0 = time.perf_counter()
    hb.synth_begin(seeds)
    for k in sched:
        hb.synth(k)   # (ends synchronised)
    return time.perf_counter() - t0, hb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="4,16,64")
    ap.add_argument("--B", default="64,1024,8192")
    ap.add_argument("--events", type=int, default=600)
    ap.add_argument("--laps", type=int, default=2, help="laps of the device route; the host route runs one more")
    ap.add_argument("--schedules", default="one-call,of-8")
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    N = args.events
    print("# members B schedule calls | (h) host: gen ms, append ms, total ms (min .. max) | (d) device: total ms (min .. max) | (h) / (d)")
    for n in (int(v) for v in args.members.split(",")):
        for B in (int(v) for v in args.B.split(",")):
            seeds = np.arange(300, 300 + B, dtype=np.uint64)
            for name, chunk in (("one-call", N), ("of-8", 8)):
                if name not in args.schedules.split(","):
                    continue
                sched = schedule(n, N, chunk)
                if args.device_only:
                    device_lap(n, B, N, seeds, sched, 0)[1].close()
                    dt, hb = device_lap(n, B, N, seeds, sched, 0)
                    hb.close()
                    print("%3d %5d %-8s %3d | (d) %9.3f ms" % (n, B, name, len(sched), 1e3 * dt), flush=True)
                    continue
                # the untimed lap: warm-up of both routes, the capacity in rounds, and equal contents
                _, hh, streams = host_lap(n, B, N, seeds, sched, 0)
                cap_rounds = int(hh.export_events()["height"].max()) + 3
                _, hd = device_lap(n, B, N, seeds, sched, cap_rounds)
                eh, ed = hh.export_events(), hd.export_events()
                assert all(np.array_equal(eh[k], ed[k]) for k in eh), (n, B, name)
                hh.close(), hd.close()
                del streams, eh, ed
                th, td = [], []
                for lap in range(args.laps):
                    t, hb, _ = host_lap(n, B, N, seeds, sched, cap_rounds)
                    hb.close()
                    th.append(t)
                    t, hb = device_lap(n, B, N, seeds, sched, cap_rounds)
                    hb.close()
                    td.append(t)
                t, hb, _ = host_lap(n, B, N, seeds, sched, cap_rounds)
                hb.close()
                th.append(t)
                gen, app, tot = (med([1e3 * t[i] for t in th]) for i in range(3))
                dev = med([1e3 * t for t in td])
                out = {"members": n, "B": B, "schedule": name, "calls": len(sched), "events": B * N,
                       "host": {"gen_ms": gen, "append_ms": app, "total_ms": tot}, "device": {"total_ms": dev},
                       "host_over_device": tot["median"] / dev["median"]}
                print("%3d %5d %-8s %3d | (h) %9.3f + %9.3f = %9.3f ms (%.3f .. %.3f) | (d) %9.3f ms (%.3f .. %.3f) | x %.2f"
                      % (n, B, name, len(sched), gen["median"], app["median"], tot["median"], tot["min"], tot["max"], dev["median"], dev["min"],
                         dev["max"], out["host_over_device"]), flush=True)
                print("JSON " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
