#!/usr/bin/env python3
"""Gossip networks in a batch (sw_network_batch_*) against the best route the library offered before for the same job.

Job: G networks of n nodes run 200 turns each (one seed for all networks of a cell: the work is the same per network).
  (b) baseline   the Python model (tests/model_batch_network.py) computes every turn's import — OUTSIDE the timed window,
                 reported as "model" —, then per turn ONE ragged append() of the puller views' new events and ONE step() for
                 all networks: 200 appends + 200 steps, the arrays of every call prepared outside the window.
  (r) run        network_begin + network_run(200): the device draws the schedule.
  (t) turns      network_begin + network_turns(schedule of synth_schedule): the explicit form, one call.
Before any lap is timed the three batches must hold equal export_events / export_rounds / export_ordered arrays.
Laps alternate b, r, t, b, r, t, b (baseline first and last); every call ends synchronised; fresh batches are made outside
the windows.  Reported: median ms per lap, aggregate turns/s and stored events/s of (r), and (b) / (r).

--device-only runs route (r) alone, once, for one cell: what a rocprofv3 --kernel-trace --stats run of its own wraps
(profiles/batch_network_kernel_stats.txt).

Usage:  python profiles/batch_network_bench.py [--out FILE] [--quick] | --device-only --members N --G G
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import model_batch_network as M  # noqa: E402

T = 200


def plan(n, seed):
    """Per turn of the model's run: (puller, the puller view's new events as arrays)."""
    t0 = time.perf_counter()
    m = M.Network(n, seed)
    m.run(T)
    arrays = [v.arrays() for v in m.views]
    at = [1] * n
    calls = []
    for i, _ in m.schedule:
        first, K = m.views[i].steps[at[i]]
        at[i] += 1
        calls.append((i, K, tuple(a[first:first + K] for a in arrays[i])))
    roots = [tuple(a[:1] for a in arrays[i]) for i in range(n)]
    return m, roots, calls, time.perf_counter() - t0


def csr(n, G, i, K, part):
    cnt = np.zeros(n * G, np.int64)
    cnt[i::n] = K
    off = np.zeros(n * G + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    return cnt, off, tuple(np.concatenate([a] * G) for a in part)


def baseline_inputs(n, G, roots, calls):
    B = n * G
    off = np.arange(B + 1, dtype=np.int64)
    root = tuple(np.concatenate([np.concatenate([r[k] for r in roots])] * G) for k in range(5))
    return (np.ones(B, np.int64), off, root), [csr(n, G, i, K, part) for i, K, part in calls]


def run_baseline(pkg, n, G, cap, inputs):
    hb = pkg.HashgraphBatch(n * G, n, cap_events=cap)
    t0 = time.perf_counter()
    for cnt, off, (cr, sp, op, t, sig) in [inputs[0]] + inputs[1]:
        hb.append(off=off, creator=cr, self_parent=sp, other_parent=op, t=t, sig=sig)
        hb.step(cnt, collect=False)
    return hb, time.perf_counter() - t0


def run_network(pkg, n, G, cap, seed, sched=None):
    hb = pkg.HashgraphBatch(n * G, n, cap_events=cap)
    t0 = time.perf_counter()
    hb.network_begin(seed)
    if sched is None:
        hb.network_run(T)
    else:
        hb.network_turns(off=np.arange(G + 1, dtype=np.int64) * T, puller=np.tile(sched[0], G), peer=np.tile(sched[1], G))
    return hb, time.perf_counter() - t0


def equal(a, b):
    for fn in ("export_events", "export_rounds", "export_ordered"):
        x, y = getattr(a, fn)(), getattr(b, fn)()
        for k in x:
            if x[k].tobytes() != y[k].tobytes():
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="G = 1 and 16 only")
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--G", type=int, default=2048)
    args = ap.parse_args()
    pkg = importlib.import_module("py-swirld_amd")
    if args.device_only:
        n = args.members
        h, s = run_network(pkg, n, args.G, n + T, 900 if n == 4 else 7)
        print("members %d, G %d: %d turns each, %.3f ms, %d launches" % (n, args.G, T, s * 1e3, h.network_stats().launches))
        h.close()
        return
    lines = ["# profiles/batch_network_bench.py: %d turns per network; ms per lap (median of laps; min-max)" % T,
             "# n  G  model_ms  (b) append+step  (r) run  (t) turns  (b)/(r)  turns/s (r)  stored events/s (r)  launches (r)"]
    for n in (4, 8, 16):
        seed = 900 if n == 4 else 7
        m, roots, calls, model_s = plan(n, seed)
        stored = sum(len(v.cr) for v in m.views)
        sched = pkg.synth_schedule(n, seed, 0, T)
        for G in ((1, 16) if args.quick else (1, 16, 256, 2048)):
            cap = n + T
            inputs = baseline_inputs(n, G, roots, calls)
            b, _ = run_baseline(pkg, n, G, cap, inputs)
            r, _ = run_network(pkg, n, G, cap, seed)
            t, _ = run_network(pkg, n, G, cap, seed, sched)
            assert equal(b, r) and equal(b, t), "the routes disagree"
            launches = r.network_stats().launches
            for h in (b, r, t):
                h.close()
            laps = {"b": [], "r": [], "t": []}
            for which in "brtbrtb":
                if which == "b":
                    h, s = run_baseline(pkg, n, G, cap, inputs)
                else:
                    h, s = run_network(pkg, n, G, cap, seed, None if which == "r" else sched)
                h.close()
                laps[which].append(s * 1e3)
            med = {k: statistics.median(v) for k, v in laps.items()}
            lines.append("%2d %5d %8.1f   %9.3f (%.3f-%.3f)  %8.3f (%.3f-%.3f)  %8.3f (%.3f-%.3f)  %6.2f  %12.0f  %12.0f  %d" % (
                n, G, model_s * 1e3, med["b"], min(laps["b"]), max(laps["b"]), med["r"], min(laps["r"]), max(laps["r"]),
                med["t"], min(laps["t"]), max(laps["t"]), med["b"] / med["r"], G * T / (med["r"] * 1e-3), G * stored / (med["r"] * 1e-3), launches))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
