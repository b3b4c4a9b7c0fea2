#!/usr/bin/env python3
"""What it costs to READ a batch step's results: the step of profiles/batch_bench.py (same inputs, same schedules) by three routes.

  (a) step(collect=False)   the results stay on the device; only the per-hashgraph summaries come back (what batch_bench.py times)
  (b) step(collect=True)    new_c and the newly ordered events of every hashgraph that took part, by the per-hashgraph getters:
                            one or two blocking copies per hashgraph and step
  (c) step_arrays()         the same, and round received and consensus timestamp of the ordered events besides, as ragged arrays
                            by two whole-batch exports (sw_export_batch_new_rounds, sw_export_batch_ordered): one launch and one
                            synchronisation each, whatever B
Every window is a whole run of the schedule on the host clock; every call in it ends synchronised (each route reads back at least
the summaries).  A fresh batch per lap, made and filled outside the window.  One untimed lap of every route first, where (b) and
(c) are compared: the same hashgraphs took part, new_c and the ordered events are equal, step by step.  Then laps alternate
b, a, c, b, a, c, ..., b — (b) first and last; median (min .. max) of the ms per step.

usage: python profiles/batch_export_bench.py [--members 4,16,64] [--B 64,1024,8192] [--events 600] [--laps 2] [--inputs fork-free,forked]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("py-swirld_amd")
from test_exact_host import add_forks  # noqa: E402  (test helper: forked stream generator)


def med(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def lap(route, n, B, lens, cat, off, chunk, cap_rounds, keep=False):
    hb = pkg.HashgraphBatch(B, n, cap_events=int(lens.max()), cap_rounds=cap_rounds)
    hb.append(off=off, creator=cat[0], self_parent=cat[1], other_parent=cat[2], t=cat[3], sig=cat[4])
    left = lens.copy()
    kept, steps = [], 0
    t0 = time.perf_counter()
    while left.any():
        K = np.minimum(left, chunk)
        if route == "a":
            r = hb.step(K, collect=False)
        elif route == "b":
            r = hb.step(K, collect=True)
        else:
            r = hb.step_arrays(K)
        if keep:
            kept.append(r)
        left -= K
        steps += 1
    dt = time.perf_counter() - t0
    assert hb.n_failed == 0
    stats = hb.export_stats()
    hb.close()
    return dt, steps, kept, stats


def same_results(by_getters, by_arrays):
    cat = lambda parts, dtype: np.concatenate(parts) if parts else np.zeros(0, dtype)
    entries = 0
    for out, sa in zip(by_getters, by_arrays):
        took = np.array([o is not None for o in out])
        assert np.array_equal(took, sa.took)
        nc, tx = [o[0] for o in out if o is not None], [o[1] for o in out if o is not None]
        assert np.array_equal(np.diff(sa.rounds_off)[took], [len(x) for x in nc]) and not np.diff(sa.rounds_off)[~took].any()
        assert np.array_equal(np.diff(sa.tx_off)[took], [len(x) for x in tx]) and not np.diff(sa.tx_off)[~took].any()
        assert np.array_equal(cat(nc, np.int32), sa.rounds) and np.array_equal(cat(tx, np.int32), sa.event)
        assert len(sa.round_received) == len(sa.time) == len(sa.event)
        entries += len(sa.event)
    return entries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="4,16,64")
    ap.add_argument("--B", default="64,1024,8192")
    ap.add_argument("--events", type=int, default=600)
    ap.add_argument("--laps", type=int, default=2, help="laps of (a) and (c); (b) runs one more")
    ap.add_argument("--inputs", default="fork-free,forked")
    ap.add_argument("--distinct", type=int, default=16)
    args = ap.parse_args()
    print("# ms per step, median (min .. max) over the laps; every call ends synchronised")
    print("# members B schedule input steps | (a) collect=False | (b) collect=True: getters | (c) step_arrays: 2 exports | (b) / (c) | (c) - (a)")
    for n in (int(v) for v in args.members.split(",")):
        for kind in args.inputs.split(","):
            base = [pkg.synth_hashgraph(n, args.events, 300 + s) for s in range(args.distinct)]
            if kind == "forked":
                base = [add_forks(st, n, 300 + s, 5) for s, st in enumerate(base)]
            hmax = 0
            for st in base:   # cap_rounds: the greatest height + 3 (what an append checks), not cap_events + 3
                ht = np.zeros(len(st[0]), np.int64)
                for e in range(len(st[0])):
                    if st[1][e] >= 0:
                        ht[e] = max(ht[st[1][e]], ht[st[2][e]]) + 1
                hmax = max(hmax, int(ht.max()))
            for B in (int(v) for v in args.B.split(",")):
                idx = np.arange(B) % len(base)
                lens = np.array([len(base[i][0]) for i in idx], np.int64)
                off = np.zeros(B + 1, np.int64)
                np.cumsum(lens, out=off[1:])
                cat = [np.concatenate([base[i][k] for i in idx]) for k in range(5)]
                for sched, chunk in (("one-step", int(lens.max())), ("steps-of-8", 8)):
                    shape = (n, B, lens, cat, off, chunk, hmax + 3)
                    lap("a", *shape)
                    _, steps, got_b, _ = lap("b", *shape, keep=True)
                    _, _, got_c, stats = lap("c", *shape, keep=True)
                    ordered = same_results(got_b, got_c)
                    assert stats.calls == 2 * steps and stats.launches <= 2 * steps
                    del got_b, got_c
                    t = {"a": [], "b": [], "c": []}
                    for _ in range(args.laps):
                        for route in "bac":
                            t[route].append(1e3 * lap(route, *shape)[0] / steps)
                    t["b"].append(1e3 * lap("b", *shape)[0] / steps)
                    m = {k: med(v) for k, v in t.items()}
                    out = {"members": n, "B": B, "schedule": sched, "input": kind, "steps": steps, "events": int(lens.sum()), "ordered": ordered,
                           "export_launches": stats.launches, "ms_per_step": m, "b_over_c": m["b"]["median"] / m["c"]["median"],
                           "c_minus_a_ms": m["c"]["median"] - m["a"]["median"]}
                    cell = lambda k: "%9.3f (%.3f .. %.3f)" % (m[k]["median"], m[k]["min"], m[k]["max"])
                    print("%3d %5d %-10s %-9s %3d | %s | %s | %s | x %7.2f | %+.3f ms"
                          % (n, B, sched, kind, steps, cell("a"), cell("b"), cell("c"), out["b_over_c"], out["c_minus_a_ms"]), flush=True)
                    print("JSON " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
