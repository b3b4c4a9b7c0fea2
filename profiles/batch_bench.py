#!/usr/bin/env python3
"""Many small hashgraphs: a batch step (sw_batch_step, csrc/batch.hip.h) against the same hashgraphs as single contexts called
one after another, which is what the library offered before.

Routes, per shape (members x B x schedule x input):
  singles  one Hashgraph per hashgraph, called in turn: divide_rounds, decide_fame, find_order per step.  Fork-free inputs run
           on the round-synchronous fast path, forked inputs on the exact path.  The route is serial, so its cost per hashgraph
           does not depend on B: it is MEASURED over min(B, --singles) hashgraphs and reported per hashgraph; the aggregate
           events/s is that of the measured ones.
  batch    one HashgraphBatch of B hashgraphs, one sw_batch_step per step (K = all events, or 8 per hashgraph and step).
Both windows are whole calls on the host clock and end in a synchronise (every call of either route reads results back);
appends are outside both windows (a context is rewound, a batch is made anew, per lap).  The singles' calls return new_c and the
ordered events to Python; the batch's step reads back the per-hashgraph summaries, and the ordered events are fetched after the
window, where the two routes are compared: rounds and transactions of every distinct stream must be equal.
Laps alternate between the routes, singles first and last; medians with min and max.  Streams: --distinct seeds, cycled over B.

usage: python profiles/batch_bench.py [--members 4,8,16,64] [--B 1,64,1024,8192] [--events 600] [--laps 2] [--singles 16]"""
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


def singles_lap(hs, lens, chunk):
    for h in hs:
        h.rewind()
    for h in hs:
        h.synchronize()
    t0 = time.perf_counter()
    steps = 0
    for h, N in zip(hs, lens):
        for a in range(0, N, chunk):
            h.divide_rounds(a, min(chunk, N - a))
            h.find_order(h.decide_fame())
            steps += 1
    return time.perf_counter() - t0, steps


def batch_lap(n, B, streams, lens, cat, off, chunk, cap_rounds):
    hb = pkg.HashgraphBatch(B, n, cap_events=int(lens.max()), cap_rounds=cap_rounds)
    hb.append(off=off, creator=cat[0], self_parent=cat[1], other_parent=cat[2], t=cat[3], sig=cat[4])
    left = lens.copy()
    t0 = time.perf_counter()
    steps = 0
    while left.any():
        K = np.minimum(left, chunk)
        failed = hb.step(K, collect=False)   # (ends in the read-back of the summaries: a synchronise)
        assert failed == 0
        left -= K
        steps += 1
    return time.perf_counter() - t0, steps, hb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="4,8,16,64")
    ap.add_argument("--B", default="1,64,1024,8192")
    ap.add_argument("--events", type=int, default=600)
    ap.add_argument("--laps", type=int, default=2, help="laps of the batch route; the singles run one more")
    ap.add_argument("--singles", type=int, default=16, help="hashgraphs the serial route is measured over, at the most")
    ap.add_argument("--distinct", type=int, default=16)
    args = ap.parse_args()
    print("# members B schedule input | batch: ms/step, events/s | singles: ms/step per hashgraph, events/s | batch / singles (events/s)")
    for n in (int(v) for v in args.members.split(",")):
        for forked in (False, True):
            base = [pkg.synth_hashgraph(n, args.events, 300 + s) for s in range(args.distinct)]
            if forked:
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
                S = min(B, args.singles)
                hs = [pkg.Hashgraph(n) for _ in range(S)]
                for h, i in zip(hs, idx):
                    h.append_events(*base[i])
                    assert h.exact == forked
                for sched, chunk in (("one-step", int(lens.max())), ("steps-of-8", 8)):
                    ts, tb, hb = [], [], None
                    singles_lap(hs, lens[:S], chunk)   # warm-up of both routes, untimed
                    batch_lap(n, B, base, lens, cat, off, chunk, hmax + 3)[2].close()
                    for lap in range(args.laps):
                        ts.append(singles_lap(hs, lens[:S], chunk))
                        if hb is not None:
                            hb.close()
                        dt, steps, hb = batch_lap(n, B, base, lens, cat, off, chunk, hmax + 3)
                        tb.append((dt, steps))
                    ts.append(singles_lap(hs, lens[:S], chunk))
                    for b in range(min(B, S, len(base))):   # same results
                        assert np.array_equal(hb.rounds(b), hs[b].rounds()), (n, B, sched, b)
                        assert np.array_equal(hb.transactions(b), hs[b].transactions()), (n, B, sched, b)
                    bytes_dev = hb.device_bytes
                    hb.close()
                    ev_b, ev_s = int(lens.sum()), int(lens[:S].sum())
                    rb = med([ev_b / t for t, _ in tb])
                    rs = med([ev_s / t for t, _ in ts])
                    ms_b = med([1e3 * t / k for t, k in tb])
                    ms_s = med([1e3 * t / k for t, k in ts])   # (k counts the steps of all measured hashgraphs)
                    out = {"members": n, "B": B, "schedule": sched, "input": "forked" if forked else "fork-free", "events": ev_b,
                           "batch": {"ms_per_step": ms_b, "events_per_s": rb, "steps": tb[0][1], "device_bytes": bytes_dev},
                           "singles": {"measured_hashgraphs": S, "ms_per_step_per_hashgraph": ms_s, "events_per_s": rs},
                           "batch_over_singles": rb["median"] / rs["median"]}
                    print("%3d %5d %-10s %-9s | %9.3f ms  %12.0f ev/s (%.0f .. %.0f) | %7.3f ms  %10.0f ev/s (%.0f .. %.0f) | x %.2f"
                          % (n, B, sched, out["input"], ms_b["median"], rb["median"], rb["min"], rb["max"], ms_s["median"], rs["median"], rs["min"],
                             rs["max"], out["batch_over_singles"]), flush=True)
                    print("JSON " + json.dumps(out), flush=True)
                for h in hs:
                    h.close()


if __name__ == "__main__":
    main()
