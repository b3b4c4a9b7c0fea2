#!/usr/bin/env python3
"""What one gossip turn costs at 256 members, and what its one signature is made of.

  (a) ONE EVENT   Hashgraph.create_event (one wavefront signs: csrc/turn.hip.h) against create_events with K = 1 (one lane
                  signs: csrc/sign.hip.h), each call timed on the host from the call to its return (both synchronise).  Then
                  the stamp table of the one-wave kernel under set_profiling: wall_clock64() at its phase boundaries.
  (b) ONE TURN    two contexts; dst is `--behind` events behind src.  Hashgraph.gossip_turn against the calls it is defined
                  by (pull_from(walk=True), lookup_event_ids, create_events K = 1, divide_rounds, decide_fame, find_order),
                  with validation and data.  Every lap runs on a fresh dst.

The driver (no --child) runs every measurement in a process of its own: with --parent-lib <libswirld_hip.so of the parent
commit> the two builds alternate, the parent first and last, as profiles/consensus_export_bench.py asks.  A parent build has
no sw_create_event / sw_gossip_turn: its processes measure create_events(K = 1) and the composed calls only.

usage: python profiles/gossip_turn_bench.py [--parent-lib PATH] [--members 256] [--laps 30] [--turn-laps 5] [--behind 600] [--out FILE]"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_pkg():
    pkg = importlib.import_module("py-swirld_amd")
    if os.environ.get("SWEEP_LIB"):   # another build of the library for this process (the loader reads the path at its first call)
        _l = importlib.import_module("py-swirld_amd._lib")
        _l.LIB_PATH = os.path.abspath(os.environ["SWEEP_LIB"])
        have = C.CDLL(_l.LIB_PATH)
        for name in [k for k in _l.SIGNATURES if not hasattr(have, k)]:
            del _l.SIGNATURES[name]
    return pkg


def seeds_of(n):
    return [bytes([77, m & 255, m >> 8]) + bytes(29) for m in range(n)]


def signer(pkg, n):
    seeds = seeds_of(n)
    h = pkg.Hashgraph(n)
    assert h.set_member_keys([pkg.node.crypto.sign_seed_keypair(s)[0] for s in seeds]) == 0
    h.set_signing_seeds(list(range(n)), seeds)
    return h


def ms(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def child_one(args):
    pkg = load_pkg()
    n = args.members
    h = signer(pkg, n)
    root = np.full(n, -1, np.int32)
    h.create_events(np.arange(n, dtype=np.int32), root, root, np.arange(n, dtype=np.float64))
    head = list(range(n))
    have_one = hasattr(h._L, "sw_create_event")
    out = {"library": os.environ.get("SWEEP_LIB", "this tree"), "members": n, "create_events_k1_ms": [], "create_event_ms": []}

    def step(i, one):
        m, o = i % n, (i * 7 + 1) % n
        o = o if o != m else (o + 1) % n
        if one:
            idx, dt = ms(lambda: h.create_event(m, head[m], head[o], 1000.0 + i, b"payload %d" % i))
        else:
            idx, dt = ms(lambda: h.create_events([m], [head[m]], [head[o]], [1000.0 + i], [b"payload %d" % i]))
        head[m] = idx
        return dt

    for i in range(4):                     # the first calls of a context allocate
        step(i, False)
        if have_one:
            step(100 + i, True)
    for i in range(args.laps):             # alternating
        out["create_events_k1_ms"].append(step(1000 + 2 * i, False))
        if have_one:
            out["create_event_ms"].append(step(1001 + 2 * i, True))
    if have_one:
        h.set_profiling(True)
        rows = []
        for i in range(9):
            step(5000 + i, True)
            rows.append(h.turn_stats()["phase_us"])
        out["phase_us_median"] = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
        out["phase_us_laps"] = rows
        out["tick_ns"] = h.turn_stats()["tick_ns"]
    print(json.dumps(out))


def turn_universe(pkg, n, P, behind, seed=5):
    N = P + behind
    cr, sp, op, t, _ = pkg.synth_hashgraph(n, N, seed)
    member = int(cr[P - 1])
    late = set()
    for e in range(P, N):                  # a node's own newer events, and what is built on them, exist nowhere else
        if cr[e] == member or int(sp[e]) in late or int(op[e]) in late:
            late.add(e)
    events = np.array([e for e in range(N) if e not in late])
    loc = {int(e): i for i, e in enumerate(events)}
    rng = np.random.default_rng(seed)
    d = [None if e % 2 else rng.integers(0, 256, 24, dtype=np.uint8).tobytes() for e in range(N)]
    src_head = max(i for i, e in enumerate(events) if cr[e] != member)
    return dict(cr=cr, sp=sp, op=op, t=t, d=d, member=member, dst_head=P - 1, events=events, loc=loc, src_head=src_head)


def holder(pkg, n, u, events):
    loc = {int(e): i for i, e in enumerate(events)}
    cr = u["cr"][events]
    sp = np.array([loc[int(p)] if p >= 0 else -1 for p in u["sp"][events]], np.int32)
    op = np.array([loc[int(p)] if p >= 0 else -1 for p in u["op"][events]], np.int32)
    h = signer(pkg, n)
    h.create_events(cr, sp, op, u["t"][events], [u["d"][int(e)] for e in events])
    h.divide_rounds(0, len(events))
    h.find_order(h.decide_fame())
    return h


def child_turn(args):
    pkg = load_pkg()
    n, P = args.members, args.prefix
    u = turn_universe(pkg, n, P, args.behind)
    src = holder(pkg, n, u, u["events"])
    have_turn = hasattr(src._L, "sw_gossip_turn")
    out = {"library": os.environ.get("SWEEP_LIB", "this tree"), "members": n, "prefix": P, "src_events": int(len(u["events"])), "gossip_turn_ms": [],
           "composed_ms": [], "stored": None}
    m, dh, sh = u["member"], u["dst_head"], u["src_head"]

    def composed(dst):
        N0 = dst.num_events
        res = dst.pull_from(src, sh, dh, True, data=True, walk=True)
        idx = int(dst.lookup_event_ids(src.event_ids(sh, 1))[0])
        dst.create_events([m], [dh], [idx], [9e8], [b"turn"])
        dst.divide_rounds(N0, dst.num_events - N0)
        dst.find_order(dst.decide_fame())
        return res[-1]

    routes = [("composed_ms", composed)]
    if have_turn:
        routes.append(("gossip_turn_ms", lambda dst: dst.gossip_turn(src, m, dh, sh, 9e8, b"turn", validate=True, data_store=True).n_stored))
    for lap in range(args.turn_laps + 1):  # lap 0 warms up (allocations of src's scratch)
        for key, fn in routes:
            dst = holder(pkg, n, u, np.arange(P))
            dst.synchronize()
            stored, dt = ms(lambda: fn(dst))
            out["stored"] = int(stored)
            if lap:
                out[key].append(dt)
            dst.close()
    print(json.dumps(out))


def stats(x):
    x = np.asarray(x, float)
    return "median %9.3f ms   [%9.3f, %9.3f]   first lap %9.3f, last lap %9.3f" % (np.median(x), x.min(), x.max(), x[0], x[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("one", "turn"))
    ap.add_argument("--parent-lib")
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--laps", type=int, default=30)
    ap.add_argument("--turn-laps", type=int, default=5)
    ap.add_argument("--prefix", type=int, default=4000)
    ap.add_argument("--behind", type=int, default=600)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child == "one":
        return child_one(args)
    if args.child == "turn":
        return child_turn(args)

    def run(mode, lib):
        env = dict(os.environ)
        env.pop("SWEEP_LIB", None)
        if lib:
            env["SWEEP_LIB"] = lib
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--members", str(args.members), "--laps", str(args.laps), "--turn-laps",
               str(args.turn_laps), "--prefix", str(args.prefix), "--behind", str(args.behind)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420)
        if r.returncode != 0:
            raise SystemExit("child %s (%s) failed with %d:\n%s" % (mode, lib or "this tree", r.returncode, r.stderr[-3000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    order = [args.parent_lib, None, args.parent_lib, None, args.parent_lib] if args.parent_lib else [None, None]
    lines, record = [], []
    for mode, title in (("one", "(a) one event"), ("turn", "(b) one turn")):
        runs = [run(mode, lib) for lib in order]
        record += runs
        lines.append("== %s, %d members; processes in this order: %s" % (title, args.members, ", ".join("parent" if l else "this tree" for l in order)))
        for r in runs:
            who = "parent build" if r["library"] != "this tree" else "this tree   "
            if mode == "one":
                lines.append("   %s create_events(K = 1)  %s" % (who, stats(r["create_events_k1_ms"])))
                if r["create_event_ms"]:
                    lines.append("   %s create_event          %s" % (who, stats(r["create_event_ms"])))
            else:
                lines.append("   %s composed calls        %s   (%d events stored, src holds %d)" % (who, stats(r["composed_ms"]), r["stored"], r["src_events"]))
                if r["gossip_turn_ms"]:
                    lines.append("   %s gossip_turn           %s" % (who, stats(r["gossip_turn_ms"])))
        if mode == "one":
            last = [r for r in runs if r["library"] == "this tree"][-1]
            tot = sum(last["phase_us_median"].values())
            lines.append("   k_sign_one, stamps of lane 0 (median of %d stamped launches, tick %.1f ns): %s;  kernel %.1f us"
                         % (len(last["phase_us_laps"]), last["tick_ns"], ", ".join("%s %.1f us" % kv for kv in last["phase_us_median"].items()), tot))
            par = [np.median(r["create_events_k1_ms"]) for r in runs if r["library"] != "this tree"]
            new = [np.median(r["create_event_ms"]) for r in runs if r["library"] == "this tree"]
            if par and new:
                lines.append("   parent create_events(K = 1) / this tree create_event = %.2f" % (np.median(par) / np.median(new)))
        else:
            par = [np.median(r["composed_ms"]) for r in runs if r["library"] != "this tree"]
            new = [np.median(r["gossip_turn_ms"]) for r in runs if r["library"] == "this tree"]
            if par and new:
                lines.append("   parent composed calls / this tree gossip_turn = %.2f" % (np.median(par) / np.median(new)))
    lines.append("   not measured here: Node.main on the host route for the same turn")
    lines.append(json.dumps(record))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    sys.exit(main())
