#!/usr/bin/env python3
"""A/B of knob configurations on a hashgraph with ONE member that falls silent mid-call (crash-fault shape), in one process:
python profiles/silent_member_ab.py [members events member frac passes] -- CFG [CFG ...]   (CFG as in knob_sweep.py).
Every event of `member` from index frac * events on is left out; other-parents that pointed at one of them point at the
member's last event before the cut.  Prints min / median ms per pass (sw_rewind + sw_divide_rounds + sw_decide_fame)."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("py-swirld_amd")


def silence(stream, member, at):
    cr, sp, op, t, sig = [np.asarray(x) for x in stream]
    idx = np.arange(len(cr))
    keep = ~((cr == member) & (idx >= at))
    last = int(idx[(cr == member) & (idx < at)].max())
    new = np.cumsum(keep) - 1
    op2 = np.where((op >= 0) & ~keep[np.maximum(op, 0)], last, op)
    sp2 = np.where(sp >= 0, new[np.maximum(sp, 0)], -1)
    op2 = np.where(op2 >= 0, new[np.maximum(op2, 0)], -1)
    return (cr[keep].astype(cr.dtype), sp2[keep].astype(sp.dtype), op2[keep].astype(op.dtype), t[keep], sig[keep])


args = sys.argv[1:]
split = args.index("--") if "--" in args else len(args)
head, cfgs = args[:split], args[split + 1:] or ["-"]
n = int(head[0]) if len(head) > 0 else 256
N0 = int(head[1]) if len(head) > 1 else 1_000_000
member = int(head[2]) if len(head) > 2 else 17
frac = float(head[3]) if len(head) > 3 else 0.5
passes = int(head[4]) if len(head) > 4 else 9
stream = silence(pkg.synth_hashgraph(n, N0, 3), member, int(N0 * frac))
N = len(stream[0])
base_env = dict(os.environ)
for cfg in cfgs:
    os.environ.clear()
    os.environ.update(base_env)
    if cfg != "-":
        for kv in cfg.split(","):
            k, v = kv.split("=")
            os.environ[k] = v
    h = pkg.Hashgraph(n)
    h.reserve(N)
    h.append_events(*stream)
    h.divide_rounds(0, N)
    h.decide_fame()
    ts = []
    for _ in range(passes):
        t0 = time.perf_counter()
        h.rewind()
        h.divide_rounds(0, N)
        h.decide_fame()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    c = h.counters()
    per = passes + 1
    print("n=%d N=%d (member %d silent from %.0f %%) %-20s min %.3f ms  med %.3f ms  %.1f M ev/s | %d iterations (%d waiting), %d rounds" % (
        n, N, member, 100 * frac, cfg, ts[0] * 1e3, ts[len(ts) // 2] * 1e3, N / ts[0] / 1e6, c["round_iterations"] // per,
        c["gated_idle_iterations"] // per, c["rounds"]), flush=True)
    h.close()
