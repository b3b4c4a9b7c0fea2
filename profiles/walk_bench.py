"""Answering a sync by the pruned walk: the device route (Hashgraph.sync_walk: k_walk_bfs + k_walk_list, the list read back;
Hashgraph.export_walk_device: walk, list and gather, the arrays left in device memory) against the host route Node.ask_sync
takes without it — the height-pruned BFS over Python dicts keyed by event id (hgutils.bfs, the trunk rule included) and the
reply dict built from it.  One process, no torch.

Per shape, on a uniform history and on the same history with a handful of forks at its end (five members equivocate once
each; the context is then on the exact path), two askers: one whose head is `--behind` events back (a typical sync), one
that knows nobody (the whole history).  Laps alternate host route and device routes; the host route runs first and last,
so a drift of the machine shows up between its first and last laps.  The device list must name exactly the host route's
events, or nothing is printed but the mismatch.

Reported, median and [min, max] over the laps, in ms: the host route (BFS + dict), sync_walk, export_walk_device; and from
one profiled lap (sw_get_walk_stats under sw_set_profiling) the levels of the walk, the host time of walk + count, list
and gather, and the walk's microseconds per level.

usage: python profiles/walk_bench.py [--laps 3] [--sizes 256x65536,256x1000000] [--behind 4000]"""
import argparse
import ctypes as C
import hashlib
import importlib
import json
import os
import sys
import time
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTH = (32, 32, 32, 1, 4, 8, 64, 4)     # ids, sp_ids, op_ids, arity, creator, t, sig, event
Event = namedtuple("Event", "d p t c s")


def stats(x):
    x = np.array(x)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "first": float(x[0]), "last": float(x[-1])}


def line(name, s):
    print("   %-22s median %10.3f ms   [%10.3f, %10.3f]   first lap %10.3f, last lap %10.3f" % (name, s["median"], s["min"], s["max"], s["first"], s["last"]))


def with_forks(stream, n, k, seed):
    """The stream with k forks at its end: k members sign a sibling of their newest event (same self-parent, another
    other-parent), and a further member builds on each sibling.  Returns (stream, events before the first fork)."""
    cr, sp, op, t = (a.tolist() for a in stream[:4])
    sig = stream[4]
    rng = np.random.default_rng(seed)
    N0 = len(cr)
    newest = {}
    for e in range(N0 - 1, -1, -1):
        newest.setdefault(cr[e], e)
        if len(newest) == n:
            break
    for m in rng.choice(n, k, replace=False).tolist():
        e = newest[m]
        if sp[e] < 0:
            continue
        other = [x for x in newest if x not in (m, cr[op[e]])]
        o2, third = (int(x) for x in rng.choice(other, 2, replace=False))
        cr.append(m); sp.append(sp[e]); op.append(newest[o2]); t.append(t[-1] + 1)
        f = len(cr) - 1
        cr.append(third); sp.append(newest[third]); op.append(f); t.append(t[-1] + 1)
        newest[third] = len(cr) - 1
    extra = rng.integers(0, 256, (len(cr) - N0, 64), dtype=np.uint8)
    return (np.array(cr, np.int32), np.array(sp, np.int32), np.array(op, np.int32), np.array(t, np.float64), np.concatenate([sig, extra])), N0


class HostView:
    """What a Node holds on the host for ask_sync: hg, height, the trunk heights (node.py, _add_event_host)."""

    def __init__(self, n, stream, ids):
        cr, sp, op, t, sig = stream
        self.ids = [bytes(i) for i in ids]
        crl, spl, opl = cr.tolist(), sp.tolist(), op.tolist()
        self.hg, self.height, self.trunk = {}, {}, {}
        chain_head = {}
        for e, h in enumerate(self.ids):
            p = () if spl[e] < 0 else (self.ids[spl[e]], self.ids[opl[e]])
            self.hg[h] = Event(None, p, float(t[e]), crl[e], b"")
            self.height[h] = 1 + max(self.height[q] for q in p) if p else 0
            c = crl[e]
            if c in chain_head and chain_head[c] != (p[0] if p else None):
                th = self.height[p[0]] if p else -1
                self.trunk[c] = min(self.trunk.get(c, th), th)
            chain_head[c] = h

    def ask_sync(self, bfs, head, asker_heights):
        """node.py, Node.ask_sync without the signing and pickling: the BFS and the dict."""
        hg, height, trunk = self.hg, self.height, self.trunk

        def missing_parents(u):
            for p in hg[u].p:
                creator = hg[p].c
                known = asker_heights.get(creator)
                if known is not None and creator in trunk:
                    known = min(known, trunk[creator])
                if known is None or height[p] > known:
                    yield p

        subset = {}
        for eid in bfs((self.ids[head],), missing_parents):
            subset[eid] = hg[eid]
        return subset


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--laps", type=int, default=3)
    ap.add_argument("--sizes", default="256x65536,256x1000000")
    ap.add_argument("--behind", type=int, default=4000)
    ap.add_argument("--forks", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    pkg = importlib.import_module("py-swirld_amd")
    bfs = importlib.import_module("py-swirld_amd.hgutils").bfs
    hip = C.CDLL(pkg.LIB_PATH)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def dmalloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(nbytes, 16)) == 0
        return p.value

    results = []
    for size in args.sizes.split(","):
        n, N = (int(x) for x in size.split("x"))
        base = pkg.synth_hashgraph(n, N, args.seed)
        for forked in (False, True):
            stream, N0 = with_forks(base, n, args.forks, args.seed) if forked else (base, N)
            NN = len(stream[0])
            ids = np.frombuffer(b"".join(hashlib.blake2b(int(k).to_bytes(8, "little"), digest_size=32).digest() for k in range(NN)), np.uint8).reshape(NN, 32)
            A = pkg.Hashgraph(n)
            A.append_events(*(a[:N0] for a in stream))
            A.divide_rounds(0, N0)                 # (the fork-free part on the fast path: the forks arrive afterwards, as they would)
            if forked:
                A.append_events(*(a[N0:] for a in stream))
                A.divide_rounds(N0, NN - N0)
            A.set_event_ids(0, ids)
            A.synchronize()
            assert bool(A.exact) == forked
            view = HostView(n, stream, ids)
            head = NN - 1
            out = [dmalloc(NN * w) for w in WIDTH]
            d_known, d_cap = dmalloc(4 * n), dmalloc(4 * n)
            trunk = A.fork_trunks()
            assert {c: int(v) for c, v in enumerate(trunk) if v != 2**31 - 1} == view.trunk
            cap = trunk if forked else None
            if forked:
                assert hip.hipMemcpy(d_cap, trunk.ctypes.data_as(C.c_void_p), 4 * n, 1) == 0
            behind = A.known_heights(N0 - 1 - args.behind)
            for name, known in (("%d events behind" % args.behind, behind), ("knows nobody", None)):
                heights = {} if known is None else {c: int(v) for c, v in enumerate(known) if v >= 0}

                def host_route():
                    t0 = time.perf_counter()
                    subset = view.ask_sync(bfs, head, heights)
                    return subset, (time.perf_counter() - t0) * 1e3

                def walk_route():
                    t0 = time.perf_counter()
                    ev = A.sync_walk(head, known, cap)
                    return ev, (time.perf_counter() - t0) * 1e3

                def export_route():
                    t0 = time.perf_counter()
                    if known is not None:      # (the asker's heights arrive in host memory here)
                        assert hip.hipMemcpy(d_known, known.ctypes.data_as(C.c_void_p), 4 * n, 1) == 0
                    K = A.export_walk_device(head, d_known if known is not None else None, d_cap if forked else None, NN, *out)
                    A.synchronize()
                    return K, (time.perf_counter() - t0) * 1e3

                walk_route(); export_route()          # warm-up: scratch allocations, code objects
                times = {"host": [], "walk": [], "export": []}
                order = ["host"] + ["walk", "export", "host"] * args.laps      # host first and last
                subset = ev = K = None
                for v in order:
                    if v == "host":
                        subset, ms = host_route()
                    elif v == "walk":
                        ev, ms = walk_route()
                    else:
                        K, ms = export_route()
                    times[v].append(ms)
                if K != len(ev) or set(subset) != set(view.ids[e] for e in ev.tolist()):
                    print("MISMATCH between the routes at %s, forked %s, asker %s: nothing is reported" % (size, forked, name))
                    return 1
                A.set_profiling(True)
                export_route()
                st = A.walk_stats()
                A.set_profiling(False)
                print("== %d members x %d events%s, asker %s: %d events; %d host laps, %d laps of each device route (alternating, host first and last); same events"
                      % (n, NN, " (%d forks, exact path)" % len(view.trunk) if forked else "", name, K, len(times["host"]), len(times["walk"])))
                r = {"members": n, "events": NN, "forked": forked, "asker": name, "answer_events": K, "levels": st["levels"]}
                for v, label in (("host", "host BFS + dict"), ("walk", "sync_walk"), ("export", "export_walk_device")):
                    r[v + "_ms"] = s = stats(times[v])
                    line(label, s)
                us_level = 1e3 * st["walk_ms"] / max(st["levels"], 1)
                r["profiled_ms"] = {"walk": st["walk_ms"], "list": st["list_ms"], "gather": st["gather_ms"]}
                r["walk_us_per_level"] = us_level
                r["host_over_walk"] = r["host_ms"]["median"] / r["walk_ms"]["median"]
                r["host_over_export"] = r["host_ms"]["median"] / r["export_ms"]["median"]
                print("   one profiled lap: %d levels, walk + count %.3f ms (%.2f us per level), list %.3f ms, gather %.3f ms;  host / sync_walk = %.2f, host / export = %.2f"
                      % (st["levels"], st["walk_ms"], us_level, st["list_ms"], st["gather_ms"], r["host_over_walk"], r["host_over_export"]))
                results.append(r)
            A.close()
            for p in out + [d_known, d_cap]:
                hip.hipFree(C.c_void_p(p))
    print(json.dumps(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
