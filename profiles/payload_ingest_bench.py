"""One shuffled sync payload addressed by event id: the device route (sw_ingest_payload_device, arrays resident on the
device) against the host route Node.sync takes without it — hgutils.toposort over the unknown ids, the `_index` dict
look-ups and parent checks of Node._parents_ok event by event, then sw_append_events.  One process, no torch.

Per size: laps alternate  reset + host route  and  reset + device route; the host route runs first and last, so a drift
of the machine shows up between its first and last laps.  The host route is what exists without this call: the baseline.
Both routes must leave the same hashgraph (creators and heights compared through the ids), or nothing is printed but
the mismatch.  Crypto is left out of both (ok = NULL): it is the same batch call in front of either.

Reported, median and [min, max] over the laps, in ms: the whole route; for the host route its split into toposort,
checks (dict look-ups, parent checks, building the index arrays) and append; for the device route the library's own
split (sw_get_payload_stats under sw_set_profiling, one extra lap: the split costs three stream synchronisations) into
resolve, waves, sort + gather, append + id commit, and the number of waves.

usage: python profiles/payload_ingest_bench.py [--laps 2] [--sizes 256x1000000,1024x2000000]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--laps", type=int, default=2)
    ap.add_argument("--sizes", default="256x1000000,1024x2000000")
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    pkg = importlib.import_module("py-swirld_amd")
    toposort = importlib.import_module("py-swirld_amd.hgutils").toposort
    hip = C.CDLL(pkg.LIB_PATH)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    for size in args.sizes.split(","):
        n, N = (int(x) for x in size.split("x"))
        cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, args.seed)
        perm = np.random.default_rng(args.seed).permutation(N)
        eid = [hashlib.blake2b(int(k).to_bytes(8, "little"), digest_size=32).digest() for k in range(N)]
        ids = np.frombuffer(b"".join(eid), np.uint8).reshape(N, 32)
        zero = np.zeros((1, 32), np.uint8)
        arrays = [ids[perm], np.where(sp[perm, None] >= 0, ids[np.maximum(sp[perm], 0)], zero), np.where(op[perm, None] >= 0, ids[np.maximum(op[perm], 0)], zero),
                  np.where(sp[perm] >= 0, 2, 0).astype(np.uint8), cr[perm], t[perm], sig[perm]]
        dev = []
        for a in arrays + [np.zeros(N, np.int32)]:
            a = np.ascontiguousarray(a)
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), a.nbytes) == 0
            assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
            dev.append(p.value)
        # the payload as Node.sync receives it: {id -> (parent ids, creator, t, sig row)} in payload order
        remote = {eid[k]: ((eid[sp[k]], eid[op[k]]) if sp[k] >= 0 else (), int(cr[k]), k) for k in perm.tolist()}
        h = pkg.Hashgraph(n)
        h.reserve(N)

        def host_lap():
            h.reset()
            h.synchronize()
            t0 = time.perf_counter()
            index, creator_of = {}, {}
            unknown = remote.keys() - index.keys()
            new = tuple(toposort(unknown, lambda u: remote[u][0]))
            t1 = time.perf_counter()
            a_cr, a_sp, a_op, src = [], [], [], []
            for e in new:
                par, c, k = remote[e]
                if par != ():      # Node._parents_ok
                    if len(par) != 2 or par[0] not in index or par[1] not in index:
                        continue
                    if creator_of[par[0]] != c or creator_of[par[1]] == c:
                        continue
                    a_sp.append(index[par[0]])
                    a_op.append(index[par[1]])
                else:
                    a_sp.append(-1)
                    a_op.append(-1)
                index[e] = len(a_cr)
                creator_of[e] = c
                a_cr.append(c)
                src.append(k)
            src = np.array(src)
            t2 = time.perf_counter()
            h.append_events(np.array(a_cr, np.int32), np.array(a_sp, np.int32), np.array(a_op, np.int32), t[src], sig[src])
            h.synchronize()
            t3 = time.perf_counter()
            dense_of = np.empty(N, np.int64)
            dense_of[src] = np.arange(len(src))
            return {"total": (t3 - t0) * 1e3, "toposort": (t1 - t0) * 1e3, "checks": (t2 - t1) * 1e3, "append": (t3 - t2) * 1e3}, dense_of

        def device_lap(profile=False):
            h.reset()
            h.set_profiling(profile)
            h.synchronize()
            t0 = time.perf_counter()
            _, stored = h.ingest_payload_device(dev[0], dev[1], dev[2], dev[3], dev[4], None, dev[5], dev[6], index_out=dev[7], count=N)
            h.synchronize()
            t1 = time.perf_counter()
            assert stored == N
            out = np.empty(N, np.int32)
            assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), dev[7], out.nbytes, 2) == 0
            dense_of = np.empty(N, np.int64)
            dense_of[perm] = out
            return {"total": (t1 - t0) * 1e3}, dense_of

        device_lap()            # warm-up: allocations
        ref_h = None
        times = {"host": [], "device": []}
        for v in ["host" if i % 2 == 0 else "device" for i in range(2 * args.laps + 1)]:   # host first and last
            tm, dense_of = host_lap() if v == "host" else device_lap()
            hts = h.heights()[dense_of]
            if ref_h is None:
                ref_h = hts
            elif not np.array_equal(hts, ref_h):
                print("MISMATCH between the routes at %s (%s lap): nothing is reported" % (size, v))
                return 1
            times[v].append(tm)
        _, dense_of = device_lap(profile=True)
        ps = h.payload_stats()
        h.set_profiling(False)
        st = h.ingest_stats()
        out = {"members": n, "events": N, "seed": args.seed, "laps": {v: len(times[v]) for v in times}, "waves": ps["waves"],
               "device_split_ms": {k: ps[k] for k in ("resolve_ms", "waves_ms", "sort_ms", "append_ms")}, "ingest_stats": st}
        print("== %d members x %d events in one shuffled payload, seed %d: %d host laps, %d device laps (alternating, host first and last); "
              "same heights by id in every lap" % (n, N, args.seed, len(times["host"]), len(times["device"])))
        for v, keys in (("host", ("total", "toposort", "checks", "append")), ("device", ("total",))):
            for key in keys:
                x = np.array([tm[key] for tm in times[v]])
                out["%s_%s_ms" % (v, key)] = {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}
                print("   %-7s %-9s median %10.3f ms   [%10.3f, %10.3f]   first lap %10.3f, last lap %10.3f"
                      % (v, key, np.median(x), x.min(), x.max(), x[0], x[-1]))
        print("   device split (one profiled lap): resolve %.3f ms, waves %.3f ms (%d waves), sort + gather %.3f ms, append + id commit %.3f ms"
              % (ps["resolve_ms"], ps["waves_ms"], ps["waves"], ps["sort_ms"], ps["append_ms"]))
        out["speedup_host_over_device"] = out["host_total_ms"]["median"] / out["device_total_ms"]["median"]
        print(json.dumps(out))
        h.close()
        for p in dev:
            hip.hipFree(C.c_void_p(p))
    return 0


if __name__ == "__main__":
    sys.exit(main())
