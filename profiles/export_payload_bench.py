"""Answering a sync: the device route (sw_export_payload_device: ranges, offsets and gather on the device, the arrays left
where sw_ingest_payload_device reads them) against the host route a caller has without it — sw_sync_diff, then
sw_get_chain_events member by member, numpy gathers of ids / parents' ids / creators / timestamps / signatures out of the
caller's host arrays, and the upload of the seven arrays.  One process, no torch.

Per shape and asker (one that knows nobody; one 10 000 events behind the head): laps alternate host route and device
route; the host route runs first and last, so a drift of the machine shows up between its first and last laps.  Both
routes must leave the same bytes in the seven device arrays, or nothing is printed but the mismatch.  Then, for the
asker that is behind: sw_sync_pull into a context holding the prefix, against host route + sw_ingest_payload_device into
the same context (the receiver is rebuilt, untimed, before every lap; both must store the same events).  Last, the lane
width of the gather (SW_EXPORT_LANES = 4, 8, 16 lanes of a wave per event, a fresh context each) on the larger export.

Reported, median and [min, max] over the laps, in ms; for the host route also its split into diff (sw_sync_diff), chains
(sw_get_chain_events), gather (numpy) and upload; for the device route the library's own split (sw_get_export_stats
under sw_set_profiling, one extra lap).

usage: python profiles/export_payload_bench.py [--laps 2] [--sizes 256x1000000,1024x2000000] [--behind 10000]"""
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

WIDTH = (32, 32, 32, 1, 4, 8, 64)     # ids, sp_ids, op_ids, arity, creator, t, sig


def stats(x):
    x = np.array(x)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "first": float(x[0]), "last": float(x[-1])}


def line(name, s):
    print("   %-22s median %10.3f ms   [%10.3f, %10.3f]   first lap %10.3f, last lap %10.3f" % (name, s["median"], s["min"], s["max"], s["first"], s["last"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--laps", type=int, default=2)
    ap.add_argument("--sizes", default="256x1000000,1024x2000000")
    ap.add_argument("--behind", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    pkg = importlib.import_module("py-swirld_amd")
    hip = C.CDLL(pkg.LIB_PATH)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]

    def dmalloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(nbytes, 16)) == 0
        return p.value

    for size in args.sizes.split(","):
        n, N = (int(x) for x in size.split("x"))
        cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, args.seed)
        ids = np.frombuffer(b"".join(hashlib.blake2b(int(k).to_bytes(8, "little"), digest_size=32).digest() for k in range(N)), np.uint8).reshape(N, 32)
        zero = np.zeros((1, 32), np.uint8)
        nobody = np.full(n, -1, np.int32)      # (sw_sync_diff takes no NULL: the asker that knows nobody, spelled out)

        def answerer():
            a_ = pkg.Hashgraph(n)
            a_.append_events(cr, sp, op, t, sig)
            a_.set_event_ids(0, ids)
            a_.divide_rounds(0, N)
            a_.synchronize()
            return a_
        A = answerer()
        head = N - 1
        dev = [[dmalloc(N * w) for w in WIDTH] for _ in range(2)]     # [0] host route, [1] device route
        d_known = dmalloc(4 * n)
        d_index = dmalloc(4 * N)

        def host_route(known, out):
            """-> (K, split in ms); the seven arrays are in `out` and the device is idle on return."""
            t0 = time.perf_counter()
            first, end, K = A.sync_diff(head, nobody if known is None else known)
            t1 = time.perf_counter()
            ev = np.concatenate([A.chain_events(m, int(first[m]), int(end[m])) for m in range(n)])
            t2 = time.perf_counter()
            s_, o_ = sp[ev], op[ev]
            arrays = (ids[ev], np.where((s_ >= 0)[:, None], ids[np.maximum(s_, 0)], zero), np.where((o_ >= 0)[:, None], ids[np.maximum(o_, 0)], zero),
                      np.where(s_ >= 0, 2, 0).astype(np.uint8), cr[ev], t[ev], sig[ev])
            t3 = time.perf_counter()
            for p, a in zip(out, arrays):
                a = np.ascontiguousarray(a)
                assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
            t4 = time.perf_counter()
            return K, {"total": (t4 - t0) * 1e3, "diff": (t1 - t0) * 1e3, "chains": (t2 - t1) * 1e3, "gather": (t3 - t2) * 1e3, "upload": (t4 - t3) * 1e3}

        def device_route(known, out):
            t0 = time.perf_counter()
            if known is not None:      # (the asker's heights arrive in host memory here; on the device they cost nothing)
                assert hip.hipMemcpy(d_known, known.ctypes.data_as(C.c_void_p), 4 * n, 1) == 0
            K = A.export_payload_device(head, d_known if known is not None else None, N, *out)
            A.synchronize()
            return K, {"total": (time.perf_counter() - t0) * 1e3}

        def same_bytes(K):
            for (a, b), w in zip(zip(dev[0], dev[1]), WIDTH):
                x, y = np.empty(K * w, np.uint8), np.empty(K * w, np.uint8)
                assert hip.hipMemcpy(x.ctypes.data_as(C.c_void_p), a, K * w, 2) == 0 and hip.hipMemcpy(y.ctypes.data_as(C.c_void_p), b, K * w, 2) == 0
                if not np.array_equal(x, y):
                    return False
            return True

        askers = (("knows nobody", None), ("%d events behind" % args.behind, A.known_heights(head - args.behind)))
        result = {"members": n, "events": N, "seed": args.seed, "laps": args.laps}
        for name, known in askers:
            device_route(known, dev[1])         # warm-up: scratch allocations
            times = {"host": [], "device": []}
            Ks = set()
            for v in ["host" if i % 2 == 0 else "device" for i in range(2 * args.laps + 1)]:   # host first and last
                K, tm = host_route(known, dev[0]) if v == "host" else device_route(known, dev[1])
                Ks.add(K)
                times[v].append(tm)
            if len(Ks) != 1 or not same_bytes(K):
                print("MISMATCH between the routes at %s, asker %s: nothing is reported" % (size, name))
                return 1
            A.set_profiling(True)
            device_route(known, dev[1])
            st = A.export_stats()
            A.set_profiling(False)
            print("== %d members x %d events, asker %s: %d events exported; %d host laps, %d device laps (alternating, host first and last); "
                  "same bytes in all seven arrays" % (n, N, name, K, len(times["host"]), len(times["device"])))
            r = {"exported": K}
            for v, keys in (("host", ("total", "diff", "chains", "gather", "upload")), ("device", ("total",))):
                for key in keys:
                    r["%s_%s_ms" % (v, key)] = s = stats([tm[key] for tm in times[v]])
                    line("%s %s" % (v, key), s)
            r["device_split_ms"] = {"ranges": st["ranges_ms"], "gather": st["gather_ms"]}
            r["speedup_host_over_device"] = r["host_total_ms"]["median"] / r["device_total_ms"]["median"]
            print("   device split (one profiled lap): ranges + count %.3f ms, gather %.3f ms;  host / device = %.1f"
                  % (st["ranges_ms"], st["gather_ms"], r["speedup_host_over_device"]))
            result[name] = r

        # ---- the whole exchange into a receiver that is `behind` events behind
        a = N - args.behind
        B = pkg.Hashgraph(n)
        B.reserve(N)
        known = askers[1][1]

        def rebuild():
            B.reset()
            B.append_events(cr[:a], sp[:a], op[:a], t[:a], sig[:a])
            B.set_event_ids(0, ids[:a])
            B.divide_rounds(0, a)
            B.synchronize()

        def pull_lap():
            rebuild()
            t0 = time.perf_counter()
            n_sent, n_stored = B.pull_from(A, head, a - 1)
            B.synchronize()
            return (n_sent, n_stored), (time.perf_counter() - t0) * 1e3

        def host_ingest_lap():
            rebuild()
            t0 = time.perf_counter()
            kn = B.known_heights(a - 1)
            K, _ = host_route(kn, dev[0])
            _, n_stored = B.ingest_payload_device(*dev[0][:5], None, dev[0][5], dev[0][6], index_out=d_index, count=K)
            B.synchronize()
            return (K, n_stored), (time.perf_counter() - t0) * 1e3

        pull_lap()
        times = {"host": [], "pull": []}
        seen = set()
        for v in ["host" if i % 2 == 0 else "pull" for i in range(2 * args.laps + 1)]:
            what, ms = host_ingest_lap() if v == "host" else pull_lap()
            seen.add(what + (B.num_events, B.heights(a, B.num_events - a).tobytes(), B.event_ids(a).tobytes()))
            times[v].append(ms)
        if len(seen) != 1:
            print("MISMATCH between pull_from and host route + ingest at %s: nothing is reported" % size)
            return 1
        print("== %d members x %d events, receiver %d events behind: %d sent, %d stored; same events, heights and ids either way" % ((n, N, args.behind) + what))
        r = {"sent": what[0], "stored": what[1]}
        for v, label in (("host", "host route + ingest"), ("pull", "pull_from")):
            r[v + "_ms"] = s = stats(times[v])
            line(label, s)
        r["speedup_host_over_pull"] = r["host_ms"]["median"] / r["pull_ms"]["median"]
        result["exchange"] = r
        B.close()

        # ---- lanes of a wave per event in the gather, on the larger export (the knob is read at sw_create: a context per width)
        A.close()
        widths = {}
        for lanes in (16, 8, 4):
            os.environ["SW_EXPORT_LANES"] = str(lanes)
            A = answerer()
            device_route(None, dev[1])
            A.set_profiling(True)
            ms = []
            for _ in range(10):
                device_route(None, dev[1])
                ms.append(A.export_stats()["gather_ms"])
            A.set_profiling(False)
            A.close()
            widths[lanes] = ms
        os.environ.pop("SW_EXPORT_LANES")
        result["gather_ms_by_lanes"] = {str(k): stats(v) for k, v in widths.items()}
        print("== gather alone (launch to completion, host clock), asker knows nobody, by lanes per event, 10 calls each:")
        for k, v in widths.items():
            line("%d lanes" % k, stats(v))
        print(json.dumps(result))
        for p in dev[0] + dev[1] + [d_known, d_index]:
            hip.hipFree(C.c_void_p(p))
    return 0


if __name__ == "__main__":
    sys.exit(main())
