"""Building the signed bytes of a sync payload: the host route Node._batch_validate took before the device encoder — two
pickle.dumps per event, Hashgraph._pack of both lists, upload of both streams — against sw_pack_events_device
(csrc/pack.hip.h), which builds the same two streams in device memory from the payload arrays.  One process, no torch.

Workload: 256 members, K events with data None, about 1 / 256 of them roots, random ids, keys and signatures (the encoder
does not look at what they mean).  At most --distinct events are held as Python objects; a larger K walks over them again
(every dumps call is still made).  Routes:
   (a) host     two pickle.dumps per event + _pack + upload of both streams and their offsets
   (b) device   upload of the payload arrays + pack_events_device
   (c) resident pack_events_device on arrays that are in device memory already (how sw_sync_pull_validated meets it)
Before anything is timed the device streams are compared with the host route's, byte for byte.  Laps alternate (a) and
(b) + (c); (a) runs first and last, so a drift of the machine shows up between its first and last laps.  Reported: min /
median / max over the laps in ms; for (c) also the bytes written per second at the median.

Afterwards: pull_from against pull_from(validate=True) between two contexts, on a hashgraph whose events are really
signed (libsodium) and really named (BLAKE2b of the pickle): a fresh pair of receivers per lap.

usage: python profiles/pack_events_bench.py [--laps 3] [--sizes 65536,1048576] [--members 256] [--distinct 65536]
                                            [--pull-events 20000] [--pull-behind 8000] [--out profiles/pack_events_bench.txt]"""
import argparse
import collections
import ctypes as C
import hashlib
import importlib
import os
import pickle
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

Event = collections.namedtuple("Event", "d p t c s")    # pickled as __main__.Event: the context is told so


def stats(x):
    x = np.array(x)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "first": float(x[0]), "last": float(x[-1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--laps", type=int, default=3)
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=65536)
    ap.add_argument("--pull-events", type=int, default=20000)
    ap.add_argument("--pull-behind", type=int, default=8000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = importlib.import_module("py-swirld_amd")
    hip = C.CDLL(pkg.LIB_PATH)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def dmalloc(nbytes):
        q = C.c_void_p()
        assert hip.hipMalloc(C.byref(q), max(int(nbytes), 16)) == 0
        return q.value

    def up(dst, a):
        assert hip.hipMemcpy(dst, p(a), a.nbytes, 1) == 0

    def down(src, nbytes):
        out = np.empty(nbytes, np.uint8)
        assert hip.hipMemcpy(p(out), src, nbytes, 2) == 0
        return out

    def line(name, s, extra=""):
        say("   %-42s min %10.3f  median %10.3f  max %10.3f ms   (first lap %10.3f, last %10.3f)%s"
            % (name, s["min"], s["median"], s["max"], s["first"], s["last"], extra))

    n = args.members
    mod, qual = Event.__module__, Event.__qualname__
    rng = np.random.default_rng(6)
    keys = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    h = pkg.Hashgraph(n)
    h.set_member_keys(keys)     # (random bytes: most are no curve points; the encoder only copies them)
    h.set_event_class(mod, qual)
    for K in [int(x) for x in args.sizes.split(",")]:
        D = min(K, args.distinct)
        reps = (K + D - 1) // D
        tile = lambda a: np.ascontiguousarray(np.concatenate([a] * reps)[:K])
        sp, op = rng.integers(0, 256, (D, 32), dtype=np.uint8), rng.integers(0, 256, (D, 32), dtype=np.uint8)
        sig = rng.integers(0, 256, (D, 64), dtype=np.uint8)
        arity = np.where(rng.random(D) < 1 / 256, 0, 2).astype(np.uint8)
        creator = rng.integers(0, n, D).astype(np.int32)
        t = 1.7e9 + rng.random(D) * 1e6
        key_b = [bytes(k) for k in keys]
        evs = [Event(None, () if arity[i] == 0 else (sp[i].tobytes(), op[i].tobytes()), float(t[i]), key_b[creator[i]], sig[i].tobytes()) for i in range(D)]
        arrays = [tile(a) for a in (sp, op, arity, creator, t, sig)]
        d_in = [dmalloc(a.nbytes) for a in arrays]
        bm, bw = h.pack_bound(K)
        d_m, d_w, d_mo, d_wo = dmalloc(bm), dmalloc(bw), dmalloc(8 * (K + 1)), dmalloc(8 * (K + 1))
        h_m, h_w, h_mo, h_wo = dmalloc(bm), dmalloc(bw), dmalloc(8 * (K + 1)), dmalloc(8 * (K + 1))
        totals = {}

        def host_route():
            t0 = time.perf_counter()
            msgs, whole = [], []
            for r in range(reps):
                for ev in (evs if (r + 1) * D <= K else evs[:K - r * D]):
                    msgs.append(pickle.dumps(ev[:-1], protocol=4))
                    whole.append(pickle.dumps(ev, protocol=4))
            t1 = time.perf_counter()
            data, off = h._pack(msgs)
            wdata, woff = h._pack(whole)
            t2 = time.perf_counter()
            for dst, a in ((h_m, data), (h_mo, off), (h_w, wdata), (h_wo, woff)):
                up(dst, a)
            t3 = time.perf_counter()
            totals["host"] = (int(off[-1]), int(woff[-1]))
            return {"total": (t3 - t0) * 1e3, "dumps": (t1 - t0) * 1e3, "_pack": (t2 - t1) * 1e3, "upload": (t3 - t2) * 1e3}

        def device_route(resident):
            t0 = time.perf_counter()
            if not resident:
                for dst, a in zip(d_in, arrays):
                    up(dst, a)
            t1 = time.perf_counter()
            h.pack_events_device(d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], d_in[5], d_m, d_mo, bm, d_w, d_wo, bw, count=K)
            h.synchronize()
            t2 = time.perf_counter()
            return {"total": (t2 - t0) * 1e3, "upload": (t1 - t0) * 1e3, "pack": (t2 - t1) * 1e3}

        # both routes write the same bytes, or nothing is reported
        host_route()
        device_route(False)
        tm, tw = totals["host"]
        same = (np.array_equal(down(d_mo, 8 * (K + 1)), down(h_mo, 8 * (K + 1))) and np.array_equal(down(d_wo, 8 * (K + 1)), down(h_wo, 8 * (K + 1)))
                and np.array_equal(down(d_m, tm), down(h_m, tm)) and np.array_equal(down(d_w, tw), down(h_w, tw)))
        if not same:
            say("MISMATCH at K = %d: the device streams are not the host route's; nothing is reported" % K)
            return 1
        times = {"host": [], "device": [], "resident": []}
        for i in range(2 * args.laps + 1):
            if i % 2 == 0:
                times["host"].append(host_route())
            else:
                times["device"].append(device_route(False))
                times["resident"].append(device_route(True))
        say("== %d members, K = %d events (%d distinct, %d roots), %d + %d bytes; %d host laps, %d device laps (alternating, host first and last); "
            "the streams are equal byte for byte" % (n, K, D, int((arrays[2] == 0).sum()), tm, tw, len(times["host"]), len(times["device"])))
        res = {}
        for v, label, parts in (("host", "(a) 2 dumps per event + _pack + upload", ("total", "dumps", "_pack", "upload")),
                                ("device", "(b) upload of the arrays + pack_events_device", ("total", "upload", "pack")),
                                ("resident", "(c) pack_events_device, resident arrays", ("total",))):
            for key in parts:
                res[v, key] = s = stats([x[key] for x in times[v]])
                extra = "   %8.1f GB/s written" % ((tm + tw) / s["median"] / 1e6) if v == "resident" else ""
                line(label if key == "total" else "   ... " + key, s, extra)
        say("   (a) / (b) = %.1f, (a) / (c) = %.1f at the medians" % (res["host", "total"]["median"] / res["device", "total"]["median"],
                                                                     res["host", "total"]["median"] / res["resident", "total"]["median"]))
        h.set_profiling(True)
        device_route(True)
        st = h.pack_stats()
        h.set_profiling(False)
        say("   one call under set_profiling (host clock, a synchronisation after each phase): lengths + scan %.3f ms, the two writers %.3f ms"
            % (st["scan_ms"], st["write_ms"]))
        for q in d_in + [d_m, d_w, d_mo, d_wo, h_m, h_w, h_mo, h_wo]:
            hip.hipFree(C.c_void_p(q))
    h.close()

    # ---- pull_from against pull_from(validate=True)
    crypto = pkg.node.crypto
    N, behind = args.pull_events, args.pull_behind
    t0 = time.perf_counter()
    cr, sp, op, t, _ = pkg.synth_hashgraph(n, N, 9)
    kps = [crypto.sign_seed_keypair(hashlib.blake2b(b"member %d" % m, digest_size=32).digest()) for m in range(n)]
    ids, sigs = [], []
    for e in range(N):
        body = (None, () if sp[e] < 0 else (ids[sp[e]], ids[op[e]]), float(t[e]), kps[cr[e]][0])
        s = crypto.sign_detached(pickle.dumps(body, protocol=4), kps[cr[e]][1])
        sigs.append(s)
        ids.append(crypto.generichash(pickle.dumps(Event(*body, s), protocol=4)))
    ids_a = np.frombuffer(b"".join(ids), np.uint8).reshape(N, 32)
    sig_a = np.frombuffer(b"".join(sigs), np.uint8).reshape(N, 64)
    say("== pull: %d members, %d signed events (built in %.1f s), the receiver %d events behind" % (n, N, time.perf_counter() - t0, behind))

    def ctx(count):
        c = pkg.Hashgraph(n)
        c.append_events(cr[:count], sp[:count], op[:count], t[:count], sig_a[:count])
        c.set_event_ids(0, ids_a[:count])
        c.divide_rounds(0, count)
        c.set_member_keys([pk for pk, _ in kps])
        c.set_event_class(mod, qual)
        c.synchronize()
        return c

    src = ctx(N)
    a = N - behind
    times = {"plain": [], "validated": []}
    counts = None
    for i in range(2 * args.laps + 1):
        dst = ctx(a)
        t0 = time.perf_counter()
        if i % 2 == 0:
            r = dst.pull_from(src, N - 1, a - 1)
            times["plain"].append((time.perf_counter() - t0) * 1e3)
        else:
            r = dst.pull_from(src, N - 1, a - 1, validate=True)
            times["validated"].append((time.perf_counter() - t0) * 1e3)
            if r[1] != r[0]:
                say("MISMATCH: %d of %d events judged valid" % (r[1], r[0]))
                return 1
            counts = r
        dst.close()
    say("   %d events sent, %d valid, %d stored" % counts)
    line("pull_from", stats(times["plain"]))
    line("pull_from(validate=True)", stats(times["validated"]))
    src.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
