"""Validating a sync payload: the member-table route (sw_validate_payload_device: one kernel against the fixed-base tables
of the members' keys, verdicts left on the device) against the route a caller has without it — sw_crypto_verify_batch with
one key per event, sw_crypto_hash_batch, the comparison of the digests with the ids on the host, and the upload of `ok`
that sw_ingest_payload then makes.  One process, no torch.

Workload: 256 members, K events signed by libsodium over messages of about 200 bytes, 1 % of them corrupted (signature,
message or id in turn).  At most --distinct events are signed; a larger K repeats them (every event still carries a real
signature, and no route caches anything per event).  Both routes start from the same packed host arrays and end with `ok`
in device memory; the new route is also timed from arrays that are resident already, which is how the sync exchange on the
device meets it.  Both must give exactly the expected verdicts, or nothing is printed but the mismatch.

Laps alternate old route and new route; the old route runs first and last, so a drift of the machine shows up between its
first and last laps.  Reported: min / median / max over the laps in ms, and signatures per second at the median.

Kernel times come from a run of their own under `rocprofv3 --kernel-trace --stats` (no counters, no other tracing):
k_validate_payload against k_verify_batch + k_blake2b_batch, which this pull request leaves byte for byte as they were.

usage: python profiles/validate_payload_bench.py [--laps 7] [--sizes 8192,65536,1048576] [--members 256] [--distinct 65536]"""
import argparse
import ctypes as C
import hashlib
import importlib
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load_sodium():
    for cand in (os.environ.get("SWIRLD_LIBSODIUM"), "/opt/conda/lib/libsodium.so", "libsodium.so.23", "libsodium.so"):
        if not cand:
            continue
        try:
            s = C.CDLL(cand)
            if s.sodium_init() >= 0:
                return s
        except OSError:
            pass
    raise SystemExit("libsodium not found: the workload is made of its signatures")


def stats(x):
    x = np.array(x)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "first": float(x[0]), "last": float(x[-1])}


def line(name, s, K):
    print("   %-34s min %10.3f  median %10.3f  max %10.3f ms   (first lap %10.3f, last %10.3f)   %8.2f M events/s"
          % (name, s["min"], s["median"], s["max"], s["first"], s["last"], K / s["median"] / 1e3))


def workload(sod, n, distinct, seed):
    rng = random.Random(seed)
    keys, sks = [], []
    for _ in range(n):
        pk, sk = C.create_string_buffer(32), C.create_string_buffer(64)
        sod.crypto_sign_seed_keypair(pk, sk, bytes(rng.getrandbits(8) for _ in range(32)))
        keys.append(pk.raw)
        sks.append(sk)
    msgs, whole, sigs, ids, creator, exp = [], [], [], [], [], []
    sig = C.create_string_buffer(64)
    for i in range(distinct):
        c = rng.randrange(n)
        ln = rng.randrange(180, 221)
        m = rng.getrandbits(8 * ln).to_bytes(ln, "little")
        sod.crypto_sign_detached(sig, None, m, C.c_ulonglong(len(m)), sks[c])
        s, w = sig.raw, m + sig.raw
        d = hashlib.blake2b(w, digest_size=32).digest()
        good = i % 100 != 50
        if not good:   # 1 %: a bit of the signature, of the message, of the id
            k = (i // 100) % 3
            if k == 0:
                s = s[:5] + bytes([s[5] ^ 2]) + s[6:]
            elif k == 1:
                m = m[:9] + bytes([m[9] ^ 1]) + m[10:]
            else:
                d = d[:20] + bytes([d[20] ^ 4]) + d[21:]
        for lst, v in ((msgs, m), (whole, w), (sigs, s), (ids, d), (creator, c), (exp, good)):
            lst.append(v)
    return keys, msgs, whole, sigs, ids, creator, exp


def pack(items, reps):
    data = np.frombuffer(b"".join(items), np.uint8)
    lens = np.tile(np.array([len(m) for m in items], np.int64), reps)
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return np.tile(data, reps), off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--laps", type=int, default=7)
    ap.add_argument("--sizes", default="8192,65536,1048576")
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=4)
    args = ap.parse_args()
    pkg = importlib.import_module("py-swirld_amd")
    L = pkg._lib.load()
    hip = C.CDLL(pkg.LIB_PATH)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def dmalloc(nbytes):
        q = C.c_void_p()
        assert hip.hipMalloc(C.byref(q), max(int(nbytes), 16)) == 0
        return q.value

    def up(dst, a):
        assert hip.hipMemcpy(dst, p(a), a.nbytes, 1) == 0

    sod = load_sodium()
    n = args.members
    sizes = [int(x) for x in args.sizes.split(",")]
    t0 = time.perf_counter()
    keys, msgs, whole, sigs, ids, creator, exp = workload(sod, n, min(args.distinct, max(sizes)), args.seed)
    print("workload: %d members, %d distinct signed events in %.1f s" % (n, len(msgs), time.perf_counter() - t0))
    key_arr = np.frombuffer(b"".join(keys), np.uint8).reshape(n, 32)
    h = pkg.Hashgraph(n)
    h.set_profiling(True)
    assert h.set_member_keys(key_arr) == 0
    h.set_profiling(False)
    print("table build (sw_set_member_keys, host clock): %.3f ms for %d members, %.1f MB" % (h.validate_stats()["table_ms"], n, (n + 1) * 512 * 96 / 1e6))
    result = {"members": n, "laps": args.laps, "table_ms": h.validate_stats()["table_ms"], "sizes": {}}
    for K in sizes:
        D = min(K, len(msgs))
        reps = (K + D - 1) // D
        cut = lambda a, w=1: np.ascontiguousarray(a[:K * w])
        data, off = pack(msgs[:D], reps)
        off = np.ascontiguousarray(off[:K + 1])
        data = np.ascontiguousarray(data[:int(off[-1])])
        wdata, woff = pack(whole[:D], reps)
        woff = np.ascontiguousarray(woff[:K + 1])
        wdata = np.ascontiguousarray(wdata[:int(woff[-1])])
        sg = cut(np.tile(np.frombuffer(b"".join(sigs[:D]), np.uint8), reps), 64)
        idb = cut(np.tile(np.frombuffer(b"".join(ids[:D]), np.uint8), reps), 32)
        cr = cut(np.tile(np.array(creator[:D], np.int32), reps))
        want = cut(np.tile(np.array(exp[:D], np.uint8), reps))
        d = {k: dmalloc(a.nbytes) for k, a in (("data", data), ("off", off), ("wdata", wdata), ("woff", woff), ("sg", sg), ("idb", idb), ("cr", cr))}
        d_ok = [dmalloc(K), dmalloc(K)]

        def old_route():
            t0 = time.perf_counter()
            pk = key_arr[cr]                                   # one key per event: what the stateless call takes
            ok, dg = np.empty(K, np.uint8), np.empty((K, 32), np.uint8)
            assert L.sw_crypto_verify_batch(0, K, p(data), p(off), p(sg), p(pk), p(ok)) == 0
            t1 = time.perf_counter()
            assert L.sw_crypto_hash_batch(0, K, p(wdata), p(woff), p(dg)) == 0
            t2 = time.perf_counter()
            ok &= (dg == idb.reshape(K, 32)).all(axis=1)
            up(d_ok[0], ok)                                    # sw_ingest_payload's upload of `ok`
            t3 = time.perf_counter()
            return {"total": (t3 - t0) * 1e3, "verify": (t1 - t0) * 1e3, "hash": (t2 - t1) * 1e3, "compare+upload": (t3 - t2) * 1e3}

        def new_route(resident):
            t0 = time.perf_counter()
            if not resident:
                for k, a in (("data", data), ("off", off), ("wdata", wdata), ("woff", woff), ("sg", sg), ("idb", idb), ("cr", cr)):
                    up(d[k], a)
            t1 = time.perf_counter()
            h.validate_payload_device(d["data"], d["off"], data.nbytes, d["sg"], d["cr"], d_ok[1], whole=d["wdata"], whole_off=d["woff"],
                                      whole_bytes=wdata.nbytes, ids=d["idb"], count=K)
            h.synchronize()
            t2 = time.perf_counter()
            return {"total": (t2 - t0) * 1e3, "upload": (t1 - t0) * 1e3, "validate": (t2 - t1) * 1e3}

        def verdicts(q):
            out = np.empty(K, np.uint8)
            assert hip.hipMemcpy(p(out), q, K, 2) == 0
            return out

        new_route(False)     # warm-up
        times = {"old": [], "new": [], "resident": []}
        for i in range(2 * args.laps + 1):    # old first and last
            if i % 2 == 0:
                times["old"].append(old_route())
            else:
                times["new"].append(new_route(False))
                times["resident"].append(new_route(True))
        if not (np.array_equal(verdicts(d_ok[0]), want) and np.array_equal(verdicts(d_ok[1]), want)):
            print("MISMATCH at K = %d: the routes do not give the expected verdicts; nothing is reported" % K)
            return 1
        print("== %d members, K = %d events (%d distinct), %d rejected; %d old laps, %d new laps (alternating, old first and last); "
              "both routes give the expected verdicts" % (n, K, D, int((want == 0).sum()), len(times["old"]), len(times["new"])))
        r = {"distinct": D}
        for v, label, keys_ in (("old", "verify_batch + hash_batch route", ("total", "verify", "hash", "compare+upload")),
                                ("new", "validate_payload_device + uploads", ("total", "upload", "validate")),
                                ("resident", "validate_payload_device, resident", ("total",))):
            for key in keys_:
                r["%s_%s_ms" % (v, key)] = s = stats([tm[key] for tm in times[v]])
                line(label if key == "total" else "   ... " + key, s, K)
        r["old_over_new"] = r["old_total_ms"]["median"] / r["new_total_ms"]["median"]
        r["old_over_resident"] = r["old_total_ms"]["median"] / r["resident_total_ms"]["median"]
        print("   old / new = %.2f from host arrays, %.2f from resident arrays" % (r["old_over_new"], r["old_over_resident"]))
        result["sizes"][str(K)] = r
        for q in list(d.values()) + d_ok:
            hip.hipFree(C.c_void_p(q))
    print(json.dumps(result))
    h.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
