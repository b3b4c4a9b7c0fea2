"""Creating a signed history on one GPU (csrc/sign.hip.h): 256 members, histories from sw_synth_hashgraph at
65 536 and 1 M events, data None — the host route against create_events, from the same index arrays.

  host    what the tests and benches of this repository did so far: per event two pickle.dumps, libsodium's
          crypto_sign_detached and hashlib.blake2b, then ONE ingest_payload of the whole history
  device  create_events of the whole history in one call: levels, one launch per level, append, id index, and the data
          store's entries (all None)

Host clock around each route, a fresh context (member keys and signing keys set, memory reserved) per lap.  Laps alternate,
host first and last; at 1 M events ONE host lap is run (it takes about 17 s), in front of the device laps.
Reported: min / median / max per route, the number of levels, the mean level width and the ms per level; the phases of one
further device lap under sw_set_profiling (levels + sort, signing, commit; profiling adds a synchronisation per phase); and
the time of ONE level of width 1, 64 and 256 (roots only, sign_events on resident keys, the signing phase of
sw_get_sign_stats under profiling, 7 calls after 2).

usage: python profiles/create_events_bench.py [--sizes 65536,1048576] > profiles/create_events_bench.txt"""
import argparse
import hashlib
import importlib
import os
import pickle
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("py-swirld_amd")
import model_pack as mpk   # noqa: E402  (the Event class that pickles as swirld.Event)

MEMBERS, SEED = 256, 20261019
crypto = pkg.node.crypto


def keypairs():
    seeds = [bytes([SEED & 255, m & 255, m >> 8]) + bytes(29) for m in range(MEMBERS)]
    return seeds, [crypto.sign_seed_keypair(s) for s in seeds]


def context(seeds, kps, N, signing):
    h = pkg.Hashgraph(MEMBERS)
    h.reserve(N)
    h.set_member_keys([pk for pk, _ in kps])
    if signing:
        h.set_signing_seeds(list(range(MEMBERS)), seeds)
    h.synchronize()
    return h


def host_lap(seeds, kps, cr, sp, op, t):
    N = len(cr)
    h = context(seeds, kps, N, False)
    crl, spl, opl, tl = cr.tolist(), sp.tolist(), op.tolist(), t.tolist()
    t0 = time.perf_counter()
    ids, sigs = [], []
    with mpk.event_class("swirld", "Event") as Event:
        for e in range(N):
            p = () if spl[e] < 0 else (ids[spl[e]], ids[opl[e]])
            pk, sk = kps[crl[e]]
            body = (None, p, tl[e], pk)
            s = crypto.sign_detached(pickle.dumps(body, protocol=4), sk)
            ids.append(hashlib.blake2b(pickle.dumps(Event(*body, s), protocol=4), digest_size=32).digest())
            sigs.append(s)
    a_ids = np.frombuffer(b"".join(ids), np.uint8).reshape(N, 32)
    a_sig = np.frombuffer(b"".join(sigs), np.uint8).reshape(N, 64)
    zero = np.zeros((N, 32), np.uint8)
    sp_ids = np.where((sp >= 0)[:, None], a_ids[np.maximum(sp, 0)], zero)
    op_ids = np.where((op >= 0)[:, None], a_ids[np.maximum(op, 0)], zero)
    t_sign = time.perf_counter() - t0
    _, stored = h.ingest_payload(a_ids, sp_ids, op_ids, np.where(sp < 0, 0, 2).astype(np.uint8), cr, t=t, sig=a_sig)
    h.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    assert stored == N
    last = h.event_ids(N - 1, 1).tobytes()
    h.close()
    return ms, 1e3 * t_sign, a_ids, last


def device_lap(seeds, kps, cr, sp, op, t, profiling=False):
    N = len(cr)
    h = context(seeds, kps, N, True)
    h.set_profiling(profiling)
    t0 = time.perf_counter()
    first = h.create_events(cr, sp, op, t)
    h.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    assert first == 0 and h.num_events == N
    st = h.sign_stats()
    ids = h.event_ids()
    h.close()
    return ms, st, ids


def spread(ms):
    return "%10.1f ms (min %.1f, max %.1f, %d laps)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def run(seeds, kps, N):
    cr, sp, op, t, _ = pkg.synth_hashgraph(MEMBERS, N, 1)
    one_host = N > 200000
    host, dev, sign_only, ref_ids, st = [], [], [], None, None
    plan = "HDD" if one_host else "HDHDHDH"
    for route in plan:
        if route == "H":
            ms, ms_sign, ref_ids, _ = host_lap(seeds, kps, cr, sp, op, t)
            host.append(ms)
            sign_only.append(ms_sign)
        else:
            ms, st, ids = device_lap(seeds, kps, cr, sp, op, t)
            dev.append(ms)
            assert np.array_equal(ids, ref_ids), "the device route gives the host route's ids"
    levels = st["levels"]
    print("%d events, %d members: %d levels, mean width %.1f; laps %s%s" % (N, MEMBERS, levels, N / levels, plan,
                                                                           " (ONE host lap at this size)" if one_host else ""))
    print("  host route   (sign + ingest_payload)  %s   of which signing %.1f ms" % (spread(host), statistics.median(sign_only)))
    print("  device route (create_events)          %s   %.4f ms per level, %.2f us per event" % (spread(dev), statistics.median(dev) / levels,
                                                                                                1e3 * statistics.median(dev) / N))
    print("  host / device = %.1f" % (statistics.median(host) / statistics.median(dev)))
    _, st, _ = device_lap(seeds, kps, cr, sp, op, t, profiling=True)
    print("  device phases under profiling: levels + sort %.2f ms, signing %.1f ms (%.4f ms per level), commit %.1f ms"
          % (st["levels_ms"], st["sign_ms"], st["sign_ms"] / levels, st["commit_ms"]))
    sys.stdout.flush()


def single_levels(seeds, kps):
    h = context(seeds, kps, 1024, True)
    h.set_profiling(True)
    for w in (1, 64, 256):
        cr = np.arange(w, dtype=np.int32)
        root = np.full(w, -1, np.int32)
        ms = []
        for _ in range(2 + 7):
            h.sign_events(cr, root, root, np.arange(w, dtype=np.float64))
            st = h.sign_stats()
            assert st["levels"] == 1
            ms.append(st["sign_ms"])
        ms = ms[2:]
        print("  one level of width %3d: signing %.4f ms (min %.4f, max %.4f)" % (w, statistics.median(ms), min(ms), max(ms)))
    h.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576")
    args = ap.parse_args()
    seeds, kps = keypairs()
    print("# creating signed events, %d members, data None (key seed %d); libsodium through %s" % (MEMBERS, SEED, "ctypes" if crypto.HAVE_SODIUM else "NO LIBSODIUM"))
    print("single levels (roots only, sign_events, signing phase under profiling):")
    single_levels(seeds, kps)
    for N in (int(x) for x in args.sizes.split(",")):
        run(seeds, kps, N)
