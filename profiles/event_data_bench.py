"""Throughput of the data store (csrc/data.hip.h) on one GPU: 256 members, 65 536 and 1 M events.

Data lengths are drawn ONCE per size with numpy's default_rng(20261019): 30 % None, the rest uniform in 1 .. 512 bytes, and
8 events of 60 000 bytes.

Reported per size (host clock around work that ends in a device synchronise; the median, with minimum and maximum):
  gather      sw_gather_event_data_device of the whole ordered stream's data on resident arrays, GB/s written; 10 calls after 3
  memcpy      a device-to-device hipMemcpy of the same byte count in the same process: the ceiling; 10 calls after 3
  host route  what a caller does today: b"".join(hg[h].d ...) over the ordered stream plus offsets plus one upload; 3 calls after 1
  store       sw_set_event_data_device of all events from resident arrays, a fresh context per call; 5 calls after 1.  This is the
              ragged copy from a caller's buffer alone, NOT the ingest
  ingest      sw_ingest_payload_device of the second half of the events into a context that holds the first half, the payload
              (src's export) and its data (src's gather) resident: without data, and with data — the difference is the ingest
              append (fold and sum, slots, second lengths + scan, copy, three synchronisations); a fresh receiver per call, 5 after 1
  pull        sw_sync_pull_data without validation between two contexts, the receiver holding the first half; a fresh receiver per
              call, 5 after 1.  The validated pull needs really signed events and is timed at 65 536 events only

usage: python profiles/event_data_bench.py [--sizes 65536,1048576] > profiles/event_data_bench.txt"""
import argparse
import ctypes as C
import importlib
import os
import pickle
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("py-swirld_amd")

WARMUP, REPEATS, SEED, MEMBERS = 3, 10, 20261019, 256


class Hip:
    def __init__(self):
        L = C.CDLL(pkg.LIB_PATH)
        L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.hipFree.argtypes = [C.c_void_p]
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.L = L

    def alloc(self, nbytes):
        p = C.c_void_p()
        if self.L.hipMalloc(C.byref(p), max(int(nbytes), 256)) != 0:
            raise MemoryError("hipMalloc(%d)" % nbytes)
        return p.value

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        assert self.L.hipMemcpy(C.c_void_p(p), a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
        return p

    def copy(self, dst, src, nbytes, kind):
        assert self.L.hipMemcpy(C.c_void_p(dst), C.c_void_p(src), nbytes, kind) == 0

    def sync(self):
        assert self.L.hipDeviceSynchronize() == 0

    def free(self, *ptrs):
        for p in ptrs:
            self.L.hipFree(C.c_void_p(p))


def timed(fn, sync, repeats=REPEATS, warmup=WARMUP):
    ms = []
    for i in range(warmup + repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if i >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms), min(ms), max(ms)


def draw_lengths(N):
    rng = np.random.default_rng(SEED)
    lens = rng.integers(1, 513, N)
    none = rng.random(N) < 0.30
    lens[none] = 0
    big = rng.choice(np.flatnonzero(~none), 8, replace=False)
    lens[big] = 60000
    return lens.astype(np.int64), none.astype(np.uint8)


def line(what, N, nbytes, ms):
    med, lo, hi = ms
    rate = "" if not nbytes else "  %8.1f GB/s" % (nbytes / med / 1e6)
    print("%-34s %9d events %12d bytes  %9.3f ms (min %.3f, max %.3f)%s" % (what, N, nbytes, med, lo, hi, rate), flush=True)


def run(hip, N):
    n = MEMBERS
    cr, sp, op, t, sig = stream = pkg.synth_hashgraph(n, N, 7)
    lens, none = draw_lengths(N)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    data = np.random.default_rng(SEED + 1).integers(0, 256, int(off[-1]), dtype=np.uint8)
    ids = np.random.default_rng(SEED + 2).integers(0, 256, (N, 32), dtype=np.uint8)
    d_data, d_off, d_none = hip.up(data), hip.up(off), hip.up(none)
    src = pkg.Hashgraph(n)
    src.append_events(*stream)
    src.set_event_ids(0, ids)
    src.set_event_data_device(0, N, d_data, d_off, len(data), d_none)
    src.divide_rounds(0, N)
    src.find_order(list(src.decide_fame()))
    K = src.num_ordered
    d_ev = hip.alloc(4 * K)
    src.export_ordered_device(0, K, event=d_ev)
    nb = src.gather_event_data_device(K, d_ev)
    g_data, g_off, g_none, spare = hip.alloc(nb + 16), hip.alloc(8 * (K + 1)), hip.alloc(K), hip.alloc(nb + 16)
    line("gather (ordered stream, resident)", K, nb, timed(lambda: src.gather_event_data_device(K, d_ev, nb, g_data, g_off, g_none), src.synchronize))
    line("memcpy device to device (ceiling)", K, nb, timed(lambda: hip.copy(spare, g_data, nb, 3), hip.sync))
    # what a caller does today
    order = src.transactions()
    raw = data.tobytes()
    datas = [None if none[e] else raw[off[e]:off[e + 1]] for e in range(N)]
    stage = hip.alloc(nb + 16)

    def host_route():
        picked = [datas[e] for e in order]
        blob = np.frombuffer(b"".join(d for d in picked if d is not None), np.uint8)
        o = np.zeros(len(picked) + 1, np.int64)
        np.cumsum([0 if d is None else len(d) for d in picked], out=o[1:])
        hip.copy(stage, blob.ctypes.data, blob.nbytes, 1)
        hip.copy(g_off, o.ctypes.data, o.nbytes, 1)
    line("host route (join, offsets, upload)", K, nb, timed(host_route, hip.sync, repeats=3, warmup=1))

    def store():
        h = pkg.Hashgraph(n)
        h.append_events(*stream)
        h.synchronize()
        t0 = time.perf_counter()
        h.set_event_data_device(0, N, d_data, d_off, len(data), d_none)
        h.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        h.close()
        return dt
    ms = [store() for _ in range(1 + 5)][1:]
    line("store from device (ragged copy alone)", N, len(data), (statistics.median(ms), min(ms), max(ms)))
    half = N // 2

    def receiver(with_data):
        h = pkg.Hashgraph(n)
        h.append_events(cr[:half], sp[:half], op[:half], t[:half], sig[:half])
        h.set_event_ids(0, ids[:half])
        if with_data:
            h.set_event_data(0, (data[:off[half]], off[:half + 1], none[:half]))
        h.divide_rounds(0, half)
        h.synchronize()
        return h

    # the payload src answers a holder of the first half with, and its data, resident
    r0 = receiver(False)
    d_known = hip.alloc(4 * n)
    r0.known_heights_device(half - 1, d_known)
    r0.synchronize()
    P = src.export_size(N - 1, d_known)
    pb = dict(ids=hip.alloc(32 * P), sp=hip.alloc(32 * P), op=hip.alloc(32 * P), ar=hip.alloc(P), cr=hip.alloc(4 * P), t=hip.alloc(8 * P),
              sig=hip.alloc(64 * P), ev=hip.alloc(4 * P), out=hip.alloc(4 * P), off=hip.alloc(8 * (P + 1)), none=hip.alloc(P))
    assert src.export_payload_device(N - 1, d_known, P, pb["ids"], pb["sp"], pb["op"], pb["ar"], pb["cr"], pb["t"], pb["sig"], pb["ev"]) == P
    pbytes = src.gather_event_data_device(P, pb["ev"])
    pb["data"] = hip.alloc(pbytes + 16)
    src.gather_event_data_device(P, pb["ev"], pbytes, pb["data"], pb["off"], pb["none"])
    src.synchronize()
    r0.close()

    def ingest(with_data):
        h = receiver(with_data)
        kw = dict(data=pb["data"], data_off=pb["off"], data_bytes=pbytes, data_none=pb["none"]) if with_data else {}
        t0 = time.perf_counter()
        _, stored = h.ingest_payload_device(pb["ids"], pb["sp"], pb["op"], pb["ar"], pb["cr"], None, pb["t"], pb["sig"], index_out=pb["out"], count=P, **kw)
        h.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        h.close()
        return dt, stored
    for with_data in (False, True):
        runs = [ingest(with_data) for _ in range(1 + 5)][1:]
        ms = [x[0] for x in runs]
        line("ingest %s (stored %d)" % ("with data" if with_data else "without data", runs[0][1]), P, pbytes if with_data else 0,
             (statistics.median(ms), min(ms), max(ms)))
    hip.free(d_known, *pb.values())

    def pull(with_data):
        h = receiver(with_data)
        t0 = time.perf_counter()
        r = h.pull_from(src, N - 1, half - 1, data=True) if with_data else h.pull_from(src, N - 1, half - 1)
        h.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        h.close()
        return dt, r
    for with_data in (False, True):
        runs = [pull(with_data) for _ in range(1 + 5)][1:]
        ms = [x[0] for x in runs]
        line("pull %s (sent %d, stored %d)" % ("with data" if with_data else "without data", runs[0][1][0], runs[0][1][-1]), runs[0][1][0], 0,
             (statistics.median(ms), min(ms), max(ms)))
    st = src.data_stats()
    print("   store: %d events, %d arena bytes; %d gather calls, %d bytes gathered" % (st["events"], st["bytes"], st["gather_calls"], st["gather_bytes"]))
    src.close()
    hip.free(d_data, d_off, d_none, d_ev, g_data, g_off, g_none, spare, stage)


def run_validated(hip, N):
    """The validated pull of really signed events with data, against the plain validated pull's cost without any."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import model_pack as mpk
    crypto = pkg.node.crypto
    n = MEMBERS
    cr, sp, op, t, _ = pkg.synth_hashgraph(n, N, 7)
    lens, none = draw_lengths(N)
    rng = np.random.default_rng(SEED + 1)
    kps = [crypto.sign_seed_keypair(bytes([m & 255, m >> 8]) + bytes(30)) for m in range(n)]
    ids, sigs, ds = [], [], []
    with mpk.event_class("swirld", "Event") as Event:
        for e in range(N):
            d = None if none[e] else rng.integers(0, 256, int(lens[e]), dtype=np.uint8).tobytes()
            p = () if sp[e] < 0 else (ids[sp[e]], ids[op[e]])
            body = (d, p, float(t[e]), kps[cr[e]][0])
            s = crypto.sign_detached(pickle.dumps(body, protocol=4), kps[cr[e]][1])
            ids.append(crypto.generichash(pickle.dumps(Event(*body, s), protocol=4)))
            sigs.append(s)
            ds.append(d)
    ids = np.frombuffer(b"".join(ids), np.uint8).reshape(N, 32)
    sig = np.frombuffer(b"".join(sigs), np.uint8).reshape(N, 64)
    keys = [pk for pk, _ in kps]

    def holder(upto):
        h = pkg.Hashgraph(n)
        h.append_events(cr[:upto], sp[:upto], op[:upto], t[:upto], sig[:upto])
        h.set_event_ids(0, ids[:upto])
        h.set_event_data(0, ds[:upto])
        h.set_member_keys(keys)
        h.divide_rounds(0, upto)
        return h
    src = holder(N)
    half = N // 2
    for validate in (False, True):
        ms, r = [], None
        for _ in range(1 + 5):
            h = holder(half)
            h.synchronize()
            t0 = time.perf_counter()
            r = h.pull_from(src, N - 1, half - 1, validate=validate, data=True)
            h.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
            h.close()
        ms = ms[1:]
        line("signed pull with data, validate=%d (stored %d)" % (validate, r[-1]), r[0], 0, (statistics.median(ms), min(ms), max(ms)))
    src.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576")
    args = ap.parse_args()
    hip = Hip()
    print("# event data store, %d members; lengths: 30 %% None, else 1 .. 512 bytes, 8 events of 60 000 (seed %d)" % (MEMBERS, SEED))
    for N in (int(x) for x in args.sizes.split(",")):
        run(hip, N)
    run_validated(hip, 65536)
