"""The wire bytes of a sync answer on the device (csrc/wire.hip.h) against the host route, on one GPU: 256
members, 65 536 and 1 M events, every d None and data of 186 bytes mean (event_data_bench's lengths: 30 % None, else
1 .. 512 bytes, 8 events of 60 000).  The answer is the whole hashgraph below the newest event (the asker knows nobody).

Whole calls, host clock, laps alternating with the host route first and last; median (min, max):
  (a) sender on the host     the dict entry per event + dumps((head, subset)) from a Node-like dict of Events (node.py, ask_sync)
  (b) sender on the device   Hashgraph.export_message: walk, export, data gather, message, copy of the bytes to the host
  (c) receiver on the host   loads(reply) + the field loop of Node._sync_payload_device (without its crypto)
  (d) receiver on the device upload of the bytes + Hashgraph.unpack_message_device into resident arrays
and the writer alone (pack_message_device) and the reader alone (unpack_message_device) on resident arrays, GB/s of message.

usage: python profiles/wire_message_bench.py [--sizes 65536,1048576] > profiles/wire_message_bench.txt"""
import argparse
import importlib
import os
import pickle
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
pkg = importlib.import_module("py-swirld_amd")
from event_data_bench import MEMBERS, SEED, Hip, draw_lengths  # noqa: E402

Event = pkg.node.Event
LAPS = 3          # device laps; the host route runs LAPS + 1 times, first and last


def stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def alternate(host, device, sync):
    h, d = [], []
    for lap in range(2 * LAPS + 1):
        fn, out = (host, h) if lap % 2 == 0 else (device, d)
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(1e3 * (time.perf_counter() - t0))
    return stats(h), stats(d)


def line(what, K, nbytes, ms, rate=False):
    med, lo, hi = ms
    r = "  %8.1f GB/s" % (nbytes / med / 1e6) if rate else ""
    print("%-44s %9d events %12d bytes  %10.3f ms (min %.3f, max %.3f)%s" % (what, K, nbytes, med, lo, hi, r), flush=True)


def run(hip, N, with_data):
    n = MEMBERS
    cr, sp, op, t, sig = stream = pkg.synth_hashgraph(n, N, 7)
    t = t + 1.7e9
    rng = np.random.default_rng(SEED + 2)
    ids = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    keys = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    lens, none = draw_lengths(N)
    if not with_data:
        lens[:], none[:] = 0, 1
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    data = np.random.default_rng(SEED + 1).integers(0, 256, int(off[-1]), dtype=np.uint8)
    src = pkg.Hashgraph(n)
    src.append_events(cr, sp, op, t, sig)
    src.set_event_ids(0, ids)
    src.set_member_keys(keys)
    src.set_event_class(Event.__module__, Event.__qualname__)
    src.set_event_data(0, (data, off, none))
    src.divide_rounds(0, N)
    head = N - 1
    tag = "data 186 B mean" if with_data else "data None"
    # ---- the Node-like state of the host route
    raw, idb, sgb = data.tobytes(), ids.tobytes(), np.ascontiguousarray(sig, np.uint8).tobytes()
    eid = [idb[32 * e:32 * e + 32] for e in range(N)]
    pks = [keys[m].tobytes() for m in range(n)]
    hg = {}
    for e in range(N):
        d = None if none[e] else raw[off[e]:off[e + 1]]
        hg[eid[e]] = Event(d, () if sp[e] < 0 else (eid[sp[e]], eid[op[e]]), float(t[e]), pks[cr[e]], sgb[64 * e:64 * e + 64])
    walk = src.sync_walk(head).tolist()
    K = len(walk)
    mindex = {pk: m for m, pk in enumerate(pks)}
    out = {}

    def host_send():
        subset = {}
        for i in walk:
            subset[eid[i]] = hg[eid[i]]
        out["reply"] = pickle.dumps((eid[head], subset))

    def dev_send():
        out["msg"] = src.export_message(head, data=with_data)
    a, b = alternate(host_send, dev_send, src.synchronize)
    msg, reply = out["msg"], out["reply"]
    assert pickle.loads(msg) == pickle.loads(reply)
    line("(a) sender, host: dict + dumps [%s]" % tag, K, len(reply), a)
    line("(b) sender, device: export_message [%s]" % tag, K, len(msg), b)
    print("    (b) < (a): %s, %.1fx" % (b[0] < a[0], a[0] / b[0]))
    # ---- the receiver
    nd = int(lens[walk].sum())
    dst = pkg.Hashgraph(n)
    dst.set_member_keys(keys)
    dst.set_event_class(Event.__module__, Event.__qualname__)
    width = dict(head=32, ids=32 * K, sp=32 * K, op=32 * K, arity=K, creator=4 * K, t=8 * K, sig=64 * K, data=nd + 16, data_off=8 * (K + 1), none=K)
    p = {k: hip.alloc(w) for k, w in width.items()}
    d_msg = hip.alloc(len(msg) + 16)
    mbuf = np.frombuffer(msg, np.uint8)
    is32 = lambda x: isinstance(x, (bytes, bytearray)) and len(x) == 32

    def host_recv():
        remote_head, remote_hg = pickle.loads(reply)
        eids = list(remote_hg)
        k = len(eids)
        par = np.zeros((2, k, 32), np.uint8)
        arity, creator, tt, sg = np.zeros(k, np.uint8), np.full(k, -1, np.int32), np.zeros(k, np.float64), np.zeros((k, 64), np.uint8)
        np.frombuffer(b"".join(bytes(e) for e in eids), np.uint8).reshape(k, 32)
        for i, e in enumerate(eids):
            ev = remote_hg[e]
            good = isinstance(ev.p, tuple) and all(is32(q) for q in ev.p) and isinstance(ev.s, (bytes, bytearray)) and len(ev.s) == 64
            if good:
                tt[i] = float(ev.t)
                sg[i] = np.frombuffer(bytes(ev.s), np.uint8)
                arity[i] = min(len(ev.p), 255)
                if len(ev.p) == 2:
                    par[0, i] = np.frombuffer(bytes(ev.p[0]), np.uint8)
                    par[1, i] = np.frombuffer(bytes(ev.p[1]), np.uint8)
                creator[i] = mindex.get(ev.c, -1)

    def dev_recv():
        hip.copy(d_msg, mbuf.ctypes.data, len(msg), 1)
        got = dst.unpack_message_device(d_msg, len(msg), K, nd, p["head"], p["ids"], p["sp"], p["op"], p["arity"], p["creator"], p["t"], p["sig"],
                                        p["data"], p["data_off"], p["none"])
        assert got == (K, nd)
    c, d = alternate(host_recv, dev_recv, dst.synchronize)
    line("(c) receiver, host: loads + field loop [%s]" % tag, K, len(reply), c)
    line("(d) receiver, device: upload + unpack [%s]" % tag, K, len(msg), d)
    print("    (d) < (c): %s, %.1fx" % (d[0] < c[0], c[0] / d[0]))
    # ---- writer and reader alone, on resident arrays (the reader's outputs are the writer's inputs)
    d_head, d_out, d_len = hip.up(ids[head]), hip.alloc(src.pack_message_bound(K, nd) + 16), hip.alloc(8)
    cap = src.pack_message_bound(K, nd)

    def write():
        src.pack_message_device(d_head, p["ids"], p["sp"], p["op"], p["arity"], p["creator"], p["t"], p["sig"], d_out, cap, d_len,
                                data=p["data"] if nd else None, data_off=p["data_off"], data_bytes=nd, data_none=p["none"], count=K)

    def read():
        dst.unpack_message_device(d_msg, len(msg), K, nd, p["head"], p["ids"], p["sp"], p["op"], p["arity"], p["creator"], p["t"], p["sig"], p["data"],
                                  p["data_off"], p["none"])
    for what, fn, h in (("writer alone: pack_message_device", write, src), ("reader alone: unpack_message_device", read, dst)):
        ms = []
        for lap in range(3 + 10):
            h.synchronize()
            t0 = time.perf_counter()
            fn()
            h.synchronize()
            if lap >= 3:
                ms.append(1e3 * (time.perf_counter() - t0))
        line("%s [%s]" % (what, tag), K, len(msg), stats(ms), rate=True)
    back = np.empty(len(msg), np.uint8)
    hip.copy(back.ctypes.data, d_out, len(msg), 2)
    assert back.tobytes() == msg, "the writer on the reader's arrays gives the message back"
    hip.free(d_msg, d_head, d_out, d_len, *p.values())
    src.close()
    dst.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576")
    args = ap.parse_args()
    hip = Hip()
    print("# wire bytes of a sync answer, %d members; whole calls, laps alternating, host first and last: median (min, max)" % MEMBERS)
    print("# k_pack_write<whole> on resident arrays, for comparison: 232 GB/s (profiles/pack_events_bench.txt)")
    for N in (int(x) for x in args.sizes.split(",")):
        for with_data in (False, True):
            run(hip, N, with_data)
