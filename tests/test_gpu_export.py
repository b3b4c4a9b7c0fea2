"""GPU (-m gpu): answering a sync on the device (sw_get_known_heights_device, sw_export_payload[_device], sw_sync_pull;
csrc/gossip.hip.h).  The exported arrays must equal tests/model_gossip.py byte for byte; the capacity protocol and the
refusals leave the context usable; what one context exports another ingests, and the receiver — mapped through
index_out or the ids — equals the oracle on the stream; a gossip replayed through pull_from between six views leaves
every view equal to the oracle on the events it holds; the export changes nothing a getter or a later call can see.

No torch here (see tests/test_gpu_ingest_device.py): device buffers come through ctypes from the HIP runtime the
library is linked against."""
import ctypes as C

import numpy as np
import pytest

import model_gossip as mg
import model_payload as mp

pytestmark = pytest.mark.gpu

H2D, D2H = 1, 2
INT32_MAX = 2**31 - 1
FIELDS = ("ids", "sp_ids", "op_ids", "arity", "creator", "t", "sig", "event")
WIDTH = dict(ids=32, sp_ids=32, op_ids=32, arity=1, creator=4, t=8, sig=64, event=4)
DTYPE = dict(ids=np.uint8, sp_ids=np.uint8, op_ids=np.uint8, arity=np.uint8, creator=np.int32, t=np.float64, sig=np.uint8, event=np.int32)


class Hip:
    def __init__(self, pkg):
        L = C.CDLL(pkg.LIB_PATH)
        self.L = L
        L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.hipFree.argtypes = [C.c_void_p]
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.bufs = []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.L.hipMalloc(C.byref(p), max(int(nbytes), 16)) == 0
        self.bufs.append(p)
        return p.value

    def up(self, a, dtype, offset=0):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype)
        p = self.alloc(a.nbytes + offset) + offset
        assert self.L.hipMemcpy(C.c_void_p(p), a.ctypes.data_as(C.c_void_p), a.nbytes, H2D) == 0
        return p

    def down(self, p, n, dtype):
        out = np.empty(n, dtype)
        assert self.L.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.nbytes, D2H) == 0
        return out

    def fill(self, p, byte, nbytes):
        assert self.L.hipMemset(C.c_void_p(p), byte, nbytes) == 0

    def free(self):
        for p in self.bufs:
            self.L.hipFree(p)
        self.bufs = []


@pytest.fixture
def hip(pkg):
    h = Hip(pkg)
    yield h
    h.free()


def ids_array(keys):
    return np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), 32)


def stream_ids(N):
    return ids_array([mp.event_id(k) for k in range(N)])


class Out:
    """Device arrays for `cap` exported events."""

    def __init__(self, hip, cap):
        self.hip, self.cap = hip, cap
        self.p = {k: hip.alloc(cap * WIDTH[k]) for k in FIELDS}

    def fill(self, byte):
        for k in FIELDS:
            self.hip.fill(self.p[k], byte, self.cap * WIDTH[k])

    def read(self, K, fields=FIELDS):
        d = {k: self.hip.down(self.p[k], K * WIDTH[k] // np.dtype(DTYPE[k]).itemsize, DTYPE[k]) for k in fields}
        for k in ("ids", "sp_ids", "op_ids"):
            d[k] = d[k].reshape(K, 32)
        if "sig" in d:
            d["sig"] = d["sig"].reshape(K, 64)
        return d


def dev_export(h, out, head, d_known, extras=True, cap=None):
    p = out.p
    x = dict(t=p["t"], sig=p["sig"], event=p["event"]) if extras else {}
    K = h.export_payload_device(head, d_known, out.cap if cap is None else cap, p["ids"], p["sp_ids"], p["op_ids"], p["arity"], p["creator"], **x)
    return K, out.read(K, FIELDS if extras else FIELDS[:5])


def host_export_plain(h, head, known, K):
    """sw_export_payload without t, sig and event (the front end always asks for them)."""
    d = dict(ids=np.empty((K, 32), np.uint8), sp_ids=np.empty((K, 32), np.uint8), op_ids=np.empty((K, 32), np.uint8),
             arity=np.empty(K, np.uint8), creator=np.empty(K, np.int32))
    kn = None if known is None else np.ascontiguousarray(known, np.int32)
    n_out = C.c_int64()
    v = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = h._L.sw_export_payload(h._h, head, v(kn), K, *[v(d[k]) for k in FIELDS[:5]], None, None, None, C.byref(n_out))
    assert rc == 0 and n_out.value == K
    return d


def same(got, exp, what):
    for k in got:
        assert got[k].tobytes() == np.ascontiguousarray(exp[k]).tobytes(), "%s: %s" % (what, k)


def make(pkg, n, N, seed, mode=0, p0=0.0, p1=0.0, divided=None):
    """(context holding the stream with its ids, divided; the model's graph of it)."""
    stream = pkg.synth_hashgraph(n, N, seed, mode, p0, p1)
    h = pkg.Hashgraph(n)
    h.append_events(*stream)
    h.set_event_ids(0, stream_ids(N))
    h.divide_rounds(0, N if divided is None else divided)
    return h, mg.Graph(n, *stream), stream


# ---- 1. equals the model, byte for byte -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N,seed,mode,p0,p1", [(5, 300, 801, 0, 0, 0), (70, 6000, 802, 2, 0.3, 0.02), (130, 20_000, 803, 3, 0.6, 0),
                                                 (1024, 24_000, 804, 0, 0, 0)])
def test_export_equals_the_model(pkg, hip, n, N, seed, mode, p0, p1):
    h, g, _ = make(pkg, n, N, seed, mode, p0, p1)
    out = Out(hip, N)
    d_known = hip.alloc(4 * n + 64)
    rng = np.random.default_rng(seed)
    cases = [(int(rng.integers(n, N)), int(rng.integers(0, N))) for _ in range(20)]
    cases += [(N - 1, "nobody"), (N - 1, "minus-one"), (N - 7, N - 7), (N - 1, "max")]
    largest = 0
    for head, asker in cases:
        if asker == "nobody":
            known, dk = None, None
        elif asker in ("minus-one", "max"):
            known = np.full(n, -1 if asker == "minus-one" else INT32_MAX, np.int32)
            dk = hip.up(known, np.int32)
        else:
            known = g.known_heights(asker)
            assert np.array_equal(h.known_heights(asker), known)
            hip.fill(d_known, 0xA5, 4 * n + 64)
            h.known_heights_device(asker, d_known)
            raw = hip.down(d_known, n + 16, np.int32)
            assert np.array_equal(raw[:n], known) and np.all(raw[n:] == np.int32(-1515870811)), "n entries and nothing behind them"
            dk = d_known
        exp = g.export(head, known)
        what = "head %d asker %s" % (head, asker)
        K = len(exp["event"])
        largest = max(largest, K)
        kn_host = np.full(n, -1, np.int32) if known is None else known
        assert h.sync_diff(head, kn_host)[2] == K, what
        assert h.export_size(head, dk) == K, what
        for extras in (True, False):
            k_dev, got = dev_export(h, out, head, dk, extras)
            assert k_dev == K, what
            same(got, exp, what + " (device)")
        got = h.export_payload(head, known)
        same(got, exp, what + " (host)")
        same(host_export_plain(h, head, known, K), exp, what + " (host, plain)")
        if asker in (head, "max"):
            assert K == 1 and exp["event"][0] == head
    assert largest >= (N * 7) // 10         # the asker that knows nobody: most of the stream, many workgroups of the gather
    st = h.export_stats()
    assert st["calls"] == 4 * len(cases) and st["events"] > 0
    h.close()


def test_every_lane_width_gives_the_same_arrays(pkg, hip, monkeypatch):
    """SW_EXPORT_LANES is read when a context is created: one context per width."""
    out = Out(hip, 6000)
    for lanes in ("4", "8", "16"):
        monkeypatch.setenv("SW_EXPORT_LANES", lanes)
        h, g, _ = make(pkg, 70, 6000, 805)
        exp = g.export(5999, None)
        out.fill(0xA5)
        K, got = dev_export(h, out, 5999, None)
        assert K == len(exp["event"])
        same(got, exp, "lanes " + lanes)
        h.close()


# ---- 2. capacity protocol ------------------------------------------------------------------------------------------------
def test_capacity_protocol(pkg, hip):
    n, N = 16, 3000
    h, g, _ = make(pkg, n, N, 811)
    known = g.known_heights(1200)
    dk = hip.up(known, np.int32)
    exp = g.export(N - 1, known)
    total = len(exp["event"])
    assert total > 500
    out = Out(hip, total)
    out.fill(0xA5)
    p = out.p
    n_out = C.c_int64(-1)
    args = [C.c_void_p(p[k]) for k in FIELDS]
    rc = h._L.sw_export_payload_device(h._h, N - 1, C.c_void_p(dk), total - 1, *args, None, C.byref(n_out))
    assert rc == -34 and n_out.value == total
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.export_payload_device(N - 1, dk, total - 1, p["ids"], p["sp_ids"], p["op_ids"], p["arity"], p["creator"], p["t"], p["sig"], p["event"])
    assert ei.value.code == -34
    for k in FIELDS:
        assert np.all(hip.down(p[k], total * WIDTH[k], np.uint8) == 0xA5), "%s was written" % k
    # the size query: cap 0, every array NULL
    n_out = C.c_int64(-1)
    rc = h._L.sw_export_payload_device(h._h, N - 1, C.c_void_p(dk), 0, *([None] * 8), None, C.byref(n_out))
    assert rc == -34 and n_out.value == total and h.export_size(N - 1, dk) == total
    n_out = C.c_int64(-1)
    kn = np.ascontiguousarray(known, np.int32)
    rc = h._L.sw_export_payload(h._h, N - 1, kn.ctypes.data_as(C.c_void_p), 0, *([None] * 8), C.byref(n_out))
    assert rc == -34 and n_out.value == total
    # cap == total
    K, got = dev_export(h, out, N - 1, dk)
    assert K == total
    same(got, exp, "cap == total")
    h.close()


# ---- 3. refusals, each leaving the context usable ------------------------------------------------------------------------
def test_refusals(pkg, hip):
    n, N = 8, 600
    stream = cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, 821)
    g = mg.Graph(n, *stream)
    h = pkg.Hashgraph(n)
    h.append_events(*stream)
    h.divide_rounds(0, N - 10)
    out = Out(hip, N)
    p = out.p
    head = N - 20
    exp = g.export(head, None)

    def works():
        K, got = dev_export(h, out, head, None)
        assert K == len(exp["event"])
        same(got, exp, "after a refusal")
        same(h.export_payload(head), exp, "after a refusal (host)")

    def refused(code, fn):
        with pytest.raises(pkg.SwirldHipError) as ei:
            fn()
        assert ei.value.code == code, str(ei.value)

    # an incomplete id index: none, then all but the last
    refused(-95, lambda: dev_export(h, out, head, None))
    refused(-95, lambda: h.export_payload(head))
    ids = stream_ids(N)
    h.set_event_ids(0, ids[:N - 1])
    refused(-95, lambda: dev_export(h, out, head, None))
    other = pkg.Hashgraph(n)
    other.append_events(cr[:50], sp[:50], op[:50], t[:50], sig[:50])
    other.set_event_ids(0, ids[:50])
    other.divide_rounds(0, 50)
    refused(-95, lambda: other.pull_from(h, head, 49))
    refused(-95, lambda: h.pull_from(other, 49, head))
    h.set_event_ids(N - 1, ids[N - 1:])
    works()
    # an undivided head
    refused(-34, lambda: dev_export(h, out, N - 5, None))
    refused(-34, lambda: h.export_payload(N - 5))
    refused(-34, lambda: h.export_payload(-1))
    refused(-34, lambda: other.pull_from(h, N - 5, 49))
    refused(-34, lambda: other.pull_from(h, head, 50))
    # a host pointer for one output array; an id array at offset 8; a host pointer for the heights
    host = np.empty(N * 64, np.uint8)
    for k in FIELDS:
        a = dict(p)
        a[k] = host.ctypes.data
        refused(-22, lambda: h.export_payload_device(head, None, N, a["ids"], a["sp_ids"], a["op_ids"], a["arity"], a["creator"], a["t"], a["sig"], a["event"]))
    for k in ("ids", "sp_ids", "op_ids", "sig"):
        a = dict(p)
        a[k] = hip.alloc(N * 64 + 16) + 8
        refused(-22, lambda: h.export_payload_device(head, None, N, a["ids"], a["sp_ids"], a["op_ids"], a["arity"], a["creator"], a["t"], a["sig"], a["event"]))
    refused(-22, lambda: h.export_payload_device(head, np.zeros(n, np.int32).ctypes.data, N, p["ids"], p["sp_ids"], p["op_ids"], p["arity"], p["creator"]))
    refused(-22, lambda: h.known_heights_device(head, np.zeros(n, np.int32).ctypes.data))
    refused(-34, lambda: h.known_heights_device(N - 5, hip.alloc(4 * n)))
    works()
    # sw_sync_pull: with itself, with another member count
    refused(-22, lambda: h.pull_from(h, head, head))
    wide = pkg.Hashgraph(n + 1)
    w_stream = pkg.synth_hashgraph(n + 1, 100, 822)
    wide.append_events(*w_stream)
    wide.set_event_ids(0, stream_ids(100))
    wide.divide_rounds(0, 100)
    refused(-22, lambda: wide.pull_from(h, head, 99))
    refused(-22, lambda: h.pull_from(wide, 99, head))
    assert wide.num_events == 100 and h.num_events == N and other.num_events == 50
    works()
    # ... and the pull that is in order works: `other` ends up with every ancestor of the head
    n_sent, n_stored = other.pull_from(h, head, 49)
    assert n_sent == len(g.export(head, g.known_heights(49))["event"]) and 0 < n_stored <= n_sent
    assert other.num_events == 50 + n_stored
    # a context that has stored a fork runs on the exact path
    f = pkg.Hashgraph(n)
    f_sp = sp.copy()
    j = int(np.nonzero(cr[100:] == cr[n + 5])[0][3]) + 100
    f_sp[j] = sp[sp[j]]
    f.append_events(cr[:200], f_sp[:200], op[:200], t[:200], sig[:200])
    assert f.exact
    f.set_event_ids(0, ids[:200])
    f.divide_rounds(0, 200)
    refused(-95, lambda: f.export_payload(150))
    refused(-95, lambda: f.export_payload_device(150, None, N, p["ids"], p["sp_ids"], p["op_ids"], p["arity"], p["creator"]))
    refused(-95, lambda: other.pull_from(f, 150, 49))
    assert f.rounds().shape == (200,)
    for x in (h, other, wide, f):
        x.close()


# ---- 4. round trip A -> B ------------------------------------------------------------------------------------------------
def ancestors_only(stream):
    """The stream restricted to the ancestors-or-self of its last event, relabelled: the last event sees all of it."""
    cr, sp, op, t, sig = stream
    N = len(cr)
    keep = np.zeros(N, bool)
    keep[N - 1] = True
    spl, opl = sp.tolist(), op.tolist()
    for e in range(N - 1, -1, -1):
        if keep[e] and spl[e] >= 0:
            keep[spl[e]] = keep[opl[e]] = True
    new = np.cumsum(keep) - 1
    rel = lambda a: np.where(a >= 0, new[np.maximum(a, 0)], -1).astype(np.int32)
    return cr[keep], rel(sp[keep]), rel(op[keep]), t[keep], sig[keep]


def oracle_run(n, stream):
    from oracle.oracle import Oracle
    o = Oracle(n)
    o.append_events(*stream)
    N = len(stream[0])
    o.divide_rounds(0, N)
    nco = list(o.decide_fame())
    return o, nco, list(o.find_order(nco))


def assert_equals_oracle(h, n, stream, dense_of, first_undivided):
    """Every view of `h`, whose event k of the stream has dense index dense_of[k], equals the oracle's on the stream."""
    N = len(stream[0])
    o, nco, txo = oracle_run(n, stream)
    h.divide_rounds(first_undivided, N - first_undivided)
    nc = list(h.decide_fame())
    tx = list(h.find_order(nc))
    assert nc == nco
    assert tx == [int(dense_of[k]) for k in txo], "transaction order"
    relabel = lambda a: np.where(a >= 0, dense_of[np.maximum(a, 0)], -1)
    assert np.array_equal(h.rounds()[dense_of], o.round), "rounds"
    assert np.array_equal(h.heights()[dense_of], o.height), "heights"
    wit, ow = h.witnesses(), o.witnesses()
    assert np.array_equal(wit, relabel(ow)), "witnesses"
    m = ow >= 0
    assert np.array_equal(h.famous()[m], o.famous_by_event[ow[m]]), "famous"
    assert np.array_equal(h.consensus(), np.isin(np.arange(wit.shape[0]), nco).astype(np.uint8)), "consensus"
    ocs = o.can_see
    for k in range(0, N, max(1, N // 200)):
        assert np.array_equal(h.can_see(int(dense_of[k]), 1)[0], relabel(ocs[k])), "can_see row of event %d" % k


@pytest.mark.parametrize("n,N0,behind,seed", [(64, 21_000, 9_000, 831), (5, 400, 40, 832)])
def test_round_trip_from_one_context_into_another(pkg, hip, n, N0, behind, seed):
    stream = cr, sp, op, t, sig = ancestors_only(pkg.synth_hashgraph(n, N0, seed))
    N = len(cr)
    a = N - behind
    assert N > N0 // 2 and a > n
    ids = stream_ids(N)
    A, B = pkg.Hashgraph(n), pkg.Hashgraph(n)
    A.append_events(*stream)
    A.set_event_ids(0, ids)
    A.divide_rounds(0, N)
    B.append_events(cr[:a], sp[:a], op[:a], t[:a], sig[:a])
    B.set_event_ids(0, ids[:a])
    B.divide_rounds(0, a)
    d_known = hip.alloc(4 * n)
    B.known_heights_device(a - 1, d_known)
    K = A.export_size(N - 1, d_known)
    assert N - a <= K <= N
    out = Out(hip, K)
    p = out.p
    assert A.export_payload_device(N - 1, d_known, K, p["ids"], p["sp_ids"], p["op_ids"], p["arity"], p["creator"], p["t"], p["sig"], p["event"]) == K
    d_index = hip.alloc(4 * K)
    _, n_stored = B.ingest_payload_device(p["ids"], p["sp_ids"], p["op_ids"], p["arity"], p["creator"], None, p["t"], p["sig"], index_out=d_index, count=K)
    index_out = hip.down(d_index, K, np.int32)
    event = hip.down(p["event"], K, np.int32)
    assert np.all(index_out >= 0) and n_stored == N - a and B.num_events == N
    if behind >= 8192:
        assert B.ingest_stats()["device_batches"] >= 1      # the bulk device append really ran
    dense_of = np.arange(N)
    dense_of[event] = index_out
    assert np.array_equal(dense_of[:a], np.arange(a)) and sorted(dense_of.tolist()) == list(range(N))
    assert np.array_equal(B.event_ids()[dense_of], ids)
    assert_equals_oracle(B, n, stream, dense_of, a)
    A.close()
    B.close()


# ---- 5. replayed gossip through pull_from --------------------------------------------------------------------------------
def test_replayed_gossip_between_six_views(pkg, hip):
    from oracle.oracle import Oracle
    n, N = 6, 500
    cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, 841)
    ids = stream_ids(N)
    of_id = {bytes(ids[k]): k for k in range(N)}
    views = []
    for m in range(n):                      # every view starts with its own root (events 0 .. n-1 are the roots)
        v = pkg.Hashgraph(n)
        v.append_events(cr[m:m + 1], sp[m:m + 1], op[m:m + 1], t[m:m + 1], sig[m:m + 1])
        v.set_event_ids(0, ids[m:m + 1])
        v.divide_rounds(0, 1)
        views.append(v)
    zero = np.zeros((1, 32), np.uint8)
    pulls = stored_total = 0
    for e in range(n, N):
        me, peer = views[cr[e]], views[cr[op[e]]]
        my_head = int(me.lookup_event_ids(ids[sp[e]:sp[e] + 1])[0])
        peer_head = int(peer.lookup_event_ids(ids[op[e]:op[e] + 1])[0])
        assert my_head >= 0 and peer_head >= 0
        # what the peer will send, and how much of it I hold already: nothing else may be turned away.  sw_sync_pull keeps its
        # index_out on the device, so "every index_out is a known or a stored index" is checked through counts: an event
        # of the payload gets a known index exactly when I hold its id (`have` of them, no id twice in a payload), every
        # other one gets either a stored index — counted by n_stored — or a reject code; n_stored == n_sent - have therefore
        # holds exactly when no reject code occurred, and the look-up afterwards shows each of them under an index.
        sent = peer.export_payload(peer_head, me.known_heights(my_head))
        have = int((me.lookup_event_ids(sent["ids"]) >= 0).sum())
        before = me.num_events
        n_sent, n_stored = me.pull_from(peer, peer_head, my_head)
        assert n_sent == len(sent["arity"]) and n_stored <= n_sent
        assert n_stored == n_sent - have and me.num_events == before + n_stored
        assert np.all(me.lookup_event_ids(sent["ids"]) >= 0)
        pulls += 1
        stored_total += n_stored
        # my own new event, addressed by id like everything else
        index_out, one = me.ingest_payload(ids[e:e + 1], ids[sp[e]:sp[e] + 1], ids[op[e]:op[e] + 1], np.array([2], np.uint8), cr[e:e + 1],
                                           None, t[e:e + 1], sig[e:e + 1])
        assert one == 1 and index_out[0] == before + n_stored
        me.divide_rounds(before, me.num_events - before)
    assert pulls == N - n and stored_total > N
    for m, v in enumerate(views):
        # the sub-stream the view holds, in its own dense order
        held = np.array([of_id[bytes(i)] for i in v.event_ids()], np.int64)
        Nv = len(held)
        assert len(set(held.tolist())) == Nv and Nv > N // 2
        dense_of = np.full(N, -1, np.int64)
        dense_of[held] = np.arange(Nv)
        rel = lambda a: np.where(a >= 0, dense_of[np.maximum(a, 0)], -1).astype(np.int32)
        sub = (cr[held], rel(sp[held]), rel(op[held]), t[held], sig[held])
        assert np.all(sub[1][sub[1] >= 0] < np.arange(Nv)[sub[1] >= 0])
        o, nco, txo = oracle_run(n, sub)
        nc = list(v.decide_fame())
        tx = list(v.find_order(nc))
        assert nc == nco and tx == txo, "view %d: fame / order" % m
        assert np.array_equal(v.rounds(), o.round) and np.array_equal(v.heights(), o.height), "view %d" % m
        ow = o.witnesses()
        assert np.array_equal(v.witnesses(), ow)
        assert np.array_equal(v.famous()[ow >= 0], o.famous_by_event[ow[ow >= 0]])
        assert [int(x) for x in v.transactions()] == txo
        v.close()


# ---- 6. read-only --------------------------------------------------------------------------------------------------------
def test_export_changes_nothing(pkg, hip):
    from oracle.oracle import Oracle
    n, N, N1 = 16, 5000, 4000
    stream = cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, 851)
    ids = stream_ids(N)
    o, h = Oracle(n), pkg.Hashgraph(n)
    for d in (o, h):
        d.append_events(cr[:N1], sp[:N1], op[:N1], t[:N1], sig[:N1])
        d.divide_rounds(0, N1)
    nco = list(o.decide_fame())
    txo = list(o.find_order(nco))
    nc = list(h.decide_fame())
    assert nc == nco and list(h.find_order(nc)) == txo
    h.set_event_ids(0, ids[:N1])

    def snapshot():
        c = h.counters()
        c.pop("kernel_launches")
        return (h.rounds().tobytes(), h.witnesses().tobytes(), h.famous().tobytes(), h.consensus().tobytes(), h.transactions().tobytes(),
                h.heights().tobytes(), h.payload_stats(), c, h.num_events, h.max_round)

    before = snapshot()
    g = mg.Graph(n, cr[:N1], sp[:N1], op[:N1], t[:N1], sig[:N1], ids[:N1])
    out = Out(hip, N1)
    d_known = hip.alloc(4 * n)
    rng = np.random.default_rng(5)
    for _ in range(6):
        head, asker = int(rng.integers(n, N1)), int(rng.integers(0, N1))
        h.known_heights_device(asker, d_known)
        K, got = dev_export(h, out, head, d_known)
        same(got, g.export(head, g.known_heights(asker)), "export")
        same(h.export_payload(head, g.known_heights(asker)), g.export(head, g.known_heights(asker)), "export (host)")
    h.export_payload(N1 - 1)
    assert snapshot() == before
    # ... and the voting goes on as if nothing had happened
    for d in (o, h):
        d.append_events(cr[N1:], sp[N1:], op[N1:], t[N1:], sig[N1:])
        d.divide_rounds(N1, N - N1)
    nco = list(o.decide_fame())
    nc = list(h.decide_fame())
    assert nc == nco and list(h.find_order(nc)) == list(o.find_order(nco))
    assert np.array_equal(h.rounds(), o.round) and np.array_equal(h.heights(), o.height)
    ow = o.witnesses()
    assert np.array_equal(h.witnesses(), ow) and np.array_equal(h.famous()[ow >= 0], o.famous_by_event[ow[ow >= 0]])
    assert [int(x) for x in h.transactions()] == list(o.transactions)
    h.close()
