"""GPU (-m gpu): the wire bytes of a sync answer built and parsed on the device (sw_pack_message[_device],
sw_unpack_message[_device], sw_export_message, sw_ingest_message; csrc/wire.hip.h).  The writer's bytes equal
tests/model_wire.py's; pickle.loads of an exported message is (head id, {id: Event}) of export_walk of the same context, on
the fast and on the exact path, with and without data; a message ingested with validation leaves what a validated pull by
the walk leaves on a twin; the malformed messages that passed the host emulation (tests/test_wire_kernels_host.py) are
refused and leave both contexts as they were; walk_pre's refusals hold for export_message."""
import pickle

import numpy as np
import pytest

import model_pack as mp
import model_wire as mw
from test_gpu_export import Hip, stream_ids
from test_gpu_sign import keypairs, signer
from test_gpu_walk import context, graph, refused
from test_wire_kernels_host import events, model, refusal_cases, sample, with_data

pytestmark = pytest.mark.gpu


@pytest.fixture
def hip(pkg):
    h = Hip(pkg)
    yield h
    h.free()


def ctx(pkg, keys, mod="swirld", qual="Event"):
    h = pkg.Hashgraph(len(keys))
    h.set_member_keys(keys)
    h.set_event_class(mod, qual)
    return h


def pack(h, a):
    return h.pack_message(a["head"], a["ids"], a["sp"], a["op"], a["arity"], a["creator"], a["t"], a["sig"], a.get("data"), a.get("data_off"),
                          a.get("data_none"))


def pack_device(h, hip, a):
    """pack_message_device between device arrays, the message buffer poisoned first: (msg_len, the whole buffer)."""
    K = len(a["arity"])
    nbytes = len(a["data"]) if "data_off" in a else 0
    cap = h.pack_message_bound(K, nbytes) + 48
    up = {k: hip.up(a[k], dt) for k, dt in (("head", np.uint8), ("ids", np.uint8), ("sp", np.uint8), ("op", np.uint8), ("arity", np.uint8),
                                             ("creator", np.int32), ("t", np.float64), ("sig", np.uint8))}
    d = {k: hip.up(a[k], dt) if k in a else None for k, dt in (("data", np.uint8), ("data_off", np.int64), ("data_none", np.uint8))}
    d_msg, d_len = hip.alloc(cap), hip.alloc(8)
    hip.fill(d_msg, 0xA5, cap)
    hip.fill(d_len, 0x77, 8)
    h.pack_message_device(up["head"], up["ids"], up["sp"], up["op"], up["arity"], up["creator"], up["t"], up["sig"], d_msg, cap, d_len,
                          data=d["data"] if nbytes else None, data_off=d["data_off"], data_bytes=nbytes, data_none=d["data_none"], count=K)
    h.synchronize()
    return int(hip.down(d_len, 1, np.int64)[0]), hip.down(d_msg, cap, np.uint8)


# ---- 1. the writer against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 70])
def test_pack_message_equals_the_model(pkg, hip, n):
    shapes = [events(K, n, 10 + K, roots) for K in (0, 1, 2, 65, 1000, 1025, 2049) for roots in ((0.4,) if K > 100 else (1.0, 0.0, 0.4))]
    lens = [0, 1, 31, 32, 255, 256, 257, 4095, 60000, 5, 0]
    none = np.zeros(len(lens), np.uint8)
    none[[2, 9]] = 1
    shapes += [with_data(events(len(lens), n, 6, r), lens, 7, none) for r in (0.0, 1.0)] + [with_data(events(len(lens), n, 8), lens, 9)]
    h = ctx(pkg, shapes[0]["keys"], "py-swirld_amd.node", "Event")
    for a in shapes:
        a["keys"] = shapes[0]["keys"]
        want = model(a, "py-swirld_amd.node", "Event")
        assert pack(h, a) == want
        ln, buf = pack_device(h, hip, a)
        assert ln == len(want) and buf[:ln].tobytes() == want
        assert (buf[ln:] == 0xA5).all(), "bytes at or behind the message's end were written"
    h.set_event_class("m", "Q")                       # the class is a setting: the next message carries the new one
    assert pack(h, shapes[3]) == model(shapes[3], "m", "Q")
    h.close()


def test_a_message_longer_than_one_trip_of_the_grid(pkg, hip, monkeypatch):
    a = with_data(events(1500, 5, 21, 0.2), [(7 * i) % 300 for i in range(1500)], 22, [i % 5 == 0 for i in range(1500)])
    monkeypatch.setenv("SW_WIRE_BLOCKS", "2")         # 2 workgroups x 256 chunks x 16 bytes a trip: some 50 trips
    h = ctx(pkg, a["keys"])
    monkeypatch.delenv("SW_WIRE_BLOCKS")
    want = model(a)
    assert len(want) > 40 * 2 * 256 * 16
    ln, buf = pack_device(h, hip, a)
    assert ln == len(want) and buf[:ln].tobytes() == want and (buf[ln:] == 0xA5).all()
    h.close()


def test_one_unencodable_event_and_no_message(pkg, hip):
    a = with_data(events(200, 6, 11), [10] * 200, 12)
    h = ctx(pkg, a["keys"])
    for field, idx, val in (("arity", 100, 3), ("creator", 5, -1), ("creator", 64, 6), ("data_off", 150, 10 ** 12)):
        b = {k: v.copy() for k, v in a.items()}
        b[field][idx] = val
        first = -model(b) - 1
        with pytest.raises(pkg.SwirldHipError) as ei:
            pack(h, b)
        assert ei.value.code == -22 and "event %d " % first in str(ei.value)
        ln, buf = pack_device(h, hip, b)
        assert ln == -1 and (buf == 0xA5).all(), "an unbuildable message was written"
    assert pack(h, a) == model(a)
    h.close()


# ---- 2. the reader ----------------------------------------------------------------------------------------------------------
def test_unpack_message_returns_the_arrays(pkg, hip):
    a = sample(1025)
    a["keys"][3] = a["keys"][1]
    h = ctx(pkg, a["keys"], "m", "Q")
    msg = model(a, "m", "Q")
    want = mw.unpack_message(msg, a["keys"], "m", "Q")
    got = h.unpack_message(msg)
    names = dict(ids="ids", sp_ids="sp", op_ids="op")
    for k, v in got.items():
        assert v.tobytes() == want[names.get(k, k)].tobytes(), k
    assert (got["creator"] != 3).all() and (got["creator"] == 1).any()
    # the device form, exact capacities, the outputs poisoned
    K, nd = 1025, len(a["data"])
    width = dict(head=32, ids=32 * K, sp_ids=32 * K, op_ids=32 * K, arity=K, creator=4 * K, t=8 * K, sig=64 * K, data=nd, data_off=8 * (K + 1), data_none=K)
    p = {k: hip.alloc(w) for k, w in width.items()}
    for k, w in width.items():
        hip.fill(p[k], 0xA5, w)
    d_msg = hip.up(np.frombuffer(msg, np.uint8), np.uint8, offset=3) # (no alignment is asked of the message)
    assert h.unpack_message_device(d_msg, len(msg), K, nd, *[p[k] for k in width]) == (K, nd)
    for k, w in width.items():
        assert hip.down(p[k], w, np.uint8).tobytes() == got[k].tobytes(), k
    # capacities: the sizes that suffice come back
    for ke, kd, code_K, need in ((K - 1, nd, K, None), (K, nd - 1, K, nd), (K, 0, K, nd)):
        n_ev, n_d = mw_unpack_raw(h, msg, ke, kd)
        assert n_ev == (-34, code_K) and (need is None and n_d >= nd or n_d == need)
    assert h.unpack_message(model(a)) is None             # (swirld.Event: another class than "m.Q")
    h.close()


def mw_unpack_raw(h, msg, ke, kd):
    """((rc, n_events), n_data_bytes) of sw_unpack_message with capacities ke, kd."""
    import ctypes as C
    buf = np.frombuffer(msg, np.uint8)
    z = lambda *s: np.zeros(s, np.uint8)
    arrs = [z(32), z(ke, 32), z(ke, 32), z(ke, 32), z(ke), np.zeros(ke, np.int32), np.zeros(ke), z(ke, 64), z(max(kd, 1)), np.zeros(ke + 1, np.int64), z(ke)]
    n, m = C.c_int64(), C.c_int64()
    rc = h._L.sw_unpack_message(h._h, buf.ctypes.data_as(C.c_void_p), len(msg), ke, kd, *[x.ctypes.data_as(C.c_void_p) for x in arrs], C.byref(n), C.byref(m))
    return (rc, int(n.value)), int(m.value)


def state(h):
    """Event count, the ids, the data store's counts."""
    d = h.data_stats()
    return h.num_events, h.event_ids().tobytes(), d["events"], d["bytes"]


def test_refusals_leave_both_contexts_unchanged(pkg):
    a, msg, cases = refusal_cases()
    src, g = graph(pkg, 5, False)
    h = context(pkg, 5, src)
    h.set_member_keys(a["keys"])
    h.set_event_data(0, [None] * g.N)
    before = state(h)
    assert h.unpack_message(msg) is not None
    for name, bad in cases:
        assert h.unpack_message(bad) is None, name
        assert h.ingest_message(bad, validate=True, data=True) is None, name
        assert h.ingest_message(bad, validate=False, data=False) is None, name
    assert h.wire_stats()["refused"] == 3 * len(cases)
    assert state(h) == before
    assert len(h.export_message(g.N - 1)) > 0 and state(h) == before
    h.close()


# ---- 3. export_message: any pickle.loads reads it ----------------------------------------------------------------------------
def loads_equals_export_walk(pkg, h, head, known, cap, data):
    keys = h.member_keys()[0]
    x = h.export_walk(head, known, cap, data=data)
    msg, K = h.export_message(head, known, cap, data=data, want_count=True)
    assert K == len(x["event"])
    with mp.event_class("swirld", "Event") as Event:
        want = {}
        dd = h.unpack_data(x["data"], x["data_off"], x["data_none"]) if data else [None] * K
        for i in range(K):
            p = () if x["arity"][i] == 0 else (x["sp_ids"][i].tobytes(), x["op_ids"][i].tobytes())
            want[x["ids"][i].tobytes()] = Event(dd[i], p, float(x["t"][i]), keys[x["creator"][i]].tobytes(), x["sig"][i].tobytes())
        got = pickle.loads(msg)
        assert got == (h.event_ids(head, 1).tobytes(), want) and list(got[1]) == list(want)
        assert pickle._loads(msg) == got
    assert mw.unpack_message(msg, keys) is not None
    return K


@pytest.mark.parametrize("forked", [False, True])
def test_pickle_loads_reads_an_exported_message(pkg, forked):
    n = 33
    stream, g = graph(pkg, n, forked)
    h = context(pkg, n, stream)
    assert h.exact == forked
    rng = np.random.default_rng(5)
    h.set_member_keys(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    datas = [None if e % 3 == 0 else rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes() for e in range(g.N)]
    h.set_event_data(0, datas)
    N = g.N
    trunk = h.fork_trunks()
    for data in (True, False):
        assert loads_equals_export_walk(pkg, h, N - 1, None, None, data) > N // 2
        assert loads_equals_export_walk(pkg, h, N - 1, h.known_heights(N // 3), trunk, data) > 10
    assert loads_equals_export_walk(pkg, h, 2, None, None, True) == 1          # the head a root
    h.close()


def test_exact_path_by_one_forked_event(pkg):
    """The construction of tests/test_gpu_consensus.py::test_exact_path_is_refused: a fork-free context turns exact by one
    event on the self-parent of a member's newest one."""
    n = 5
    stream, g = graph(pkg, n, False)
    h = context(pkg, n, stream)
    h.set_member_keys(np.arange(n * 32, dtype=np.uint8).reshape(n, 32))
    cr, sp = stream[0], stream[1]
    newest, other = int(np.flatnonzero(cr == 0)[-1]), int(np.flatnonzero(cr == 1)[-1])
    h.append_events(np.array([0], np.int32), np.array([sp[newest]], np.int32), np.array([other], np.int32), np.array([1e6]), np.zeros((1, 64), np.uint8))
    assert h.exact
    h.set_event_ids(g.N, np.full((1, 32), 0xEE, np.uint8))
    h.divide_rounds(g.N, 1)
    h.set_event_data(0, [b"x" * (e % 7) for e in range(g.N + 1)])
    for data in (True, False):
        assert loads_equals_export_walk(pkg, h, g.N, None, None, data) > g.N // 2
    h.close()


# ---- 4. the round trip against a validated pull on a twin --------------------------------------------------------------------
def test_ingest_message_leaves_what_a_validated_pull_leaves(pkg):
    n, N, seed = 5, 400, 905
    cr, sp, op, t, _ = pkg.synth_hashgraph(n, N, seed)
    rng = np.random.default_rng(seed)
    d = [None if e % 4 == 0 else b"" if e % 4 == 1 else rng.integers(0, 256, 300 if e % 4 == 3 else int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
         for e in range(N)]
    seeds, kps = keypairs(pkg, n, seed)
    A = signer(pkg, n, seeds, kps)
    assert A.create_events(cr, sp, op, t, d) == 0
    A.divide_rounds(0, N)
    twins = []
    for _ in range(2):
        B = signer(pkg, n, seeds, kps, members=[int(cr[0])])
        assert B.create_events(cr[:1], sp[:1], op[:1], t[:1], d[:1]) == 0
        B.divide_rounds(0, 1)
        twins.append(B)
    B, B2 = twins
    n_sent, n_valid, n_stored = B2.pull_from(A, N - 1, 0, validate=True, data=True, walk=True)
    before = state(A)
    msg = A.export_message(N - 1, B.known_heights(0), data=True)
    assert state(A) == before
    r = B.ingest_message(msg, validate=True, data=True)
    assert (r["n_events"], r["n_valid"], r["n_stored"]) == (n_sent, n_valid, n_stored) and n_stored > 300
    assert r["head"] == A.event_ids(N - 1, 1).tobytes() and (r["index"] >= 0).sum() == n_stored
    assert B.num_events == B2.num_events == 1 + n_stored
    assert np.array_equal(B.event_ids(), B2.event_ids())
    B.divide_rounds(1, n_stored)
    B2.divide_rounds(1, n_stored)
    xa, xb = B.export_walk(n_stored, data=True), B2.export_walk(n_stored, data=True)
    for k in xa:
        assert xa[k].tobytes() == xb[k].tobytes(), k
    assert B.unpack_data(*B.get_event_data()) == B2.unpack_data(*B2.get_event_data())
    # a forged timestamp inside a canonical message: the message is read, that event and its descendants are not stored
    keys = A.member_keys()[0]
    u = mw.unpack_message(msg, keys)
    u["t"][n_sent // 2] += 1.0
    forged = mw.pack_message(u["head"], keys, u["ids"], u["sp"], u["op"], u["arity"], u["creator"], u["t"], u["sig"], u["data"], u["data_off"],
                             u["data_none"])
    C3 = signer(pkg, n, seeds, kps, members=[int(cr[0])])
    assert C3.create_events(cr[:1], sp[:1], op[:1], t[:1], d[:1]) == 0
    C3.divide_rounds(0, 1)
    r3 = C3.ingest_message(forged, validate=True, data=True)
    assert r3["n_events"] == n_sent and r3["n_valid"] == n_valid - 1 and r3["n_stored"] < n_stored
    for h in (A, B, B2, C3):
        h.close()


# ---- 5. preconditions --------------------------------------------------------------------------------------------------------
def test_export_message_keeps_the_refusals_of_the_walk(pkg):
    n = 5
    stream, g = graph(pkg, n, False)
    N = g.N
    keys = np.arange(n * 32, dtype=np.uint8).reshape(n, 32)
    h = context(pkg, n, stream, ids=False, divided=N - 10)
    refused(pkg, -95, lambda: h.export_message(N - 20, data=False))          # no member keys, no ids
    h.set_member_keys(keys)
    refused(pkg, -95, lambda: h.export_message(N - 20, data=False))          # an incomplete id index
    h.set_event_ids(0, stream_ids(N))
    refused(pkg, -95, lambda: h.export_message(N - 20, data=True))           # an incomplete data store
    refused(pkg, -34, lambda: h.export_message(N - 5, data=False))           # a head that is not divided
    refused(pkg, -34, lambda: h.export_message(N, data=False))
    msg = h.export_message(N - 20, data=False)
    with mp.event_class("swirld", "Event"):
        assert pickle.loads(msg)[0] == h.event_ids(N - 20, 1).tobytes()
    h.close()
    w = pkg.Hashgraph(n)                                                     # the windowed table is out of scope
    w.set_window(True)
    w.append_events(*stream)
    w.set_event_ids(0, stream_ids(N))
    w.divide_rounds(0, N)
    w.set_member_keys(keys)
    refused(pkg, -95, lambda: w.export_message(N - 1, data=False))
    w.close()
