"""GPU (-m gpu): the entry protocol of the device-array call forms (every sw_*_device entry point, sw_export_rows and
sw_import_rows), one table row each, on a hashgraph of 4 members and 40 events, with K in {0, 1, 3} events a call:

1. K = 0 (or, for the forms whose count is a capacity, capacity 0) returns what the row says and writes only what it says;
2. a host (numpy) pointer in place of each array in turn is refused with SW_EINVAL (-22);
3. each array the form wants aligned, moved by half its alignment, is refused with -22 and the word "aligned";
4. a valid call on a stream of the caller's, its outputs read back by copies enqueued on that SAME stream and nothing but
   that stream synchronised, gives byte for byte what the host-array form gives (outputs, counts, and the state left behind).

No torch here (see tests/test_gpu_ingest_device.py): device buffers and streams come through ctypes from the HIP runtime the
library is linked against."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_export import Hip, stream_ids
from test_gpu_sign import keypairs, signer

pytestmark = pytest.mark.gpu

H2D, D2H = 1, 2
EINVAL, ERANGE = -22, -34
POISON = 0xA5
N_MEMBERS, N_EVENTS, N_ORDERED = 4, 40, 400


class Dev(Hip):
    """Hip with a stream of the caller's."""

    def __init__(self, pkg):
        super().__init__(pkg)
        L = self.L
        L.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        L.hipStreamDestroy.argtypes = [C.c_void_p]
        L.hipStreamSynchronize.argtypes = [C.c_void_p]
        L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        s = C.c_void_p()
        assert L.hipStreamCreate(C.byref(s)) == 0
        self.stream = s

    def read_on_stream(self, ptrs):
        """{name: (address, bytes)} -> {name: uint8 array}: copies enqueued on the stream, then the stream alone synchronised."""
        out = {k: np.empty(nb, np.uint8) for k, (_, nb) in ptrs.items()}
        for k, (p, nb) in ptrs.items():
            assert self.L.hipMemcpyAsync(out[k].ctypes.data_as(C.c_void_p), C.c_void_p(p), nb, D2H, self.stream) == 0
        assert self.L.hipStreamSynchronize(self.stream) == 0
        return out

    def free(self):
        super().free()
        if self.stream is not None:
            self.L.hipStreamDestroy(self.stream)
            self.stream = None


@pytest.fixture
def dev(pkg):
    d = Dev(pkg)
    yield d
    d.free()


class World:
    """One signed hashgraph with data, divided and ordered (context A), and its events as the arrays a payload call takes."""

    def __init__(self, pkg):
        n, N = N_MEMBERS, N_EVENTS
        self.pkg, self.n, self.N = pkg, n, N
        self.cr, self.sp, self.op, self.t, _ = pkg.synth_hashgraph(n, N, 77)
        self.d = [None if e % 4 == 3 else bytes([e + 1]) * (e % 5 + 1) for e in range(N)]
        self.seeds, self.kps = keypairs(pkg, n, 77)
        A = self.A = self.signing()
        assert A.create_events(self.cr, self.sp, self.op, self.t, self.d) == 0
        A.divide_rounds(0, N)
        # (4 members decide their first rounds behind some 250 events: the ordered stream comes from a longer, unsigned hashgraph)
        O = self.O = self.bare()
        O.append_events(*pkg.synth_hashgraph(n, N_ORDERED, 78))
        O.set_event_ids(0, stream_ids(N_ORDERED))
        O.divide_rounds(0, N_ORDERED)
        O.find_order(O.decide_fame())
        self.n_ordered = O.num_ordered
        self.x = A.export_walk(N - 1, data=True)
        self.known = np.ascontiguousarray(A.known_heights(N // 3), np.int32)
        self.trunks = np.ascontiguousarray(A.fork_trunks(), np.int32)

    def bare(self):
        return self.pkg.Hashgraph(self.n)

    def keyed(self):
        h = self.bare()
        assert h.set_member_keys([pk for pk, _ in self.kps]) == 0
        return h

    def signing(self):
        return signer(self.pkg, self.n, self.seeds, self.kps)

    def payload(self, K):
        """The first K events of the export (ascending dense index: closed under parents), and their data."""
        x = self.x
        p = {k: np.ascontiguousarray(x[k][:K]) for k in ("ids", "sp_ids", "op_ids", "arity", "creator", "t", "sig")}
        p["data_off"] = np.ascontiguousarray(x["data_off"][:K + 1], np.int64)
        p["data"] = np.ascontiguousarray(x["data"][:int(p["data_off"][K])], np.uint8)
        p["data_none"] = np.ascontiguousarray(x["data_none"][:K], np.uint8)
        p["ok"] = np.ones(K, np.uint8)
        return p

    def packed(self, K):
        """sw_pack_events of payload(K) on A: the signed bytes and the whole events, with their offsets."""
        A, p = self.A, self.payload(K)
        bm, bw = C.c_int64(), C.c_int64()
        assert A._L.sw_pack_bound(A._h, K, len(p["data"]), C.byref(bm), C.byref(bw)) == 0
        o = dict(msgs=np.zeros(bm.value + 16, np.uint8), msg_off=np.zeros(K + 1, np.int64), whole=np.zeros(bw.value + 16, np.uint8),
                 whole_off=np.zeros(K + 1, np.int64), enc=np.zeros(max(K, 1), np.uint8))
        tm, tw = C.c_int64(), C.c_int64()
        rc = A._L.sw_pack_events(A._h, K, *[_np(p[k]) for k in ("sp_ids", "op_ids", "arity", "creator", "t", "sig", "data", "data_off")],
                                 len(p["data"]), _np(p["data_none"]), _np(o["msgs"]), _np(o["msg_off"]), bm.value, _np(o["whole"]), _np(o["whole_off"]),
                                 bw.value, _np(o["enc"]), C.byref(tm), C.byref(tw))
        assert rc == 0, _err(A)
        o["msgs"], o["whole"] = o["msgs"][:max(tm.value, 1)].copy(), o["whole"][:max(tw.value, 1)].copy()
        return o, tm.value, tw.value, bm.value, bw.value

    def message(self, K):
        """sw_pack_message of payload(K) on A, the head the last of them (K = 0: the first event)."""
        A, p = self.A, self.payload(K)
        head = np.ascontiguousarray(self.x["ids"][max(K - 1, 0)])
        bound = C.c_int64()
        assert A._L.sw_pack_message_bound(A._h, K, len(p["data"]), C.byref(bound)) == 0
        msg, ln = np.zeros(bound.value, np.uint8), C.c_int64()
        rc = A._L.sw_pack_message(A._h, K, _np(head), *[_np(p[k]) for k in ("ids", "sp_ids", "op_ids", "arity", "creator", "t", "sig", "data", "data_off")],
                                  len(p["data"]), _np(p["data_none"]), _np(msg), bound.value, C.byref(ln))
        assert rc == 0, _err(A)
        return msg[:ln.value].copy(), bound.value


@pytest.fixture(scope="module")
def world(pkg):
    w = World(pkg)
    yield w
    w.A.close()
    w.O.close()


def _np(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)


def _err(h):
    return (h._L.sw_last_error(h._h) or b"").decode()


def state(h):
    """What a call that stores events leaves behind."""
    N = h.num_events
    ds = h.data_stats()
    ids = h.event_ids().tobytes() if N and h._L.sw_get_event_ids(h._h, 0, N, _np(np.empty((N, 32), np.uint8))) == 0 else b""
    data = tuple(a.tobytes() for a in h.get_event_data()) if ds["events"] else ()
    return N, h.heights().tobytes() if N else b"", ids, ds["events"], ds["bytes"], data


class Arr:
    """One array of a call: its initial bytes (outputs: poison), the alignment the form checks (0: none), whether the form
    checks that it lies in device memory."""

    def __init__(self, init, align=0, out=False, resident=True, nbytes=None):
        if init is None:
            init = np.full(nbytes, POISON, np.uint8)
        self.host = np.ascontiguousarray(init).view(np.uint8).reshape(-1).copy()
        self.align, self.out, self.resident = align, out, resident


def Out(nbytes, align=0, resident=True):
    return Arr(None, align, True, resident, max(int(nbytes), 16))


class Scalars:
    """The int64 results a form returns through pointers, by name."""

    def __init__(self):
        self.v = {}

    def __call__(self, name):
        self.v[name] = C.c_int64(-77)
        return C.byref(self.v[name])

    def values(self):
        return {k: int(x.value) for k, x in self.v.items()}


class Case:
    """dev / host: the two symbols; ctx: a fresh context for each (None: the world's A, which the call does not change; a
    Hashgraph: that one);
    arrays: {name: Arr}; dev_args / host_args: (pointers by name, Scalars[, stream]) -> the arguments behind the context;
    rc: what both return; prefix: {array: results -> bytes that count} (default: all of it); zero: the K = 0 expectation,
    (rc, {array: bytes at its front}, {scalar: value}) with every other output byte still poison; after: context -> what it
    left behind, compared between the forms; check: (device outputs, the host form's results) -> bool, for what only the
    device form writes."""

    def __init__(self, dev, host, arrays, dev_args, host_args, ctx=None, rc=0, prefix=None, zero=None, after=None, check=None):
        self.dev, self.host, self.arrays, self.dev_args, self.host_args = dev, host, arrays, dev_args, host_args
        self.ctx, self.rc, self.prefix, self.zero, self.after, self.check = ctx, rc, prefix or {}, zero, after, check


# ---- the table: one function per entry point, (world, K) -> Case ---------------------------------------------------------------
def row_append(W, K):
    a = dict(cr=Arr(W.cr[:K]), sp=Arr(W.sp[:K]), op=Arr(W.op[:K]), t=Arr(W.t[:K]), sig=Arr(W.x["sig"][:K]))
    order = ("cr", "sp", "op", "t", "sig")
    return Case("sw_append_events_device", "sw_append_events", a, lambda p, S, s: [K] + [p[k] for k in order] + [s],
                lambda p, S: [K] + [p[k] for k in order], ctx=W.bare, after=state, zero=(0, {}, {}))


PAYLOAD = ("ids", "sp_ids", "op_ids", "arity", "creator", "ok", "t", "sig")


def payload_arrays(W, K, align):
    p = W.payload(K)
    a = {k: Arr(p[k], align if k in ("ids", "sp_ids", "op_ids") else 0) for k in PAYLOAD}
    a["index"] = Out(4 * K)
    return p, a


def row_ingest_payload(W, K):
    _, a = payload_arrays(W, K, 8)
    return Case("sw_ingest_payload_device", "sw_ingest_payload", a, lambda p, S, s: [K] + [p[k] for k in PAYLOAD] + [s, p["index"], S("n_stored")],
                lambda p, S: [K] + [p[k] for k in PAYLOAD] + [p["index"], S("n_stored")], ctx=W.bare, after=state, zero=(0, {}, {"n_stored": 0}))


def row_ingest_payload_data(W, K):
    pl, a = payload_arrays(W, K, 8)
    a.update(data=Arr(pl["data"]), data_off=Arr(pl["data_off"], 8), data_none=Arr(pl["data_none"]))
    nb = len(pl["data"])
    tail = lambda p: [p["data"], p["data_off"], nb, p["data_none"]]
    return Case("sw_ingest_payload_data_device", "sw_ingest_payload_data", a,
                lambda p, S, s: [K] + [p[k] for k in PAYLOAD] + [s, p["index"], S("n_stored")] + tail(p),
                lambda p, S: [K] + [p[k] for k in PAYLOAD] + [p["index"], S("n_stored")] + tail(p), ctx=W.keyed, after=state,
                zero=(0, {}, {"n_stored": 0}))


def row_known_heights(W, K):
    head = W.N - 1 - K
    return Case("sw_get_known_heights_device", "sw_get_known_heights", dict(out=Out(4 * W.n)), lambda p, S, s: [head, p["out"], s],
                lambda p, S: [head, p["out"]], prefix={"out": lambda r: 4 * W.n})


EXPORT = ("ids", "sp_ids", "op_ids", "arity", "creator", "t", "sig", "event")
EXPORT_WIDTH = dict(ids=32, sp_ids=32, op_ids=32, arity=1, creator=4, t=8, sig=64, event=4)


def export_arrays(cap):
    return {k: Out(cap * EXPORT_WIDTH[k], 16 if k in ("ids", "sp_ids", "op_ids", "sig") else 0) for k in EXPORT}


def row_export_payload(W, K):
    cap = W.N if K else 0
    a = dict(known=Arr(W.known), **export_arrays(cap))
    head = W.N - 1
    total = len(W.A.export_payload(head, W.known)["event"])
    return Case("sw_export_payload_device", "sw_export_payload", a, lambda p, S, s: [head, p["known"], cap] + [p[k] for k in EXPORT] + [s, S("n_out")],
                lambda p, S: [head, p["known"], cap] + [p[k] for k in EXPORT] + [S("n_out")], zero=(ERANGE, {}, {"n_out": total}))


def row_export_walk(W, K):
    cap = W.N if K else 0
    a = dict(known=Arr(W.known), trunks=Arr(W.trunks), **export_arrays(cap))
    head = W.N - 1
    total = len(W.A.sync_walk(head, W.known, W.trunks))
    return Case("sw_export_walk_device", "sw_export_walk", a,
                lambda p, S, s: [head, p["known"], p["trunks"], cap] + [p[k] for k in EXPORT] + [s, S("n_out")],
                lambda p, S: [head, p["known"], p["trunks"], cap] + [p[k] for k in EXPORT] + [S("n_out")], zero=(ERANGE, {}, {"n_out": total}))


def row_export_ordered(W, K):
    assert W.n_ordered >= 4, "the world orders too few events for this row"
    a = dict(event=Out(4 * K), ids=Out(32 * K, 16), creator=Out(4 * K), rr=Out(4 * K), time=Out(8 * K))
    order = ("event", "ids", "creator", "rr", "time")
    return Case("sw_export_ordered_device", "sw_export_ordered", a, lambda p, S, s: [1, K] + [p[k] for k in order] + [s],
                lambda p, S: [1, K] + [p[k] for k in order], ctx=W.O, zero=(0, {}, {}))


def row_validate(W, K):
    pl = W.payload(K)
    o, tm, tw, _, _ = W.packed(K)
    a = dict(msgs=Arr(o["msgs"]), msg_off=Arr(o["msg_off"], 8), whole=Arr(o["whole"]), whole_off=Arr(o["whole_off"], 8), sig=Arr(pl["sig"]),
             creator=Arr(pl["creator"]), ids=Arr(pl["ids"], 8), ok=Out(K))
    args = lambda p: [K, p["msgs"], p["msg_off"], tm, p["whole"], p["whole_off"], tw, p["sig"], p["creator"], p["ids"], p["ok"]]
    return Case("sw_validate_payload_device", "sw_validate_payload", a, lambda p, S, s: args(p) + [s], lambda p, S: args(p), zero=(0, {}, {}))


def row_pack_events(W, K):
    pl = W.payload(K)
    _, tm, tw, bm, bw = W.packed(K)
    ins = ("sp_ids", "op_ids", "arity", "creator", "t", "sig", "data", "data_off")
    al = dict(sp_ids=16, op_ids=16, sig=16, t=8, data_off=8, creator=4)
    a = {k: Arr(pl[k], al.get(k, 0)) for k in ins + ("data_none",)}
    a.update(msgs=Out(bm + 16, 16), msg_off=Out(8 * (K + 1), 8), whole=Out(bw + 16, 16), whole_off=Out(8 * (K + 1), 8), enc=Out(K))
    nb = len(pl["data"])
    args = lambda p: [K] + [p[k] for k in ins] + [nb, p["data_none"], p["msgs"], p["msg_off"], bm, p["whole"], p["whole_off"], bw, p["enc"]]
    return Case("sw_pack_events_device", "sw_pack_events", a, lambda p, S, s: args(p) + [s], lambda p, S: args(p) + [S("tm"), S("tw")],
                prefix={"msgs": lambda r: tm, "whole": lambda r: tw, "msg_off": lambda r: 8 * (K + 1), "whole_off": lambda r: 8 * (K + 1), "enc": lambda r: K},
                zero=(0, {"msg_off": bytes(8), "whole_off": bytes(8)}, {}))


def row_set_event_data(W, K):
    pl = W.payload(K)
    a = dict(data=Arr(pl["data"]), data_off=Arr(pl["data_off"], 8), data_none=Arr(pl["data_none"]))
    nb = len(pl["data"])

    def ctx():
        h = W.bare()
        h.append_events(W.cr[:3], W.sp[:3], W.op[:3], W.t[:3])
        return h
    args = lambda p: [0, K, p["data"], p["data_off"], nb, p["data_none"]]
    return Case("sw_set_event_data_device", "sw_set_event_data", a, lambda p, S, s: args(p) + [s], lambda p, S: args(p), ctx=ctx, after=state, zero=(0, {}, {}))


def row_gather_event_data(W, K):
    ev = np.array([5, 0, 9][:K], np.int32)
    total = int(sum(len(W.d[e] or b"") for e in ev))
    cap = total + 16
    a = dict(event=Arr(ev, 4) if K else Arr(np.zeros(1, np.int32), 4), data=Out(cap, 16), data_off=Out(8 * (K + 1), 8), data_none=Out(K))
    return Case("sw_gather_event_data_device", "sw_gather_event_data", a,
                lambda p, S, s: [K, p["event"], cap, p["data"], p["data_off"], p["data_none"], s, S("n_bytes")],
                lambda p, S: [K, p["event"], cap, p["data"], p["data_off"], p["data_none"], S("n_bytes")],
                prefix={"data": lambda r: total, "data_off": lambda r: 8 * (K + 1), "data_none": lambda r: K},
                zero=(0, {"data_off": bytes(8)}, {"n_bytes": 0}))


WIRE = ("ids", "sp_ids", "op_ids", "arity", "creator", "t", "sig", "data", "data_off")


def row_pack_message(W, K):
    pl = W.payload(K)
    want, bound = W.message(K)
    al = dict(ids=16, sp_ids=16, op_ids=16, sig=16, t=8, data_off=8, creator=4)
    a = {k: Arr(pl[k], al.get(k, 0)) for k in WIRE + ("data_none",)}
    a.update(head=Arr(W.x["ids"][max(K - 1, 0)]), msg=Out(bound + 16, 16), msg_len=Out(8, 8))
    nb = len(pl["data"])
    args = lambda p: [K, p["head"]] + [p[k] for k in WIRE] + [nb, p["data_none"], p["msg"], bound]
    return Case("sw_pack_message_device", "sw_pack_message", a, lambda p, S, s: args(p) + [p["msg_len"], s], lambda p, S: args(p) + [S("msg_bytes")],
                prefix={"msg": lambda r: len(want), "msg_len": lambda r: 0},
                check=lambda got, r: int(got["msg_len"][:8].view(np.int64)[0]) == r["msg_bytes"] == len(want), zero=(0, {"msg": want.tobytes(), "msg_len": np.int64(len(want)).tobytes()}, {}))


UNPACK = ("head", "ids", "sp_ids", "op_ids", "arity", "creator", "t", "sig", "data", "data_off", "data_none")


def row_unpack_message(W, K):
    msg, _ = W.message(K)
    nd = len(W.payload(K)["data"])
    width = dict(head=32, ids=32 * K, sp_ids=32 * K, op_ids=32 * K, arity=K, creator=4 * K, t=8 * K, sig=64 * K, data=nd + 16, data_off=8 * (K + 1), data_none=K)
    al = dict(data=16, data_off=8, t=8, creator=4)
    a = {k: Out(w, al.get(k, 0)) for k, w in width.items()}
    a["msg"] = Arr(msg)
    args = lambda p: [p["msg"], len(msg), K, nd + 16] + [p[k] for k in UNPACK]
    width["data"] = nd
    return Case("sw_unpack_message_device", "sw_unpack_message", a, lambda p, S, s: args(p) + [s, S("n_events"), S("n_data")],
                lambda p, S: args(p) + [S("n_events"), S("n_data")], prefix={k: (lambda r, w=w: w) for k, w in width.items()})


def row_export_message(W, K):
    head, cap = W.N - 1 - K, 1 << 16
    a = dict(known=Arr(W.known), trunks=Arr(W.trunks), msg=Out(cap))
    return Case("sw_export_message_device", "sw_export_message", a,
                lambda p, S, s: [head, p["known"], p["trunks"], 1, p["msg"], cap, s, S("msg_bytes"), S("n_events")],
                lambda p, S: [head, p["known"], p["trunks"], 1, p["msg"], cap, S("msg_bytes"), S("n_events")])


def row_ingest_message(W, K):
    msg, _ = W.message(K)
    a = dict(msg=Arr(msg), head=Out(32), index=Out(4 * len(msg)))
    return Case("sw_ingest_message_device", "sw_ingest_message", a,
                lambda p, S, s: [p["msg"], len(msg), 1, 1, p["head"], p["index"], s, S("n_events"), S("n_valid"), S("n_stored")],
                lambda p, S: [p["msg"], len(msg), 1, 1, p["head"], p["index"], S("n_events"), S("n_valid"), S("n_stored")], ctx=W.keyed, after=state,
                prefix={"head": lambda r: 32, "index": lambda r: 4 * K})


def sign_inputs(W, K):
    data, off, none = W.pkg.Hashgraph.pack_data(W.d[:K])
    a = dict(cr=Arr(W.cr[:K], 4), sp=Arr(W.sp[:K], 4), op=Arr(W.op[:K], 4), t=Arr(W.t[:K], 8), data=Arr(data), data_off=Arr(off, 8), data_none=Arr(none))
    return a, len(data)


SIGN_IN = ("cr", "sp", "op", "t", "data", "data_off")


def row_sign_events(W, K):
    a, nb = sign_inputs(W, K)
    a.update(ids=Out(32 * K, 16), sp_ids=Out(32 * K, 16), op_ids=Out(32 * K, 16), arity=Out(K), sig=Out(64 * K, 16))
    args = lambda p: [K] + [p[k] for k in SIGN_IN] + [nb, p["data_none"]] + [p[k] for k in ("ids", "sp_ids", "op_ids", "arity", "sig")]
    return Case("sw_sign_events_device", "sw_sign_events", a, lambda p, S, s: args(p) + [s], lambda p, S: args(p), ctx=W.signing, after=state, zero=(0, {}, {}))


def row_create_events(W, K):
    a, nb = sign_inputs(W, K)
    a.update(ids=Out(32 * K, 16), sig=Out(64 * K, 16))
    args = lambda p: [K] + [p[k] for k in SIGN_IN] + [nb, p["data_none"]]
    return Case("sw_create_events_device", "sw_create_events", a, lambda p, S, s: args(p) + [s, S("first"), p["ids"], p["sig"]],
                lambda p, S: args(p) + [S("first"), p["ids"], p["sig"]], ctx=W.signing, after=state, zero=(0, {}, {"first": 0}))


ROWS = [row_append, row_ingest_payload, row_ingest_payload_data, row_known_heights, row_export_payload, row_export_walk, row_export_ordered,
        row_validate, row_pack_events, row_set_event_data, row_gather_event_data, row_pack_message, row_unpack_message, row_export_message,
        row_ingest_message, row_sign_events, row_create_events]
# the forms whose K = 0 is a call like any other (an empty message is a message)
NO_ZERO = (row_known_heights, row_unpack_message, row_export_message, row_ingest_message)


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def on_device(dev, case):
    """Every array of the case in device memory, with room for a misaligned start: {name: address}."""
    ptr = {}
    for k, a in case.arrays.items():
        base = dev.alloc(a.host.nbytes + 64)
        assert dev.L.hipMemcpy(C.c_void_p(base), a.host.ctypes.data_as(C.c_void_p), a.host.nbytes, H2D) == 0
        ptr[k] = base
    return ptr


def contexts(W, case):
    if case.ctx is None or not callable(case.ctx):
        h = case.ctx or W.A
        return h, h, lambda: None
    hh, hd = case.ctx(), case.ctx()
    return hh, hd, lambda: (hh.close(), hd.close())


def call(h, name, args):
    return getattr(h._L, name)(h._h, *args)


@pytest.mark.parametrize("row,K", [(r, K) for r in ROWS for K in ((0, 1, 3) if r in NO_ZERO else (1, 3))], ids=lambda v: v.__name__[4:] if callable(v) else str(v))
def test_device_form_on_a_stream_equals_the_host_form(pkg, dev, world, row, K):
    case = row(world, K)
    hh, hd, close = contexts(world, case)
    try:
        host = {k: a.host.copy() for k, a in case.arrays.items()}
        Sh, Sd = Scalars(), Scalars()
        rc = call(hh, case.host, case.host_args({k: v.ctypes.data for k, v in host.items()}, Sh))
        assert rc == case.rc, _err(hh)
        ptr = on_device(dev, case)
        rc = call(hd, case.dev, case.dev_args(ptr, Sd, dev.stream))
        assert rc == case.rc, _err(hd)
        got = dev.read_on_stream({k: (ptr[k], a.host.nbytes) for k, a in case.arrays.items() if a.out})
        res = Sh.values()
        for k in got:
            nb = case.prefix[k](res) if k in case.prefix else len(got[k])
            assert got[k][:nb].tobytes() == host[k][:nb].tobytes(), k
        for k, v in Sd.values().items():
            assert v == res[k], k
        assert case.check is None or case.check(got, res)
        if case.after:
            assert case.after(hd) == case.after(hh)
    finally:
        close()


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.__name__[4:])
def test_host_pointers_and_misaligned_arrays_are_refused(pkg, dev, world, row):
    case = row(world, 3)
    _, hd, close = contexts(world, case)
    try:
        before = state(hd)
        ptr = on_device(dev, case)
        for k, a in case.arrays.items():
            if a.resident:
                bad = dict(ptr)
                bad[k] = a.host.ctypes.data
                assert call(hd, case.dev, case.dev_args(bad, Scalars(), dev.stream)) == EINVAL, "a host pointer for " + k
            if a.align:
                bad = dict(ptr)
                bad[k] = ptr[k] + a.align // 2
                assert call(hd, case.dev, case.dev_args(bad, Scalars(), dev.stream)) == EINVAL, "misaligned " + k
                assert "aligned" in _err(hd), k
        assert state(hd) == before
        got = dev.read_on_stream({k: (ptr[k], a.host.nbytes) for k, a in case.arrays.items() if a.out})
        assert all((v == POISON).all() for v in got.values()), "a refused call wrote to its outputs"
    finally:
        close()


@pytest.mark.parametrize("row", [r for r in ROWS if r not in NO_ZERO], ids=lambda r: r.__name__[4:])
def test_no_events(pkg, dev, world, row):
    case = row(world, 0)
    rc_want, front, scalars = case.zero
    _, hd, close = contexts(world, case)
    try:
        before = state(hd)
        ptr = on_device(dev, case)
        S = Scalars()
        assert call(hd, case.dev, case.dev_args(ptr, S, dev.stream)) == rc_want, _err(hd)
        got = dev.read_on_stream({k: (ptr[k], a.host.nbytes) for k, a in case.arrays.items() if a.out})
        for k, v in got.items():
            f = front.get(k, b"")
            assert v[:len(f)].tobytes() == f and (v[len(f):] == POISON).all(), k
        res = S.values()
        for k, v in scalars.items():
            assert res[k] == v, k
        assert state(hd) == before
    finally:
        close()


# ---- sw_export_rows / sw_import_rows: the bracket is around the stream of the can_see sweeps ----------------------------------
@pytest.mark.parametrize("K", [1, 3])
def test_rows_travel_on_the_callers_stream(pkg, dev, world, K):
    W, A = world, world.A
    stride = A.row_stride
    nb = K * stride * 4
    d_rows = dev.alloc(nb)
    dev.fill(d_rows, POISON, nb)
    assert call(A, "sw_export_rows", [2, K, d_rows, dev.stream]) == 0, _err(A)
    rows = dev.read_on_stream({"rows": (d_rows, nb)})["rows"].view(np.int32).reshape(K, stride)
    assert np.array_equal(rows[:, :W.n], A.can_see(2, K))
    # the rows of the first K events into a context that has not divided them: it then divides from the imported rows
    d_first = dev.alloc(nb)
    assert call(A, "sw_export_rows", [0, K, d_first, dev.stream]) == 0, _err(A)
    B = W.bare()
    try:
        B.append_events(W.cr, W.sp, W.op, W.t)
        assert call(B, "sw_import_rows", [0, K, d_first, dev.stream]) == 0, _err(B)
        assert dev.L.hipStreamSynchronize(dev.stream) == 0
        B.divide_rounds(0, K)
        assert np.array_equal(B.can_see(0, K), A.can_see(0, K)) and np.array_equal(B.rounds(0, K), A.rounds(0, K))
        assert call(B, "sw_import_rows", [0, K, d_first, dev.stream]) == EINVAL      # divided already
    finally:
        B.close()
