"""CPU: Node._batch_validate's array route (the signed bytes built by Hashgraph.pack_events instead of two dumps per event)
with the device backend swapped for the CPU oracle plus tests/model_pack.py — the host glue of node.py: the plain-event
predicate, the arrays built from the unpickled events, the verdicts mapped back to ids, the fallback to the dumps route as
soon as one event of the payload is not plain.  The GPU run is tests/test_gpu_pack.py."""
import contextlib
import io

import numpy as np

import model_pack as mp
import oracle_backend


class ModelPackHashgraph(oracle_backend.OracleHashgraph):
    """OracleHashgraph + set_member_keys, set_event_class, pack_events and validate_payload of engine.Hashgraph, by the
    model and the host crypto."""
    crypto = None

    def __init__(self, n_members, *a, **kw):
        super().__init__(n_members, *a, **kw)
        self.keys = None
        self.cls = ("swirld", "Event")
        self.packs, self.validations = [], []

    def set_member_keys(self, keys):
        self.keys = np.frombuffer(b"".join(bytes(k) for k in keys), np.uint8).reshape(-1, 32)
        return 0

    def set_event_class(self, module, qualname):
        self.cls = (module, qualname)

    def pack_events(self, sp_ids, op_ids, arity, creator, t, sig, data=None, data_off=None, data_none=None):
        out = mp.pack(self.keys, sp_ids, op_ids, arity, creator, t, sig, data, data_off, data_none, *self.cls)
        self.packs.append(len(arity))
        return out[0], out[1], out[2], out[3], out[4].astype(bool)

    def validate_payload(self, msgs, sig, creator, whole=None, ids=None):
        def split(x):
            if isinstance(x, tuple):
                return [x[0][x[1][i]:x[1][i + 1]].tobytes() for i in range(len(x[1]) - 1)]
            return list(x)
        m, w = split(msgs), split(whole)
        sig, ids = np.asarray(sig, np.uint8).reshape(-1, 64), np.asarray(ids, np.uint8).reshape(-1, 32)
        ok = np.zeros(len(m), bool)
        for i in range(len(m)):
            if not 0 <= creator[i] < len(self.keys):
                continue
            try:
                self.crypto.verify_detached(sig[i].tobytes(), m[i], self.keys[creator[i]].tobytes())
            except ValueError:
                continue
            ok[i] = self.crypto.generichash(w[i]) == ids[i].tobytes()
        self.validations.append((isinstance(msgs, tuple), m, w))
        return ok


def make_nodes(pkg, monkeypatch, n=4):
    ModelPackHashgraph.crypto = pkg.node.crypto
    monkeypatch.setattr(pkg.node, "Hashgraph", ModelPackHashgraph)
    kps = [pkg.node.crypto.sign_seed_keypair(bytes([i + 1]) * 32) for i in range(n)]
    stake = {pk: 1 for pk, _ in kps}
    with contextlib.redirect_stdout(io.StringIO()):
        return [pkg.Node(kp, {}, n, stake) for kp in kps]


def payload(pkg, nodes, extra=0):
    """{id -> Event}: the roots of all nodes and a few events built on them by node 0 and 1 alternately."""
    Event, crypto, dumps = pkg.node.Event, pkg.node.crypto, pkg.node.dumps
    evs = {nd.head: nd.hg[nd.head] for nd in nodes}
    heads = [nd.head for nd in nodes]
    for k in range(extra):
        me, other = k % 2, 2 + k % 2
        p = (heads[me], heads[other])
        t = 1.0e9 + k
        s = crypto.sign_detached(dumps((None, p, t, nodes[me].pk)), nodes[me].sk)
        ev = Event(None, p, t, nodes[me].pk, s)
        h = crypto.generichash(dumps(ev))
        evs[h] = ev
        heads[me] = h
    return evs


def test_plain_event_predicate(pkg):
    Event, plain = pkg.node.Event, pkg.Node._is_plain
    i32, c, s, a, b = b"i" * 32, b"c" * 32, b"s" * 64, b"a" * 32, b"b" * 32
    assert plain(i32, Event(None, (), 1.5, c, s))
    assert plain(i32, Event(None, (a, b), 1.5, c, s))
    for ev in (Event(b"", (), 1.5, c, s), Event(b"tx", (a, b), 1.5, c, s),          # data
               Event(None, (), 1, c, s), Event(None, (), np.float64(1.5), c, s),      # timestamp not exactly a float
               Event(None, [], 1.5, c, s), Event(None, (a,), 1.5, c, s), Event(None, (a, b, b), 1.5, c, s),
               Event(None, (a, b"b" * 31), 1.5, c, s), Event(None, (bytearray(a), b), 1.5, c, s), Event(None, (a, a), 1.5, c, s),
               Event(None, (), 1.5, b"c" * 31, s), Event(None, (), 1.5, bytearray(c), s), Event(None, (), 1.5, c, b"s" * 63),
               (None, (), 1.5, c, s)):                                               # not an Event
        assert not plain(i32, ev), ev
    assert not plain(b"i" * 31, Event(None, (), 1.5, c, s))
    assert not plain(bytearray(i32), Event(None, (), 1.5, c, s))


def test_arrays_through_the_model_equal_dumps(pkg, monkeypatch):
    nodes = make_nodes(pkg, monkeypatch)
    nd = nodes[0]
    evs = payload(pkg, nodes, extra=9)
    eids = list(evs)
    assert all(pkg.Node._is_plain(h, evs[h]) for h in eids)
    sp, op, arity, creator, t, sig, ids = pkg.Node._payload_arrays(eids, evs, nd._mindex)
    keys = np.frombuffer(b"".join(nd._members), np.uint8).reshape(-1, 32)
    Event = pkg.node.Event
    msgs, moff, whole, woff, enc = mp.pack(keys, sp, op, arity, creator, t, sig, mod=Event.__module__, qual=Event.__qualname__)
    assert enc.all() and ids.tobytes() == b"".join(eids)
    for i, h in enumerate(eids):
        assert msgs[moff[i]:moff[i + 1]].tobytes() == pkg.node.dumps(evs[h][:-1]), i
        assert whole[woff[i]:woff[i + 1]].tobytes() == pkg.node.dumps(evs[h]), i
        assert pkg.node.crypto.generichash(whole[woff[i]:woff[i + 1]].tobytes()) == h


def test_batch_validate_takes_the_array_route_for_plain_payloads(pkg, monkeypatch):
    nodes = make_nodes(pkg, monkeypatch)
    nd = nodes[0]
    evs = payload(pkg, nodes, extra=9)
    eids = list(evs)
    victim, stranger = eids[6], eids[8]
    evs[victim] = evs[victim]._replace(t=evs[victim].t + 1.0)                        # signature and id no longer fit
    evs[stranger] = evs[stranger]._replace(c=b"\x07" * 32)                          # not a member
    res = nd._batch_validate(eids, evs)
    assert nd._dev.cls == (pkg.node.Event.__module__, pkg.node.Event.__qualname__)
    assert nd._dev.packs == [len(eids)] and nd._plain_payloads == 1
    assert len(nd._dev.validations) == 1 and nd._dev.validations[0][0]               # (data, offsets) pairs went in
    for h in eids:
        assert res[h] == ((False, None) if h in (victim, stranger) else (True, h))
    # the bytes the backend judged are the ones the dumps route would have sent
    _, m, w = nd._dev.validations[0]
    for i, h in enumerate(eids):
        if h != stranger:
            assert m[i] == pkg.node.dumps(evs[h][:-1]) and w[i] == pkg.node.dumps(evs[h])
        else:
            assert m[i] == b"" and w[i] == b""


def test_one_event_that_is_not_plain_sends_the_payload_down_the_dumps_route(pkg, monkeypatch):
    nodes = make_nodes(pkg, monkeypatch)
    nd = nodes[0]
    evs = payload(pkg, nodes, extra=5)
    Event, crypto, dumps = pkg.node.Event, pkg.node.crypto, pkg.node.dumps
    p = (nodes[1].head, nodes[2].head)
    s = crypto.sign_detached(dumps((b"tx", p, 2.0e9, nodes[1].pk)), nodes[1].sk)
    ev = Event(b"tx", p, 2.0e9, nodes[1].pk, s)
    h = crypto.generichash(dumps(ev))
    evs[h] = ev
    eids = list(evs)
    res = nd._batch_validate(eids, evs)
    assert nd._dev.packs == [] and nd._plain_payloads == 0
    assert len(nd._dev.validations) == 1 and not nd._dev.validations[0][0]           # lists of byte strings went in
    assert all(res[x] == (True, x) for x in eids)
