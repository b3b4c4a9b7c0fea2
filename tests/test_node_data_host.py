"""CPU: Node.device_data (py-swirld_amd/node.py) with the device backend swapped for the CPU oracle plus tests/model_pack.py
and a list that plays the data store — the host glue only: off, nothing new is called; on, the store is caught up before
every divide_rounds with exactly the events' data, payloads whose events carry bytes take _batch_validate's array route,
ordered_data() reads the consensus stream's payloads back, and data that is neither None nor bytes falls back to the host
routes.  The GPU run is tests/test_gpu_event_data.py."""
import contextlib
import io
import random

import numpy as np
import pytest

from test_node_host import _SortedNetwork
from test_node_pack_host import ModelPackHashgraph


class DataHashgraph(ModelPackHashgraph):
    """ModelPackHashgraph + set_event_data and export_ordered(data=True) of engine.Hashgraph, on Python lists."""
    engine = None

    def __init__(self, n_members, *a, **kw):
        super().__init__(n_members, *a, **kw)
        self.data_calls, self.store, self.order, self.exports = [], [], [], 0

    def set_event_data(self, first, datas):
        datas = list(datas)
        assert first == len(self.store) and first + len(datas) <= self.num_events
        assert all(d is None or (type(d) is bytes and len(d) <= 60000) for d in datas)
        self.data_calls.append((first, datas))
        self.store += datas

    def find_order(self, rounds):
        out = super().find_order(rounds)
        self.order += [int(x) for x in out]
        return out

    def export_ordered(self, first=0, K=None, ids=None, *, data=False):
        ev = self.order[first:] if K is None else self.order[first:first + K]
        d = dict(event=np.array(ev, np.int32))
        if data:
            d["data"], d["data_off"], d["data_none"] = self.engine.Hashgraph.pack_data([self.store[e] for e in ev])
        self.exports += 1
        return d


def make_nodes(pkg, monkeypatch, n=4):
    DataHashgraph.crypto, DataHashgraph.engine = pkg.node.crypto, pkg.engine
    monkeypatch.setattr(pkg.node, "Hashgraph", DataHashgraph)
    kps = [pkg.node.crypto.sign_seed_keypair(bytes([i + 1]) * 32) for i in range(n)]
    stake = {pk: 1 for pk, _ in kps}
    with contextlib.redirect_stdout(io.StringIO()):
        return [pkg.Node(kp, {}, n, stake) for kp in kps]


def simulate(pkg, monkeypatch, n_turns, payloads):
    """pkg.test() with seeded gossip, a deterministic clock and `payloads(turn)` as what each turn's new event carries."""
    DataHashgraph.crypto, DataHashgraph.engine = pkg.node.crypto, pkg.engine
    monkeypatch.setattr(pkg.node, "Hashgraph", DataHashgraph)
    rng = random.Random(20261019)
    monkeypatch.setattr(pkg.node.crypto, "randombytes", lambda k: bytes(rng.getrandbits(8) for _ in range(k)))
    clock = iter(range(1, 1 << 30))
    monkeypatch.setattr(pkg.node, "time", lambda: 1.0e9 + 0.001 * next(clock))
    crypto = pkg.node.crypto
    kps = sorted((crypto.sign_seed_keypair(bytes([i + 1]) * 32) for i in range(4)), key=lambda kp: kp[0])
    network = _SortedNetwork()
    stake = {kp[0]: 1 for kp in kps}
    with contextlib.redirect_stdout(io.StringIO()):
        nodes = [pkg.Node(kp, network, 4, stake) for kp in kps]
        for nd in nodes:
            network[nd.pk] = nd.ask_sync
        mains = [nd.main() for nd in nodes]
        for m in mains:
            next(m)
        for turn in range(n_turns):
            mains[rng.randrange(4)].send(payloads(turn))
    return nodes


def mixed(turn):
    return (None, b"", b"tx %d" % turn, b"x" * 300, 5, ("a", "tuple"))[turn % 6]


def test_off_nothing_new_is_called(pkg, monkeypatch):
    assert pkg.Node.device_data is False
    nodes = simulate(pkg, monkeypatch, 120, mixed)
    for nd in nodes:
        assert nd._dev.data_calls == [] and nd._dev.exports == 0 and nd._dev_data == 0 and len(nd._ids) > 50
        with pytest.raises(RuntimeError):
            nd.ordered_data()


def test_on_the_store_is_caught_up_with_exactly_the_events_data(pkg, monkeypatch):
    monkeypatch.setattr(pkg.Node, "device_data", True)
    nodes = simulate(pkg, monkeypatch, 300, mixed)
    storable = pkg.Node._storable_data
    assert storable(None) is None and storable(b"") == b"" and storable(b"x" * 60000) == b"x" * 60000
    assert storable(b"x" * 60001) is None and storable(5) is None and storable(bytearray(b"ab")) is None
    for nd in nodes:
        calls = nd._dev.data_calls
        assert len(calls) > 20 and [c[0] for c in calls] == list(np.cumsum([0] + [len(c[1]) for c in calls[:-1]]))
        assert nd._dev_data == len(nd._ids) == len(nd._dev.store)
        kinds = {type(nd.hg[h].d) for h in nd._ids}
        assert {type(None), bytes, int, tuple} <= kinds
        # bytes and None exactly; what the store cannot hold is None there, and hg keeps the object
        assert nd._dev.store == [nd.hg[h].d if type(nd.hg[h].d) is bytes else None for h in nd._ids]
        # the consensus stream with its payloads, in one export
        assert len(nd.transactions) > 50
        before = nd._dev.exports
        got = nd.ordered_data()
        assert nd._dev.exports == before + 1
        assert got == [(h, storable(nd.hg[h].d)) for h in nd.transactions]
        assert [(h, d) for h, d in got if type(nd.hg[h].d) is bytes] == [(h, nd.hg[h].d) for h in nd.transactions if type(nd.hg[h].d) is bytes]
        assert nd.ordered_data(7, 20) == got[7:27] and nd.ordered_data(len(got)) == []


def data_payload(pkg, nodes, datas):
    """{id -> Event}: the roots of all nodes and one event per entry of `datas` built on them by node 0 and 1 alternately."""
    Event, crypto, dumps = pkg.node.Event, pkg.node.crypto, pkg.node.dumps
    evs = {nd.head: nd.hg[nd.head] for nd in nodes}
    heads = [nd.head for nd in nodes]
    for k, d in enumerate(datas):
        me, other = k % 2, 2 + k % 2
        p = (heads[me], heads[other])
        t = 1.0e9 + k
        ev = Event(d, p, t, nodes[me].pk, crypto.sign_detached(dumps((d, p, t, nodes[me].pk)), nodes[me].sk))
        h = crypto.generichash(dumps(ev))
        evs[h] = ev
        heads[me] = h
    return evs


def test_plain_or_data_predicate(pkg):
    Event, ok = pkg.node.Event, pkg.Node._is_plain_or_data
    i32, c, s, a, b = b"i" * 32, b"c" * 32, b"s" * 64, b"a" * 32, b"b" * 32
    for d in (None, b"", b"tx", b"x" * 255, b"x" * 256, b"x" * 60000):
        assert ok(i32, Event(d, (), 1.5, c, s)) and ok(i32, Event(d, (a, b), 1.5, c, s)), d
    for ev in (Event(b"x" * 60001, (), 1.5, c, s), Event(bytearray(b"tx"), (), 1.5, c, s), Event(5, (), 1.5, c, s), Event("tx", (), 1.5, c, s),
               Event(c, (), 1.5, c, s), Event(s, (), 1.5, c, s), Event(a, (a, b), 1.5, c, s),         # one object twice: a memo read
               Event(b"tx", (a, a), 1.5, c, s), Event(b"tx", (), 1, c, s), Event(b"tx", [], 1.5, c, s),   # what _is_plain refuses
               (b"tx", (), 1.5, c, s)):
        assert not ok(i32, ev), ev
    assert ok(i32, Event(bytes(bytearray(c)), (), 1.5, c, s))        # equal to the key, another object


def test_on_payloads_with_bytes_take_the_array_route(pkg, monkeypatch):
    monkeypatch.setattr(pkg.Node, "device_data", True)
    nodes = make_nodes(pkg, monkeypatch)
    nd = nodes[0]
    evs = data_payload(pkg, nodes, [b"tx", b"", None, b"y" * 300, b"z" * 255, None, b"\x00", b"tx"])
    eids = list(evs)
    victim = eids[7]                                                                 # (four roots first: the 300-byte event)
    evs[victim] = evs[victim]._replace(d=evs[victim].d + b"!")                       # signature and id no longer fit
    res = nd._batch_validate(eids, evs)
    assert nd._dev.packs == [len(eids)] and nd._plain_payloads == 1
    assert len(nd._dev.validations) == 1 and nd._dev.validations[0][0]               # (data, offsets) pairs went in
    for h in eids:
        assert res[h] == ((False, None) if h == victim else (True, h))
    _, m, w = nd._dev.validations[0]
    for i, h in enumerate(eids):                                                     # the bytes the backend judged
        assert m[i] == pkg.node.dumps(evs[h][:-1]) and w[i] == pkg.node.dumps(evs[h])


def test_on_data_that_is_not_bytes_falls_back(pkg, monkeypatch):
    monkeypatch.setattr(pkg.Node, "device_data", True)
    nodes = make_nodes(pkg, monkeypatch)
    nd = nodes[0]
    evs = data_payload(pkg, nodes, [b"tx", 5, None])
    eids = list(evs)
    res = nd._batch_validate(eids, evs)
    assert nd._dev.packs == [] and nd._plain_payloads == 0
    assert len(nd._dev.validations) == 1 and not nd._dev.validations[0][0]           # lists of byte strings went in
    assert all(res[x] == (True, x) for x in eids)


def test_off_payloads_with_bytes_stay_on_the_dumps_route(pkg, monkeypatch):
    nodes = make_nodes(pkg, monkeypatch)
    nd = nodes[0]
    evs = data_payload(pkg, nodes, [b"tx", b"", None])
    res = nd._batch_validate(list(evs), evs)
    assert nd._dev.packs == [] and not nd._dev.validations[0][0] and all(res[x] == (True, x) for x in evs)
