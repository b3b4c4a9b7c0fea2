"""CPU: Node.sync's device payload route (Node.device_payload_threshold) with the device backend swapped for the CPU
oracle plus tests/model_payload.py — the host glue of node.py: ids registered before the call, the arrays built from
the unpickled events, the dicts of the view filled from index_out in dense order.  Two runs of one seeded gossip
simulation, with and without the route, must end in the same state by event id.  The GPU run of the same comparison is
tests/test_gpu_payload.py::test_node_takes_the_device_route."""
import contextlib
import io
import random

import numpy as np

import model_payload as mp
import oracle_backend
from test_node_host import _run_simulation


class ModelPayloadHashgraph(oracle_backend.OracleHashgraph):
    """OracleHashgraph + the id index and ingest_payload of engine.Hashgraph, by the model."""

    def __init__(self, n_members, *a, **kw):
        super().__init__(n_members, *a, **kw)
        self._idx = mp.Index(n_members)
        self._creators = []
        self.calls = []

    def append_events(self, creator, self_parent, other_parent, t=None, sig=None):
        super().append_events(creator, self_parent, other_parent, t, sig)
        self._creators += np.asarray(creator).tolist()

    def set_event_ids(self, first, ids):
        ids = np.asarray(ids, np.uint8).reshape(-1, 32)
        assert first == len(self._idx.ids) and first + len(ids) <= self.num_events
        for i, row in enumerate(ids):
            self._idx.add(bytes(row), self._creators[first + i])

    def ingest_payload(self, ids, sp_ids, op_ids, arity, creator, ok=None, t=None, sig=None):
        assert len(self._idx.ids) == self.num_events, "the index must be complete"
        K = len(ids)
        events = [(bytes(ids[i]), () if arity[i] == 0 else (bytes(sp_ids[i]), bytes(op_ids[i])) if arity[i] == 2 else (b"?",) * int(arity[i]),
                   int(creator[i]), 1 if ok is None else int(ok[i])) for i in range(K)]
        out, order, waves, parents = mp.ingest(self._idx, events)
        if order:
            self.append_events(np.array([events[i][2] for i in order], np.int32), np.array([parents[i][0] for i in order], np.int32),
                               np.array([parents[i][1] for i in order], np.int32), np.asarray(t)[order], np.asarray(sig)[order])
        self.calls.append((K, len(order)))
        return out, len(order)


def _gossip(pkg, monkeypatch, threshold, turns=260):
    monkeypatch.setattr(pkg.node, "Hashgraph", ModelPayloadHashgraph)
    rng = random.Random(20261018)
    monkeypatch.setattr(pkg.node.crypto, "randombytes", lambda k: bytes(rng.getrandbits(8) for _ in range(k)))
    clock = iter(range(1, 1 << 30))
    monkeypatch.setattr(pkg.node, "time", lambda: 1.0e9 + 0.001 * next(clock))
    monkeypatch.setattr(pkg.node, "randrange", lambda k: rng.randrange(k))
    monkeypatch.setattr(pkg.Node, "device_payload_threshold", threshold)
    with contextlib.redirect_stdout(io.StringIO()):
        return _run_simulation(pkg, 4, turns, rng)


def test_device_route_equals_the_host_loop(pkg, monkeypatch):
    a = _gossip(pkg, monkeypatch, 1)
    b = _gossip(pkg, monkeypatch, None)
    assert all(nd._device_payloads > 0 and sum(s for _, s in nd._dev.calls) > 50 for nd in a)
    assert all(nd._device_payloads == 0 and not nd._dev.calls for nd in b)
    for x, y in zip(a, b):
        assert x.pk == y.pk and set(x.hg) == set(y.hg) and len(x.hg) > 150
        assert x.transactions == y.transactions and len(x.transactions) > 30
        assert {h: x.round[h] for h in x.hg} == {h: y.round[h] for h in y.hg}
        assert dict(x.famous) == dict(y.famous) and x.consensus == y.consensus
        assert x.height == y.height and x.tbd == y.tbd and x.head == y.head and x.idx == y.idx
        assert x._dev._idx.ids[:x._dev_ids] == x._ids[:x._dev_ids]            # ids registered in dense order
        for c in range(4):                                                    # chains in chain order
            assert [x.hg[h].p[0] for h in x._chains[c][1:]] == x._chains[c][:-1]
        assert x._index == {h: i for i, h in enumerate(x._ids)}


def test_invalid_events_are_dropped_by_the_device_route(pkg, monkeypatch):
    """A payload with a tampered event: the route stores the rest, like the host loop (the reference's behaviour)."""
    monkeypatch.setattr(pkg.node, "Hashgraph", ModelPayloadHashgraph)
    monkeypatch.setattr(pkg.Node, "device_payload_threshold", 1)
    with contextlib.redirect_stdout(io.StringIO()):
        nodes = _run_simulation(pkg, 4, 60, random.Random(5))
    a, b = nodes[0], nodes[1]
    reply = pkg.node.loads(pkg.node.crypto.sign_open(b.ask_sync(a.pk, pkg.node.crypto.sign(pkg.node.dumps({}), a.sk)), b.pk))
    head, remote = reply
    fresh = pkg.Node((a.pk, a.sk), {b.pk: None}, 4, a.stake)
    # every event of b's view except fresh's own root (same key: a's root is in b's view already), one of them tampered
    victim = next(h for h, ev in remote.items() if ev.p and ev.c != a.pk)
    bad = remote[victim]._replace(t=remote[victim].t + 1.0)
    remote = dict(remote)
    remote[victim] = bad
    fresh.network[b.pk] = lambda pk, info: pkg.node.crypto.sign(pkg.node.dumps((head, remote)), b.sk)
    before = set(fresh.hg)
    with contextlib.redirect_stdout(io.StringIO()):
        added = fresh.sync(b.pk, None)
    assert fresh._device_payloads == 1 and victim not in fresh.hg
    # whatever was stored has both parents stored, and nothing built on the victim got in
    for h in added:
        assert all(p in fresh.hg for p in fresh.hg[h].p)
    desc = {victim}
    for h in pkg.node.toposort(set(remote), lambda u: [p for p in remote[u].p if p in remote]):
        if any(p in desc for p in remote[h].p):
            desc.add(h)
    assert not (desc & set(fresh.hg)) and len(set(fresh.hg) - before) > 5
    assert set(fresh.hg) - before - {fresh.head} == set(remote) - desc - before
