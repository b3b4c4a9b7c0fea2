"""CPU: Node.device_wire (py-swirld_amd/node.py) with the device backend swapped for the CPU oracle plus the models of the
payload ingest, the walk, the event encoder and the wire form — the host glue only.  Off: ask_sync / sync make the calls
they make today.  On: a reply in the canonical wire form never reaches pickle.loads, any other reply does, and the
simulation ends in the state of the run without the switch, by event id.  The GPU route is tests/test_gpu_wire.py."""
import contextlib
import io
import pickle
import random

import numpy as np
import pytest

import model_walk as mwalk
import model_wire as mw
from test_node_data_host import DataHashgraph
from test_node_host import _SortedNetwork
from test_node_payload_host import ModelPayloadHashgraph


class WireHashgraph(DataHashgraph, ModelPayloadHashgraph):
    """The stand-ins of the existing host Node tests + export_message / unpack_message of engine.Hashgraph, by the models."""
    exported, unpacked = 0, 0

    def append_events(self, creator, self_parent, other_parent, t=None, sig=None):
        rec = self.__dict__.setdefault("_rec", ([], [], [], [], []))
        for dst, a in zip(rec, (creator, self_parent, other_parent, t, np.asarray(sig, np.uint8).reshape(-1, 64))):
            dst.extend(list(np.asarray(a)))
        super().append_events(creator, self_parent, other_parent, t, sig)

    def set_event_ids(self, first, ids):
        self.__dict__.setdefault("_id_rows", []).extend(bytes(r) for r in np.asarray(ids, np.uint8).reshape(-1, 32))
        super().set_event_ids(first, ids)

    def ingest_payload(self, ids, sp_ids, op_ids, arity, creator, ok=None, t=None, sig=None, *, data=None, data_off=None, data_none=None):
        before = self.num_events
        out, stored = super().ingest_payload(ids, sp_ids, op_ids, arity, creator, ok, t, sig)
        self._id_rows += [bytes(ids[int(j)]) for j in np.argsort(out, kind="stable")[len(out) - stored:]] if stored else []
        if data_off is not None:
            assert len(self.store) == before, "the data store must be complete"
            datas = self.engine.Hashgraph.unpack_data(data, data_off, data_none)
            self.store += [datas[int(j)] for j in np.argsort(out, kind="stable")[len(out) - stored:]] if stored else []
        return out, stored

    def export_message(self, head, known=None, cap=None, *, data=True):
        cr, sp, op, t, sig = self._rec
        N = len(cr)
        assert len(self._id_rows) == N and (not data or len(self.store) == N), "ids and data store caught up"
        ids = np.frombuffer(b"".join(self._id_rows), np.uint8).reshape(N, 32)
        ev = mwalk.WalkGraph(self.n, cr, sp, op, ids=ids).walk(head, known, cap)
        zero = np.zeros(32, np.uint8)
        datas = [self.store[e] if data else None for e in ev]
        d, off, none = self.engine.Hashgraph.pack_data(datas)
        WireHashgraph.exported += 1
        return mw.pack_message(ids[head], self.keys, ids[ev], [ids[sp[e]] if sp[e] >= 0 else zero for e in ev], [ids[op[e]] if op[e] >= 0 else zero for e in ev],
                               [0 if sp[e] < 0 else 2 for e in ev], [cr[e] for e in ev], np.array([t[e] for e in ev], np.float64),
                               np.array([sig[e] for e in ev], np.uint8).reshape(len(ev), 64), d, off, none, *self.cls)

    def unpack_message(self, msg):
        WireHashgraph.unpacked += 1
        u = mw.unpack_message(msg, self.keys, *self.cls)
        if u is None:
            return None
        return dict(u, sp_ids=u["sp"], op_ids=u["op"])


def simulate(pkg, monkeypatch, n_turns, wire, seen):
    """A seeded gossip of four nodes whose events carry None or bytes; pickle.loads of node.py is watched: `seen` counts the
    replies by kind, and a canonical one that reaches it raises."""
    WireHashgraph.crypto, WireHashgraph.engine = pkg.node.crypto, pkg.engine
    monkeypatch.setattr(pkg.node, "Hashgraph", WireHashgraph)
    monkeypatch.setattr(pkg.Node, "device_data", True)
    monkeypatch.setattr(pkg.Node, "device_wire", wire)
    rng = random.Random(20261019)
    monkeypatch.setattr(pkg.node.crypto, "randombytes", lambda k: bytes(rng.getrandbits(8) for _ in range(k)))
    clock = iter(range(1, 1 << 30))
    monkeypatch.setattr(pkg.node, "time", lambda: 1.0e9 + 0.001 * next(clock))
    prefix = pkg.node.WIRE_PREFIX

    def watched_loads(b):
        canonical = bytes(b[:len(prefix)]) == prefix
        seen["canonical" if canonical else "other"] += 1
        if canonical and wire:
            raise AssertionError("a canonical reply reached pickle.loads")
        return pickle.loads(b)
    monkeypatch.setattr(pkg.node, "loads", watched_loads)
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
            mains[rng.randrange(4)].send((None, b"", b"tx %d" % turn, b"x" * 300)[turn % 4])
    return nodes


def test_off_the_calls_of_today(pkg, monkeypatch):
    assert pkg.Node.device_wire is False
    WireHashgraph.exported = WireHashgraph.unpacked = 0
    seen = dict(canonical=0, other=0)
    nodes = simulate(pkg, monkeypatch, 120, False, seen)
    assert WireHashgraph.exported == 0 and WireHashgraph.unpacked == 0
    assert seen["canonical"] == 0 and seen["other"] >= 240          # every request and every reply is unpickled
    assert all(nd._wire_replies == 0 and nd._wire_intakes == 0 and len(nd._ids) > 50 for nd in nodes)


def test_on_a_canonical_reply_never_reaches_pickle_loads(pkg, monkeypatch):
    off = simulate(pkg, monkeypatch, 300, False, dict(canonical=0, other=0))
    WireHashgraph.exported = WireHashgraph.unpacked = 0
    seen = dict(canonical=0, other=0)
    on = simulate(pkg, monkeypatch, 300, True, seen)
    assert seen["canonical"] == 0                                   # (watched_loads raises on one)
    replies, intakes = sum(nd._wire_replies for nd in on), sum(nd._wire_intakes for nd in on)
    assert replies == WireHashgraph.exported > 100 and intakes == WireHashgraph.unpacked == replies
    # a reply that is not canonical is unpickled as before: the first answers of a node come before its head is divided
    assert seen["other"] >= 300 + (300 - replies)
    for a, b in zip(off, on):
        assert set(a.hg) == set(b.hg) and all(a.hg[h] == b.hg[h] for h in a.hg)
        assert a.transactions == b.transactions and len(a.transactions) > 20
        assert b._dev.store == [b.hg[h].d for h in b._ids]


def test_on_a_reply_that_is_not_canonical_reaches_pickle_loads(pkg, monkeypatch):
    seen = dict(canonical=0, other=0)
    nodes = simulate(pkg, monkeypatch, 40, True, seen)
    a, b = nodes[0], nodes[1]
    crypto = pkg.node.crypto
    before = dict(seen)
    b.device_wire = False                     # b answers with pickle.dumps: a, with the switch on, unpickles it
    a.network[b.pk] = b.ask_sync
    new = a.sync(b.pk, b"plain")
    assert seen["other"] == before["other"] + 2 and new       # b's loads of the request, a's loads of the reply
    a.divide_rounds(new)
    # the canonical header in front of something else: refused by the strict reader, nothing taken, nothing unpickled
    b.device_wire = True
    real = b.ask_sync

    def tampered(pk, info):
        body = bytearray(crypto.sign_open(real(pk, info), b.pk))
        assert bytes(body[:len(pkg.node.WIRE_PREFIX)]) == pkg.node.WIRE_PREFIX
        body[-2] ^= 1
        return crypto.sign(bytes(body), b.sk)
    a.network[b.pk] = tampered
    n_before, loads_before = len(a._ids), seen["other"]
    assert a.sync(b.pk, b"tampered") == () and len(a._ids) == n_before
    assert seen["other"] == loads_before + 1                  # (b's loads of the request only)
