"""GPU (-m gpu): the drop-in Node with Node.exact_history = True in the equivocator scenario of tests/test_node_host.py (seven
nodes, member B signs two events on one self-parent), on the real device backend: after the stored fork votes,
round_received and consensus_time go on answering.  Every append / divide_rounds / decide_fame / find_order call the node
makes on its context is recorded and replayed, call for call, on the CPU oracle (votes by event, order) and on the host
build of the exact path with its history (tests/exact_history_host.cpp: round received, consensus time, bit for bit).
Then DeviceNetwork(..., exact_history=True): the switch reaches every context, and a fork-free run answers as without it."""
import contextlib
import io
import random

import numpy as np
import pytest

from oracle.oracle import Oracle
from test_exact_history_host import HistoryHost
from test_node_host import _build_on, _seven_nodes

pytestmark = pytest.mark.gpu

REPLAYED = ("append_events", "divide_rounds", "decide_fame", "find_order")


class Recorder:
    """A context that notes the consensus calls made on it."""

    def __init__(self, dev):
        self.__dict__["_dev"], self.__dict__["log"] = dev, []

    def __getattr__(self, name):
        f = getattr(self._dev, name)
        if name not in REPLAYED:
            return f

        def call(*a):
            self.log.append((name, sorted(int(r) for r in a[0]) if name == "find_order" else tuple(np.array(x) for x in a)))
            return f(*a)
        return call


def replay(log, n):
    o, x = Oracle(n), HistoryHost(n)
    for name, a in log:
        if name == "append_events":
            for d in (o, x):
                d.append_events(*a)
        elif name == "divide_rounds":
            for d in (o, x):
                d.divide_rounds(int(a[0]), int(a[1]))
        elif name == "decide_fame":
            assert list(o.decide_fame()) == list(x.decide_fame())
        else:
            assert list(o.find_order(a)) == list(x.find_order(a))
    return o, x


def test_node_keeps_votes_and_consensus_values_after_a_stored_fork(pkg, monkeypatch):
    real = pkg.node.Hashgraph
    monkeypatch.setattr(pkg.node, "Hashgraph", lambda *a, **kw: Recorder(real(*a, **kw)))
    monkeypatch.setattr(pkg.Node, "exact_history", True)
    with contextlib.redirect_stdout(io.StringIO()):
        a, b, c, rest = _seven_nodes(pkg)
        assert a._dev.exact_history and not a._dev.exact
        hb = b.head
        h1, e1 = b.new_event(b"one", (hb, b._chain_head[a.pk]))
        h2, e2 = b.new_event(b"two", (hb, b._chain_head[c.pk]))   # same self-parent: B equivocates
        a.add_event(h1, e1)
        a.add_event(h2, e2)
        ha = _build_on(a, h1, b"on-one")
        a.divide_rounds((h1, h2, ha))
        assert a._dev.exact
        a.find_order(a.decide_fame())
        c.add_event(h2, e2)
        hc = _build_on(c, h2, b"on-two")
        c.divide_rounds((h2, hc))
        c.divide_rounds(c.sync(a.pk, b"after-fork"))
        c.find_order(c.decide_fame())
        rng = random.Random(5)
        honest = [a, c] + rest
        for _ in range(300):
            x, y = rng.sample(honest, 2)
            x.divide_rounds(x.sync(y.pk, b"more"))
            x.find_order(x.decide_fame())
    assert a.consensus and len(a.transactions) > 0 and a.round[a.head] >= 3
    o, x = replay(a._dev.log, 7)
    assert [a._index[h] for h in a.transactions] == o.transactions.tolist()
    # votes, by event: the Mapping protocol, and every entry against the oracle
    votes = a.votes
    per_voter = votes[a.head]
    assert len(per_voter) == sum(1 for _ in per_voter)
    n_entries = 0
    for yh in votes:
        for xh, v in votes[yh].items():
            assert o.vote(a._index[yh], a._index[xh]) == int(v)
            assert xh in votes[yh]
            n_entries += 1
    assert n_entries == o.num_votes > 0 and len(votes) == len(list(votes))
    with pytest.raises(KeyError):
        votes[a.head][b"\0" * 32]
    # round received / consensus time: exactly the ordered events, the values of the host build under the same schedule
    rr, cts = x.consensus()
    assert list(a.round_received) == a.transactions == list(a.consensus_time)
    for h in a.transactions:
        e = a._index[h]
        assert a.round_received[h] == rr[e]
        assert np.float64(a.consensus_time[h]).view(np.uint64) == cts[e]
    assert a.tbd and next(iter(a.tbd)) not in a.round_received


def test_device_network_passes_the_switch_on(pkg):
    """DeviceNetwork(..., exact_history=True): every context is created with the history; on a run without forks
    votes(i), round_received(i) and consensus_time(i) are those of a network without it."""
    seeds = [bytes([77, m]) + bytes(30) for m in range(4)]
    ev = pkg.node.Event
    nets = []
    for hist in (False, True):
        rng = random.Random(11)
        clock = iter(range(1, 1 << 30))
        tick = lambda: 1.0e9 + 0.001 * next(clock)   # noqa: E731
        net = pkg.DeviceNetwork(seeds, event_class=(ev.__module__, ev.__qualname__), clock=tick, exact_history=hist)
        assert all(h.exact_history == hist for h in net.ctx)
        net.run(120, rng.randrange, tick)
        nets.append(net)
    plain, kept = nets
    assert any(len(plain.votes(i)) > 0 for i in range(4))
    for i in range(4):
        assert not kept.ctx[i].exact and kept.ctx[i].votes_available
        assert kept.votes(i) == plain.votes(i)
        assert kept.round_received(i) == plain.round_received(i)
        assert kept.transactions(i) == plain.transactions(i)
        y, x, v = kept.ctx[i].vote_entries()
        ids = [bytes(q) for q in kept.ctx[i].event_ids()]
        by_event = {}
        for a, b, c in zip(y.tolist(), x.tolist(), v.tolist()):
            by_event.setdefault(ids[a], {})[ids[b]] = bool(c)
        assert by_event == plain.votes(i)
    for net in nets:
        net.close()


def test_device_network_with_one_equivocator(pkg):
    """Seven contexts; member B signs a second event on the self-parent of its head, and every honest context ingests it
    beside the first: all six move to the exact path, B falls silent, the honest ones go on gossiping.  votes(i),
    round_received(i), consensus_time(i) and the ordered data of every honest context against the oracle and the host
    build of the exact path, both replaying that context's own schedule (per turn: the events it brought, divide_rounds,
    decide_fame, find_order)."""
    n, B = 7, 1
    honest = [i for i in range(n) if i != B]
    seeds = [bytes([91, m]) + bytes(30) for m in range(n)]
    ev = pkg.node.Event
    clock = iter(range(1, 1 << 30))
    tick = lambda: 1.0e9 + 0.001 * next(clock)   # noqa: E731
    net = pkg.DeviceNetwork(seeds, event_class=(ev.__module__, ev.__qualname__), clock=tick, exact_history=True)
    rng = random.Random(17)
    log = [[(0, 1, None)] for _ in range(n)]     # per context: (first event, end, new_c of the call | None: divided only)
    payload_of = {}

    def turn(i, j, payload=None):
        N0 = net.ctx[i].num_events
        r = net.turn(i, j, payload, tick())
        assert r.new_head >= 0 and r.stage == 5
        log[i].append((N0, net.ctx[i].num_events, r.new_rounds.tolist()))
        payload_of[net.head(i)] = payload

    for k in range(60):
        i = rng.randrange(n)
        turn(i, rng.choice([j for j in range(n) if j != i]), b"warm %d" % k if k % 2 else None)
    prev = net.heads[B]
    turn(B, 0)                                   # B's head: the first sibling, on `prev`
    for i in honest:
        turn(i, B)                               # everybody knows it, and with it every event B's context holds
    hb = net.ctx[B]
    w = hb.export_walk(net.heads[B])
    first_op = int(w["event"][[bytes(x) for x in w["ids"]].index(bytes(w["op_ids"][-1]))])
    op2 = max(int(e) for e, c in zip(w["event"], w["creator"]) if c != B and e != first_op and e < net.heads[B])
    t2 = tick()
    s = hb.sign_events([B], [prev], [op2], [t2])   # the second sibling: same creator, same self-parent, nothing stored
    for i in honest:
        h = net.ctx[i]
        assert not h.exact
        idx, stored = h.ingest_payload(s["ids"], s["sp_ids"], s["op_ids"], s["arity"], [B], t=[t2], sig=s["sig"], data=[None])
        assert stored == 1 and int(idx[0]) == h.num_events - 1 and h.exact
        h.divide_rounds(h.num_events - 1, 1)
        log[i].append((h.num_events - 1, h.num_events, None))
    for k in range(220):
        i, j = rng.sample(honest, 2)
        turn(i, j, b"tx %d" % k if k % 3 else None)

    sib = dict(id=bytes(s["ids"][0]), sp=bytes(s["sp_ids"][0]), op=bytes(s["op_ids"][0]), t=t2, sig=s["sig"][0])
    checked_votes = 0
    for i in honest:
        h = net.ctx[i]
        assert h.exact and h.exact_history and h.votes_available
        ids = [bytes(q) for q in h.event_ids()]
        N = len(ids)
        dense = {q: e for e, q in enumerate(ids)}
        cr, sp, op = np.full(N, -1, np.int32), np.full(N, -1, np.int32), np.full(N, -1, np.int32)
        t, sig, have = np.zeros(N), np.zeros((N, 64), np.uint8), np.zeros(N, bool)
        w = h.export_walk(net.heads[i])           # every event but the second sibling is an ancestor of the head
        for k, e in enumerate(w["event"]):
            cr[e], t[e], sig[e], have[e] = w["creator"][k], w["t"][k], w["sig"][k], True
            if w["arity"][k]:
                sp[e], op[e] = dense[bytes(w["sp_ids"][k])], dense[bytes(w["op_ids"][k])]
        e = dense[sib["id"]]
        assert not have[e]
        cr[e], sp[e], op[e], t[e], sig[e], have[e] = B, dense[sib["sp"]], dense[sib["op"]], sib["t"], sib["sig"], True
        assert have.all()
        o, x = Oracle(n), HistoryHost(n)
        for a, b, new_c in log[i]:
            for d in (o, x):
                d.append_events(cr[a:b], sp[a:b], op[a:b], t[a:b], sig[a:b])
                d.divide_rounds(a, b - a)
            if new_c is not None:
                nc = o.decide_fame()
                assert sorted(nc) == sorted(x.decide_fame()) == sorted(new_c)
                assert list(o.find_order(nc)) == list(x.find_order(nc))
        assert log[i][-1][1] == N
        tx = o.transactions.tolist()
        assert net.transactions(i) == [ids[e] for e in tx] and len(tx) > 0
        votes = net.votes(i)
        assert sum(len(v) for v in votes.values()) == o.num_votes > 0
        for yh, row in votes.items():
            for xh, v in row.items():
                assert o.vote(dense[yh], dense[xh]) == int(v)
                checked_votes += 1
        rr, cts = x.consensus()
        assert net.round_received(i) == {ids[e]: int(rr[e]) for e in tx}
        got = net.consensus_time(i)
        assert list(got) == [ids[e] for e in tx]
        assert all(np.float64(got[ids[e]]).view(np.uint64) == cts[e] for e in tx)
        # the ordered stream with its data, on the exact path
        want = [payload_of.get(ids[e]) for e in tx]
        assert net.ordered_data(i) == want and any(d is not None for d in want)
        od = h.export_ordered(data=True)
        assert np.array_equal(od["event"], tx) and h.unpack_data(od["data"], od["data_off"], od["data_none"]) == want
        assert np.array_equal(od["round_received"], rr[tx])
    assert checked_votes > 0 and not net.ctx[B].exact
    net.close()


@pytest.mark.parametrize("case", [(4, 260, 31, 6), (5, 400, 32, 10), (3, 150, 33, 4)], ids=lambda c: "%d_%d_%d_%d" % c)
def test_node_agrees_with_the_reference_node_on_forked_schedules(pkg, monkeypatch, case):
    """The observer of test_node_vs_reference.forked_run — a Byzantine member forks, the observer calls divide_rounds /
    decide_fame / find_order on the reference's schedule — on the real device with Node.exact_history = True, against what
    the UNMODIFIED reference Node kept under the same schedule (tests/golden/node/forked_history_*, recorded by
    tests/golden/make_node_history_golden.py): the whole votes dict, round received and consensus time bit for bit, and
    ordered_data() after the fork."""
    import test_node_vs_reference as T
    ref = T.load("forked_history_%d_%d_%d_%d" % case)
    monkeypatch.setattr(pkg.node, "dumps", T._class_free_dumps)
    monkeypatch.setattr(pkg.node, "time", T._clock())
    monkeypatch.setattr(pkg.Node, "exact_history", True)
    monkeypatch.setattr(pkg.Node, "device_data", True)
    obs, _ = T.forked_run(pkg.node.crypto.sign_seed_keypair, *case, lambda kp, n_, stake: pkg.Node(kp, {}, n_, stake, accept_forks=True))
    assert obs._dev.exact and obs._dev.exact_history
    assert [h.hex() for h in obs.transactions] == ref["transactions"]
    want = {}
    for y, x, v in ref["votes"]:
        want.setdefault(bytes.fromhex(y), {})[bytes.fromhex(x)] = v
    got = {y: dict(obs.votes[y].items()) for y in obs.votes}
    assert {y: row for y, row in got.items() if row} == want and len(want) > 0
    y, row = next(iter(want.items()))
    x = next(iter(row))
    assert obs.votes[y][x] == row[x] and x in obs.votes[y] and len(obs.votes[y]) == len(row)
    assert [obs.round_received[h] for h in obs.transactions] == ref["round_received"]
    assert [float(obs.consensus_time[h]).hex() for h in obs.transactions] == ref["consensus_time"]
    assert list(obs.round_received) == obs.transactions == list(obs.consensus_time)
    assert obs.ordered_data() == [(h, obs.hg[h].d) for h in obs.transactions]
    if case[0] > 3:
        assert len(obs.transactions) > 0 and any(d is not None for _, d in obs.ordered_data())
