"""CPU: Node.ask_sync with device_sync_walk = True against the host BFS of the same node, at every call of a small gossip
simulation with one equivocator.  The device backend is the CPU oracle of tests/oracle_backend.py with sync_walk added from
tests/model_walk.py, so what is checked here is the HOST side of the route: the heights array built from the asker's
dict, the cap built from Node._trunk_height, the reply built from the returned dense indices.  The GPU route itself is
covered by tests/test_gpu_walk.py."""
import contextlib
import io
import random

import numpy as np

import model_walk as mw
import oracle_backend
from test_node_host import _build_on, _seven_nodes


class WalkOracleHashgraph(oracle_backend.OracleHashgraph):
    """OracleHashgraph + sync_walk: the model's walk over the events appended so far."""

    walk_calls = 0
    capped_calls = 0

    def append_events(self, creator, self_parent, other_parent, t=None, sig=None):
        rec = self.__dict__.setdefault("_rec", ([], [], []))
        for dst, a in zip(rec, (creator, self_parent, other_parent)):
            dst.extend(np.asarray(a).tolist())
        super().append_events(creator, self_parent, other_parent, t, sig)

    def sync_walk(self, head, known=None, cap=None):
        cr, sp, op = self._rec
        g = mw.WalkGraph(self.n, cr, sp, op, ids=np.zeros((len(cr), 32), np.uint8))
        assert known is None or (np.asarray(known).dtype == np.int32 and np.asarray(known).shape == (self.n,))
        assert cap is None or (np.asarray(cap).dtype == np.int32 and (np.asarray(cap) >= -1).all())
        WalkOracleHashgraph.walk_calls += 1
        WalkOracleHashgraph.capped_calls += cap is not None
        return g.walk(head, known, cap)


def test_ask_sync_by_the_walk_equals_the_host_bfs_at_every_call(pkg, monkeypatch):
    monkeypatch.setattr(pkg.node, "Hashgraph", WalkOracleHashgraph)
    WalkOracleHashgraph.walk_calls = WalkOracleHashgraph.capped_calls = 0
    crypto, loads = pkg.node.crypto, pkg.node.loads
    assert pkg.Node.device_sync_walk is False
    calls = []

    def checked(nd):
        def ask(pk, info):
            nd.device_sync_walk = False
            host = nd.ask_sync(pk, info)
            nd.device_sync_walk = True
            walk = nd.ask_sync(pk, info)
            nd.device_sync_walk = False
            (h0, s0), (h1, s1) = loads(crypto.sign_open(host, nd.pk)), loads(crypto.sign_open(walk, nd.pk))
            assert h0 == h1 and set(s0) == set(s1) and all(s0[k] == s1[k] for k in s0)
            idx = [nd._index[k] for k in s1]
            assert idx == sorted(idx)                      # the reply is filled in ascending dense index
            calls.append((len(s0), nd._dev.exact))
            return host
        return ask

    with contextlib.redirect_stdout(io.StringIO()):
        a, b, c, rest = _seven_nodes(pkg)
        for nd in [a, b, c] + rest:
            nd.network[nd.pk] = checked(nd)
        hb = b.head
        h1, e1 = b.new_event(b"one", (hb, b._chain_head[a.pk]))
        h2, e2 = b.new_event(b"two", (hb, b._chain_head[c.pk]))   # same self-parent: B equivocates
        a.add_event(h1, e1)
        a.add_event(h2, e2)
        ha = _build_on(a, h1, b"on-one")
        a.divide_rounds((h1, h2, ha))
        c.add_event(h2, e2)
        hc = _build_on(c, h2, b"on-two")
        c.divide_rounds((h2, hc))
        new = c.sync(a.pk, b"after-fork")          # A answers with the cap: C receives the sibling of equal height
        assert h1 in c.hg and ha in c.hg
        c.divide_rounds(new)
        rng = random.Random(7)
        honest = [a, c] + rest
        for _ in range(120):
            x, y = rng.sample(honest, 2)
            x.divide_rounds(x.sync(y.pk, b"more"))
    assert len(calls) > 100 and WalkOracleHashgraph.walk_calls == len(calls)
    assert WalkOracleHashgraph.capped_calls > 50 and any(exact for _, exact in calls) and any(k > 1 for k, _ in calls)
    assert hc in a.hg and all(h1 in nd.hg and h2 in nd.hg for nd in honest)
