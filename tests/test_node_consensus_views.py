"""CPU: Node.round_received / Node.consensus_time (py-swirld_amd/node.py), the lazy views over what find_order decided per
event, with the device backend swapped for a CPU one: tests/oracle_backend.py (the backend the other host tests of the Node
use — it has the whole call protocol, which tests/model_backend.py's partition model lacks) plus the two getters, answered
by tests/model_consensus.py from the backend's own state.  A golden stream is fed through the real Node methods
(add_event / divide_rounds / decide_fame / find_order) on the stored schedule: the views hold exactly the events of
Node.transactions, raise KeyError for anything else, give the reference's values (tests/golden/consensus), and fetch every
position once."""
import contextlib
import io
from unittest import mock

import numpy as np
import pytest

import model_consensus as mc
import oracle_backend
from conftest import load_golden
from refharness import event_id, member_pk
from test_model_consensus import load_consensus, same_bits


class ConsensusBackend(oracle_backend.OracleHashgraph):
    """OracleHashgraph + round_received / consensus_time from the model."""
    fetched = 0

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._stake = np.ones(self.n, np.int64) if len(a) < 2 or a[1] is None else np.asarray(a[1], np.int64)
        self._cr, self._sp, self._t, self._seq = [], [], [], []

    def append_events(self, creator, self_parent, other_parent, t=None, sig=None):
        super().append_events(creator, self_parent, other_parent, t, sig)
        self._cr += list(creator); self._sp += list(self_parent); self._t += list(t)

    def find_order(self, rounds):
        self._seq += sorted(int(r) for r in rounds)
        return super().find_order(rounds)

    def _values(self, first, K):
        if self.exact:
            from importlib import import_module
            raise import_module("py-swirld_amd")._lib.SwirldHipError(-95, "not available on the exact (forked-hashgraph) path")
        o = self._o
        type(self).fetched += K
        wit = o.witnesses()
        return mc.consensus_values(np.arange(first, first + K), self._seq, o.can_see, wit, o.famous_table(), np.array(self._cr), np.array(self._sp),
                                   o.height, np.array(self._t), self._stake)

    def round_received(self, first=0, K=None):
        return self._values(first, self.num_events - first if K is None else K)[0]

    def consensus_time(self, first=0, K=None):
        return self._values(first, self.num_events - first if K is None else K)[1]


def node_on_golden(pkg, monkeypatch, name, t, after_call=None):
    """A Node holding the golden stream (ids of tests/refharness.py), driven through the stored schedule."""
    monkeypatch.setattr(pkg.node, "Hashgraph", ConsensusBackend)
    g = load_golden(name)
    n, N = g["n"], len(g["creator"])
    pks = [member_pk(c) for c in range(n)]
    # (no root event of its own, swirld.py:75-80: the stream brings every member's root)
    with mock.patch.object(pkg.Node, "new_event", lambda self, d, p: (None, None)), \
            mock.patch.object(pkg.Node, "add_event", lambda self, h, ev: None), \
            mock.patch.object(pkg.Node, "divide_rounds", lambda self, events: None):
        nd = pkg.Node((pks[0], b"\0" * 64), {}, n, {pk: int(s) for pk, s in zip(pks, g["stake"])})
    ids = [event_id(e) for e in range(N)]
    with contextlib.redirect_stdout(io.StringIO()):
        for call, (a, b) in enumerate(g["batches"]):
            for e in range(a, b):
                p = () if g["self_parent"][e] < 0 else (ids[g["self_parent"][e]], ids[g["other_parent"][e]])
                nd.add_event(ids[e], pkg.node.Event(None, p, float(t[e]), pks[int(g["creator"][e])], bytes(g["sig"][e])))
            nd.divide_rounds(ids[a:b])
            nd.find_order(nd.decide_fame())
            if after_call:
                after_call(nd, call)
    return nd, g, ids


@pytest.mark.parametrize("name,v", [("n7_s2_chunk13", "wallclock"), ("n10_s1_stake", "asis")])
def test_views_hold_exactly_the_ordered_events_with_the_reference_values(pkg, monkeypatch, name, v):
    f = load_consensus(name)
    t = f["wallclock_t"] if v == "wallclock" else load_golden(name)["t"]
    ConsensusBackend.fetched = 0
    nd, g, ids = node_on_golden(pkg, monkeypatch, name, t)
    tx = f["wallclock_transactions"] if v == "wallclock" else g["transactions"]
    rr, cts = f[v + "_round_received"], f[v + "_consensus_time"]
    assert [nd._index[h] for h in nd.transactions] == list(tx) and len(tx) > 100
    for view, exp in ((nd.round_received, rr), (nd.consensus_time, cts)):
        assert list(view) == nd.transactions and len(view) == len(tx)           # keys: the order itself
        got = np.array([view[h] for h in nd.transactions])
        assert same_bits(got, exp[tx]) if exp.dtype == np.float64 else np.array_equal(got, exp[tx])
        assert dict(view.items()) == {h: view[h] for h in nd.transactions}
    assert type(nd.round_received[nd.transactions[0]]) is int and type(nd.consensus_time[nd.transactions[0]]) is float
    # KeyError: a stored event that is not ordered yet, and an unknown id
    pending = [h for h in ids if h not in nd.idx]
    assert pending
    for key in (pending[0], pending[-1], b"\0" * 32):
        for view in (nd.round_received, nd.consensus_time):
            assert key not in view
            with pytest.raises(KeyError):
                view[key]
    # cached: looking again asks the backend for nothing
    before = ConsensusBackend.fetched
    assert nd.round_received[nd.transactions[-1]] == int(rr[tx[-1]]) and len(nd.consensus_time) == len(tx)
    assert ConsensusBackend.fetched == before


def test_views_extend_with_later_calls(pkg, monkeypatch):
    """looked at after every find_order call, the views grow by that call's positions, and only those are fetched"""
    name = "n4_s6_chunk7"
    f, g0 = load_consensus(name), load_golden(name)
    sizes = []

    def look(nd, call):
        sizes.append(len(nd.round_received))
        if nd.transactions:
            h = nd.transactions[-1]
            assert nd.consensus_time[h] == f["asis_consensus_time"][nd._index[h]]
            assert nd.round_received[h] == f["asis_round_received"][nd._index[h]]

    ConsensusBackend.fetched = 0
    nd, g, _ = node_on_golden(pkg, monkeypatch, name, g0["t"], after_call=look)
    assert sizes == [int(x) for x in g["tx_off"][1:]] and sizes[-1] == len(nd.transactions) > 0
    assert len(set(sizes)) >= 4                                  # several calls ordered something, each extended the views
    # every position was asked for once: a range of events per growing call, never the whole stream again
    assert ConsensusBackend.fetched < 2 * 4 * len(g["creator"])


def test_exact_path_raises_not_implemented(pkg, monkeypatch):
    nd, g, ids = node_on_golden(pkg, monkeypatch, "n4_s1_batch", load_golden("n4_s1_batch")["t"])
    assert len(nd.round_received) > 0
    nd._dev.exact = True          # what a stored forked event does to the real context
    for view in (nd.round_received, nd.consensus_time):
        with pytest.raises(NotImplementedError, match="exact"):
            view[nd.transactions[0]]
        with pytest.raises(NotImplementedError):
            len(view)
        with pytest.raises(NotImplementedError):
            list(view)
