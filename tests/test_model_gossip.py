"""CPU: tests/model_gossip.py against the reference's own statements, on oracle states.  For random (head, asker) pairs,
the asker's heights taken from its can_see row as Node.sync does (swirld.py:125-126), the model's exported SET equals
ask_sync's height-pruned BFS (swirld.py:154-161), restated here on dense indices; the slots come member-major and in
chain order, and carry the parents' ids (zeros for a root)."""
from collections import deque

import numpy as np
import pytest

import model_gossip as mg


def bfs_subset(head, sp, op, cr, ht, known):
    """swirld.py:154-161 with utils.bfs (utils.py:24-34): walk back from the head, not into what the asker knows."""
    seen, q = {head}, deque([head])
    while q:
        u = q.popleft()
        for p in (sp[u], op[u]):
            if p < 0:
                continue
            if (known[cr[p]] < 0 or ht[p] > known[cr[p]]) and p not in seen:
                seen.add(p)
                q.append(p)
    return seen


@pytest.mark.parametrize("n,N,seed,mode,p0,p1", [(5, 300, 701, 0, 0, 0), (40, 4000, 702, 2, 0.3, 0.02), (130, 8000, 703, 3, 0.6, 0)])
def test_model_equals_the_reference_walk(pkg, n, N, seed, mode, p0, p1):
    from oracle.oracle import Oracle
    cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, seed, mode, p0, p1)
    o = Oracle(n)
    o.append_events(cr, sp, op, t, sig)
    o.divide_rounds(0, N)
    g = mg.Graph(n, cr, sp, op, t, sig)
    ht, cs = np.asarray(o.height), np.asarray(o.can_see)
    assert np.array_equal(g.height, ht)
    rng = np.random.default_rng(seed)
    spl, opl, crl, htl = sp.tolist(), op.tolist(), cr.tolist(), ht.tolist()
    pairs = [(int(rng.integers(n, N)), int(rng.integers(0, N))) for _ in range(20)] + [(N - 1, 0), (N - 1, N - 1)]
    for head, asker in pairs:
        assert np.array_equal(g.row(head), cs[head]) and np.array_equal(g.row(asker), cs[asker])
        known = g.known_heights(asker)
        assert np.array_equal(known, np.where(cs[asker] >= 0, ht[np.maximum(cs[asker], 0)], -1))
        x = g.export(head, known)
        ev = x["event"].astype(np.int64)
        assert len(set(ev.tolist())) == len(ev)
        assert set(ev.tolist()) == bfs_subset(head, spl, opl, crl, htl, known.tolist())
        # member-major, chain order inside a member; the ranges add up
        key = cr[ev].astype(np.int64) * N + ev
        assert np.all(np.diff(key) > 0)
        assert len(ev) == int((x["end"] - x["first"]).sum()) and np.array_equal(x["creator"], cr[ev])
        for m in range(n):
            assert np.array_equal(ev[cr[ev] == m], g.chains[m][x["first"][m]:x["end"][m]])
        # contents
        assert np.array_equal(x["ids"], g.ids[ev]) and np.array_equal(x["t"], t[ev]) and np.array_equal(x["sig"], sig[ev])
        root = sp[ev] < 0
        assert np.array_equal(x["arity"], np.where(root, 0, 2))
        assert not x["sp_ids"][root].any() and not x["op_ids"][root].any()
        assert np.array_equal(x["sp_ids"][~root], g.ids[sp[ev][~root]]) and np.array_equal(x["op_ids"][~root], g.ids[op[ev][~root]])
    # an asker that knows nobody gets every ancestor of the head; asker == head gets the head alone
    allx = g.export(N - 1, None)
    assert set(allx["event"].tolist()) == bfs_subset(N - 1, spl, opl, crl, htl, [-1] * n)
    assert g.export(N - 1, g.known_heights(N - 1))["event"].tolist() == [N - 1]
    assert g.export(N // 2, np.full(n, 2**31 - 1, np.int32))["event"].tolist() == [N // 2]
