"""CPU: tests/model_walk.py against itself and against tests/model_gossip.py.  The two definitions of a forked member's
trunk height — the order-independent one the kernel computes, and the arrival-order one of Node._add_event_host — agree
on random forked streams, in index order and in other topological orders, a second root included.  On fork-free streams
the walk's set equals the chain ranges of sw_sync_diff when the heights come from a real can_see row, and is a subset of
them for arbitrary heights — a STRICT subset on a committed case, which the test demands so that it cannot pass
vacuously."""
import heapq

import numpy as np
import pytest

import model_walk as mw
from test_exact_host import add_forks


def forked_graph(pkg, n, N, seed, n_forks, second_root=None):
    stream = add_forks(pkg.synth_hashgraph(n, N, seed), n, seed + 1000, n_forks)
    if second_root is not None:
        stream = mw.with_second_root(stream, second_root, seed)
    return mw.WalkGraph(n, *stream)


def random_topological_order(g, seed):
    rng = np.random.default_rng(seed)
    key = rng.permutation(g.N).tolist()
    kids = [[] for _ in range(g.N)]
    need = [0] * g.N
    for e in range(g.N):
        for p in {g._spl[e], g._opl[e]} - {-1}:
            kids[p].append(e)
            need[e] += 1
    ready = [(key[e], e) for e in range(g.N) if need[e] == 0]
    heapq.heapify(ready)
    out = []
    while ready:
        _, e = heapq.heappop(ready)
        out.append(e)
        for k in kids[e]:
            need[k] -= 1
            if need[k] == 0:
                heapq.heappush(ready, (key[k], k))
    assert len(out) == g.N
    return out


@pytest.mark.parametrize("n,N,seed,n_forks,second_root", [(4, 200, 21, 3, None), (7, 500, 22, 8, 2), (33, 1200, 23, 12, None),
                                                         (12, 600, 24, 0, None), (12, 600, 25, 5, 0)])
def test_trunk_definitions_agree(pkg, n, N, seed, n_forks, second_root):
    g = forked_graph(pkg, n, N, seed, n_forks, second_root)
    a = g.trunks()
    assert np.array_equal(a, g.trunks_by_arrival())
    for k in range(3):
        assert np.array_equal(a, g.trunks_by_arrival(random_topological_order(g, seed + k)))
    if n_forks == 0:
        assert (a == mw.NO_CAP).all()
    else:
        assert (a != mw.NO_CAP).any() and (a[a != mw.NO_CAP] >= -1).all()
    if second_root is not None:
        assert a[second_root] == -1
    # a prefix of the stream is a hashgraph too: the trunk can only go down as events arrive
    assert (g.trunks(g.N // 2) >= a).all()


@pytest.mark.parametrize("n,N,seed,mode,p0,p1", [(5, 300, 31, 0, 0, 0), (33, 1500, 32, 2, 0.3, 0.02), (70, 2500, 33, 3, 0.6, 0)])
def test_real_heights_give_the_chain_ranges(pkg, n, N, seed, mode, p0, p1):
    g = mw.WalkGraph(n, *pkg.synth_hashgraph(n, N, seed, mode, p0, p1))
    rng = np.random.default_rng(seed)
    for head, asker in [(int(rng.integers(n, N)), int(rng.integers(0, N))) for _ in range(8)] + [(N - 1, 0), (N - 1, N - 1), (2, N - 1)]:
        known = g.known_heights(asker)
        w = g.walk(head, known)
        assert np.all(np.diff(w) > 0) and w[-1] == head
        assert set(w.tolist()) == mw.ranges_set(g, head, known)
        assert np.array_equal(g.ancestors_heights(asker), known)
    assert set(g.walk(N - 1).tolist()) == mw.ranges_set(g, N - 1, None)
    assert g.walk(N - 1, np.full(n, mw.NO_CAP)).tolist() == [N - 1]


def test_arbitrary_heights_give_a_subset_and_once_a_strict_one(pkg):
    assert mw.STRICT_CASE in mw.ARBITRARY_CASES
    strict = []
    for case in mw.ARBITRARY_CASES:
        n, N, seed, head, hseed = case
        g = mw.WalkGraph(n, *pkg.synth_hashgraph(n, N, seed))
        known = mw.arbitrary_heights(g, head, hseed)
        w, r = set(g.walk(head, known).tolist()), mw.ranges_set(g, head, known)
        assert w <= r and head in w
        if w < r:
            strict.append(case)
    assert mw.STRICT_CASE in strict


def test_levels_enter_every_event_once_and_the_cap_lowers_the_heights(pkg):
    g = forked_graph(pkg, 7, 500, 41, 6)
    head = g.N - 1
    lv = g.levels(head)
    flat = [e for l in lv for e in l]
    assert len(flat) == len(set(flat)) and lv[0] == [head]
    known = g.ancestors_heights(g.N // 2)
    cap = g.trunks()
    assert (cap != mw.NO_CAP).any()
    a, b = g.walk(head, known), g.walk(head, known, cap)
    assert set(a.tolist()) <= set(b.tolist()) and len(b) > len(a)
    assert np.array_equal(b, g.walk(head, np.minimum(known, cap)))
    x = g.export_walk(head, known, cap)
    assert np.array_equal(x["event"], b) and np.array_equal(x["creator"], g.cr[b])
    root = g.sp[b] < 0
    assert not x["sp_ids"][root].any() and np.array_equal(x["sp_ids"][~root], g.ids[g.sp[b][~root]])
