"""CPU: the fixtures of tests/golden/network/ — the UNMODIFIED reference's own simulation test(n, turns), recorded by
tests/golden/make_network_golden.py — replayed through the Python model of the turn (tests/model_batch_network.py) and the C
oracle per view: the schedule the reference took, its timestamps and its signatures go in, and every recorded field must come
out equal: the network's DAG by event number, and per node the events held, their rounds, the witnesses, fame, the decided
rounds, the ordered transactions, tbd and the head's can_see row.  Local indices differ from the reference's storage order
(ascending index of the peer against its toposort); nothing compared depends on them.  tests/test_gpu_batch_network.py runs
the same fixtures on the device."""
import functools
import glob
import os

import numpy as np
import pytest

from conftest import ROOT
import model_batch_network as M

DIR = os.path.join(ROOT, "tests", "golden", "network")
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DIR, "*.npz")))
# (nodes, turns, coin period) the issue names
WANTED = [(3, 120, 6), (4, 250, 6), (5, 300, 6), (7, 400, 6), (4, 250, 2)]


@functools.lru_cache(maxsize=None)
def load(name):
    with np.load(os.path.join(DIR, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def replay(name):
    """The model fed the fixture's schedule, timestamps and signatures; computed once, shared, not modified."""
    g = load(name)
    n = int(g["n"])
    m = M.Network(n, 0, g["t"][:n], g["sig"][:n])
    for k in range(int(g["turns"])):
        m.turn(int(g["puller"][k]), int(g["peer"][k]), g["t"][n + k], g["sig"][n + k])
    return m


def assert_node_equals_fixture(g, i, num, rounds, can_see_head, wit, famous, consensus, tx, tbd):
    """num: the view's event numbers by local index; the other arguments by local index / local event, as a view gives them."""
    n = int(g["n"])
    num = np.asarray(num)
    pre = "node%d_" % i
    held = g[pre + "held"]
    assert sorted(num.tolist()) == sorted(held.tolist()) and len(set(num.tolist())) == len(num), "events held"
    by_number = {int(x): k for k, x in enumerate(num)}
    assert [int(rounds[by_number[int(x)]]) for x in held] == g[pre + "round"].tolist(), "round"
    assert [int(famous[by_number[int(x)]]) for x in held] == g[pre + "famous"].tolist(), "famous"
    to_num = lambda a: np.where(np.asarray(a) >= 0, num[np.maximum(np.asarray(a), 0)], -1)
    assert np.array_equal(to_num(wit), g[pre + "witnesses"]), "witnesses"
    assert np.array_equal(to_num(can_see_head), g[pre + "can_see_head"]), "can_see of the head"
    assert np.flatnonzero(consensus).tolist() == g[pre + "consensus"].tolist(), "consensus"
    assert num[np.asarray(tx, np.int64)].tolist() == g[pre + "transactions"].tolist(), "transactions"
    assert sorted(num[np.flatnonzero(tbd)].tolist()) == g[pre + "tbd"].tolist(), "tbd"
    assert len(rounds) == len(num) and np.asarray(wit).shape[1] == n


def test_the_cases_the_fixtures_cover():
    got = sorted((int(load(nm)["n"]), int(load(nm)["turns"]), int(load(nm)["coin_period"])) for nm in NAMES)
    assert got == sorted(WANTED)


@pytest.mark.parametrize("name", NAMES)
def test_replay_equals_the_reference(name):
    g = load(name)
    n, period = int(g["n"]), int(g["coin_period"])
    m = replay(name)
    # the network's DAG, by event number
    assert [e[0] for e in m.events] == g["creator"].tolist()
    assert [e[1] for e in m.events] == g["self_parent"].tolist() and [e[2] for e in m.events] == g["other_parent"].tolist()
    for i, v in enumerate(m.views):
        o, tx, failed = M.oracle_of_view(n, v, None, period)
        assert failed is None
        N = len(v.cr)
        assert_node_equals_fixture(g, i, v.num, o.round[:N], o.can_see[v.head], o.witnesses(), o.famous_by_event[:N], o.consensus(), tx, o.tbd[:N])


@pytest.mark.parametrize("name", NAMES)
def test_what_makes_the_fixture_worth_having(name):
    """Every node has ordered an event — except at 3 nodes and 120 turns, where the reference alone never does (see the
    generator: 3 nodes decide a witness only on a unanimous vote) and the fixture pins rounds, witnesses and votes cast."""
    g = load(name)
    n = int(g["n"])
    ordered = [len(g["node%d_transactions" % i]) for i in range(n)]
    if (n, int(g["turns"])) == (3, 120):
        assert min(int(g["node%d_round" % i].max()) for i in range(n)) >= 3
    else:
        assert min(ordered) >= 1, ordered
    if int(g["coin_period"]) == 2:
        assert int(g["coin_votes"]) >= 1
