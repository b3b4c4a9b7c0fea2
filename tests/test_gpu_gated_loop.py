"""GPU (-m gpu): the gated round loop (SW_GATED=1, the default) — ONE round loop per large divide_rounds call, which waits on
the device for the can_see sweep of each sub-batch instead of running one loop per sub-batch.  Members whose visible chain
ends before their next-round event wait in the round in progress until the sweep publishes more events; the results must
be exactly the reference algorithm's (oracle) and exactly those of the per-sub-batch loops (SW_GATED=0), for several cut
plans, short first shots (SW_SHOT_PCT=50: every call tops up) and incremental call schedules that end mid-round."""
import numpy as np
import pytest

from oracle_pool import compare_state
from synth_util import silence

pytestmark = pytest.mark.gpu


def run(pkg, n, stream, chunk, env, monkeypatch):
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        h = pkg.Hashgraph(n)   # (knobs are read when the context is created)
    N = len(stream[0])
    h.reserve(N)
    ncs = []
    for a in range(0, N, chunk):
        b = min(N, a + chunk)
        h.append_events(*[x[a:b] for x in stream])
        h.divide_rounds(a, b - a)
        ncs.append([int(r) for r in h.decide_fame()])
    return h, ncs


def oracle_run(n, stream, chunk):
    from oracle.oracle import Oracle
    o = Oracle(n)
    N = len(stream[0])
    ncs = []
    for a in range(0, N, chunk):
        b = min(N, a + chunk)
        o.append_events(*[x[a:b] for x in stream])
        o.divide_rounds(a, b - a)
        ncs.append([int(r) for r in o.decide_fame()])
    return o, ncs


CUTS_12 = ",".join("%.4f" % (k / 12) for k in range(1, 12))


@pytest.mark.parametrize("n,N,seed,mode,p0,p1,env", [
    (8, 70000, 31, 0, 0, 0, {}),
    (64, 100000, 32, 0, 0, 0, {}),
    (64, 100000, 33, 2, 0.3, 0.03, {}),                      # coin-round stress
    (128, 100000, 34, 1, 0.5, 0.02, {"SW_CUTS": "0.5"}),      # two cliques, 2 sub-batches
    (200, 120000, 35, 0, 0, 0, {"SW_CUTS": CUTS_12}),         # 12 sub-batches
    (256, 120000, 36, 0, 0, 0, {"SW_CUTS": "0.04,0.2,0.4,0.6,0.8"}),   # a head of ~4 k events
    (256, 120000, 37, 0, 0, 0, {"SW_SHOT_PCT": "50"}),        # short first shots: top-ups
])
def test_gated_loop_matches_oracle(pkg, monkeypatch, n, N, seed, mode, p0, p1, env):
    stream = pkg.synth_hashgraph(n, N, seed, mode, p0, p1)
    o, onc = oracle_run(n, stream, N)
    for k, v in env.items():   # (SW_CUTS is read by every divide_rounds call, not when the context is created: set for the whole test)
        monkeypatch.setenv(k, v)
    h, ncs = run(pkg, n, stream, N, dict(env, SW_GATED="1"), monkeypatch)
    assert h.counters()["gated_calls"] == 1, "the call must take the gated loop"
    assert ncs == onc
    assert o.max_round >= 3, "the case must span several rounds"
    compare_state(h, o, N, can_see_step=20_000)
    assert np.array_equal(h.find_order(ncs[0]), o.find_order(onc[0]))
    h.close()


def digest(h):
    wit = h.witnesses()
    m = wit >= 0
    return h.rounds().copy(), wit.copy(), h.famous()[m].copy()


@pytest.mark.parametrize("n,N,chunk,seed,mode,p0,p1", [
    (64, 210000, 70001, 41, 0, 0, 0),        # calls that end mid-round
    (256, 200000, 66667, 42, 0, 0, 0),
    (128, 200000, 99991, 43, 2, 0.3, 0.03),
])
def test_gated_equals_per_subbatch_loops_incremental(pkg, monkeypatch, n, N, chunk, seed, mode, p0, p1):
    stream = pkg.synth_hashgraph(n, N, seed, mode, p0, p1)
    hg, ncg = run(pkg, n, stream, chunk, {"SW_GATED": "1"}, monkeypatch)
    hu, ncu = run(pkg, n, stream, chunk, {"SW_GATED": "0"}, monkeypatch)
    big = sum(1 for a in range(0, N, chunk) if min(N, a + chunk) - a >= 65536)
    assert hg.counters()["gated_calls"] == big, "every call of >= 64 k events takes the gated loop"
    assert hu.counters()["gated_calls"] == 0
    assert ncg == ncu
    for a, b in zip(digest(hg), digest(hu)):
        assert np.array_equal(a, b)
    o, onc = oracle_run(n, stream, chunk)
    assert ncg == onc
    compare_state(hg, o, N, can_see_step=40_000)
    hg.close()
    hu.close()


@pytest.mark.parametrize("n,N,member,frac", [(64, 150000, 5, 0.4), (256, 200000, 17, 0.5)])
def test_gated_loop_member_falls_silent(pkg, monkeypatch, n, N, member, frac):
    """A member that stops gossiping mid-call: its chain stops growing in an early sub-batch, so it is exhausted there and
    does not hold the later rounds back (the loop must not wait for the last sweep)."""
    stream = silence(pkg.synth_hashgraph(n, N, 51), member, int(N * frac))
    N = len(stream[0])
    o, onc = oracle_run(n, stream, N)
    hg, ncg = run(pkg, n, stream, N, {"SW_GATED": "1"}, monkeypatch)
    hu, ncu = run(pkg, n, stream, N, {"SW_GATED": "0"}, monkeypatch)
    assert hg.counters()["gated_calls"] == 1
    assert ncg == onc and ncu == onc
    compare_state(hg, o, N, can_see_step=20_000)
    for a, b in zip(digest(hg), digest(hu)):
        assert np.array_equal(a, b)
    hg.close()
    hu.close()


def test_gated_full_size_256x1M(pkg, monkeypatch):
    """bench.py's workload: every row and the order against the per-sub-batch loops; the working iterations at most the
    single-loop count (SW_PIPE=1: one sub-batch, nothing to wait for) + 2."""
    n, N = 256, 1_000_000
    stream = pkg.synth_hashgraph(n, N, 3)
    res = {}
    for name, env in (("split", {"SW_GATED": "0"}), ("gated", {"SW_GATED": "1"}), ("single", {"SW_PIPE": "1"})):
        h, nc = run(pkg, n, stream, N, env, monkeypatch)
        c0 = h.counters()
        h.rewind()   # a second pass: the first shot is sized from the first one
        h.divide_rounds(0, N)
        nc2 = [int(r) for r in h.decide_fame()]
        assert nc2 == nc[0]
        c1 = h.counters()
        its = (c1["round_iterations"] - c0["round_iterations"]) - (c1["gated_idle_iterations"] - c0["gated_idle_iterations"])
        res[name] = (digest(h), nc[0], h.find_order(nc[0]), its, c1["gated_calls"])
        h.close()
    assert res["gated"][4] == 2 and res["split"][4] == 0 and res["single"][4] == 0
    for a, b in zip(res["split"][0], res["gated"][0]):
        assert np.array_equal(a, b)
    assert res["split"][1] == res["gated"][1]
    assert np.array_equal(res["split"][2], res["gated"][2])
    # no round searched twice
    assert res["gated"][3] <= res["single"][3] + 2, (res["gated"][3], res["single"][3], res["split"][3])
    assert res["gated"][3] < res["split"][3], (res["gated"][3], res["split"][3])
