"""CPU: everything that takes a coin period and runs on the host, at periods other than the reference's own 6, against
tests/golden/coin_period/ — the UNMODIFIED reference run with its module constant C set to 1, 2, 3 or 50
(tests/golden/make_coin_period_golden.py).  At period 2 or 3 the coin branch (swirld.py:267-272) is the second or third
level of every election, so that hashgraphs of a few hundred events hold thousands of coin votes; at 1 every level from
the second on is a coin round and nothing is ever decided; at 50 there is none.

  * the oracle (oracle/swirld_oracle.c), every field — on which the GPU tests of tests/test_gpu_coin_period.py rest;
  * the numpy models of the votes table (tests/model_votes.py) and of the candidate-major elections (tests/model_bulk.py);
  * the host builds of the device code: exact.hip.h (tests/exact_host.cpp), batch.hip.h (tests/batch_host.cpp), both in
    the 1-lane and the 16-fiber build, and the votes kernels (tests/votes_emul.cpp);
  * the drop-in `Node` (py-swirld_amd/node.py), which hands its module constant C to its context: its gossip simulation
    with C = 3 against the reference's own with C = 3 (tests/test_node_vs_reference.py at 6)."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import coin_period_cases as cp
import model_votes as mv
from batch_hostlib import BatchHost
from oracle.oracle import Oracle
from test_batch_host import same_bits
from test_exact_host import ExactHost
from test_model_bulk import check as bulk_check
from test_model_votes import as_set
from test_oracle_golden import replay
from test_votes_kernels_host import emul, run as run_votes_emul  # noqa: F401  (emul: the module's fixture, built once)

import test_node_vs_reference as TN

NAMES = cp.names()
FORKFREE = [nm for nm in NAMES if not cp.is_forked(nm)]


def test_the_cases_the_fixtures_are_to_hold():
    assert len(NAMES) == 25
    for stream in ("n4_s1_batch", "n7_s2_chunk13"):
        assert {"%s_c%d" % (stream, k) for k in (1, 2, 3, 50)} <= set(NAMES)
    for stream in ("n16_s8_slow", "n10_s1_stake", "n6_s3_stuck_stake", "n70_s3_batch") + cp.FORKED:
        assert {"%s_c%d" % (stream, k) for k in (2, 3)} <= set(NAMES)
    assert "n4_s5_chunk1_c2" in NAMES and cp.load("n4_s5_chunk1_c2")["chunk"] == 1


def test_the_reference_itself_cast_coin_votes_of_both_kinds():
    """Non-vacuity, from the fixtures alone (the counts were taken on the running reference)."""
    excepted = []
    for nm in NAMES:
        g = cp.load(nm)
        if g["coin_period"] > 3:
            assert g["coin_votes"] == 0 and g["coin_flips"] == 0, nm      # the period is larger than the number of rounds
            continue
        if nm in cp.NO_ELECTION:
            assert g["witnesses"].shape[0] == 1 and len(g["votes"]) == 0
            excepted.append(nm)
            continue
        assert g["coin_votes"] > 0 and 0 < g["coin_flips"] < g["coin_votes"], (nm, g["coin_votes"], g["coin_flips"])
        if g["coin_period"] == 1:
            assert not g["consensus"].any() and (g["famous"] == -1).all() and len(g["transactions"]) == 0
    assert len(excepted) <= 2
    # a round decided AFTER a coin round, on the small fixtures too
    for nm in ("n4_s1_batch_c3", "n7_s2_chunk13_c3", "n7_s2_chunk13_c2", "n10_s1_stake_c3", "n12_s14_forks_stake_chunk40_c3"):
        g = cp.load(nm)
        assert g["consensus"].any() and g["max_vote_distance"] > g["coin_period"], nm


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference(name):
    g = cp.load(name)
    o = Oracle(g["n"], g["stake"], g["coin_period"])
    replay(o, g)
    assert np.array_equal(o.round, g["round"])
    assert np.array_equal(o.height, g["height"])
    assert np.array_equal(o.can_see, g["can_see"])
    assert np.array_equal(o.witnesses(), g["witnesses"])
    for r, order in enumerate(g["wit_order"]):
        assert np.array_equal(o.witness_order(r), order), "dict order of witnesses[%d]" % r
    assert np.array_equal(o.famous_by_event, g["famous"])
    assert np.array_equal(o.consensus(), g["consensus"])
    assert np.array_equal(o.transactions, g["transactions"])
    assert np.array_equal(o.tbd, g["tbd"])
    assert o.num_votes == len(g["votes"])
    for y, x, v in g["votes"]:
        assert o.vote(y, x) == v
    c = o.counters()
    assert (c["coin_votes"], c["coin_flips"], c["max_vote_distance"]) == (g["coin_votes"], g["coin_flips"], g["max_vote_distance"])


@pytest.mark.parametrize("name", FORKFREE)
def test_votes_model_equals_the_reference_votes(name):
    g = cp.load(name)
    t = mv.model_votes(g, coin_period=g["coin_period"])
    tr = mv.triples(t["row_voter"], t["row_cand_round"], t["exists"], t["value"], g["witnesses"])
    exp = as_set(g["votes"])
    assert len(tr) == len(exp) == len(g["votes"]) == t["n_entries"]
    assert as_set(tr) == exp
    assert not (t["value"] & ~t["exists"]).any()
    assert t["n_coin"] == g["coin_flips"], "the entries the model took from the signature bit, every evaluation counted"
    if g["coin_period"] == 1:
        assert (t["dec_call"] == -1).all()


@pytest.mark.parametrize("name", [nm for nm in FORKFREE if cp.load(nm)["chunk"] >= len(cp.load(nm)["creator"])])
def test_bulk_elections_model_matches_the_reference(name):
    g = cp.load(name)
    new_c, _ = bulk_check(g["n"], g["creator"], g["self_parent"], g["other_parent"], g["sig"], g["stake"].astype(np.int64), g,
                          K=3, MCAP=4 * g["n"], coin_period=g["coin_period"])
    assert list(new_c) == list(g["new_c_flat"])


def _lane_cases():   # (a fiber switch per lane and sync: the many-call schedules stay with the 1-lane build)
    return [pytest.param(nm, lanes, id="%s-%s" % (nm, "16lanes" if lanes else "1lane")) for nm in NAMES for lanes in (False, True)
            if not (lanes and len(cp.load(nm)["batches"]) > 40)]


@pytest.mark.parametrize("name,lanes", _lane_cases())
def test_exact_host_matches_the_reference(name, lanes):
    g = cp.load(name)
    x = ExactHost(g["n"], g["stake"], coin_period=g["coin_period"], lanes=lanes)
    for call, (a, b) in enumerate(g["batches"]):
        x.append_events(g["creator"][a:b], g["self_parent"][a:b], g["other_parent"][a:b], g["t"][a:b], g["sig"][a:b])
        x.divide_rounds(a, b - a)
        nc = x.decide_fame()
        assert list(nc) == cp.new_c_of(g, call), call
        assert list(x.find_order(nc)) == cp.tx_of(g, call), call
    st = x.state()
    assert np.array_equal(st["round"], g["round"])
    assert np.array_equal(st["can_see"], g["can_see"])
    assert np.array_equal(st["wit"], g["witnesses"])
    for r, order in enumerate(g["wit_order"]):
        assert np.array_equal(st["worder"][r], order)
    assert np.array_equal(st["fam"], g["famous"])
    assert np.array_equal(st["cons"], g["consensus"])
    assert np.array_equal(st["tbd"], g["tbd"])


@pytest.mark.parametrize("name,lanes", _lane_cases())
def test_batch_step_host_matches_the_reference(name, lanes):
    """The fixture in the middle of a batch of three created with its period; the neighbours stay as created."""
    g = cp.load(name)
    n, N = g["n"], len(g["creator"])
    stake = np.ones((3, n), np.uint64)
    stake[1] = g["stake"]
    x = BatchHost(3, n, stake, coin_period=g["coin_period"], cap_events=N, lanes=lanes)
    for call, (a, b) in enumerate(g["batches"]):
        x.append(1, g["creator"][a:b], g["self_parent"][a:b], g["other_parent"][a:b], g["t"][a:b], g["sig"][a:b])
        nc, tx = x.step(1, b - a)
        assert list(nc) == cp.new_c_of(g, call), call
        assert list(tx) == cp.tx_of(g, call), call
    st = x.state(1)
    assert np.array_equal(st["height"], g["height"])
    assert np.array_equal(st["round"], g["round"])
    assert np.array_equal(st["can_see"], g["can_see"])
    assert np.array_equal(st["wit"], g["witnesses"])
    for r, order in enumerate(g["wit_order"]):
        assert np.array_equal(st["worder"][r], order)
    assert np.array_equal(st["fam"], g["famous"])
    assert np.array_equal(st["cons"], g["consensus"])
    assert np.array_equal(st["tbd"], g["tbd"])
    ev, rr, ts = x.log(1)
    assert np.array_equal(ev, g["transactions"])
    assert np.array_equal(rr, g["asis_round_received"][ev])
    assert same_bits(ts, g["asis_consensus_time"][ev])
    assert len(ev) == int((g["asis_round_received"] >= 0).sum())
    for b in (0, 2):
        assert x.summary(b) == dict(divided=0, rounds=0, ordered=0, n_new=0, n_out=0, stage=0, code=0, event=0)


@pytest.mark.parametrize("name", ["n4_s1_batch_c1", "n4_s1_batch_c2", "n4_s1_batch_c3", "n7_s2_chunk13_c2", "n7_s2_chunk13_c3",
                                  "n10_s1_stake_c2", "n10_s1_stake_c3", "n70_s3_batch_c2", "n4_s5_chunk1_c2", "n7_s2_chunk13_c50"])
def test_votes_kernels_on_the_host_reproduce_the_reference_votes(emul, tmp_path, name):   # noqa: F811
    g = cp.load(name)
    k = g["coin_period"]
    t = mv.model_votes(g, coin_period=k)
    seen = t["calls"][-1][1]
    got = run_votes_emul(emul, tmp_path, g, t, 0, seen, coin_period=k)
    assert got["n_rows"] == len(t["row_voter"]) and got["n_entries"] == len(g["votes"])
    tr = mv.triples(got["row_voter"], got["row_cand_round"], got["exists"], got["value"], g["witnesses"])
    assert as_set(tr) == as_set(g["votes"])
    for f in ("row_voter", "row_cand_round", "exists", "value"):
        assert np.array_equal(got[f], t[f]), f


def _node_simulation_child(n, turns, seed, period):
    """The drop-in's simulation with node.C = period (in a child process, as tests/test_node_vs_reference.py runs it)."""
    import importlib
    sys.path[:0] = [TN.ROOT, TN.HERE]
    node = importlib.import_module("py-swirld_amd").node
    old_c = node.C
    node.C = period
    try:
        return TN._mirror_simulation(n, turns, seed)
    finally:
        node.C = old_c


def test_node_simulation_with_period_3_matches_the_reference(pkg):
    n, turns, seed, period = 4, 250, 11, 3
    with gzip.open(os.path.join(cp.GOLDEN_DIR, cp.SUB, "node_sim_%d_%d_%d_c%d.json.gz" % (n, turns, seed, period)), "rt") as f:
        ref = json.load(f)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), str(turns), str(seed), str(period)], capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, PYTHONHASHSEED=TN.HASH_SEED))
    assert p.returncode == 0, p.stderr[-2000:]
    ours = json.loads(p.stdout.strip().splitlines()[-1])
    assert ref["members"] == ours["members"]
    at_6 = TN.load("sim_%d_%d_%d" % (n, turns, seed))
    for a, b, c in zip(ref["nodes"], ours["nodes"], at_6["nodes"]):
        a, b, c = dict(a), dict(b), dict(c)
        for field in ("head", "parents", "rounds", "witnesses", "famous", "consensus", "can_see_head", "tbd", "transactions"):
            assert a[field] == b[field], field
        assert len(a["transactions"]) > 50
        assert a["consensus"] != c["consensus"], "the period changes what this simulation decides: a Node that ignored C would fail"
    assert len(ref["nodes"]) == len(ours["nodes"]) == n


if __name__ == "__main__":
    print(json.dumps(_node_simulation_child(*[int(a) for a in sys.argv[1:5]])))
