#!/usr/bin/env python3
"""Generates tests/golden/network/net_<n>_<turns>_<seed>_c<C>.npz: the UNMODIFIED reference's own gossip simulation
test(n, turns) (swirld.py:331-345), run through tests/refharness.py with the pysodium stand-in and the clock, pickling and
hash-seed discipline of make_node_golden.py, recorded for the gossip networks of a batch (tests/test_batch_network_golden.py).
Only module ATTRIBUTES are set around the run (time, dumps, C, and Node.sync wrapped to log who asked whom) and put back; the
file is not touched and nothing of it is copied.  The fixtures hold recorded data only.

Events are named by their creation order inside the network (root i is number i, turn k creates number n + k).  Stored:
    n, turns, seed, coin_period
    puller, peer                       the schedule actually taken (who asked whom), per turn
    creator, self_parent, other_parent per created event, in creation order; parents as numbers (-1: a root)
    t, sig                             its timestamp and its 64 signature bytes
    and per node i (prefix node<i>_): held (the numbers of the events it holds, in its own storage order), round (per held
    event), witnesses ([rounds][n] numbers, -1), famous (per held event: -1 undecided, 0, 1), consensus (rounds),
    transactions (numbers, in order), tbd (numbers), can_see_head ([n] numbers, -1).

The generator ASSERTS what makes a fixture worth having — every node has ordered at least one event (one case excepted, see
CASES); with C = 2 some vote was cast at a distance that is a positive multiple of C, i.e. a coin-round vote (coin_votes
counts them) — and tries seeds upwards from the case's first one until the reference alone satisfies it.

Usage:  python tests/golden/make_network_golden.py [--check]     (--check: compare with the stored files, write nothing)
"""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

OUT = os.path.join(HERE, "network")
# nodes, turns, first seed to try, coin period, whether every node must have ordered an event.
# (3, 120): with 3 nodes of unit stake a witness is decided only when all three voters agree AND each strongly sees all
# three (min_s = 2, "t > min_s" needs t = 3, swirld.py:44, 262), and in 120 turns each node divides about 40 events of its
# own: NO seed in 1..1600 lets every node of test(3, 120) order an event (searched with this file's --sim), so the
# reference alone cannot satisfy the condition there.  The case is recorded all the same, at its first seed: it pins the
# schedule, the DAG, rounds, witnesses, the votes' outcome (nothing famous) and tbd of three views to the reference.
CASES = [(3, 120, 1, 6, 0), (4, 250, 1, 6, 1), (5, 300, 1, 6, 1), (7, 400, 1, 6, 1), (4, 250, 1, 2, 1)]
SEEDS_TRIED = 400


def simulate(n, turns, seed, period, need_order=1):
    """(child process, fixed hash seed) the recorded run as a JSON-able dict, or None where the seed does not qualify"""
    import refharness
    import test_node_vs_reference as T
    sw = refharness.import_reference()
    import pysodium  # the stand-in of tests/_pysodium_standin
    pysodium.set_rng(T._rng_bytes(seed))
    old = (sw.time, sw.dumps, sw.C, sw.Node.sync)
    sw.time, sw.dumps, sw.C = T._clock(), T._class_free_dumps, period
    log = []

    def sync(self, pk, payload):
        out = old[3](self, pk, payload)
        log.append((self.pk, pk, self.head))
        return out
    sw.Node.sync = sync
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            nodes = sw.test(n, turns)
    finally:
        sw.time, sw.dumps, sw.C, sw.Node.sync = old
    mi = {nd.pk: i for i, nd in enumerate(nodes)}
    num, ids = {}, []
    for i, nd in enumerate(nodes):
        root = [h for h, ev in nd.hg.items() if ev.p == () and ev.c == nd.pk]
        assert len(root) == 1
        num[root[0]] = i
        ids.append(root[0])
    for k, (_, _, h) in enumerate(log):
        assert h not in num
        num[h] = n + k
        ids.append(h)
    assert len(log) == turns
    ev_of = {}
    for nd in nodes:
        ev_of.update(nd.hg)
    assert set(ev_of) == set(num)
    if need_order and not all(len(nd.transactions) >= 1 for nd in nodes):
        return None
    # votes[y][x] cast at a distance that is a positive multiple of C (>= 2: at distance 1 the vote is "x in s", swirld.py:257-258)
    coin = sum(1 for nd in nodes for y, d in nd.votes.items() for x in d
               if nd.round[y] - nd.round[x] >= 2 and (nd.round[y] - nd.round[x]) % period == 0)
    if period != 6 and not coin:
        return None
    out = dict(n=n, turns=turns, seed=seed, coin_period=period, coin_votes=coin,
               puller=[mi[a] for a, _, _ in log], peer=[mi[b] for _, b, _ in log],
               creator=[mi[ev_of[h].c] for h in ids], self_parent=[num[ev_of[h].p[0]] if ev_of[h].p else -1 for h in ids],
               other_parent=[num[ev_of[h].p[1]] if ev_of[h].p else -1 for h in ids], t=[ev_of[h].t for h in ids],
               sig=[ev_of[h].s.hex() for h in ids], nodes=[])
    for nd in nodes:
        R = max(nd.witnesses) + 1
        wit = [[-1] * n for _ in range(R)]
        for r, d in nd.witnesses.items():
            for pk, h in d.items():
                wit[r][mi[pk]] = num[h]
        row = [-1] * n
        for pk, h in nd.can_see[nd.head].items():
            row[mi[pk]] = num[h]
        out["nodes"].append(dict(held=[num[h] for h in nd.hg], round=[int(nd.round[h]) for h in nd.hg], witnesses=wit,
                                 famous=[int(nd.famous[h]) if h in nd.famous else -1 for h in nd.hg],
                                 consensus=sorted(int(r) for r in nd.consensus), transactions=[num[h] for h in nd.transactions],
                                 tbd=sorted(num[h] for h in nd.tbd), can_see_head=row))
    return out


def arrays(obj):
    n = obj["n"]
    out = dict(n=np.int32(n), turns=np.int32(obj["turns"]), seed=np.int64(obj["seed"]), coin_period=np.int32(obj["coin_period"]),
               coin_votes=np.int64(obj["coin_votes"]),
               puller=np.array(obj["puller"], np.int32), peer=np.array(obj["peer"], np.int32), creator=np.array(obj["creator"], np.int32),
               self_parent=np.array(obj["self_parent"], np.int32), other_parent=np.array(obj["other_parent"], np.int32),
               t=np.array(obj["t"], np.float64), sig=np.frombuffer(bytes.fromhex("".join(obj["sig"])), np.uint8).reshape(-1, 64))
    for i, nd in enumerate(obj["nodes"]):
        for k, dt in (("held", np.int32), ("round", np.int32), ("famous", np.int8), ("consensus", np.int32), ("transactions", np.int32),
                      ("tbd", np.int32), ("can_see_head", np.int32)):
            out["node%d_%s" % (i, k)] = np.array(nd[k], dt)
        out["node%d_witnesses" % i] = np.array(nd["witnesses"], np.int32).reshape(-1, n)
    return out


def case_path(n, turns, seed, period):
    return os.path.join(OUT, "net_%d_%d_%d_c%d.npz" % (n, turns, seed, period))


def main(check=False):
    import test_node_vs_reference as T
    os.makedirs(OUT, exist_ok=True)
    for n, turns, seed0, period, need_order in CASES:
        for seed in range(seed0, seed0 + SEEDS_TRIED):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--sim", str(n), str(turns), str(seed), str(period), str(need_order)], check=True,
                               capture_output=True, text=True, env=dict(os.environ, PYTHONHASHSEED=T.HASH_SEED))
            obj = json.loads(p.stdout.strip().splitlines()[-1])
            if obj is not None:
                break
        else:
            raise SystemExit("no seed in [%d, %d) qualifies for (%d, %d, C = %d)" % (seed0, seed0 + SEEDS_TRIED, n, turns, period))
        out, path = arrays(obj), case_path(n, turns, seed, period)
        if check:
            with np.load(path) as z:
                assert sorted(z.files) == sorted(out), path
                for f in z.files:
                    assert np.array_equal(z[f], out[f]), (path, f)
        else:
            np.savez_compressed(path, **out)
        print("%-28s seed %3d  events per node %s  ordered %s  %5.1f KB" % (
            os.path.basename(path), seed, [len(nd["held"]) for nd in obj["nodes"]], [len(nd["transactions"]) for nd in obj["nodes"]],
            os.path.getsize(path) / 1024))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--sim"]:
        print(json.dumps(simulate(*[int(a) for a in sys.argv[2:7]])))
    else:
        main(check="--check" in sys.argv[1:])
