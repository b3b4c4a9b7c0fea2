#!/usr/bin/env python3
"""Generates tests/golden/coin_period/<name>_c<k>.npz: the UNMODIFIED reference run with its module constant C
(swirld.py:17, the coin period) set to k instead of 6, on streams STORED in existing goldens (tests/golden/<name>.npz,
some cut to a prefix), on the stored call schedule.  Only the module ATTRIBUTE is set, around each run, and put back;
the file is not touched and nothing of it is copied.

Each fixture stores what make_golden.run_case stores (the stream, the schedule and every piece of Node state, the
complete `votes` array included), and beside it

    coin_period                       k
    coin_votes, coin_flips            how often decide_fame took the coin branch (swirld.py:267-272) and, of those, the
                                      branch that reads the signature bit (:272).  Counted on the running reference: the
                                      inner dicts of Node.votes are a dict subclass that counts assignments at a voter
                                      distance that is a multiple of k, and the name `bool` — used once in the module, on
                                      line 272 — is shadowed by a counting wrapper during decide_fame.  An election that
                                      stays open is evaluated again by later calls; every evaluation counts, as in the
                                      oracle's counters of the same names.
    max_vote_distance                 the largest r_ - r (>= 2) at which majority() was taken (from the same subclass, and one
                                      of Node.famous for the levels that decide and store nothing)
    asis_round_received, asis_consensus_time
                                      per event, of make_consensus_golden.py (its capture, imported unchanged)
    wallclock_*                       the forked cases only: what tests/golden/consensus_forked/ carries
                                      (make_forked_consensus_golden.py), at this period.

And node_sim_<n>_<turns>_<seed>_c<k>.json.gz: the end state of every node of the reference's own gossip simulation
test(n, turns) at C = k, recorded as tests/golden/make_node_golden.py records it at 6 (its reference_simulation, imported
unchanged, in a child process under the fixed hash seed of tests/test_node_vs_reference.py).

Runs only where the reference tree is present (tests/refharness.py); the fixtures hold recorded data only.

Usage:  python tests/golden/make_coin_period_golden.py [--check]     (--check: compare with the stored files, write nothing)
"""
import builtins
import gzip
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

from make_consensus_golden import capture_find_order, load_stored, wallclock_times  # noqa: E402
from refharness import RefRun  # noqa: E402

OUT = os.path.join(HERE, "coin_period")

FORKED = ["n8_s11_forks", "n8_s12_forks_chunk9", "n5_s13_forks_chunk1", "n12_s14_forks_stake_chunk40"]

# stored golden, prefix (None = the whole stream), chunk (None = the stored schedule), periods
CASES = [
    ("n4_s1_batch", None, None, (1, 2, 3, 50)),
    ("n7_s2_chunk13", None, None, (1, 2, 3, 50)),
    ("n16_s8_slow", 1200, None, (2, 3)),
    ("n10_s1_stake", 1000, None, (2, 3)),
    ("n6_s3_stuck_stake", None, None, (2, 3)),
    ("n70_s3_batch", 2500, None, (2, 3)),
    ("n4_s5_chunk1", None, None, (2,)),
] + [(name, None, None, (2, 3)) for name in FORKED]


class CountingVotes(dict):
    """Node.votes[y]: counts the assignments made at a distance that is a multiple of the period (swirld.py:269, 272)."""

    def __init__(self, run, y):
        super().__init__()
        self.run, self.y = run, y

    def __setitem__(self, x, v):
        rnd = self.run.ref.node.round
        d = rnd[self.y] - rnd[x]
        if d >= 2:
            self.run.max_dist = max(self.run.max_dist, d)
            if d % self.run.period == 0:
                self.run.coin_votes += 1
        super().__setitem__(x, v)


class VotesTable(dict):
    """Node.votes itself: a defaultdict whose default knows its key."""

    def __init__(self, run):
        super().__init__()
        self.run = run

    def __getitem__(self, y):
        self.run.last_key = y
        return super().__getitem__(y)

    def __missing__(self, y):
        d = CountingVotes(self.run, y)
        super().__setitem__(y, d)
        return d


class FamousTable(dict):
    """Node.famous: a decision (swirld.py:263) stores no vote; its distance is that of the votes majority() just read
    (Node.votes[w] of the round below the voter's) plus one."""

    def __init__(self, run):
        super().__init__()
        self.run = run

    def __setitem__(self, x, v):
        rnd = self.run.ref.node.round
        self.run.max_dist = max(self.run.max_dist, rnd[self.run.last_key] + 1 - rnd[x])
        super().__setitem__(x, v)


class PeriodRun:
    def __init__(self, g, period, t):
        self.g, self.period, self.t = g, int(period), t
        self.coin_votes = self.coin_flips = self.max_dist = 0

    def decide_fame(self):
        sw = self.ref.sw
        real_majority = sw.majority
        run = self

        def counting_bool(v):
            run.coin_flips += 1
            return builtins.bool(v)

        sw.bool = counting_bool
        try:
            return self.ref.decide_fame()
        finally:
            del sw.bool
            assert sw.majority is real_majority

    def run(self):
        g, t = self.g, self.t
        n, N = int(g["n"]), len(g["creator"])
        chunk = int(g["chunk"]) or N
        cr, sp, op, sig = g["creator"], g["self_parent"], g["other_parent"], g["sig"]
        self.ref = ref = RefRun(n, g["stake"])
        ref.node.votes = VotesTable(self)
        ref.node.famous = FamousTable(self)
        old_c = ref.sw.C
        ref.sw.C = self.period
        rr = np.full(N, -1, np.int32)
        cts = np.full(N, np.nan, np.float64)
        new_c_flat, new_c_off, tx_off = [], [0], [0]
        try:
            for a in range(0, N, chunk):
                b = min(N, a + chunk)
                ref.append(cr[a:b], sp[a:b], op[a:b], t[a:b], sig[a:b])
                ref.divide_rounds(a, b - a)
                nc = self.decide_fame()
                capture_find_order(ref, nc, rr, cts)
                new_c_flat += list(nc)
                new_c_off.append(len(new_c_flat))
                tx_off.append(len(ref.node.transactions))
        finally:
            ref.sw.C = old_c
        ex = ref.extract()
        return ex, rr, cts, new_c_flat, new_c_off, tx_off


def record(g, period):
    pr = PeriodRun(g, period, g["t"])
    ex, rr, cts, new_c_flat, new_c_off, tx_off = pr.run()
    n, N = int(g["n"]), len(g["creator"])
    wo_flat = np.concatenate(ex["wit_order"]) if ex["wit_order"] else np.zeros(0, np.int32)
    wo_off = np.cumsum([0] + [len(o) for o in ex["wit_order"]]).astype(np.int32)
    return dict(
        n=np.int32(n), stake=np.asarray(g["stake"], np.uint64), chunk=np.int64(int(g["chunk"]) or N),
        creator=g["creator"], self_parent=g["self_parent"], other_parent=g["other_parent"], t=g["t"], sig=g["sig"],
        round=ex["round"], height=ex["height"], can_see=ex["can_see"],
        witnesses=ex["witnesses"], wit_order_flat=wo_flat.astype(np.int32), wit_order_off=wo_off,
        famous=ex["famous"], consensus=ex["consensus"], votes=ex["votes"],
        transactions=ex["transactions"], tbd=ex["tbd"],
        new_c_flat=np.array(new_c_flat, np.int32), new_c_off=np.array(new_c_off, np.int32),
        tx_off=np.array(tx_off, np.int64),
        coin_period=np.int32(period), coin_votes=np.int64(pr.coin_votes), coin_flips=np.int64(pr.coin_flips),
        max_vote_distance=np.int32(pr.max_dist), asis_round_received=rr, asis_consensus_time=cts)


def record_wallclock(g, period, seed):
    tw = wallclock_times(len(g["creator"]), seed)
    assert np.all(np.diff(tw) > 0)
    ex, rr, cts, _, _, tx_off = PeriodRun(g, period, tw).run()
    return dict(wallclock_t=tw, wallclock_transactions=ex["transactions"], wallclock_tx_off=np.array(tx_off, np.int64),
                wallclock_round_received=rr, wallclock_consensus_time=cts)


def cut(g, prefix):
    if prefix is None:
        return g
    assert int(g["chunk"]) >= len(g["creator"]), "a prefix of a one-call stream only"
    g = dict(g)
    for k in ("creator", "self_parent", "other_parent", "t", "sig"):
        g[k] = g[k][:prefix]
    g["chunk"] = np.int64(prefix)
    return g


NODE_SIMS = [(4, 250, 11, 3)]   # nodes, turns, seed, period


def node_sim_name(n, turns, seed, k):
    return "node_sim_%d_%d_%d_c%d" % (n, turns, seed, k)


def node_simulation(n, turns, seed, k):
    """(child process) make_node_golden.reference_simulation with the reference's C set to k around it"""
    import make_node_golden
    import refharness
    sw = refharness.import_reference()
    old_c = sw.C
    sw.C = k
    try:
        return make_node_golden.reference_simulation(n, turns, seed)
    finally:
        sw.C = old_c


def main_node_sims(check):
    import test_node_vs_reference as T
    for case in NODE_SIMS:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--node-sim"] + [str(a) for a in case], check=True,
                           capture_output=True, text=True, env=dict(os.environ, PYTHONHASHSEED=T.HASH_SEED))
        obj = json.loads(p.stdout.strip().splitlines()[-1])
        path = os.path.join(OUT, node_sim_name(*case) + ".json.gz")
        if check:
            with gzip.open(path, "rt") as f:
                assert json.load(f) == obj, path
        else:
            with gzip.GzipFile(path, "wb", mtime=0) as f:
                f.write(json.dumps(obj, separators=(",", ":")).encode())
        print("%-36s events per node %s  ordered %s  %6.1f KB" % (
            os.path.basename(path), obj["hg_sizes"], [len(dict(nd)["transactions"]) for nd in obj["nodes"]], os.path.getsize(path) / 1024))


def case_names():
    return ["%s_c%d" % (name, k) for name, _, _, periods in CASES for k in periods]


def main(check=False):
    os.makedirs(OUT, exist_ok=True)
    for name, prefix, chunk, periods in CASES:
        g = cut(load_stored(name), prefix)
        if chunk is not None:
            g["chunk"] = np.int64(chunk)
        for k in periods:
            t0 = time.time()
            out = record(g, k)
            if name in FORKED:
                out.update(record_wallclock(g, k, 7400 + 10 * FORKED.index(name) + k))
            path = os.path.join(OUT, "%s_c%d.npz" % (name, k))
            if check:
                with np.load(path) as z:
                    assert sorted(z.files) == sorted(out), path
                    for f in z.files:
                        assert np.array_equal(z[f], out[f], equal_nan=z[f].dtype.kind == "f"), (path, f)
            else:
                np.savez_compressed(path, **out)
            print("%-36s N=%5d calls=%4d R=%3d consensus=%3d tx=%5d votes=%6d coin %6d / by the bit %6d  dist %2d  %5.1f s %6.1f KB" % (
                os.path.basename(path), len(out["creator"]), len(out["new_c_off"]) - 1, out["witnesses"].shape[0],
                int(out["consensus"].sum()), len(out["transactions"]), len(out["votes"]), int(out["coin_votes"]),
                int(out["coin_flips"]), int(out["max_vote_distance"]), time.time() - t0, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--node-sim"]:
        print(json.dumps(node_simulation(*[int(a) for a in sys.argv[2:6]])))
    else:
        main(check="--check" in sys.argv[1:])
        main_node_sims(check="--check" in sys.argv[1:])
