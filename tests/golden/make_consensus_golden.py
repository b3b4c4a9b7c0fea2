#!/usr/bin/env python3
"""Generates tests/golden/consensus/<name>.npz: the round received and the consensus timestamp the UNMODIFIED reference
computes for every event it orders (swirld.py:283 `r`, swirld.py:305 `ts[x]`), for every fork-free case of
make_golden.py's CASES.  The reference keeps neither value (both are locals of find_order), so they are captured without
touching its text: around each find_order call the name `sorted` is shadowed in the imported module —

    the call without `key`            is sorted(new_c) (swirld.py:283): the rounds of this call, in order;
    each later call, with `key`       is one of those rounds (swirld.py:306): its items are the events the round
                                      receives, and key(x)[0] is ts[x].

Runs only where the reference tree is present (tests/refharness.py), like the other generators; the fixtures hold
recorded data only.

Two variants per case, in one file:
    asis_*        the stored stream and schedule of tests/golden/<name>.npz (t = float(index): every median is an integer
                  or a half): asis_round_received[N] (-1 = not ordered), asis_consensus_time[N] (NaN = not ordered).
    wallclock_*   the same stream with t replaced by wall-clock-like doubles, increasing with the index
                  (1.7e9 + 0.013 * index + seeded jitter below 0.013): at 1.7e9 the sum of two timestamps rounds, so another
                  formula for the mean shows up bit for bit.  wallclock_t[N], the resulting wallclock_transactions and
                  wallclock_tx_off, wallclock_round_received[N], wallclock_consensus_time[N].

Usage:  python tests/golden/make_consensus_golden.py
"""
import builtins
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

from make_golden import CASES  # noqa: E402
from refharness import RefRun  # noqa: E402

OUT = os.path.join(HERE, "consensus")


def wallclock_times(N, seed):
    rng = np.random.default_rng(seed)
    return 1.7e9 + 0.013 * np.arange(N) + rng.uniform(0.0, 0.0129, N)


def load_stored(name):
    with np.load(os.path.join(HERE, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def capture_find_order(ref, new_c, rr, cts):
    """ref.find_order(new_c) with `sorted` shadowed in the reference module; fills rr / cts of the events it orders."""
    state = {"rounds": None, "k": 0}

    def shadow(it, key=None, reverse=False):
        out = builtins.sorted(it, key=key, reverse=reverse)
        if key is None:
            assert state["rounds"] is None
            state["rounds"] = list(out)
        else:
            r = state["rounds"][state["k"]]
            state["k"] += 1
            for x in out:
                e = ref.id_index[x]
                assert rr[e] == -1
                rr[e] = r
                cts[e] = key(x)[0]
        return out

    ref.sw.sorted = shadow
    try:
        got = ref.find_order(new_c)
    finally:
        del ref.sw.sorted
    assert state["rounds"] == builtins.sorted(new_c) and state["k"] == len(state["rounds"])
    return got


def run(g, t):
    n, N = int(g["n"]), len(g["creator"])
    chunk = int(g["chunk"]) or N
    cr, sp, op, sig = g["creator"], g["self_parent"], g["other_parent"], g["sig"]
    ref = RefRun(n, g["stake"])
    rr = np.full(N, -1, np.int32)
    cts = np.full(N, np.nan, np.float64)
    tx_off = [0]
    for a in range(0, N, chunk):
        b = min(N, a + chunk)
        ref.append(cr[a:b], sp[a:b], op[a:b], t[a:b], sig[a:b])
        ref.divide_rounds(a, b - a)
        capture_find_order(ref, ref.decide_fame(), rr, cts)
        tx_off.append(len(ref.node.transactions))
    tx = np.array([ref.id_index[h] for h in ref.node.transactions], np.int32)
    ordered = np.zeros(N, bool)
    ordered[tx] = True
    assert np.array_equal(ordered, rr >= 0) and np.array_equal(ordered, ~np.isnan(cts))
    return tx, np.array(tx_off, np.int64), rr, cts


def main():
    os.makedirs(OUT, exist_ok=True)
    for k, case in enumerate(CASES):
        name = case[0]
        g = load_stored(name)
        t0 = time.time()
        tx, tx_off, rr, cts = run(g, g["t"])
        assert np.array_equal(tx, g["transactions"]) and np.array_equal(tx_off, g["tx_off"]), name   # the capture changes nothing
        tw = wallclock_times(len(g["creator"]), 7000 + k)
        assert np.all(np.diff(tw) > 0)
        wtx, wtx_off, wrr, wcts = run(g, tw)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, asis_round_received=rr, asis_consensus_time=cts, wallclock_t=tw, wallclock_transactions=wtx,
                            wallclock_tx_off=wtx_off, wallclock_round_received=wrr, wallclock_consensus_time=wcts)
        print("%-24s ordered %5d / %5d   wallclock ordered %5d   %5.1f s  %6.1f KB" % (
            name, len(tx), len(rr), len(wtx), time.time() - t0, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
