#!/usr/bin/env python3
"""Records what the UNMODIFIED reference Node keeps on FORKED hashgraphs beyond the order, for
tests/test_gpu_exact_history_node.py, into tests/golden/node/forked_history_*.json.gz: the observer of
test_node_vs_reference.forked_run (same cases, same schedule) — its complete `votes` dict, and the round received
(swirld.py:283) and consensus timestamp (swirld.py:305) of every event it orders.  The two values are locals of find_order:
they are captured as tests/golden/make_consensus_golden.py captures them, by shadowing the name `sorted` in the imported
module around each call, without touching the reference's text.  Events are named by their ids (hex), timestamps are
written as float.hex().  Needs the reference tree (tests/refharness.py); the fixtures are committed.

Usage:  python tests/golden/make_node_history_golden.py
"""
import builtins
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import refharness  # noqa: E402
import test_node_vs_reference as T  # noqa: E402
from make_node_golden import save  # noqa: E402


def capturing(sw, node):
    node.kept = {"rr": {}, "cts": {}}
    plain = node.find_order

    def find_order(new_c):
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
                    assert x not in node.kept["rr"]
                    node.kept["rr"][x] = r
                    node.kept["cts"][x] = key(x)[0]
            return out

        sw.sorted = shadow
        try:
            return plain(new_c)
        finally:
            del sw.sorted

    node.find_order = find_order
    return node


def reference_history(n, steps, seed, n_forks):
    sw = refharness.import_reference()
    import pysodium
    sw.dumps, sw.time = T._class_free_dumps, T._clock()
    obs, calls = T.forked_run(pysodium.crypto_sign_seed_keypair, n, steps, seed, n_forks,
                              lambda kp, n_, stake: capturing(sw, sw.Node(kp, {}, n_, stake)))
    assert list(obs.kept["rr"]) == list(obs.transactions)
    return {"transactions": [h.hex() for h in obs.transactions],
            "votes": [[y.hex(), x.hex(), bool(v)] for y, row in obs.votes.items() for x, v in row.items()],
            "round_received": [int(obs.kept["rr"][h]) for h in obs.transactions],
            "consensus_time": [float(obs.kept["cts"][h]).hex() for h in obs.transactions]}


def main():
    for case in T.FORK_CASES:
        out = reference_history(*case)
        print("%s: %d ordered, %d votes" % (case, len(out["transactions"]), len(out["votes"])))
        save("forked_history_%d_%d_%d_%d" % case, out)


if __name__ == "__main__":
    main()
