"""Inputs the CPU and the GPU tests of the batch share (tests/test_batch_host.py, tests/test_gpu_batch.py): forked random
streams with their ragged schedules, the oracle's record of a run, and the hashgraph that ends in the reference's
IndexError.  No GPU, no pytest."""
import numpy as np

from oracle.oracle import Oracle, OracleError
from synth_util import synth
from test_exact_host import add_forks


def forked_stream(n, N, seed, forks):
    """A synthetic hashgraph of about N events (each fork adds two); forks = 0 leaves it fork-free."""
    s = synth(n, N, seed)
    return add_forks(s, n, seed, forks) if forks else s


def ragged_schedule(N, seed, lo=1, hi=None):
    """Call sizes that sum to N, each drawn anew between lo and hi."""
    rng = np.random.default_rng(1000 + seed)
    hi = hi or N
    out, left = [], N
    while left:
        k = int(min(left, rng.integers(lo, hi + 1)))
        out.append(k)
        left -= k
    return out


class Record:
    """What the oracle computes for a stream under a schedule: per call (new_c, transactions), or the call that raised."""

    def __init__(self, n, stream, sched, stake=None, coin_period=6):
        cr, sp, op, t, sig = stream
        self.o = o = Oracle(n, stake, coin_period)
        self.calls, self.failed_call, self.error = [], None, None
        a = 0
        for k in sched:
            o.append_events(cr[a:a + k], sp[a:a + k], op[a:a + k], t[a:a + k], sig[a:a + k])
            o.divide_rounds(a, k)
            try:
                nc = o.decide_fame()
                tx = o.find_order(nc)
            except OracleError as e:
                self.failed_call, self.error = len(self.calls), str(e)
                break
            self.calls.append((list(nc), list(tx)))
            a += k


# The frozen hashgraph: 8 members, the "whale" pattern of tests/wide_stake_cases.py (half of the members without stake, one
# member with more than half of the total).  The whale's famous witness alone receives an event, and the median of ONE
# timestamp is the reference's IndexError (swirld.py:305) — here in the third call of a schedule of 50 events per call.
WHALE_N, WHALE_EVENTS, WHALE_SEED, WHALE_CHUNK, WHALE_FAILS_AT = 8, 300, 1, 50, 2


def whale_stake():
    n = WHALE_N
    p = np.random.default_rng(WHALE_SEED).permutation(n)
    st = np.ones(n, np.uint64)
    st[p[:n // 2]] = 0
    st[p[n // 2]] = n - n // 2
    return st


def whale_stream():
    return synth(WHALE_N, WHALE_EVENTS, WHALE_SEED)


# A second one of the same pattern that raises in a LATER round of new_c: 400 events in calls of 200, the second call
# decides several rounds and orders 75 events of the earlier ones before a round raises.  The reference has appended those
# 75 to its transactions by then (swirld.py:307-309 run once per round).
LATE_WHALE_EVENTS, LATE_WHALE_SEED, LATE_WHALE_CHUNK, LATE_WHALE_FAILS_AT, LATE_WHALE_ORDERED_BY_THE_FAILING_CALL = 400, 14, 200, 1, 75


def late_whale_stake():
    n = WHALE_N
    p = np.random.default_rng(LATE_WHALE_SEED).permutation(n)
    st = np.ones(n, np.uint64)
    st[p[:n // 2]] = 0
    st[p[n // 2]] = n - n // 2
    return st


def late_whale_stream():
    return synth(WHALE_N, LATE_WHALE_EVENTS, LATE_WHALE_SEED)
