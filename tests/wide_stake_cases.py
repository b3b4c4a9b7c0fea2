"""Test scaffolding: the shared case table of the weighted-stake tests at 65 to 1024 members (two to sixteen mask words),
the stake patterns, the pass driver and the comparison function.  tests/test_wide_stake_cases.py proves on the CPU, with the
oracle alone, that every case discriminates a weighted pass from a unit-stake one; tests/test_gpu_wide_stake.py runs the
HIP path on the same cases.  Never imported by the product.

The reference compares a COUNT of members with 2 * tot_stake / 3 (swirld.py:216-219, Q2 of SURVEY.md's appendix), so rounds
advance only while T < 1.5 n: every pattern here is near-unit."""
import importlib
from collections import namedtuple

import numpy as np

from oracle_backend import OracleHashgraph

Case = namedtuple("Case", "name n N seed mode p0 p1 pattern chunk index_error")


def _perm(n, seed):
    return np.random.default_rng(4200 + seed).permutation(n)


def _twos(n, seed):
    st = np.ones(n, np.uint64)
    st[_perm(n, seed)[:n // 10]] = 2
    return st


def _spread(n, seed):
    """3 on a twelfth of the members, 2 on another twelfth: T ~ 1.25 n"""
    st, p, k = np.ones(n, np.uint64), _perm(n, seed), n // 12
    st[p[:k]] = 3
    st[p[k:2 * k]] = 2
    return st


def _edge(res):
    """`spread` with one stake-1 member raised by 0, 1 or 2 so that T % 3 == res: thr3 = floor(2 T / 3) + 1 and 3 x > 2 T
    round differently in each residue"""
    def f(n, seed):
        st, p = _spread(n, seed), _perm(n, seed)
        st[p[2 * (n // 12)]] += np.uint64((res - int(st.sum())) % 3)
        return st
    return f


def _zeros(n, seed):
    """`twos`, and stake 0 on n // 16 other members: a member in the round decision, no weight in any tally"""
    st, p = _twos(n, seed), _perm(n, seed)
    st[p[n // 10:n // 10 + n // 16]] = 0
    return st


def _whale(n, seed):
    """Half of the members without stake and one member that holds more than half of the total — with stakes of at least 1
    such a member needs T >= 2 n - 1, where no round ever completes.  Its famous witness alone receives an event
    (swirld.py:293), and the median of ONE timestamp is the reference's IndexError (swirld.py:305)."""
    st, p = np.ones(n, np.uint64), _perm(n, seed)
    st[p[:n // 2]] = 0
    st[p[n // 2]] = n - n // 2
    return st


PATTERNS = {"twos": _twos, "spread": _spread, "edge0": _edge(0), "edge1": _edge(1), "edge2": _edge(2), "zeros": _zeros, "whale": _whale}


def stake_of(case):
    return PATTERNS[case.pattern](case.n, case.seed)


def mask_words(n):
    nw = 1
    while nw * 64 < n:
        nw *= 2
    return nw


# name, members, events, seed, synth mode, p0, p1, stake pattern, chunk (None: one call), ends in the reference's IndexError
#
# The event counts are the smallest multiples of 1000 (65 to 257 members) / 2000 (449 and 1024 members) at which the
# conditions of tests/test_wide_stake_cases.py hold.  Beside each row, measured with the oracle (that test prints them under -s):
# decided rounds / ordered events / events whose round differs from the unit-stake pass / oracle seconds.
# Condition 4 (an election entry whose stake-weighted vote differs from the head count, tests/model_votes.py) is required up
# to 257 members: the numpy model replays every election level as an [n][n] integer product and takes minutes at 449 and more.
#
# At 130 members `spread` has T = 160 = 1 (mod 3) and at 257 members T = 320 = 2 (mod 3): there edge1 / edge2 raise nothing and
# ARE the spread pattern of that width.  A first decided round is round 0, whose famous witnesses are roots and order nothing
# (a root is seen by one witness): ordering takes two decided rounds, which at 1024 members is beyond what the oracle
# follows in two minutes — the 449 and 1024 member cases are held to one decided round.
CASES = [Case(*row) for row in (
    # two mask words (npad 128): the default pass runs k_elections_tiled<2, false, 128> — the tiled elections start at an npad
    # of 128, which is 65 members — and k_elections<2, false> runs under SW_ELECT_IMPL=0 only (test_both_election_kernels)
    ("n65_twos", 65, 4000, 1, 0, 0.0, 0.0, "twos", None, False),                        # 3 / 1228 / 427 / 0.05 s
    ("n65_spread_chunked", 65, 4000, 2, 0, 0.0, 0.0, "spread", 1201, False),            # 3 / 1347 / 1006 / 0.06 s
    ("n65_whale", 65, 2000, 9, 0, 0.0, 0.0, "whale", None, True),                       # 2 / 0 (IndexError in the first call that orders) / 157 / 0.02 s
    # four mask words: voter masks of the tiled elections in LDS
    ("n130_twos_chunked", 130, 7000, 3, 0, 0.0, 0.0, "twos", 2101, False),              # 2 / 1051 / 539 / 0.4 s
    ("n130_edge0", 130, 8000, 4, 0, 0.0, 0.0, "edge0", None, False),                    # 2 / 1191 / 1393 / 0.4 s
    ("n130_edge1", 130, 7000, 5, 0, 0.0, 0.0, "edge1", None, False),                    # 2 / 1171 / 909 / 0.3 s    (= spread)
    ("n130_edge2", 130, 7000, 6, 0, 0.0, 0.0, "edge2", None, False),                    # 2 / 1119 / 1371 / 0.3 s
    # ... and one call long enough for the gated round loop (65 536 events and more, up to four mask words): not the smallest
    # count that orders, the smallest the existing gated-lag cases use
    ("n130_spread_gated", 130, 66000, 17, 0, 0.0, 0.0, "spread", None, False),          # 35 / 58273 / 55666 / 3.4 s
    # eight mask words: voter masks of the tiled elections in global memory
    ("n257_twos", 257, 15000, 7, 0, 0.0, 0.0, "twos", None, False),                     # 2 / 2344 / 1125 / 2.7 s
    ("n257_edge0", 257, 19000, 8, 0, 0.0, 0.0, "edge0", None, False),                   # 3 / 6388 / 3547 / 3.3 s
    ("n257_edge1_chunked", 257, 15000, 10, 0, 0.0, 0.0, "edge1", 4501, False),          # 2 / 2524 / 2539 / 3.1 s
    ("n257_edge2", 257, 15000, 11, 0, 0.0, 0.0, "edge2", None, False),                  # 2 / 2439 / 2049 / 3.1 s   (= spread)
    ("n257_zeros", 257, 18000, 12, 0, 0.0, 0.0, "zeros", None, False),                  # 2 / 2121 / 539 / 3.2 s
    ("n449_twos_slow", 449, 26000, 13, 2, 0.3, 0.05, "twos", None, False),              # 1 / 0 / 2294 / 8.9 s      (30 % of the members 20x less active)
    ("n449_spread_cliques", 449, 28000, 14, 1, 0.5, 0.02, "spread", None, False),       # 2 / 4664 / 3919 / 11.9 s  (two cliques, half of the gossip across)
    # sixteen mask words, in steps of 4000 events (64 000 and 76 000 decide nothing).  The oracle takes 2.5 to 3 times what it
    # takes for the 40 000 events of test_find_order_matches_oracle's 1024-member case: a round of weighted gossip is some
    # 16 000 events at this width and round 0 is decided in the fifth
    ("n1024_twos_cliques", 1024, 68000, 15, 1, 0.5, 0.02, "twos", None, False),                    # 1 / 0 / 2263 / 142 s
    ("n1024_spread_slow_chunked", 1024, 80000, 16, 2, 0.3, 0.05, "spread", 24001, False),          # 1 / 0 / 29935 / 147 s
)]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


def stream_of(case):
    """(creator, self-parent, other-parent, t, sig) of a case; wall-clock-like timestamps near 1.7e9 s, so that a consensus
    time needs the whole mantissa of the double (tests/test_model_consensus.py)"""
    pkg = importlib.import_module("py-swirld_amd")
    cr, sp, op, t, sig = pkg.synth_hashgraph(case.n, case.N, case.seed, case.mode, case.p0, case.p1)
    t = 1.7e9 + 0.013 * np.arange(case.N) + np.random.default_rng(case.seed).uniform(0.0, 0.0129, case.N)
    return cr, sp, op, t, sig


def calls_of(case):
    k = case.chunk or case.N
    return [(a, min(case.N, a + k)) for a in range(0, case.N, k)]


class OracleSide(OracleHashgraph):
    """the oracle behind the Hashgraph interface, with the getters run_pass reads"""

    def transactions(self):
        return self._o.transactions

    def heights(self):
        return self._o.height


Pass = namedtuple("Pass", "new_c orders failed_call kept_nothing round can_see witnesses famous consensus transactions")


def run_pass(d, stream, calls, errors, appended=0):
    """Drive `d` (a Hashgraph, or the oracle behind its interface) through the call schedule and record everything the
    comparison looks at: new_c and the order of every call, and the final tables.  A find_order that raises one of `errors`
    ends the pass: `failed_call` is its index, `kept_nothing` whether the order is what it was before the call.  `d` already
    holds the first `appended` events of the stream (appended, not yet divided into rounds)."""
    new_c, orders, failed, kept = [], [], None, None
    for i, (a, b) in enumerate(calls):
        if b > appended:
            d.append_events(*[x[max(a, appended):b] for x in stream])
        d.divide_rounds(a, b - a)
        nc = [int(r) for r in d.decide_fame()]
        new_c.append(nc)
        before = np.array(d.transactions())
        try:
            orders.append(np.array(d.find_order(nc)))
        except errors:
            failed, kept = i, bool(np.array_equal(d.transactions(), before))
            break
    return Pass(new_c, orders, failed, kept, np.array(d.rounds()), np.array(d.can_see()), np.array(d.witnesses()), np.array(d.famous()),
                np.array(d.consensus()), np.array(d.transactions()))


def compare_pass(got, exp):
    """Every field of two passes, bit for bit; AssertionError names the first that differs.  `exp` is the oracle's."""
    assert len(got.new_c) == len(exp.new_c), "number of calls made"
    for i, (a, b) in enumerate(zip(got.new_c, exp.new_c)):
        assert a == b, "new_c of call %d: %s, expected %s" % (i, a, b)
    assert got.failed_call == exp.failed_call, "find_order raised in call %s, expected %s" % (got.failed_call, exp.failed_call)
    assert len(got.orders) == len(exp.orders)
    for i, (a, b) in enumerate(zip(got.orders, exp.orders)):
        assert np.array_equal(a, b), "find_order of call %d" % i
    assert np.array_equal(got.round, exp.round), "round"
    assert np.array_equal(got.can_see, exp.can_see), "can_see"
    assert np.array_equal(got.witnesses, exp.witnesses), "witness table"
    assert np.array_equal(got.famous, exp.famous), "famous"
    assert np.array_equal(got.consensus, exp.consensus), "consensus"
    if exp.failed_call is None:
        assert np.array_equal(got.transactions, exp.transactions), "transactions"
    else:    # (the reference keeps the rounds in front of the one that raised; the library's call keeps nothing)
        assert got.kept_nothing, "a failed find_order keeps nothing"
        assert np.array_equal(got.transactions, np.concatenate(exp.orders) if exp.orders else np.zeros(0, np.int32)), "transactions"


def oracle_pass(case, stake, stream=None):
    from oracle.oracle import OracleError
    side = OracleSide(case.n, stake)
    return side, run_pass(side, stream_of(case) if stream is None else stream, calls_of(case), OracleError)
