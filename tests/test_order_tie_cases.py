"""CPU: the inputs of tests/test_gpu_order_ties.py (tests/order_tie_cases.py) and the oracle's comparison behind the first key
bytes.

1. The oracle reproduces, call by call, what the unmodified reference computed on the recorded cases
   (tests/golden/order_ties, tests/golden/make_order_ties_golden.py): order_cmp's memcmp over all 64 key bytes.
2. Every case does what it claims, proven with the oracle alone — conditions on the INPUTS, not measurements of a kernel:
   the order with bytes 8..63 of the crafted events redrawn differs from the case's own, and in a windowed case only in
   positions that crafted events occupy; with the numpy model of the consensus timestamps (tests/model_consensus.py) on the
   oracle's tables: the rounds with two events equal in (consensus time, bytes 0..7) are the ones expected — all of them
   where every event is crafted, some but not all in a windowed case, oversize rounds among both in the big-sort case — and
   the median cases hold events with more than 64 samples and long runs of equal values around the middle.

tests/model_backend.py and tests/model_consensus.py compute rounds, fame and (round received, consensus time); neither orders
events inside a round, so there is no truncated key in the models to fix."""
import time

import numpy as np
import pytest

import model_consensus as mc
import order_tie_cases as T

_runs = {}


def runs(name):
    """(case, stream, stake, crafted, deep, oracle run, oracle, run with redrawn tails, oracle seconds), once per case"""
    if name not in _runs:
        case = T.BY_NAME[name]
        stream, stake, crafted, deep = T.build(case)
        t0 = time.time()
        run, o = T.oracle_run(case, stream, stake)
        sec = time.time() - t0
        run2, _ = T.oracle_run(case, T.redrawn_of(case, stream, crafted), stake)
        _runs[name] = (case, stream, stake, crafted, deep, run, o, run2, sec)
    return _runs[name]


def model_values(case, stream, stake, run, o, sample_lists=None):
    """(round received, consensus time) by event index of everything the oracle ordered, from the model on the oracle's tables"""
    cr, sp, op, t, sig = stream
    tx = run.transactions
    seq = [r for nc in run.new_c for r in sorted(nc)]
    st = np.ones(case.n, np.int64) if stake is None else stake.astype(np.int64)
    rr, ct = mc.consensus_values(tx, seq, o.can_see, o.witnesses(), o.famous_table(), cr, sp, o.height, t, st, sample_lists)
    RR, CT = np.full(case.N, -1, np.int32), np.full(case.N, np.nan)
    RR[tx], CT[tx] = rr, ct
    assert (rr >= 0).all()
    return RR, CT


def test_the_table_covers_what_the_issue_names():
    assert len(set(T.NAMES)) == len(T.CASES)
    rec = [T.BY_NAME[nm] for nm in T.RECORDED]
    assert 3 <= len(rec) <= 4 and all(c.N <= 2000 and c.source.startswith("golden:") for c in rec)
    assert any(c.chunk for c in rec) and any("stake" in c.source for c in rec)
    for c in T.CASES:
        assert c.q >= 16 or c.n < 100, "at 100 members and more one event's samples hold long runs of equal values"
        assert c.window is T.ALL or 0 <= c.window[0] < c.window[1] <= c.window[2]
    assert {(c.n, c.q) for c in T.CASES if c.name.startswith(("n130_q", "n300_q"))} == {(130, 16), (130, 64), (300, 16), (300, 64)}
    assert {c.n for c in T.CASES if c.name in ("n33_window", "n130_window")} == {33, 130}


@pytest.mark.parametrize("name", ["ref_n16_chunk250_all", "ref_n7_chunk13_window", "n33_window"])
def test_crafted_streams_are_what_the_module_says(name):
    case = T.BY_NAME[name]
    base, _ = T.base_stream(case)
    stream, stake, crafted, deep = T.build(case)
    cr, sp, op, t, sig = stream
    N = case.N
    for x, y in zip(base[:3], stream[:3]):
        assert np.array_equal(x, y)
    # timestamps: rank // q — finite, non-negative, runs of exactly q equal values (the last one may be shorter)
    assert np.isfinite(t).all() and (t >= 0).all() and np.array_equal(np.sort(t), np.arange(N) // case.q)
    assert np.array_equal(np.argsort(t, kind="stable"), np.argsort(base[3], kind="stable"))
    # signatures
    assert np.array_equal(crafted, T.crafted_mask(N, case.window)) and (deep <= crafted).all()
    assert (crafted.all() if case.window is T.ALL else 0 < crafted.sum() < N)
    assert 0.55 * crafted.sum() < deep.sum() < 0.8 * crafted.sum() and (crafted & ~deep).sum() > 0
    assert np.array_equal(sig[~crafted], np.asarray(base[4])[~crafted])
    assert len(np.unique(sig[crafted][:, :8], axis=0)) == 1
    assert len(np.unique(sig[deep][:, :61], axis=0)) == 1
    assert len(np.unique(sig[deep][:, 61:], axis=0)) == deep.sum()
    assert np.array_equal(sig[crafted & ~deep][:, 8:], np.asarray(base[4])[crafted & ~deep][:, 8:])
    assert len(np.unique(sig, axis=0)) == N
    # the second version: only bytes 8..63 of the crafted events change, and all of those events change
    s2 = T.redrawn_of(case, stream, crafted)
    for x, y in zip(stream[:4], s2[:4]):
        assert np.array_equal(x, y)
    assert np.array_equal(s2[4][:, :8], sig[:, :8]) and np.array_equal(s2[4][~crafted], sig[~crafted])
    assert (s2[4][crafted][:, 8:] != sig[crafted][:, 8:]).any(axis=1).all() and len(np.unique(s2[4], axis=0)) == N
    # deterministic: a function of the case
    again = T.build(case)
    assert np.array_equal(again[0][4], sig) and np.array_equal(again[0][3], t)


def test_tied_rounds_by_hand():
    sig = np.zeros((8, 64), np.uint8)
    sig[:, 7] = [1, 1, 2, 1, 1, 3, 3, 9]
    sig[:, 20] = np.arange(8)                                   # (bytes behind the 8th do not count)
    rr = np.array([5, 5, 5, 6, 6, 7, 7, -1])
    ct = np.array([1.0, 1.0, 1.0, 2.0, 2.5, 4.0, 4.0, np.nan])
    ev = np.arange(7)
    assert T.tied_rounds(ev, rr, ct, sig).tolist() == [5, 7]      # 6: equal key, other times
    assert T.tied_rounds(ev[1:], rr, ct, sig).tolist() == [7]     # 5: equal times, other keys
    assert T.tied_rounds(ev[:0], rr, ct, sig).tolist() == []
    sig[6, 0] = 1                                                # the FIRST byte is the most significant one
    assert T.tied_rounds(ev, rr, ct, sig).tolist() == [5]
    assert T.k8_of(sig)[6] == (1 << 56) + 3
    rr2 = rr.copy()
    rr2[1] = 6                                                   # equal time and key in two different rounds
    assert T.tied_rounds(np.array([0, 1]), rr2, ct, sig).tolist() == []


@pytest.mark.parametrize("name", T.RECORDED)
def test_oracle_reproduces_the_recorded_reference(name):
    from oracle.oracle import Oracle
    case = T.BY_NAME[name]
    g = T.load_recorded(name)
    stream, stake, crafted, deep = T.build(case)
    for key, x in zip(("creator", "self_parent", "other_parent", "t", "sig"), stream):
        assert np.array_equal(g[key], x), "the fixture holds the case's own stream: " + key
    assert np.array_equal(g["crafted"], crafted) and np.array_equal(g["deep"], deep)
    assert [int(k) for k in g["sched"]] == [b - a for a, b in T.calls_of(case)]
    assert np.array_equal(g["stake"], np.ones(case.n) if stake is None else stake)
    o = Oracle(case.n, stake)
    for i, (a, b) in enumerate(T.calls_of(case)):
        o.append_events(*[x[a:b] for x in stream])
        o.divide_rounds(a, b - a)
        nc = o.decide_fame()
        assert list(nc) == list(g["new_c_flat"][g["new_c_off"][i]:g["new_c_off"][i + 1]]), "new_c of call %d" % i
        assert list(o.find_order(nc)) == list(g["tx_flat"][g["tx_off"][i]:g["tx_off"][i + 1]]), "find_order of call %d" % i
    assert np.array_equal(o.transactions, g["tx_flat"]) and len(g["tx_flat"]) > case.N // 2


@pytest.mark.parametrize("name", T.NAMES)
def test_order_depends_on_key_bytes_8_to_63(name):
    case, stream, stake, crafted, deep, run, o, run2, sec = runs(name)
    a, b = run.transactions, run2.transactions
    assert run.new_c == run2.new_c and len(a) == len(b) > 0 and np.array_equal(np.sort(a), np.sort(b))
    diff = np.flatnonzero(a != b)
    print("\n[%s] n=%d N=%d q=%d crafted=%s: %d ordered (%d crafted), %d positions differ with redrawn tails, oracle %.2f s"
          % (name, case.n, case.N, case.q, "all" if case.window is T.ALL else "[%d N/%d, %d N/%d)" % (case.window[0], case.window[2], case.window[1],
             case.window[2]), len(a), int(crafted[a].sum()), len(diff), sec))
    assert len(diff) * 20 >= crafted[a].sum() > 0, "the bytes behind the 8th decide at least 5 % of the crafted positions"
    assert crafted[a[diff]].all() and crafted[b[diff]].all(), "only positions that crafted events occupy differ"
    assert np.array_equal(crafted[a], crafted[b])
    # call by call as well: what one call returns differs in at least one call
    assert any(not np.array_equal(x, y) for x, y in zip(run.orders, run2.orders))
    if case.window is not T.ALL:
        assert 0 < crafted[a].sum() < len(a)
        r_ev = np.flatnonzero(~crafted[a])
        assert np.array_equal(a[r_ev], b[r_ev])


FORK_FREE = [nm for nm in T.NAMES if "forks" not in nm]
_values = {}


def values(name):
    if name not in _values:
        case, stream, stake, crafted, deep, run, o, run2, sec = runs(name)
        lists = {}
        RR, CT = model_values(case, stream, stake, run, o, lists)
        _values[name] = (RR, CT, lists)
    return _values[name]


@pytest.mark.parametrize("name", FORK_FREE)
def test_rounds_that_tie_in_time_and_8_bytes(name):
    """what tests/test_gpu_order_ties.py expects of order_rounds_host_sorted, here from the model on the oracle's tables"""
    case, stream, stake, crafted, deep, run, o, run2, sec = runs(name)
    RR, CT, _ = values(name)
    tx = run.transactions
    for part in run.orders:      # (round received, consensus time) never decreases along what one call returns
        assert mc.order_key_ok(part, RR, CT)
    rounds = np.unique(RR[tx])
    tied = T.tied_rounds(tx, RR, CT, stream[4])
    sizes = {int(r): int((RR[tx] == r).sum()) for r in rounds}
    print("\n[%s] %d rounds ordered, %d expected tied: %s; events per round %s" % (name, len(rounds), len(tied), tied.tolist(), sizes))
    assert set(tied.tolist()) <= set(rounds.tolist()) and len(rounds) >= 2
    if case.window is T.ALL:
        assert len(tied) == len(rounds), "every round is tied where every event is crafted"
    else:
        assert 0 < len(tied) < len(rounds), "rounds with and without ties"
        # the ties are the crafted events': the random signatures never agree in 8 bytes
        assert set(tied.tolist()) == set(T.tied_rounds(tx[crafted[tx]], RR, CT, stream[4]).tolist())
        assert len(T.tied_rounds(tx[~crafted[tx]], RR, CT, stream[4])) == 0
    if name == "n256_big_window":
        big = {r for r, k in sizes.items() if k > 4096}
        assert big & set(tied.tolist()) and big - set(tied.tolist()), "oversize rounds with and without ties"
        assert len(tx) > 4096 * 3 and len(tx) / sum(len(c) for c in run.new_c) > 4096     # (test_rounds_larger_than_the_lds_sort's own)


def median_conditions(lists, events):
    """(events with more than 64 samples whose middle value occurs at least three times, events whose two middle samples differ)"""
    long_dup = [e for e in events if len(lists[e]) > 64 and int((lists[e] == lists[e][len(lists[e]) // 2]).sum()) >= 3]
    split = [e for e in events if lists[e][len(lists[e]) // 2] != lists[e][(len(lists[e]) + 1) // 2]]
    return long_dup, split


@pytest.mark.parametrize("name", ["n130_q16", "n130_q64", "n300_q16", "n300_q64"])
def test_median_cases_hold_long_runs_of_equal_samples(name):
    case, stream, stake, crafted, deep, run, o, run2, sec = runs(name)
    RR, CT, lists = values(name)
    tx = run.transactions
    long_dup, split = median_conditions(lists, tx.tolist())
    most = max(len(s) for s in lists.values())
    print("\n[%s] %d ordered: %d with > 64 samples and >= 3 equal to the middle one, %d whose two middle samples differ, up to %d samples"
          % (name, len(tx), len(long_dup), len(split), most))
    assert most > 96 and len(long_dup) * 2 > len(tx) and len(split) >= 100
    # a run of equal values that straddles the two middle positions of an ODD list, and one that ends between them
    odd = [e for e in tx.tolist() if len(lists[e]) % 2 == 1 and len(lists[e]) > 64]
    assert any(lists[e][len(lists[e]) // 2] == lists[e][len(lists[e]) // 2 + 1] for e in odd)
    assert any(lists[e][len(lists[e]) // 2] != lists[e][len(lists[e]) // 2 + 1] for e in odd)
    # equal consensus times inside a round: most events share theirs with another event of the round
    key = np.stack([RR[tx].astype(np.float64), CT[tx]], 1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    assert (cnt[inv.reshape(-1)] > 1).sum() * 2 > len(tx)
