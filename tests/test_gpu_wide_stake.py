"""GPU (-m gpu): weighted stakes at 65 to 1024 members — two to sixteen mask words — against the CPU oracle, bit for bit.
A stake vector that is not all ones changes the kernel at almost every step of a pass: the column-lane tally
k_tally_candidates<NW, false>, the bit loop of the voter masks, k_elections<NW, false> / k_elections_tiled<NW, false, CG>
(stake sums against tot2, voter masks from LDS up to four words and from global memory beyond), k_votes_values<false>, and the
stake table of k_order_prep.  The cases and the comparison are tests/wide_stake_cases.py's; tests/test_wide_stake_cases.py
proves on the CPU that each of them tells a weighted pass from a unit-stake one.  The oracle passes run on the threads of
tests/oracle_pool.py; those of 449 and 1024 members are started when the session begins (`heavy`)."""
import numpy as np
import pytest

import model_consensus as mc
import wide_stake_cases as W
from oracle_pool import WIDE_STAKE
from test_gpu_gated_lag import lag_env, run as lag_run
from test_gpu_votes import check_table, entries, lookup, sample_pairs
from test_model_consensus import same_bits

pytestmark = pytest.mark.gpu

ENOTSUP = -95


def params(names):
    """cases as parameters; from 449 members on the oracle pass takes ten seconds and more: started with the session"""
    return [pytest.param(nm, marks=pytest.mark.heavy(WIDE_STAKE + nm)) if W.BY_NAME[nm].n >= 449 else nm for nm in names]


ALL = W.NAMES
# (the default pass of EVERY case runs the tiled elections: fame_launch takes them from two mask words on, 65 members and more)
TILED = ["n65_twos", "n65_spread_chunked", "n130_twos_chunked", "n257_twos", "n130_edge1", "n257_edge2", "n130_edge0", "n257_edge1_chunked", "n257_zeros", "n1024_twos_cliques"]
# (cases that ORDER events: two to eight mask words.  Both 1024-member cases end after their first decided round, round 0, whose
# famous witnesses are roots and order nothing, so weighted find_order has no case at sixteen mask words: a second decided
# round there is beyond what the oracle follows in minutes, see the comment above W.CASES)
ORDERING = ["n65_spread_chunked", "n130_edge1", "n130_twos_chunked", "n257_twos", "n257_zeros", "n449_spread_cliques"]
VOTES = ["n65_twos", "n65_spread_chunked", "n130_twos_chunked", "n130_edge0", "n449_spread_cliques", "n449_twos_slow"]
GATED = ["n130_spread_gated", "n1024_twos_cliques"]
assert {W.mask_words(W.BY_NAME[nm].n) for nm in TILED} == {2, 4, 8, 16}, "both election kernels at every mask width above one word"


SPLIT_CASE = "n130_twos_chunked"     # test_split_refuses_weighted's: a schedule of four calls
_uses = {}                           # case -> selected tests of this module that have yet to ask for its oracle run


@pytest.fixture(scope="module")
def expected(request, oracle_pool):
    """name -> the finished oracle run of a case (oracle_pool.WideStakeRun).  All selected cases are queued at the first
    request, the longest first; the pool lets go of a run when the last test that uses it has asked for it (the can_see
    table of a 1024-member case is some 300 MB), so nothing of this module outlives it."""
    if not _uses:
        for it in request.session.items:
            if it.module is request.module:
                cs = getattr(it, "callspec", None)
                nm = cs.params.get("case") if cs is not None else SPLIT_CASE if it.name == "test_split_refuses_weighted" else None
                if nm in W.BY_NAME:
                    _uses[nm] = _uses.get(nm, 0) + 1
    for nm in sorted((nm for nm in _uses if _uses[nm] > 0), key=lambda nm: -W.BY_NAME[nm].n * W.BY_NAME[nm].N):
        oracle_pool.start(WIDE_STAKE + nm)

    def get(name):
        run = oracle_pool.get(WIDE_STAKE + name)
        _uses[name] = _uses.get(name, 0) - 1
        if _uses[name] <= 0:
            oracle_pool.drop(WIDE_STAKE + name)
        return run
    return get


def weighted_context(pkg, run):
    return pkg.Hashgraph(run.case.n, run.stake)


def assert_weighted_kernels_ran(h):
    assert h._L.sw_get_tally_impl(h._h) == 0, "the weighted tally (k_tally_candidates<NW, false>), not a bit-sliced one"
    assert h.counters()["majority_evals"] > 0, "elections were evaluated"


# ---- 1. the whole pass ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", params(ALL))
def test_pass_matches_oracle(pkg, expected, case):
    """the case's call schedule (one call, or calls of `chunk` events): new_c and find_order's list of every call, then
    rounds, can_see, the witness table, fame, consensus and the whole order.  The one case built to end in the reference's
    IndexError (swirld.py:305): SwirldHipError from find_order, and the call keeps nothing."""
    run = expected(case)
    c = run.case
    h = weighted_context(pkg, run)
    got = W.run_pass(h, run.stream, W.calls_of(c), pkg.SwirldHipError)
    W.compare_pass(got, run.expected)
    if c.index_error:
        assert got.failed_call is not None and got.kept_nothing and h.num_ordered == len(got.transactions)
    else:
        assert got.failed_call is None
    assert_weighted_kernels_ran(h)
    assert h.counters()["rounds"] == run.side.counters()["rounds"]
    if c.chunk is None and not c.index_error:      # (the V / P2 counters are compared for batch schedules, as in test_gpu_parity.py)
        ch, co = h.counters(), run.side.counters()
        assert ch["voter_evals"] == co["voter_evals"] and ch["majority_evals"] == co["majority_evals"]
    h.close()


# ---- 2. both election kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ["0", "1"])      # k_elections<NW, false> / k_elections_tiled<NW, false, CG>
@pytest.mark.parametrize("case", params(TILED))
def test_both_election_kernels(pkg, expected, case, impl, monkeypatch):
    """SW_ELECT_IMPL=0 and =1 on the same pass.  The tiled kernel is the default from two mask words on (an npad of 128:
    65 members and more), so only SW_ELECT_IMPL=0 launches k_elections<NW, false> at all.  Both `twos` and `spread` at two
    mask words; per pattern group (twos; spread and its edges; zeros, which the table holds at eight words only) one case
    of four mask words and one of eight or sixteen: weighted, both kernels run at NW = 2, 4, 8 and 16, and both give the
    oracle's new_c, fame and consensus — and everything else compare_pass looks at."""
    run = expected(case)
    c = run.case
    assert W.mask_words(c.n) >= 2, "fame_launch takes the tiled kernel from two mask words on"
    monkeypatch.setenv("SW_ELECT_IMPL", impl)
    h = weighted_context(pkg, run)
    got = W.run_pass(h, run.stream, W.calls_of(c), pkg.SwirldHipError)
    assert got.new_c == run.expected.new_c
    assert np.array_equal(got.famous, run.expected.famous), "famous"
    assert np.array_equal(got.consensus, run.expected.consensus), "consensus"
    W.compare_pass(got, run.expected)
    assert_weighted_kernels_ran(h)
    h.close()


# ---- 3. both find_order paths ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", params(ORDERING))
def test_find_order_paths(pkg, expected, case, monkeypatch):
    """SW_ORDER_BULK=0 (the searches) and =1 (the first-descendant table): the oracle's order from both; round received and
    the consensus time agree bit for bit between them, and equal tests/model_consensus.py — numpy's
    .5 * (times[len // 2] + times[(len + 1) // 2]) recomputed from the ORACLE's can_see rows, witness and fame tables with the
    case's stakes — on a seeded sample of 200 ordered events.  Two to eight mask words: see ORDERING."""
    run = expected(case)
    c, exp = run.case, run.expected
    N = c.N
    res = {}
    for bulk in ("0", "1"):
        monkeypatch.setenv("SW_ORDER_BULK", bulk)
        h = weighted_context(pkg, run)
        got = W.run_pass(h, run.stream, W.calls_of(c), pkg.SwirldHipError)
        assert got.failed_call is None
        for i, (a, b) in enumerate(zip(got.orders, exp.orders)):
            assert np.array_equal(a, b), "find_order of call %d, SW_ORDER_BULK=%s" % (i, bulk)
        assert np.array_equal(got.transactions, exp.transactions)
        res[bulk] = (h.round_received(), h.consensus_time())
        h.close()
    rr, ct = res["0"]
    assert np.array_equal(rr, res["1"][0]), "round received: the two paths"
    ordered = np.zeros(N, bool)
    ordered[exp.transactions] = True
    assert np.array_equal(rr >= 0, ordered) and np.array_equal(np.isnan(ct), ~ordered)
    assert same_bits(ct[ordered], res["1"][1][ordered]) and np.array_equal(np.isnan(res["1"][1]), ~ordered), "consensus time: the two paths"
    tx = exp.transactions
    assert len(tx) >= 200, "every case of ORDERING orders events"
    ev = np.sort(np.random.default_rng(c.seed).choice(tx, 200, replace=False))
    cr, sp, op, t, sig = run.stream
    round_seq = [r for nc in exp.new_c for r in sorted(nc)]
    m_rr, m_ct = mc.consensus_values(ev, round_seq, exp.can_see, exp.witnesses, exp.famous, cr, sp, run.side.heights(), t,
                                     run.stake.astype(np.int64))
    assert np.array_equal(m_rr, rr[ev]) and same_bits(m_ct, ct[ev])
    for a, b in zip(np.cumsum([0] + [len(o) for o in exp.orders])[:-1], np.cumsum([len(o) for o in exp.orders])):
        assert mc.order_key_ok(tx[a:b], rr, ct)


# ---- 4. the votes table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", params(VOTES))
def test_votes_export(pkg, expected, case):
    """Hashgraph.votes_triples() (k_votes_values<false>: yes / no as stake sums against tot2) against Oracle.vote(y, x): every
    exported entry up to 200 000 of them, a seeded sample of 200 000 beyond; the entry count against the oracle's; pairs
    without an entry through the table's own lookup."""
    run = expected(case)
    c, o = run.case, run.side._o
    h = weighted_context(pkg, run)
    got = W.run_pass(h, run.stream, W.calls_of(c), pkg.SwirldHipError)
    assert got.new_c == run.expected.new_c
    table = h.export_votes()
    check_table(h, table)
    tr = h.votes_triples()
    assert len(tr) == o.num_votes == entries(table)
    assert len(tr) > 0
    rng = np.random.default_rng(c.seed)
    pick = tr if len(tr) <= 200_000 else tr[rng.choice(len(tr), 200_000, replace=False)]
    for y, x, v in pick.tolist():
        assert o.vote(y, x) == v, "votes[%d][%d]" % (y, x)
    at = lookup(h, table)
    cr = run.stream[0]
    for y, x in sample_pairs(h.witnesses(), tr, rng, 5000, 1000):
        assert at(y, x, cr) == o.vote(y, x), "votes[%d][%d]" % (y, x)
    h.close()


# ---- 5. the gated round loop under a forced sweep lag ---------------------------------------------------------------------------
@pytest.mark.parametrize("hs", [(2, 1), (256, 1)], ids=lambda v: "h%s_s%d" % v)     # two of test_gpu_gated_lag.LAGS
@pytest.mark.parametrize("case", params(GATED))
def test_gated_lag(pkg, expected, case, hs, monkeypatch):
    """One call of more than 64 k events under SW_GATE_LAG / SW_GATE_STEP.  Up to four mask words the call takes the gated
    loop (asserted); with sixteen the library keeps the per-sub-batch loops whatever the knob says, and the same comparison
    holds."""
    run = expected(case)
    c, exp = run.case, run.expected
    assert c.chunk is None and c.N >= 65536
    h, ncs, (its, idle, calls) = lag_run(pkg, c.n, run.stream, run.stake, None, lag_env({}, *hs), monkeypatch)
    assert calls == (1 if W.mask_words(c.n) <= 4 else 0)
    assert ncs == exp.new_c
    assert np.array_equal(h.rounds(), exp.round), "round"
    assert np.array_equal(h.witnesses(), exp.witnesses), "witness table"
    assert np.array_equal(h.famous(), exp.famous) and np.array_equal(h.consensus(), exp.consensus)
    assert_weighted_kernels_ran(h)
    if hs == (256, 1) and calls:
        assert idle > 0, "a lag of 256 iterations per stage makes the loop wait"
    h.close()


# ---- 6. the split loop refuses weights ------------------------------------------------------------------------------------------
def test_split_refuses_weighted(pkg, expected):
    """sw_split_link on weighted contexts: SW_ENOTSUP (the split kernels are the unit-stake tally; the refusal itself is
    tests/test_gpu_split_loop.py's) — and the refused link leaves both contexts as they were: each goes on from the events
    it held when the link was asked for, WITHOUT a reset, and its pass of four calls equals the oracle."""
    run = expected(SPLIT_CASE)
    c = run.case
    calls = W.calls_of(c)
    assert len(calls) > 1
    a, b = weighted_context(pkg, run), weighted_context(pkg, run)
    held = calls[0][1]
    for h in (a, b):
        h.append_events(*[x[:held] for x in run.stream])
    with pytest.raises(pkg.SwirldHipError) as ei:
        pkg.Hashgraph.split_link([a, b])
    assert ei.value.code == ENOTSUP
    for h in (a, b):
        assert h.num_events == held
        W.compare_pass(W.run_pass(h, run.stream, calls, pkg.SwirldHipError, appended=held), run.expected)
        assert_weighted_kernels_ran(h)
        h.close()
