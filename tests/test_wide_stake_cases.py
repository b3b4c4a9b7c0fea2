"""CPU: the inputs of tests/test_gpu_wide_stake.py (tests/wide_stake_cases.py) are proven discriminating by the oracle alone.
Every case runs Oracle(n, stake) and Oracle(n) on the same stream and call schedule; the assertions are conditions on the
INPUTS — that a weighted pass decides rounds, orders events and differs from the unit-stake pass in rounds, fame, order and
in at least one election that a head count would settle differently — not measurements of any kernel.  The last test feeds
the unit-stake pass to the comparison function the GPU tests use and expects it to be rejected."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import model_votes as mv
import wide_stake_cases as W

MODEL_MAX_MEMBERS = 257      # condition 4 through the numpy model of the elections (see the comment above W.CASES)
_runs = {}


@pytest.fixture(scope="module", autouse=True)
def long_passes(request):
    """the oracle passes of the selected cases of 449 and 1024 members (ten seconds to two minutes each) side by side on
    background threads, started with the module's first test"""
    names = []
    for it in request.session.items:
        cs = getattr(it, "callspec", None)
        nm = cs.params.get("name") if it.module is request.module and cs is not None else None
        if nm in W.BY_NAME and W.BY_NAME[nm].n >= 449 and nm not in names:
            names.append(nm)
    if not names:
        yield
        return
    from oracle import oracle as _o
    _o.lib()       # (built and loaded once, before any thread asks for it)
    with ThreadPoolExecutor(max_workers=4) as ex:
        for nm in sorted(names, key=lambda nm: -W.BY_NAME[nm].n * W.BY_NAME[nm].N):
            _pending[nm] = ex.submit(_compute, nm)
        yield
        for f in _pending.values():
            f.cancel()
    _pending.clear()


_pending = {}


def runs(name):
    """(stream, stake, weighted side, weighted pass, unit-stake pass, oracle seconds of the weighted pass), once per case"""
    if name not in _runs:
        _runs[name] = _pending.pop(name).result() if name in _pending else _compute(name)
    return _runs[name]


def _compute(name):
    """the two passes side by side (the oracle's C calls release the GIL)"""
    case = W.BY_NAME[name]
    stream, stake = W.stream_of(case), W.stake_of(case)

    def weighted():
        t0 = time.time()
        side, wp = W.oracle_pass(case, stake, stream)
        return side, wp, time.time() - t0

    with ThreadPoolExecutor(max_workers=2) as ex:
        fw, fu = ex.submit(weighted), ex.submit(W.oracle_pass, case, None, stream)
        (side, wp, sec), (_, up) = fw.result(), fu.result()
    return stream, stake, side, wp, up, sec


def by_stake_entries(case, stream, stake, side, wp):
    """n_by_stake of tests/model_votes.py on the oracle's tables (the model also replays new_c of every call and asserts it)"""
    g = {"witnesses": wp.witnesses, "round": wp.round, "can_see": wp.can_see, "stake": stake, "sig": stream[4],
         "batches": W.calls_of(case)[:len(wp.new_c)]}
    return mv.model_votes(g, wp.new_c)["n_by_stake"]


def test_the_table_covers_what_the_issue_names():
    assert len(W.CASES) <= 18 and len(set(W.NAMES)) == len(W.CASES)
    assert {c.n for c in W.CASES} == {65, 130, 257, 449, 1024}
    assert {W.mask_words(c.n) for c in W.CASES} == {2, 4, 8, 16}
    for n in (65, 130, 257, 449, 1024):
        assert any(c.pattern == "twos" for c in W.CASES if c.n == n), n
        # (an edge case that raises nothing IS the spread pattern)
        assert any(np.array_equal(W.stake_of(c), W.PATTERNS["spread"](c.n, c.seed)) for c in W.CASES if c.n == n), n
    narrow = {c.n for c in W.CASES if c.pattern.startswith("edge") and W.mask_words(c.n) <= 4}
    wide = {c.n for c in W.CASES if c.pattern.startswith("edge") and W.mask_words(c.n) >= 8}
    for group in (narrow, wide):     # all three residues of T % 3 at ONE member count per group
        assert any({"edge0", "edge1", "edge2"} <= {c.pattern for c in W.CASES if c.n == n} for n in group)
    assert sum(c.index_error for c in W.CASES) == 1
    for words in ((2, 4), (8, 16)):     # batch and chunked call schedules on narrow and on wide masks
        assert any(c.chunk for c in W.CASES if W.mask_words(c.n) in words) and any(not c.chunk for c in W.CASES if W.mask_words(c.n) in words)
    assert any(c.N >= 65536 and c.chunk is None and W.mask_words(c.n) == 4 for c in W.CASES), "one call that takes the gated round loop"
    for c in W.CASES:
        if c.n >= 449:
            assert c.mode in (1, 2), "slow members or cliques at 449 and 1024 members"


@pytest.mark.parametrize("name", W.NAMES)
def test_case_is_discriminating(name):
    case = W.BY_NAME[name]
    stream, stake, side, wp, up, sec = runs(name)
    n, N = case.n, case.N
    T = int(stake.sum())
    assert not (stake == 1).all() and T < 1.5 * n, "near-unit stakes: the only weighted kind whose rounds advance"
    if case.pattern.startswith("edge"):                                                        # 5.
        assert T % 3 == int(case.pattern[-1])
    if case.pattern in ("zeros", "whale"):
        assert (stake == 0).any()
    decided = sum(len(c) for c in wp.new_c)
    print("\n[%s] n=%d N=%d T=%d: %d rounds, %d decided, %d ordered, %d events with another round than unit stake, oracle %.2f s"
          % (name, n, N, T, wp.witnesses.shape[0], decided, len(wp.transactions), int((wp.round != up.round).sum()), sec))
    if case.index_error:                                                                       # 1.
        assert wp.failed_call is not None, "the case is built to end in the reference's IndexError (swirld.py:305)"
        assert up.failed_call is None
    else:
        assert wp.failed_call is None and len(wp.orders) == len(W.calls_of(case))
    if n <= 257:                                                                               # 2.
        assert decided >= 2
        assert len(wp.transactions) >= 1 or case.index_error
    else:
        assert decided >= 1
    assert (wp.round != up.round).sum() * 100 >= N, "round differs from the unit-stake pass in at least 1 % of the events"   # 3.
    fw = famous_by_event(wp, N)
    assert np.array_equal(fw, side._o.famous_by_event)
    assert (fw != famous_by_event(up, N)).any(), "famous differs on at least one witness"
    if len(wp.transactions) and len(up.transactions):
        assert not np.array_equal(wp.transactions, up.transactions)
    if n <= MODEL_MAX_MEMBERS:                                                                 # 4.
        assert by_stake_entries(case, stream, stake, side, wp) > 0, "no election entry that a head count would settle differently"


def famous_by_event(p, N):
    """famous per event (-1 / 0 / 1) from a pass's witness and fame tables"""
    f = np.full(N, -1, np.int8)
    m = p.witnesses >= 0
    f[p.witnesses[m]] = p.famous[m]
    return f


@pytest.mark.parametrize("name", W.NAMES)
def test_unit_stake_answer_is_rejected(name):
    """the comparison function of the GPU tests tells the two passes apart: a library that ignored the weights (a UNIT kernel
    launched for a weighted context) would give the unit-stake pass, and fail"""
    stream, stake, side, wp, up, sec = runs(name)
    W.compare_pass(wp, wp)
    with pytest.raises(AssertionError):
        W.compare_pass(up, wp)


def test_stake_patterns():
    for n in (65, 130, 257, 449, 1024):
        for seed in (1, 2):
            tw, sp_, ze = W.PATTERNS["twos"](n, seed), W.PATTERNS["spread"](n, seed), W.PATTERNS["zeros"](n, seed)
            assert sorted(np.unique(tw)) == [1, 2] and (tw == 2).sum() == n // 10
            assert (sp_ == 3).sum() == n // 12 and (sp_ == 2).sum() == n // 12 and set(np.unique(sp_)) == {1, 2, 3}
            assert (ze == 0).sum() == n // 16 and (ze == 2).sum() == n // 10
            for res in (0, 1, 2):
                e = W.PATTERNS["edge%d" % res](n, seed)
                assert int(e.sum()) % 3 == res and (e != sp_).sum() <= 1 and 0 <= int(e.sum()) - int(sp_.sum()) <= 2
            assert np.array_equal(tw, W.PATTERNS["twos"](n, seed)), "a function of (n, seed)"
