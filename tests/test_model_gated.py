"""CPU: the GATED round loop (one loop per call, its stages latched from the can_see sweep's progress word)
as an executable specification — tests/model_bulk.py, bulk_rounds_gated — against the sequential oracle, under stage
schedules the device cannot be made to choose on its own: always ahead, a stage every h iterations, jumps of several
stages, MAXIMAL LAG (a stage is published only after an iteration in which every searching member waited) and seeded
random ones.  The model asserts inside itself that nothing beyond the current stage is read and that no chain position
is tallied twice for a round; three one-line mutants of the wait / resume / latch rules must each be caught."""
import numpy as np
import pytest

import model_bulk as mb
from oracle.oracle import Oracle
from synth_util import silence

# name -> (members, events, seed, mode, p0, p1, (silent member, from which fraction of the stream) or None, stakes or None)
STREAMS = {
    "uniform": (12, 3000, 71, 0, 0, 0, None, None),
    "cliques": (16, 3200, 63, 1, 0.03, 0, None, None),
    "slow": (12, 3000, 62, 2, 0.3, 0.02, None, None),
    "stale": (20, 3000, 64, 3, 0.6, 0, None, None),
    "silent_mid": (12, 3000, 72, 0, 0, 0, (5, 0.5), None),
    "ends_in_head": (10, 2600, 73, 0, 0, 0, (3, 0.03), None),     # (its last event lies in the first sub-batch of the 2 / 6 / 12 plans)
    "stake": (9, 2400, 74, 0, 0, 0, None, (1, 1, 2, 1, 1, 1, 2, 1, 1)),   # (the reference counts MEMBERS against 2/3 of the total stake: 8 of these 9)
}
# cut plans as fractions of the stream
PLANS = {
    "2": [0.5],
    "6": [k / 6 for k in range(1, 6)],
    "12": [k / 12 for k in range(1, 12)],
    "short_head": [0.002, 0.3, 0.6],                               # a head of ~6 events: most members have none in it
    "nothing_for_some": [0.4, 0.402, 0.404, 0.7],                  # two sub-batches of ~6 events: they add nothing to several members
}
KNOBS = dict(K=4, NEARCAP=48, gallop_after=2, skip=1)

_cache = {}


def case(name):
    """(n, stream, stake, oracle results): one oracle run per stream."""
    if name not in _cache:
        import importlib
        pkg = importlib.import_module("py-swirld_amd")
        n, N, seed, mode, p0, p1, sil, stk = STREAMS[name]
        stream = pkg.synth_hashgraph(n, N, seed, mode, p0, p1)
        if sil:
            stream = silence(stream, sil[0], int(N * sil[1]))
        stake = np.ones(n, np.int64) if stk is None else np.array(stk, np.int64)
        o = Oracle(n, stake=stake.astype(np.uint64))
        o.append_events(*stream)
        N = len(stream[0])
        o.divide_rounds(0, N)
        nc = [int(r) for r in o.decide_fame()]
        exp = dict(round=o.round.copy(), wit=o.witnesses().copy(), famous=o.famous_by_event.copy(), cons=o.consensus().copy(),
                   new_c=nc, can_see=o.can_see.copy())
        _, lo3, st3 = mb.bulk_rounds_v3(n, *stream[:3], stake, **KNOBS)
        _cache[name] = (n, stream, stake, exp, lo3, st3["iters"])
    return _cache[name]


def cuts_of(plan, N):
    out = []
    for f in PLANS[plan]:
        b = int(f * N)
        if b > (out[-1] if out else 0) and b < N:
            out.append(b)
    return out + [N]


def every(h, s=1):
    """What the library's SW_GATE_LAG=h / SW_GATE_STEP=s hook does: `s` more stages behind every piece of h iterations."""
    return lambda t: 1 + (t // h) * s


class MaximalLag:
    """The next stage is published only once an iteration has been idle (every searching member waiting)."""
    def __init__(self, S):
        self.stats, self.pub, self.idle_seen, self.S = {}, 1, 0, S

    def __call__(self, t):
        if self.stats.get("idle", 0) > self.idle_seen:
            self.idle_seen = self.stats["idle"]
            self.pub = min(self.S, self.pub + 1)
        return self.pub


def random_schedule(rng, S):
    """Non-decreasing, stalls of 0 .. 40 iterations, jumps of 1 .. 3 stages."""
    at, v = 0, min(S, int(rng.integers(0, 3)))
    steps = [(0, v)]
    while v < S:
        at += int(rng.integers(0, 41))
        v = min(S, v + int(rng.integers(1, 4)))
        steps.append((at, v))
    return lambda t: max(v_ for a_, v_ in steps if a_ <= t)


def run_model(name, cuts, vis, mutant=None, stats=None):
    n, stream, stake, exp, lo3, it3 = case(name)
    cr, sp, op, t, sig = stream
    return mb.bulk_rounds_gated(n, cr, sp, op, stake, cuts, vis, mutant=mutant, stats=stats, **KNOBS)


def check(name, L, lo):
    """lo and, through finalize / voter masks / elections, everything decide_fame reports: equal to the oracle's."""
    n, stream, stake, exp, lo3, it3 = case(name)
    cr, sp, op, t, sig = stream
    assert np.array_equal(lo, lo3)
    assert np.array_equal(L, exp["can_see"])
    rnd, S_, wit = mb.finalize(n, cr, L, lo)
    assert np.array_equal(rnd, exp["round"])
    assert np.array_equal(wit, exp["wit"])
    Sw = mb.voter_masks(n, L, rnd, S_, wit, stake)
    fam = np.full(wit.shape, -1, np.int8)
    cons = np.zeros(wit.shape[0], np.uint8)
    new_c, _ = mb.elections(n, wit, Sw, stake, sig[:, 0] >= 128, fam, cons)
    m = wit >= 0
    assert np.array_equal(fam[m], exp["famous"][wit[m]])
    assert np.array_equal(cons, exp["cons"])
    assert list(new_c) == exp["new_c"]


def h_values(name, S):
    """small / medium (loop and sweep neck and neck) / large (the loop always catches up) lags for this stream."""
    it3 = case(name)[5]
    return 2, max(2, (it3 // S) & ~1), 2 * it3 + 16


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("name", list(STREAMS))
def test_gated_model_matches_oracle(name, plan):
    n, stream, stake, exp, lo3, it3 = case(name)
    assert exp["round"].max() >= 3, "the stream must span several rounds"
    N = len(stream[0])
    cuts = cuts_of(plan, N)
    S = len(cuts)
    assert S == len(PLANS[plan]) + 1
    h_small, h_mid, h_large = h_values(name, S)
    # always ahead: the stage still latches one iteration late.  Working iterations: at most those of bulk_rounds_v3 on the
    # whole stream + 2, counted in v3's unit (passes whose tally had candidates: v3 does not count the last launch, which
    # finds no active member and searches nothing) — checked with an unbounded band, where v3 and the kernel take the same
    # steps; with the capped band of KNOBS v3 is no reference for the count even of an ungated loop (it lets a far candidate
    # inherit from a member that resolved by inheritance in the same pass; the kernel, and this model, decide every far
    # candidate of an iteration on the state in front of it), so there the reference is this model on ONE stage — the
    # model's SW_PIPE=1 — + 2, as tests/test_gpu_gated_loop.py has it for the device.
    wide = dict(KNOBS, NEARCAP=N)
    _, lo_w, st_w = mb.bulk_rounds_gated(n, *stream[:3], stake, cuts, lambda t: S, **wide)
    _, lo3w, st3w = mb.bulk_rounds_v3(n, *stream[:3], stake, **wide)
    assert np.array_equal(lo_w, lo3w)
    assert st_w["tallies"] == st_w["iters"] - st_w["idle"] - 1
    assert st_w["tallies"] <= st3w["iters"] + 2, (st_w["iters"], st_w["idle"], st3w["iters"])
    L, lo, st = run_model(name, cuts, lambda t: S)
    check(name, L, lo)
    _, _, st1 = mb.bulk_rounds_gated(n, *stream[:3], stake, [N], lambda t: 1, **KNOBS)
    # (an iteration without candidates is counted as idle by the kernel's rule even when nobody waits: a strided window
    # that ended exactly at the end of a complete chain)
    assert st["iters"] - st["idle"] <= st1["iters"] - st1["idle"] + 2, (st["iters"], st["idle"], st1["iters"], st1["idle"])
    assert st["stage_at"][:2] == [1, S]
    for h in (h_small, h_mid, h_large):
        L, lo, st = run_model(name, cuts, every(h))
        check(name, L, lo)
        if h == h_large:
            assert st["idle"] > 0 and st["member_waits"] > 0, st
    for s in (2, 3):   # jumps
        L, lo, st = run_model(name, cuts, every(h_mid, s))
        check(name, L, lo)
    ml = MaximalLag(len(cuts))
    L, lo, st = run_model(name, cuts, ml, stats=ml.stats)
    check(name, L, lo)
    assert st["idle"] >= S - 1 and st["member_waits"] > 0, st
    assert ml.pub == S and st["stage_at"][-1] == S


@pytest.mark.parametrize("name", list(STREAMS))
def test_gated_model_random_schedules(name):
    n, stream, stake, exp, lo3, it3 = case(name)
    N = len(stream[0])
    rng = np.random.default_rng(1000 + sorted(STREAMS).index(name))
    plans = sorted(PLANS)
    for k in range(20):
        cuts = cuts_of(plans[int(rng.integers(0, len(plans)))], N)
        vis = random_schedule(rng, len(cuts))
        L, lo, st = run_model(name, cuts, vis)
        check(name, L, lo)
        assert all(a <= b for a, b in zip(st["stage_at"], st["stage_at"][1:])) and st["stage_at"][-1] == len(cuts)


MUTANT_CASES = [(name, plan) for name in ("uniform", "slow", "stake") for plan in ("6", "short_head")]


@pytest.mark.parametrize("mutant", ["no_wait", "reset_cursor", "early_latch"])
def test_gated_model_tests_bite(mutant):
    """Each one-line mutant of the model — the wait rule dropped, the cursor reset to the round's start when a member
    waits, the stage used by the windows in the iteration that loads it while band and limit stay one behind — is caught
    by the checks above (a result that differs from the oracle's, or one of the model's own assertions) in at least one
    of a few cases under maximal lag and a large fixed lag; the unmutated model passes the same cases."""
    caught = 0
    for name, plan in MUTANT_CASES:
        N = len(case(name)[1][0])
        cuts = cuts_of(plan, N)
        for sched in ("max", "large"):
            def vis_of():
                ml = MaximalLag(len(cuts))
                return (ml, ml.stats) if sched == "max" else (every(h_values(name, len(cuts))[2]), None)
            vis, stats = vis_of()
            L, lo, st = run_model(name, cuts, vis, stats=stats)
            check(name, L, lo)
            vis, stats = vis_of()
            try:
                L, lo, st = run_model(name, cuts, vis, mutant=mutant, stats=stats)
                check(name, L, lo)
            except AssertionError:
                caught += 1
    assert caught >= 1, "mutant %s passes every case" % mutant
