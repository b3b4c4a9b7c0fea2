"""GPU (-m gpu): the gated round loop under a FORCED sweep lag.  SW_GATE_LAG=h / SW_GATE_STEP=s (test hooks) make
the host publish the loop's stages itself — s more behind every piece of h iterations — so that which iteration sees which
stage is a fixed function of (h, s) instead of the outcome of a race with the sweep stream: iteration t loads vis = min(S, 1 + (t // h) * s).
With a large h the loop catches up with the "sweep" at every stage boundary and the wait / resume path of k_resolve_band runs
in every case; everything is compared with the C oracle (rounds, witness table, fame, consensus, can_see rows, V / P2
counters, new_c per call, find_order), the iteration counts are bounded, and for small member counts they are compared with
the executable specification of the loop (tests/model_bulk.py, bulk_rounds_gated) run on the same cuts and schedule.

The oracle runs once per stream: the runs of all selected cases are started on a few host threads behind the first case that
asks for one (the oracle's C calls release the GIL) and every case waits for its own."""
import importlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle_pool import compare_state
from synth_util import silence
from test_gpu_gated_loop import CUTS_12, digest

pytestmark = pytest.mark.gpu

# ---- streams: name -> (members, events, seed, mode, p0, p1, [(silent member, from fraction)], chunk or None, stake seed or None)
MATRIX = {   # the seven shapes of test_gated_loop_matches_oracle, with their knobs
    "m8": ((8, 70000, 31, 0, 0, 0, (), None, None), {}),
    "m64": ((64, 100000, 32, 0, 0, 0, (), None, None), {}),
    "m64coin": ((64, 100000, 33, 2, 0.3, 0.03, (), None, None), {}),
    "m128cliques": ((128, 100000, 34, 1, 0.5, 0.02, (), None, None), {"SW_CUTS": "0.5"}),
    "m200x12": ((200, 120000, 35, 0, 0, 0, (), None, None), {"SW_CUTS": CUTS_12}),
    "m256head": ((256, 120000, 36, 0, 0, 0, (), None, None), {"SW_CUTS": "0.04,0.2,0.4,0.6,0.8"}),
    "m256shot": ((256, 120000, 37, 0, 0, 0, (), None, None), {"SW_SHOT_PCT": "50"}),
}
INCR = {     # the three schedules of test_gated_equals_per_subbatch_loops_incremental
    "i64": ((64, 210000, 41, 0, 0, 0, (), 70001, None), {}),
    "i256": ((256, 200000, 42, 0, 0, 0, (), 66667, None), {}),
    "i128coin": ((128, 200000, 43, 2, 0.3, 0.03, (), 99991, None), {}),
}
SILENT = {   # the two of test_gated_loop_member_falls_silent + three members whose chains end in the head sub-batch
    "s64": ((64, 150000, 51, 0, 0, 0, ((5, 0.4),), None, None), {}),
    "s256": ((256, 200000, 51, 0, 0, 0, ((17, 0.5),), None, None), {}),
    "s64head": ((64, 150000, 52, 0, 0, 0, ((3, 0.1), (20, 0.1), (41, 0.1)), None, None), {"SW_CUTS": "0.15,0.4,0.6,0.8"}),
}
MODEL = {    # small member counts: the numpy model follows the whole call on the host
    "a8": ((8, 70000, 38, 0, 0, 0, (), None, None), {"SW_CUTS": "0.06,0.12,0.5"}),       # (short early stages: the loop waits at h = 256)
    "a16slow": ((16, 66000, 39, 2, 0.3, 0.05, (), None, None), {"SW_CUTS": "0.07,0.3,0.5,0.7,0.9"}),
}
LAGS = [(0, 1), (2, 1), (2, 2), (16, 1), (64, 1), (256, 1)]


def draw(seed):
    """One draw of the knob sweep: 66 k - 100 k events, knobs that keep the call on the gated loop."""
    rng = np.random.default_rng(9100 + seed)
    n = int(rng.choice([8, 33, 64, 100, 130, 200, 256]))
    N = int(rng.integers(66000, 100001))
    mode = int(rng.integers(0, 4))
    p0, p1 = float(rng.uniform(0.01, 0.7)), float(rng.uniform(0.002, 0.2))
    env = {"SW_CANSEE_IMPL": "6", "SW_GATED": "1"}
    env["SW_TALLY_K"] = str(int(rng.choice([4, 8, 16, 28, 32, 60])))
    env["SW_TALLY_IMPL"] = str(int(rng.choice([0, 1, 2])))
    env["SW_SKIP"] = str(int(rng.choice([0, 1, 2, 3, 7])))
    if rng.random() < 0.5:
        env["SW_GALLOP"] = str(int(rng.choice([0, 1, 2, 3])))
    env["SW_BAND"] = str(int(rng.choice([64, 256, 1024])))     # (small: the band cap doubles while members wait)
    if rng.random() < 0.5:
        env["SW_BAND_MAX"] = str(int(rng.choice([1024, 1 << 20])))
    env["SW_FIN_BAND"] = str(int(rng.choice([0, 1, 1])))
    env["SW_BAND_FAST"] = str(int(rng.choice([0, 1, 1])))
    env["SW_TALLY_FILTER"] = str(int(rng.choice([0, 1])))
    env["SW_GRAPH"] = str(int(rng.choice([0, 1])))
    env["SW_SHOT_PCT"] = str(int(rng.choice([50, 100])))
    parts = int(rng.integers(2, 13))
    env["SW_CUTS"] = ",".join("%.4f" % f for f in np.sort(rng.uniform(0.03, 0.97, parts - 1)))
    h, s = LAGS[int(rng.integers(0, len(LAGS)))]
    if h:
        env["SW_GATE_LAG"], env["SW_GATE_STEP"] = str(h), str(s)
    stake_seed = 9300 + seed if seed % 3 == 2 else None             # a third of the draws: integer stakes 1 .. 5
    return (n, N, 9200 + seed, mode, p0, p1, (), None, stake_seed), env


KNOBS = {"k%d" % i: draw(i) for i in range(24)}
FULL = {"full": ((256, 1_000_000, 3, 0, 0, 0, (), None, None), {})}
CASES = dict(MATRIX, **INCR, **SILENT, **MODEL, **KNOBS)      # (the full-size case has no oracle run: it compares with SW_GATED=0)


def make_stream(spec):
    pkg = importlib.import_module("py-swirld_amd")
    n, N, seed, mode, p0, p1, sil, chunk, stake_seed = spec
    stream = pkg.synth_hashgraph(n, N, seed, mode, p0, p1)
    for member, frac in sil:
        stream = silence(stream, member, int(N * frac))
    stake = None
    if stake_seed is not None:
        stake = np.random.default_rng(stake_seed).integers(1, 6, n).astype(np.uint64)
    return stream, stake


def oracle_job(spec):
    from oracle.oracle import Oracle
    stream, stake = make_stream(spec)
    n, chunk = spec[0], spec[7]
    N = len(stream[0])
    o = Oracle(n, stake)
    ncs = []
    for a in range(0, N, chunk or N):
        b = min(N, a + (chunk or N))
        o.append_events(*[x[a:b] for x in stream])
        o.divide_rounds(a, b - a)
        ncs.append([int(r) for r in o.decide_fame()])
    try:    # (the reference's find_order is stateful: asked once, here, and kept with the run)
        order = np.array(o.find_order(ncs[-1])) if chunk is None else None
    except Exception:   # (weighted stakes: IndexError of the reference with a single seeing witness, as in test_gpu_random.py)
        assert stake is not None
        order = None
    return stream, stake, (o, order), ncs


@pytest.fixture(scope="module")
def oracles(request, pkg):
    """name -> (stream, stake, oracle, new_c per call) of the selected cases, computed once each on background threads."""
    wanted = []
    for it in request.session.items:
        cs = getattr(it, "callspec", None)
        if it.module is request.module and cs is not None and cs.params.get("case") in CASES and cs.params["case"] not in wanted:
            wanted.append(cs.params["case"])
    pool = ThreadPoolExecutor(max_workers=8)
    futs = {name: pool.submit(oracle_job, CASES[name][0]) for name in wanted}

    class Get:
        def __call__(self, name, keep=True):
            res = futs[name].result()
            if not keep:
                del futs[name]
            return res
    yield Get()
    pool.shutdown(wait=True, cancel_futures=True)


def cut_plan(K, env, pipe=5):
    """The event limits of the sub-batches of a divide_rounds call over events [0, K) — plan_cuts' plan (csrc/swirld_hip.hip): SW_CUTS fractions,
    else a head of K / 16 and five graduated parts, every boundary rounded down to a multiple of 4096."""
    cut = [0]
    if "SW_CUTS" in env and K >= 65536:
        for f in env["SW_CUTS"].split(","):
            b = (int(float(f) * K) >> 12) << 12
            if cut[-1] < b < K:
                cut.append(b)
    elif K >= 65536:
        head = K // 16
        w = [0.5, 0.9, 1.2] + [1.0] * (pipe - 3)
        acc = 0.0
        for x in w:
            b = ((head + int((K - head) * (acc / sum(w)))) >> 12) << 12
            acc += x
            if cut[-1] < b < K:
                cut.append(b)
    return cut[1:] + [K]


def run(pkg, n, stream, stake, chunk, env, monkeypatch):
    """A fresh context under `env`, the stream in calls of `chunk` events; (context, new_c per call, counters).  `env` stays
    set for the whole run: most knobs are read when the context is created, SW_CUTS by every divide_rounds call."""
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        h = pkg.Hashgraph(n, stake)
        N = len(stream[0])
        h.reserve(N)
        ncs = []
        for a in range(0, N, chunk or N):
            b = min(N, a + (chunk or N))
            h.append_events(*[x[a:b] for x in stream])
            h.divide_rounds(a, b - a)
            ncs.append([int(r) for r in h.decide_fame()])
    c = h.counters()
    return h, ncs, (int(c["round_iterations"]), int(c["gated_idle_iterations"]), int(c["gated_calls"]))


def lag_env(env, h, s):
    return dict(env, SW_GATED="1", SW_GATE_LAG=str(h), SW_GATE_STEP=str(s)) if h else dict(env, SW_GATED="1")


_base = {}


def baseline(pkg, monkeypatch, name, stream, stake, env, chunk=None):
    """Per case, once: (iterations, idle) of the free-running gated loop and the iterations of the same configuration as ONE
    loop (SW_PIPE=1: one sub-batch, nothing to wait for) — the references of the lag h_mid and of the iteration bound."""
    if name not in _base:
        n = CASES.get(name, FULL.get(name))[0][0]
        hg, _, cg = run(pkg, n, stream, stake, chunk, dict(env, SW_GATED="1"), monkeypatch)
        hg.close()
        one = {k: v for k, v in env.items() if k != "SW_CUTS"}
        h1, _, c1 = run(pkg, n, stream, stake, chunk, dict(one, SW_PIPE="1"), monkeypatch)
        h1.close()
        assert c1[2] == 0
        _base[name] = (cg[0], cg[1], c1[0])
    return _base[name]


def even(x):
    """A lag the hook accepts: even, 2 .. 256."""
    return min(256, max(2, int(x) & ~1))


def bound(single, stages, calls=1):
    """Working iterations the lagged loop may take: the single loop's + 2 (what test_gated_full_size_256x1M grants the
    free-running loop) + 2 per stage boundary — a boundary can split one round's search into the iteration in which some
    members published while others began to wait and the one in which the waiters resume, and the latch is one late."""
    return single + calls * (2 + 2 * (stages - 1))


def check_vs_oracle(h, ncs, o_, onc, N, stake=None, step=20_000):
    o, order = o_
    assert ncs == onc
    compare_state(h, o, N, can_see_step=step)
    if order is None:   # (call schedules: the order is test_gpu_order.py's; weighted stakes: the reference raised)
        assert stake is not None or len(ncs) > 1
        return
    assert np.array_equal(h.find_order(ncs[-1]), order)


@pytest.mark.parametrize("hs", [(2, 1), (2, 3), ("mid", 1), (256, 1)], ids=lambda v: "h%s_s%d" % v)
@pytest.mark.parametrize("case", list(MATRIX))
def test_lag_matrix_matches_oracle(pkg, monkeypatch, oracles, case, hs):
    """(256, 1): the loop is done with every stage long before the next one is published, so it must report waiting
    iterations; h_mid = the free-running loop's iterations per sub-batch: loop and sweep neck and neck.
    Measured on an MI355X (iterations / idle / working, bound): (2, 1) and (2, 3) idle 0 - 2 everywhere; h_mid idle 1 - 51
    (64 members, coin rounds, h = 36: 279 / 51 / 228, bound 237); (256, 1): 8 members 1903 / 326 / 1577 (1587), 64 members
    1316 / 1163 / 153 (160), two cliques 292 / 225 / 67 (70), 12 sub-batches 2825 / 2764 / 61 (74), 256 members 1291 / 1250 /
    41 (48)."""
    spec, env = MATRIX[case]
    n = spec[0]
    stream, stake, o, onc = oracles(case)
    N = len(stream[0])
    S = len(cut_plan(N, env))
    its0, idle0, single = baseline(pkg, monkeypatch, case, stream, stake, env)
    h_, s_ = hs
    if h_ == "mid":
        h_ = even(its0 // S)
    hg, ncs, (its, idle, calls) = run(pkg, n, stream, stake, None, lag_env(env, h_, s_), monkeypatch)
    print("\n[lag] %s n=%d N=%d S=%d h=%d s=%d: %d iterations, %d idle, %d working | free-running %d + %d idle, single loop %d, bound %d"
          % (case, n, N, S, h_, s_, its, idle, its - idle, its0 - idle0, idle0, single, bound(single, S)))
    assert calls == 1, "the call must take the gated loop"
    assert o[0].max_round >= 3, "the case must span several rounds"
    check_vs_oracle(hg, ncs, o, onc, N)
    hg.close()
    if hs == (256, 1):
        assert idle > 0, "a lag of 256 iterations per stage must make the loop wait"
    assert its - idle <= bound(single, S), (its, idle, single, S)


@pytest.mark.parametrize("hs", [(16, 1), (256, 1)], ids=lambda v: "h%s_s%d" % v)
def test_lag_hook_is_deterministic(pkg, monkeypatch, hs):
    """Two fresh contexts under the same (h, s): every input of every iteration is fixed by the order of launches on the loop
    stream, so both iteration counts are equal."""
    spec, env = MATRIX["m64"]
    stream, stake = make_stream(spec)
    res = []
    for _ in range(2):
        h, ncs, cnt = run(pkg, spec[0], stream, stake, None, lag_env(env, *hs), monkeypatch)
        res.append((cnt, ncs, digest(h)))
        h.close()
    print("\n[determinism] h=%d s=%d: %r / %r" % (hs + (res[0][0], res[1][0])))
    assert res[0][0][2] == 1
    assert res[0][0] == res[1][0]
    assert res[0][1] == res[1][1]
    for a, b in zip(res[0][2], res[1][2]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("hs", [(16, 1), (64, 2), (256, 1)], ids=lambda v: "h%s_s%d" % v)
@pytest.mark.parametrize("case", list(MODEL))
def test_lagged_loop_agrees_with_model(pkg, monkeypatch, oracles, case, hs):
    """bulk_rounds_gated on the host with the device's cuts, knobs and schedule: the same lo table, and — the model mirroring
    k_resolve_band's rules step by step — the same idle and working iteration counts as the device reports (asserted
    EXACTLY; the model's `iters` is the device's `round_iterations`: every launch up to the one that finds no active
    member).  Measured on an MI355X: equal in all six cases, no constant between them — 8 members at (256, 1) 2952 iterations
    of which 192 idle on both sides, 16 members with slow ones 1738 of which 170 idle; at (16, 1) and (64, 2) neither waits."""
    import model_bulk as mb
    spec, env0 = MODEL[case]
    n = spec[0]
    env = dict(env0, SW_TALLY_IMPL="1", SW_TALLY_K="8", SW_SKIP="1", SW_GALLOP="2", SW_BAND="64", SW_BAND_MAX=str(1 << 20))
    stream, stake, o, onc = oracles(case)
    N = len(stream[0])
    cuts = cut_plan(N, env)
    h_, s_ = hs
    hg, ncs, (its, idle, calls) = run(pkg, n, stream, stake, None, lag_env(env, h_, s_), monkeypatch)
    assert calls == 1
    check_vs_oracle(hg, ncs, o, onc, N)
    wit = hg.witnesses().copy()
    hg.close()
    cr, sp, op = stream[:3]
    L, lo, st = mb.bulk_rounds_gated(n, cr, sp, op, np.ones(n, np.int64), cuts, lambda t: 1 + (t // h_) * s_,
                                     K=8, NEARCAP=64, CAPMAX=1 << 20, gallop_after=2, skip=1)
    print("\n[model] %s n=%d N=%d S=%d h=%d s=%d: device %d iterations, %d idle | model %d iterations, %d idle, %d member-iterations waiting"
          % (case, n, N, len(cuts), h_, s_, its, idle, st["iters"], st["idle"], st["member_waits"]))
    rnd, S_, wit_m = mb.finalize(n, cr, L, lo)
    assert np.array_equal(rnd, o[0].round) and np.array_equal(wit_m, wit)
    assert (st["idle"], st["iters"] - st["idle"]) == (idle, its - idle)


@pytest.mark.parametrize("hs", [("mid", 1), (256, 1)], ids=lambda v: "h%s_s%d" % v)
@pytest.mark.parametrize("case", list(INCR))
def test_lagged_incremental_matches_oracle_and_per_subbatch_loops(pkg, monkeypatch, oracles, case, hs):
    """Calls that end mid-round, gated calls that start at r_start > 0 with a dirty row 0 — under lag."""
    spec, env = INCR[case]
    n, chunk = spec[0], spec[7]
    stream, stake, o, onc = oracles(case)
    N = len(stream[0])
    lens = [min(N, a + chunk) - a for a in range(0, N, chunk)]
    big = sum(1 for k in lens if k >= 65536)
    S = max(len(cut_plan(k, env)) for k in lens)
    its0, idle0, single = baseline(pkg, monkeypatch, case, stream, stake, env, chunk)
    h_, s_ = hs
    if h_ == "mid":
        h_ = even(its0 // (big * S))
    hg, ncg, (its, idle, calls) = run(pkg, n, stream, stake, chunk, lag_env(env, h_, s_), monkeypatch)
    hu, ncu, cu = run(pkg, n, stream, stake, chunk, dict(env, SW_GATED="0"), monkeypatch)
    print("\n[incremental] %s h=%d s=%d: %d iterations, %d idle | free-running %d + %d idle, single loops %d, bound %d"
          % (case, h_, s_, its, idle, its0 - idle0, idle0, single, bound(single, S, big)))
    assert calls == big, "every call of >= 64 k events takes the gated loop"
    assert cu[2] == 0
    assert ncg == ncu
    for a, b in zip(digest(hg), digest(hu)):
        assert np.array_equal(a, b)
    check_vs_oracle(hg, ncg, o, onc, N, step=40_000)
    hg.close()
    hu.close()
    if hs == (256, 1):
        assert idle > 0
    assert its - idle <= bound(single, S, big), (its, idle, single, S, big)


@pytest.mark.parametrize("case", list(SILENT))
def test_lagged_loop_silent_members(pkg, monkeypatch, oracles, case):
    """Members whose chains stop growing in an early sub-batch, at (256, 1): they are exhausted where their chains end, and
    the loop does not wait past the last publication — each of the S publications comes at most h iterations after the loop
    could have used it, so at most h * S iterations are idle."""
    spec, env = SILENT[case]
    n = spec[0]
    stream, stake, o, onc = oracles(case)
    N = len(stream[0])
    S = len(cut_plan(N, env))
    hg, ncs, (its, idle, calls) = run(pkg, n, stream, stake, None, lag_env(env, 256, 1), monkeypatch)
    print("\n[silent] %s N=%d S=%d: %d iterations, %d idle (h * S = %d)" % (case, N, S, its, idle, 256 * S))
    assert calls == 1
    check_vs_oracle(hg, ncs, o, onc, N)
    hg.close()
    assert 0 < idle <= 256 * S


@pytest.mark.parametrize("case", list(KNOBS))
def test_knobs_gated_lag_sweep(pkg, monkeypatch, oracles, case):
    spec, env = KNOBS[case]
    n = spec[0]
    stream, stake, o, onc = oracles(case, keep=False)
    N = len(stream[0])
    hg, ncs, (its, idle, calls) = run(pkg, n, stream, stake, None, env, monkeypatch)
    print("\n[knobs] %s n=%d N=%d mode=%d stake=%s %s: %d iterations, %d idle" % (
        case, n, N, spec[3], "unit" if stake is None else "1..5", " ".join("%s=%s" % kv for kv in sorted(env.items())), its, idle))
    assert calls >= 1, "the draw must stay on the gated loop"
    check_vs_oracle(hg, ncs, o, onc, N, stake)
    hg.close()


def test_lagged_full_size_256x1M(pkg, monkeypatch):
    """bench.py's workload under (h_mid, 1) and (256, 1): every row, new_c and the order against the per-sub-batch loops."""
    spec, env = FULL["full"]
    n, N = spec[0], spec[1]
    stream, stake = make_stream(spec)
    S = len(cut_plan(N, env))
    its0, idle0, single = baseline(pkg, monkeypatch, "full", stream, stake, env)
    hu, ncu, cu = run(pkg, n, stream, stake, None, {"SW_GATED": "0"}, monkeypatch)
    ref = (digest(hu), ncu, hu.find_order(ncu[0]))
    hu.close()
    assert cu[2] == 0
    for h_, s_ in ((even(its0 // S), 1), (256, 1)):
        hg, ncg, (its, idle, calls) = run(pkg, n, stream, stake, None, lag_env(env, h_, s_), monkeypatch)
        print("\n[full size] h=%d s=%d: %d iterations, %d idle | free-running %d + %d idle, single loop %d, bound %d"
              % (h_, s_, its, idle, its0 - idle0, idle0, single, bound(single, S)))
        assert calls == 1
        for a, b in zip(ref[0], digest(hg)):
            assert np.array_equal(a, b)
        assert ncg == ref[1]
        assert np.array_equal(hg.find_order(ncg[0]), ref[2])
        hg.close()
        if h_ == 256:
            assert idle > 0
        assert its - idle <= bound(single, S), (its, idle, single, S)
