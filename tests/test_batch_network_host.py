"""CPU: the gossip networks of a batch (csrc/batch_network.hip.h, swbn::begin / swbn::turns) through
tests/batch_network_main.cpp, a stand-alone program built with AddressSanitizer and UBSan and linked with nothing else.  The
program runs the very turn function k_batch_network_turns runs (one lane), every slab segment an allocation of exactly its
size, and writes what every view holds; the tests compare that with the Python model (tests/model_batch_network.py: the
literal BFS of swirld.py:154-159) event by event, and with the C oracle fed each view's stored events under the view's own
step sizes.  Also here: the model against its closed form (the schedule alone fixes the DAG; a view is the ancestors of
its head), the drawn schedule against sw_synth_schedule, the split of a long call, and a network that stops.

The stopping network: whale stakes (tests/batch_cases.py: half of the members without stake, one with more than half of
the total), drawn schedules of at most 300 turns, seeds searched upwards from 0 with the model and the oracle until a
puller's step raises the reference's IndexError (swirld.py:305).  No Python code runs under a sanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import model_batch_network as M
from model_batch_network import oracle_of_view


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("batch_network") / "batch_network_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "batch_network_main.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def prog_lanes(tmp_path_factory):
    """The same program as 16 cooperative lanes (no sanitizers: they do not follow swapcontext)."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("batch_network_lanes") / "batch_network_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-DSW_EXACT_HOST_LANES=16", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "batch_network_main.cpp"), "-o", exe])
    return exe


def run_program(prog, tmp_path, n, cap_events, seed, T, sched=None, given=None, stake=None, coin_period=6, chunk=0):
    """given: (t [T], sig [T][64], root_t [n], root_sig [n][64]).  Returns (network words, list of views as dicts)."""
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as f:
        np.array([n, coin_period, cap_events, seed, T, sched is None, given is not None, chunk], np.int64).tofile(f)
        np.asarray(np.ones(n) if stake is None else stake, np.uint64).tofile(f)
        if sched is not None:
            np.asarray(sched[0], np.int32).tofile(f)
            np.asarray(sched[1], np.int32).tofile(f)
        if given is not None:
            np.asarray(given[0], np.float64).tofile(f)
            np.asarray(given[1], np.uint8).tofile(f)
            np.asarray(given[2], np.float64).tofile(f)
            np.asarray(given[3], np.uint8).tofile(f)
    r = subprocess.run([prog, case, out], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    raw = open(out, "rb").read()
    at = 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a
    net = dict(zip(("begun", "turns", "created", "imported", "stage", "code", "view"), take(np.int64, 7).tolist()))
    views = []
    for _ in range(n):
        w = take(np.int64, 11)
        N = int(w[0])
        v = dict(events=N, head=int(w[1]), hmax=int(w[2]), summary=w[3:])
        for name in ("cr", "sp", "op", "ht", "round", "num"):
            v[name] = take(np.int32, N)
        v["t"], v["sig"], v["tbd"], v["fam_ev"] = take(np.float64, N), take(np.uint8, N * 64).reshape(N, 64), take(np.uint8, N), take(np.int8, N)
        v["can_see"] = take(np.int32, int(w[3]) * n).reshape(-1, n)
        m = int(w[5])
        v["log_ev"], v["log_rr"], v["log_ts"] = take(np.int32, m), take(np.int32, m), take(np.float64, m)
        views.append(v)
    assert at == len(raw)
    return net, views


def assert_view_equals_model(v, mv, n):
    cr, sp, op, t, sig = mv.arrays()
    assert v["events"] == len(cr) and v["head"] == mv.head and v["hmax"] == max(mv.ht)
    for name, want in (("cr", cr), ("sp", sp), ("op", op), ("ht", mv.ht), ("num", mv.num)):
        assert np.array_equal(v[name], want), name
    assert np.array_equal(v["t"].view(np.uint64), t.view(np.uint64)) and np.array_equal(v["sig"], sig)
    assert np.array_equal(v["can_see"], np.array(mv.can_see, np.int32)[:len(v["can_see"])])


def assert_view_equals_oracle(v, o, tx):
    N = v["events"]
    assert o.N == N
    assert np.array_equal(v["round"], o.round[:N]) and np.array_equal(v["can_see"], o.can_see[:N])
    assert np.array_equal(v["fam_ev"], o.famous_by_event[:N]) and np.array_equal(v["tbd"] != 0, np.asarray(o.tbd[:N]) != 0)
    assert list(v["log_ev"]) == list(tx)


def random_schedule(n, T, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, T)
    b = rng.integers(0, n - 1, T)
    return a.astype(np.int32), (b + (b >= a)).astype(np.int32)


# ---- the model against its closed form ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 16])
def test_model_equals_the_closed_form(n):
    for seed in range(4):
        T = 40 + 20 * n
        a, b = random_schedule(n, T, 100 * n + seed)
        net = M.Network(n, seed)
        for i, j in zip(a, b):
            net.turn(int(i), int(j))
        events, anc = M.closed_form(n, list(zip(a.tolist(), b.tolist())))
        assert net.events == events
        for i, v in enumerate(net.views):
            assert set(v.num) == anc[i] and len(v.num) == len(anc[i]), (n, seed, i)
            assert v.num[v.head] == max(k for k, e in enumerate(events) if e[0] == i)
            for e in range(len(v.cr)):   # every stored event is the network's event of its number, parents by number
                want = events[v.num[e]]
                assert (v.cr[e], -1 if v.sp[e] < 0 else v.num[v.sp[e]], -1 if v.op[e] < 0 else v.num[v.op[e]]) == want


def test_model_schedule_equals_sw_synth_schedule(pkg):
    for n, seed in ((2, 0), (3, 7), (16, 2 ** 63 + 5), (70, 12345)):
        a, b = pkg.synth_schedule(n, seed, 0, 200)
        ma, mb = M.schedule(n, seed, 0, 200)
        assert np.array_equal(a, ma) and np.array_equal(b, mb)
        assert (a != b).all() and a.min() >= 0 and a.max() < n and b.min() >= 0 and b.max() < n
        a2, b2 = pkg.synth_schedule(n, seed, 150, 50)
        assert np.array_equal(a2, a[150:]) and np.array_equal(b2, b[150:])


# ---- the turn function under the sanitizers -----------------------------------------------------------------------------
@pytest.mark.parametrize("n,T", [(2, 60), (3, 120), (4, 200), (16, 150), (70, 90)])
def test_explicit_turns_equal_model_and_oracle(prog, tmp_path, n, T):
    rng = np.random.default_rng(n)
    sched = random_schedule(n, T, 5 + n)
    given = (np.cumsum(rng.random(T)) + n, rng.integers(0, 256, (T, 64), dtype=np.uint8), rng.random(n), rng.integers(0, 256, (n, 64), dtype=np.uint8))
    net, views = run_program(prog, tmp_path, n, n + T, 9, T, sched, given)
    m = M.Network(n, 9, given[2], given[3])
    for k in range(T):
        m.turn(int(sched[0][k]), int(sched[1][k]), given[0][k], given[1][k])
    assert (net["begun"], net["turns"], net["created"], net["stage"]) == (1, T, n + T, 0)
    assert net["imported"] == sum(len(v.cr) for v in m.views) - n - T
    for i in range(n):
        assert_view_equals_model(views[i], m.views[i], n)
        o, tx, failed = oracle_of_view(n, m.views[i])
        assert failed is None
        assert_view_equals_oracle(views[i], o, tx)
    if n == 4:
        assert min(len(v["log_ev"]) for v in views) > 0   # every node ordered events (2 and 3 members hardly ever decide a round)


@pytest.mark.parametrize("n", [2, 4, 16, 70])
def test_drawn_turns_equal_the_explicit_form_and_split_calls(prog, tmp_path, pkg, n):
    T, seed = 130, 40 + n
    one = run_program(prog, tmp_path, n, n + T, seed, T)
    split = run_program(prog, tmp_path, n, n + T, seed, T, chunk=7)
    explicit = run_program(prog, tmp_path, n, n + T, seed, T, pkg.synth_schedule(n, seed, 0, T))
    m = M.Network(n, seed)
    m.run(T)
    for net, views in (one, split, explicit):
        assert (net["turns"], net["created"], net["stage"]) == (T, n + T, 0)
        for i in range(n):
            assert_view_equals_model(views[i], m.views[i], n)
            for k in ("round", "fam_ev", "tbd", "log_ev", "log_rr", "summary"):
                assert np.array_equal(views[i][k], one[1][i][k]), k
            assert np.array_equal(views[i]["log_ts"].view(np.uint64), one[1][i]["log_ts"].view(np.uint64))


def test_weighted_stake_and_coin_period_2_equal_the_oracle(prog, tmp_path):
    n, T, seed = 5, 220, 3
    stake = np.array([3, 1, 2, 1, 1], np.uint64)
    net, views = run_program(prog, tmp_path, n, n + T, seed, T, stake=stake, coin_period=2)
    m = M.Network(n, seed)
    m.run(T)
    assert net["stage"] == 0
    for i in range(n):
        assert_view_equals_model(views[i], m.views[i], n)
        o, tx, failed = oracle_of_view(n, m.views[i], stake, 2)
        assert failed is None
        assert_view_equals_oracle(views[i], o, tx)


@pytest.mark.parametrize("n", [2, 4, 16, 33])
def test_cooperative_lanes_equal_one_lane(prog, prog_lanes, tmp_path, n):
    """16 lanes that run one at a time from sync to sync: the level counters, the claims and the import list need only the syncs."""
    T, seed = 120, 7 + n
    one = run_program(prog, tmp_path, n, n + T, seed, T)
    lanes = run_program(prog_lanes, tmp_path, n, n + T, seed, T, chunk=50)
    assert one[0] == lanes[0] and one[0]["turns"] == T
    for a, b in zip(one[1], lanes[1]):
        for k in a:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y), k


# ---- a network that stops ------------------------------------------------------------------------------------------------
def test_the_pinned_stopping_seed_is_the_first_the_search_finds():
    """The search the GPU test does not repeat: seeds upwards from 0 under the whale stakes, drawn schedules of 300 turns."""
    assert M.find_stopping_seed() == M.STOPPING_NETWORK


def test_a_stopping_network_stops_where_the_reference_raises(prog, tmp_path):
    from batch_cases import WHALE_N, whale_stake
    seed, (turn, who) = M.STOPPING_NETWORK
    n, stake, T = WHALE_N, whale_stake(), 300
    net, views = run_program(prog, tmp_path, n, n + T, seed, T, stake=stake, chunk=64)
    # the network ran the failing turn and none after it, in that call or the later ones
    assert (net["turns"], net["created"], net["view"]) == (turn + 1, n + turn + 1, who)
    assert net["stage"] == 3 and net["code"] == -3   # find_order, IndexError (swirld.py:305)
    m = M.Network(n, seed)
    m.run(turn + 1)
    for i in range(n):
        assert_view_equals_model(views[i], m.views[i], n)
        o, tx, failed = oracle_of_view(n, m.views[i], stake)
        assert (failed is not None) == (i == who)
        assert np.array_equal(views[i]["round"], o.round[:views[i]["events"]])
        assert (views[i]["summary"][5] != 0) == (i == who)   # only the puller's view is frozen


# ---- the reference's own runs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,chunk", [("net_4_250_1_c6", 0), ("net_4_250_6_c2", 7), ("net_7_400_1_c6", 64)])
def test_reference_fixtures_through_the_turn_function(prog, tmp_path, name, chunk):
    """A case file written from a fixture of tests/golden/network/: the reference's schedule, timestamps and signatures; every
    recorded field of every node comes back equal (tests/test_batch_network_golden.py states the comparison)."""
    import test_batch_network_golden as G
    g = G.load(name)
    n, T = int(g["n"]), int(g["turns"])
    given = (g["t"][n:], g["sig"][n:], g["t"][:n], g["sig"][:n])
    net, views = run_program(prog, tmp_path, n, n + T, 0, T, (g["puller"], g["peer"]), given, coin_period=int(g["coin_period"]), chunk=chunk)
    assert (net["turns"], net["created"], net["stage"]) == (T, n + T, 0)
    m = G.replay(name)
    for i, v in enumerate(views):
        assert_view_equals_model(v, m.views[i], n)
        ordered = np.zeros(v["events"], bool)
        wit = np.full((int(v["round"].max()) + 1, n), -1, np.int32)
        for e in range(v["events"]):   # the witness table from rounds and self-parents (swirld.py:221-222)
            if v["sp"][e] < 0 or v["round"][e] > v["round"][v["sp"][e]]:
                wit[v["round"][e], v["cr"][e]] = e
        cons = np.zeros(len(wit), np.uint8)
        cons[g["node%d_consensus" % i]] = 1   # (the program writes no consensus column: the ordered log below depends on it)
        G.assert_node_equals_fixture(g, i, v["num"], v["round"], v["can_see"][v["head"]], wit, v["fam_ev"], cons, v["log_ev"], v["tbd"])
