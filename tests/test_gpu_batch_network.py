"""GPU (-m gpu): gossip networks in a batch (sw_network_batch_*, csrc/batch_network.hip.h): consecutive hashgraphs are the
nodes' views of one network, one wavefront runs a network's turns.  The references: the Python model of the turn
(tests/model_batch_network.py: the literal BFS of swirld.py:154-159), a batch FED by append + step with the model's events
under each view's own step sizes (the route the library had before), and the C oracle per view.  Comparisons are
equalities of arrays; doubles are compared as bytes.  The turn function on the CPU, under the sanitizers and as cooperative
lanes: tests/test_batch_network_host.py."""
import functools
import types

import numpy as np
import pytest

import model_batch_network as M

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -22, -34


@functools.lru_cache(maxsize=None)
def model(n, seed, T):
    """The model's network after T drawn turns; computed once, shared, not modified."""
    m = M.Network(n, seed)
    m.run(T)
    return m


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return a.shape == b.shape and np.array_equal(a, b)


def assert_view(hb, b, mv):
    """Every stored field of view b against the model's view: events, numbers, heights, head."""
    N = len(mv.cr)
    assert hb.summary(b).events == N, b
    got = hb.events(b)
    for x, y, name in zip(got, mv.arrays(), ("creator", "self_parent", "other_parent", "t", "sig")):
        assert same(x, y), (b, name)
    assert same(hb.event_numbers(b), np.array(mv.num, np.int32)), b
    assert same(hb.heights(b), np.array(mv.ht, np.int32)), b
    assert same(hb.can_see(b), np.array(mv.can_see, np.int32)[:hb.summary(b).divided]), b
    assert hb.network_heads()[b] == mv.head


def assert_network(hb, g, m):
    n = m.n
    st = hb.network_status(g)
    assert (st.begun, st.turns, st.created, st.stage) == (1, m.turns, m.created, 0), st
    for i in range(n):
        assert_view(hb, g * n + i, m.views[i])


def results(hb, b):
    """What consensus left in hashgraph b, as bytes."""
    return [np.asarray(x).tobytes() for x in (hb.rounds(b), hb.can_see(b), hb.witnesses(b), hb.famous(b), hb.famous_events(b), hb.consensus(b))
            + hb.ordered(b) + hb.events(b)]


def assert_networks_equal(x, gx, y, gy, n):
    assert x.network_status(gx) == y.network_status(gy)
    for i in range(n):
        bx, by = gx * n + i, gy * n + i
        assert results(x, bx) == results(y, by), i
        assert same(x.event_numbers(bx), y.event_numbers(by)) and x.summary(bx) == y.summary(by), i
    assert same(x.network_heads()[gx * n:(gx + 1) * n], y.network_heads()[gy * n:(gy + 1) * n])


def fed_batch(pkg, m, stake=None, coin_period=6, cap_events=None):
    """One network's views as a batch filled by append + step: view i's events under its own step sizes, the root's divide
    merged into the first turn's step (divide goes event by event, and a decide_fame over one root decides nothing)."""
    n = m.n
    hb = pkg.HashgraphBatch(n, n, stake, coin_period, cap_events=cap_events or m.created)
    arrays = [v.arrays() for v in m.views]
    steps = [[(0, v.steps[0][1] + v.steps[1][1])] + v.steps[2:] if len(v.steps) > 1 else list(v.steps) for v in m.views]
    for k in range(max(len(s) for s in steps)):
        parts, K = [None] * n, np.zeros(n, np.int64)
        for i in range(n):
            if k < len(steps[i]):
                a, c = steps[i][k]
                parts[i] = tuple(x[a:a + c] for x in arrays[i])
                K[i] = c
        hb.append(parts)
        assert hb.step(K, collect=False) == 0
    return hb


def assert_equals_fed(hb, g, fed, n):
    """Summaries, rounds, witnesses, fame, the ordered log with round received and consensus time: the fed batch's."""
    for i in range(n):
        b = g * n + i
        assert results(hb, b) == results(fed, i), i
        sa, sb = hb.summary(b), fed.summary(i)
        assert (sa.events, sa.divided, sa.rounds, sa.ordered, sa.stage) == (sb.events, sb.divided, sb.rounds, sb.ordered, sb.stage), i


# ---- 1. the drawn form, the explicit form, instalments, the model, the fed batch -------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 16, 64, 70])
def test_drawn_form_equals_explicit_form_and_model(pkg, n):
    """Network 0 draws 150 turns in one call, network 1 gets sw_synth_schedule's turns, network 2 draws 61 then 89,
    network 3 runs them one per call.  64 and 70 members: the member loops stride past the wavefront."""
    T, seed = 150, 900 if n == 4 else 900 + n   # (seed 900 at 4 members: every node orders 88 events, by the oracle)
    m = model(n, seed, T)
    pu, pe = pkg.synth_schedule(n, seed, 0, T)
    assert list(zip(pu.tolist(), pe.tolist())) == m.schedule
    hb = pkg.HashgraphBatch(4 * n, n, cap_events=n + T)
    hb.network_begin(seed)
    assert hb.network_run([T, 0, 61, 0]) == 0
    assert hb.network_turns([None, (pu, pe), None, None]) == 0
    assert hb.network_run([0, 0, T - 61, 0]) == 0
    for k in range(T):
        assert hb.network_run([0, 0, 0, 1]) == 0
    assert_network(hb, 0, m)
    for g in (1, 2, 3):
        assert_networks_equal(hb, 0, hb, g, n)
    if n <= 16:
        fed = fed_batch(pkg, m)
        assert_equals_fed(hb, 0, fed, n)
        fed.close()
    if n == 4:
        assert [s.ordered for s in hb.summary()] == [88] * 16   # every node ordered events
    st = hb.network_stats()
    per = lambda k: -(-k // 64)   # launches of a call whose longest network runs k turns
    assert (st.calls, st.turns, st.launches) == (3 + T, 4 * T, 1 + per(T) + per(T) + per(T - 61) + T)
    assert st.imported == 4 * (sum(len(v.cr) for v in m.views) - n - T)
    x = hb.export_event_numbers()
    for b in (0, n, 4 * n - 1):
        assert same(x["numbers"][x["off"][b]:x["off"][b + 1]], hb.event_numbers(b))
    hb.close()


# ---- 2. every view against the C oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,coin_period,weighted", [(4, 2, True), (16, 6, True), (70, 2, False), (4, 6, False)])
def test_every_view_equals_the_oracle(pkg, n, coin_period, weighted):
    T, seed = 200 if n == 4 else 150, 31 + n
    stake = None
    if weighted:
        stake = (1 + np.random.default_rng(n).integers(0, 3, n)).astype(np.uint64)
    m = model(n, seed, T)
    hb = pkg.HashgraphBatch(n, n, stake, coin_period, cap_events=n + T)
    hb.network_begin(seed)
    assert hb.network_run(T) == 0
    assert_network(hb, 0, m)
    for i in range(n):
        stored = types.SimpleNamespace(arrays=lambda i=i: hb.events(i), steps=m.views[i].steps)   # the view's STORED events
        o, tx, failed = M.oracle_of_view(n, stored, stake, coin_period)
        assert failed is None
        N = hb.summary(i).events
        assert same(hb.rounds(i), o.round[:N]) and same(hb.can_see(i), o.can_see[:N]) and same(hb.famous_events(i), o.famous_by_event[:N])
        assert same(hb.witnesses(i), o.witnesses()) and same(hb.consensus(i), o.consensus())
        assert list(hb.transactions(i)) == list(tx)
    hb.close()


# ---- 3. the same event in every view ---------------------------------------------------------------------------------------
def test_an_event_is_the_same_in_every_view(pkg):
    n, T, seed = 16, 150, 5
    hb = pkg.HashgraphBatch(n, n, cap_events=n + T)
    hb.network_begin(seed)
    hb.network_run(T)
    events, _ = M.closed_form(n, model(n, seed, T).schedule)
    seen = {}
    for b in range(n):
        cr, sp, op, t, sig = hb.events(b)
        num, ht = hb.event_numbers(b), hb.heights(b)
        for e in range(len(cr)):
            me = (int(cr[e]), -1 if sp[e] < 0 else int(num[sp[e]]), -1 if op[e] < 0 else int(num[op[e]]), t[e].tobytes(), sig[e].tobytes(), int(ht[e]))
            assert me[:3] == events[num[e]]
            assert seen.setdefault(int(num[e]), me) == me
    assert len(seen) == n + T   # some view holds every event of the network: its creator's
    hb.close()


# ---- 4. the reference's own runs: fixtures, every field per view ------------------------------------------------------------
def fixture_names():
    import test_batch_network_golden as G
    return G.NAMES


@pytest.mark.parametrize("name", fixture_names())
def test_reference_fixtures_under_five_chunkings(pkg, name):
    """tests/golden/network/: the unmodified reference's test(n, turns) — its schedule, timestamps and signatures go in, and
    every recorded field of every node must come out.  Five copies of the network in one batch: all turns in one call, 1 per
    call, 7 per call, two copies sitting out alternate calls of 20 turns, the last of them begun later."""
    import test_batch_network_golden as G
    g = G.load(name)
    n, T, C, copies = int(g["n"]), int(g["turns"]), int(g["coin_period"]), 5
    pu, pe, t, sig = g["puller"], g["peer"], g["t"][n:], g["sig"][n:]
    roots = dict(root_t=np.tile(g["t"][:n], (copies, 1)), root_sig=np.tile(g["sig"][:n], (copies, 1, 1)))
    part = lambda a, z: (pu[a:z], pe[a:z], t[a:z], sig[a:z])
    hb = pkg.HashgraphBatch(copies * n, n, coin_period=C, cap_events=n + T)
    hb.network_begin(0, which=[1, 1, 1, 1, 0], **roots)
    assert hb.network_turns([part(0, T), None, None, None, None]) == 0
    for k in range(T):
        hb.network_turns([None, part(k, k + 1), None, None, None])
    for a in range(0, T, 7):
        hb.network_turns([None, None, part(a, min(T, a + 7)), None, None])
    hb.network_begin(0, which=[0, 0, 0, 0, 1], **roots)
    for k, a in enumerate(range(0, T, 20)):
        z = min(T, a + 20)
        hb.network_turns([None, None, None, part(a, z) if k % 2 == 0 else None, part(a, z) if k % 2 else None])
        hb.network_turns([None, None, None, part(a, z) if k % 2 else None, part(a, z) if k % 2 == 0 else None])
    m = G.replay(name)
    heads = hb.network_heads()
    for c in range(copies):
        st = hb.network_status(c)
        assert (st.turns, st.created, st.stage) == (T, n + T, 0), (c, st)
        for i in range(n):
            b = c * n + i
            if c == 0:
                assert_view(hb, b, m.views[i])
            num = hb.event_numbers(b)
            tbd = np.ones(len(num), np.uint8)
            tbd[hb.transactions(b)] = 0   # (an event leaves tbd exactly when it is ordered, swirld.py:294-295, 309)
            G.assert_node_equals_fixture(g, i, num, hb.rounds(b), hb.can_see(b, int(heads[b]), 1)[0], hb.witnesses(b), hb.famous_events(b),
                                         hb.consensus(b), hb.transactions(b), tbd)
        if c:
            assert_networks_equal(hb, 0, hb, c, n)
    hb.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def refused(pkg, code, fn, *a, **k):
    with pytest.raises(pkg.SwirldHipError) as ei:
        fn(*a, **k)
    assert ei.value.code == code, ei.value


def test_refusals_leave_no_trace(pkg):
    n, T = 4, 30
    one = pkg.HashgraphBatch(7, n, cap_events=64)
    refused(pkg, EINVAL, one.network_begin, 1)   # 7 hashgraphs are no multiple of 4
    one.close()
    solo = pkg.HashgraphBatch(2, 1, cap_events=8)
    refused(pkg, EINVAL, solo.network_begin, 1)   # fewer than 2 members
    solo.close()
    stake = np.ones((3 * n, n), np.uint64)
    stake[2 * n + 1, 0] = 2   # network 2: view 1 has another stake row
    hb = pkg.HashgraphBatch(3 * n, n, stake, cap_events=n + T)
    fresh = pkg.HashgraphBatch(3 * n, n, stake, cap_events=n + T)
    refused(pkg, EINVAL, hb.network_begin, 1)                       # network 2's stake rows differ
    refused(pkg, EINVAL, hb.network_run, [1, 0, 0])                # never begun
    hb.synth_begin(3, which=np.arange(3 * n) == n)
    refused(pkg, EINVAL, hb.network_begin, 1, which=[0, 1, 0])     # a view with generator parameters
    hb.network_begin([7, 8, 9], which=[1, 0, 0])
    fresh.network_begin([7, 8, 9], which=[1, 0, 0])
    refused(pkg, EINVAL, hb.network_begin, 1, which=[1, 0, 0])     # views that are not empty
    refused(pkg, EINVAL, hb.network_run, [1, 1, 0])                # network 1 was never begun
    refused(pkg, EINVAL, hb.network_turns, [([0, 1], [1, 1]), None, None])    # puller == peer
    refused(pkg, EINVAL, hb.network_turns, [([0, 4], [1, 0]), None, None])    # a node outside 0..n-1
    refused(pkg, EINVAL, hb.network_turns, [([0, 1], [1, -1]), None, None])
    refused(pkg, ERANGE, hb.network_run, [T + 1, 0, 0])            # n + turns > cap_events
    small = pkg.HashgraphBatch(n, n, cap_events=64, cap_rounds=20)
    small.network_begin(1)
    refused(pkg, ERANGE, small.network_run, 14)                    # n + 14 + 3 > cap_rounds
    assert small.network_run(13) == 0
    small.close()
    parts = [None] * (3 * n)
    parts[1] = (np.array([0], np.int32), np.array([-1], np.int32), np.array([-1], np.int32))
    refused(pkg, EINVAL, hb.append, parts)                         # append on a view
    K = np.zeros(3 * n, np.int64)
    K[2] = n
    refused(pkg, EINVAL, hb.synth, K)                              # synth on a view
    assert hb.step(collect=False) == 0 and hb.network_status(0).turns == 0   # nothing undivided in the views
    # after all of it: an admissible call gives what a fresh batch gives
    assert hb.network_run([T, 0, 0]) == 0 and fresh.network_run([T, 0, 0]) == 0
    assert_networks_equal(hb, 0, fresh, 0, n)
    assert_network(hb, 0, model(n, 7, T))
    # the hashgraphs of the other networks behave as before: generated and stepped
    hb.synth(np.where(np.arange(3 * n) == n, 20, 0))
    assert hb.step(collect=False) == 0
    s = hb.summary(n)
    assert (s.events, s.divided, s.stage) == (20, 20, 0)
    st = hb.network_status()
    assert (st[1].begun, st[1].view, st[2].begun) == (0, -1, 0) and (hb.network_heads()[n:] == -1).all()
    refused(pkg, EINVAL, hb.event_numbers, n)
    hb.close(), fresh.close()


# ---- 6. more workgroups than the machine holds -------------------------------------------------------------------------------
def test_2048_networks_in_one_launch(pkg):
    n, G, T = 4, 2048, 40
    seeds = (np.arange(G) % 16 + 50).astype(np.uint64)
    hb = pkg.HashgraphBatch(G * n, n, cap_events=n + T)
    hb.network_begin(seeds)
    before = hb.network_stats().launches
    assert hb.network_run(T) == 0
    assert hb.network_stats().launches == before + 1
    rep = pkg.HashgraphBatch(16 * n, n, cap_events=n + T)
    for g in range(16):   # every seed's representative runs alone
        rep.network_begin(seeds[:16], which=np.arange(16) == g)
        rep.network_run(np.where(np.arange(16) == g, T, 0))
    for g in range(16):
        assert_network(rep, g, model(n, int(seeds[g]), T))
    ev, rn, od, nm = hb.export_events(), hb.export_rounds(), hb.export_ordered(), hb.export_event_numbers()
    rev, rrn, rod, rnm = rep.export_events(), rep.export_rounds(), rep.export_ordered(), rep.export_event_numbers()
    for x, r in ((ev, rev), (rn, rrn), (od, rod), (nm, rnm)):
        size = np.diff(x["off"]).reshape(G // 16, 16 * n)
        assert (size == np.diff(r["off"])).all()
        for k in x:
            if k != "off":
                per = len(r[k])
                assert same(x[k].reshape((G // 16, per) + x[k].shape[1:]), np.broadcast_to(r[k], (G // 16,) + r[k].shape)), k
    assert same(hb.summary_array().reshape(G // 16, 16 * n, 9), np.broadcast_to(rep.summary_array(), (G // 16, 16 * n, 9)))
    hb.close(), rep.close()


# ---- 7. beyond 4 GiB ----------------------------------------------------------------------------------------------------------
def test_a_network_beyond_4_gib(pkg):
    """2048 hashgraphs of 4 members and 16384 events: the slabs take more than 4 GiB, the last network's puller and peer
    lie beyond 32-bit offsets from the base, and so do its columns of the network state."""
    B, n, E, T = 2048, 4, 16384, 50
    need = pkg.HashgraphBatch.bytes_needed(B, n, E, 64)
    assert need > 4 << 30
    hb = pkg.HashgraphBatch(B, n, cap_events=E, cap_rounds=64)
    G = B // n
    which = np.zeros(G, np.uint8)
    which[[0, G - 1]] = 1
    hb.network_begin(11, which=which)
    assert hb.network_run(np.where(which, T, 0)) == 0
    m = model(n, 11, T)
    assert_network(hb, 0, m)
    assert_network(hb, G - 1, m)
    assert_networks_equal(hb, 0, hb, G - 1, n)
    s = hb.summary_array()
    assert (s[n:B - n, :8] == 0).all(), "the other hashgraphs were not touched"
    hb.close()


# ---- 8. a call longer than a launch takes --------------------------------------------------------------------------------------
def test_a_long_call_is_split_into_launches(pkg):
    n, T = 2, 165   # 64 turns per launch: 3 launches (2 members decide no round, every turn re-votes them all: keep it short)
    hb = pkg.HashgraphBatch(2 * n, n, cap_events=n + T)
    hb.network_begin(4)
    l0 = hb.network_stats().launches
    assert hb.network_run([T, 0]) == 0
    assert hb.network_stats().launches == l0 + 3
    for k in range(T):
        hb.network_run([0, 1])
    assert hb.network_stats().launches == l0 + 3 + T
    assert_networks_equal(hb, 0, hb, 1, n)
    assert hb.network_status(0).turns == T and hb.summary(0).events + hb.summary(1).events > T
    hb.close()


# ---- 9. a network that stops, among healthy ones -------------------------------------------------------------------------------
def test_a_stopping_network_among_healthy_ones(pkg):
    from batch_cases import WHALE_N, whale_stake
    seed, (turn, who) = M.STOPPING_NETWORK   # found on the CPU (tests/test_batch_network_host.py asserts the search)
    n, G, W, T = WHALE_N, 4, 2, 300
    stake = np.ones((G * n, n), np.uint64)
    stake[W * n:(W + 1) * n] = whale_stake()
    hb = pkg.HashgraphBatch(G * n, n, stake, cap_events=n + T)
    hb.network_begin(seed)
    stopped = [hb.network_run(100) for _ in range(3)]
    assert sum(stopped) == 1 and stopped[turn // 100] == 1
    st = hb.network_status()
    assert (st[W].turns, st[W].created, st[W].stage, st[W].code, st[W].view) == (turn + 1, n + turn + 1, 3, -3, who)   # find_order, IndexError
    m = model(n, seed, turn + 1)
    for i in range(n):
        assert_view(hb, W * n + i, m.views[i])
        assert (hb.summary(W * n + i).stage != 0) == (i == who)
    healthy = model(n, seed, T)
    for g in (0, 1, 3):
        assert_network(hb, g, healthy)
    assert hb.network_run(0) == 0 and hb.network_turns([None, None, ([0], [1]), None]) == 0   # skipped, whatever the schedule says
    assert hb.network_status(W).turns == turn + 1
    hb.close()
