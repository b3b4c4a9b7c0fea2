"""GPU (-m gpu): gossip histories generated on the device (sw_synth_batch*, csrc/batch_synth.hip.h) and the stored events
read back (sw_get_batch_events).  The reference of every comparison is the host route: synth_hashgraph per hashgraph
(csrc/synth.cpp), the heights computed from its parents (swirld.py:117-120), and batches filled by append().  Comparisons
are equalities of arrays; timestamps are compared as bytes.  The generator on the CPU, under the sanitizers:
tests/test_batch_synth_host.py."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# mode, p0, p1: one parameter set per gossip mode
MODES = [(0, 0.0, 0.0), (1, 0.1, 0.0), (2, 0.4, 0.02), (3, 0.3, 0.0)]
EINVAL, ERANGE = -22, -34


@functools.lru_cache(maxsize=None)
def _host(n, N, seed, mode, p0, p1):
    import importlib
    pkg = importlib.import_module("py-swirld_amd")
    cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, seed, mode, p0, p1)
    ht = np.zeros(N, np.int32)
    for i in range(n, N):
        ht[i] = max(ht[sp[i]], ht[op[i]]) + 1
    for a in (cr, sp, op, t, sig, ht):
        a.setflags(write=False)
    return cr, sp, op, t, sig, ht


def host(n, N, seed, mode=0, p0=0.0, p1=0.0):
    """(creator, self_parent, other_parent, t, sig, height) of the host function; computed once, shared, read-only."""
    return _host(int(n), int(N), int(seed), int(mode), float(p0), float(p1))


def params(B, seed0=1000):
    m = np.array([MODES[b % 4] for b in range(B)])
    return np.arange(seed0, seed0 + B, dtype=np.uint64), m[:, 0].astype(np.int32), m[:, 1].copy(), m[:, 2].copy()


def assert_events(hb, b, want, N=None):
    N = len(want[0]) if N is None else N
    got = hb.events(b, 0, N)
    for k, name in enumerate(("creator", "self_parent", "other_parent")):
        assert np.array_equal(got[k], want[k][:N]), (b, name)
    assert np.array_equal(got[3].view(np.uint64), want[3][:N].view(np.uint64)), (b, "t")
    assert np.array_equal(got[4], want[4][:N]), (b, "sig")


def assert_exports_equal(x, y):
    for fn in ("export_events", "export_rounds", "export_ordered"):
        dx, dy = getattr(x, fn)(), getattr(y, fn)()
        assert dx.keys() == dy.keys()
        for k in dx:
            a, b = dx[k], dy[k]
            if a.dtype == np.float64:
                a, b = a.view(np.uint64), b.view(np.uint64)
            assert np.array_equal(a, b), (fn, k)


# ---- 1. events, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 16, 64])
def test_events_equal_the_host_function(pkg, n):
    B = 37
    seed, mode, p0, p1 = params(B)
    K = np.random.default_rng(n).choice([0, n, n + 1, 130], size=B).astype(np.int64)
    K[:4] = [0, n, n + 1, 130]
    hb = pkg.HashgraphBatch(B, n, cap_events=130)
    hb.synth_begin(seed, mode, p0, p1)
    assert hb.synth(K) == K.sum()
    summ = hb.summary_array()
    assert np.array_equal(summ[:, 0], K)
    for b in range(B):
        if K[b] == 0:
            assert len(hb.events(b)[0]) == 0
            continue
        want = host(n, K[b], seed[b], mode[b], p0[b], p1[b])
        assert_events(hb, b, want)
        assert np.array_equal(hb.heights(b, 0, int(K[b])), want[5]), b
    st = hb.synth_stats()
    assert (st.calls, st.events, st.launches, st.mirror_refreshes) == (1, K.sum(), 2, 0)
    hb.close()


# ---- 2. downstream ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 4])
def test_step_and_exports_equal_a_batch_filled_by_append(pkg, n):
    """16 members x 300 events reach 3 rounds and order nothing yet; 4 members x 300 events decide rounds and order events."""
    B, N = 8, 300
    seed, mode, p0, p1 = params(B, 77)
    gen = pkg.HashgraphBatch(B, n, cap_events=N)
    gen.synth_begin(seed, mode, p0, p1)
    assert gen.synth(N) == B * N
    fed = pkg.HashgraphBatch(B, n, cap_events=N)
    fed.append([host(n, N, seed[b], mode[b], p0[b], p1[b])[:5] for b in range(B)])
    assert gen.step(collect=False) == 0 and fed.step(collect=False) == 0
    s = gen.summary_array()
    assert np.array_equal(s, fed.summary_array())
    assert np.array_equal(s[:, 0], np.full(B, N)) and np.array_equal(s[:, 1], s[:, 0]) and s[:, 2].min() >= 2
    if n == 4:
        assert s[:, 3].sum() > 0   # rounds are decided and events ordered
    assert_exports_equal(gen, fed)
    gen.close(), fed.close()


# ---- 3. instalments --------------------------------------------------------------------------------------------------
def test_instalments_equal_one_call(pkg):
    B, n = 5, 4
    sched = [n, 1, 7, 0, 64, 65]
    N = sum(sched)
    seed, mode, p0, p1 = params(B, 5)
    a = pkg.HashgraphBatch(B, n, cap_events=N)
    a.synth_begin(seed, mode, p0, p1)
    for k in sched:
        assert a.synth(k) == B * k
        a.step(collect=False)
    one = pkg.HashgraphBatch(B, n, cap_events=N)
    one.synth_begin(seed, mode, p0, p1)
    assert one.synth(N) == B * N
    for k in sched:
        if k:   # (the same schedule of steps: it is part of the reference's semantics)
            one.step(np.full(B, k, np.int64), collect=False)
    for b in range(B):
        want = host(n, N, seed[b], mode[b], p0[b], p1[b])
        assert_events(a, b, want)
        assert_events(one, b, want)
        assert np.array_equal(a.heights(b, 0, N), want[5])
    assert a.summary_array()[:, 3].sum() > 0
    assert_exports_equal(a, one)
    assert a.synth_stats().calls == 5 and one.synth_stats().calls == 1
    a.close(), one.close()


def test_two_members_roots_then_one_event(pkg):
    hb = pkg.HashgraphBatch(3, 2, cap_events=3)
    hb.synth_begin([7, 8, 9])
    assert hb.synth(2) == 6
    for b in range(3):
        assert_events(hb, b, host(2, 2, 7 + b))
    assert hb.synth([1, 0, 1]) == 2
    for b, N in enumerate((3, 2, 3)):
        want = host(2, N, 7 + b)
        assert_events(hb, b, want)
        assert np.array_equal(hb.heights(b, 0, N), want[5])
    hb.close()


# ---- 4. atomicity ----------------------------------------------------------------------------------------------------
def snapshot(hb):
    s = hb.summary_array()
    return s, [hb.events(b, 0, int(s[b, 0])) for b in range(hb.B)]


def assert_unchanged(hb, snap):
    s, ev = snapshot(hb)
    assert np.array_equal(s, snap[0])
    for got, was in zip(ev, snap[1]):
        assert all(np.array_equal(x, y) for x, y in zip(got, was))


def test_beyond_cap_events_nothing_is_stored(pkg):
    B, n = 5, 4
    seed, mode, p0, p1 = params(B, 31)
    hb, twin = (pkg.HashgraphBatch(B, n, cap_events=50) for _ in range(2))
    for x in (hb, twin):
        x.synth_begin(seed, mode, p0, p1)
        assert x.synth(20) == 100
    snap = snapshot(hb)
    with pytest.raises(pkg.SwirldHipError) as ei:
        hb.synth([10, 10, 31, 10, 10])
    assert ei.value.code == ERANGE and "hashgraph 2" in str(ei.value) and "cap_events" in str(ei.value)
    assert_unchanged(hb, snap)
    K = [10, 10, 30, 10, 10]
    assert hb.synth(K) == 70 and twin.synth(K) == 70
    for b in range(B):
        want = host(n, 20 + K[b], seed[b], mode[b], p0[b], p1[b])
        assert_events(hb, b, want)
        assert_events(twin, b, want)
        assert np.array_equal(hb.heights(b, 0, 20 + K[b]), want[5])
    hb.close(), twin.close()


def test_beyond_cap_rounds_nothing_is_stored(pkg):
    B, n = 5, 2
    assert host(n, 42, 1)[5].max() == 40   # the premise: height 40 needs 43 rounds of capacity
    seed = np.array([5, 4, 3, 1, 2], np.uint64)
    hb = pkg.HashgraphBatch(B, n, cap_events=64, cap_rounds=16)
    hb.synth_begin(seed)
    snap = snapshot(hb)
    with pytest.raises(pkg.SwirldHipError) as ei:
        hb.synth([10, 10, 10, 42, 10])
    assert ei.value.code == ERANGE and "hashgraph 3" in str(ei.value) and "cap_rounds" in str(ei.value)
    assert_unchanged(hb, snap)
    assert np.array_equal(hb.summary_array()[:, 0], np.zeros(B, np.int64))
    assert hb.synth_stats().calls == 0 and hb.synth_stats().events == 0
    assert hb.synth(10) == 50
    for b in range(B):
        want = host(n, 10, seed[b])
        assert_events(hb, b, want)
        assert np.array_equal(hb.heights(b, 0, 10), want[5])
    hb.close()


def test_a_refused_instalment_does_not_advance_the_generators(pkg):
    """The refusal that is known only after the kernel has run, in the middle of a history."""
    B, n = 5, 2
    seed = np.array([5, 4, 3, 1, 2], np.uint64)
    hb = pkg.HashgraphBatch(B, n, cap_events=64, cap_rounds=16)
    hb.synth_begin(seed)
    assert hb.synth(6) == 30
    snap = snapshot(hb)
    with pytest.raises(pkg.SwirldHipError) as ei:
        hb.synth([3, 3, 3, 36, 3])
    assert ei.value.code == ERANGE
    assert_unchanged(hb, snap)
    assert hb.synth(4) == 20
    for b in range(B):
        assert_events(hb, b, host(n, 10, seed[b]))
    hb.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def refused(pkg, hb, call, word=None):
    before = hb.summary_array()
    with pytest.raises(pkg.SwirldHipError) as ei:
        call()
    assert ei.value.code == EINVAL, str(ei.value)
    assert word is None or word in str(ei.value), str(ei.value)
    assert np.array_equal(hb.summary_array(), before)


def test_refusals_change_nothing(pkg):
    B, n = 4, 4
    hb = pkg.HashgraphBatch(B, n, cap_events=40)
    refused(pkg, hb, lambda: hb.synth(n), "parameters")                      # synth before begin
    refused(pkg, hb, lambda: hb.synth_begin(1, mode=[0, 1, 4, 2]), "mode")   # mode 4
    hb.synth_begin([1, 2, 3, 4], which=[1, 1, 1, 0])
    refused(pkg, hb, lambda: hb.synth([n, n, n, n]), "hashgraph 3")          # ... and for the hashgraph begin left out
    refused(pkg, hb, lambda: hb.synth([n, n - 1, n, 0]), "roots")            # a first instalment short of the roots
    refused(pkg, hb, lambda: hb.synth([n, -1, n, 0]), "negative")
    assert hb.synth([n, 0, n + 2, 0]) == 2 * n + 2
    refused(pkg, hb, lambda: hb.synth_begin(9, which=[0, 0, 1, 0]), "already holds")   # begin on a hashgraph with events
    hb.synth_begin(22, which=[0, 1, 0, 0])                                   # still empty: the parameters are replaced
    w = host(n, n, 1)
    hb.append([None, None, None, tuple(a[:n] for a in w[:5])])               # a host-fed hashgraph ...
    refused(pkg, hb, lambda: hb.synth_begin(9, which=[0, 0, 0, 1]), "already holds")
    one = host(n, n + 1, 1)
    hb.append([tuple(a[n:n + 1] for a in one[:5]), None, None, None])        # ... and a generated one that takes an append
    refused(pkg, hb, lambda: hb.synth([1, 0, 0, 0]), "host append")
    # none of it has moved a generator
    assert hb.synth([0, 10, 5, 0]) == 15
    assert_events(hb, 0, one)
    assert_events(hb, 1, host(n, 10, 22))
    assert_events(hb, 2, host(n, n + 7, 3))
    hb.close()
    lone = pkg.HashgraphBatch(2, 1, cap_events=8)
    refused(pkg, lone, lambda: lone.synth_begin(1), "members")               # a 1-member batch
    lone.close()


# ---- 6. host append behind generated events ---------------------------------------------------------------------------
def test_append_behind_generated_events(pkg):
    B, n, N = 3, 4, 20
    hb = pkg.HashgraphBatch(B, n, cap_events=N + 2)
    hb.synth_begin([11, 12, 13])
    assert hb.synth(N) == B * N
    cr, sp, op, t, sig, ht = host(n, N, 12)
    last = [int(np.nonzero(cr == m)[0][-1]) for m in range(n)]
    assert hb.synth_stats().mirror_refreshes == 0
    ev = (np.array([0], np.int32), np.array([last[0]], np.int32), np.array([last[1]], np.int32))
    hb.append([None, ev, None])
    assert hb.synth_stats().mirror_refreshes == 1
    assert hb.summary(1).events == N + 1
    assert hb.heights(1, N, 1)[0] == max(ht[last[0]], ht[last[1]]) + 1
    got = hb.events(1, N, 1)
    assert (got[0][0], got[1][0], got[2][0]) == (0, last[0], last[1])
    # a self-parent by another member: refused here as on a host-fed batch
    bad = (np.array([0], np.int32), np.array([last[2]], np.int32), np.array([last[1]], np.int32))
    fed = pkg.HashgraphBatch(1, n, cap_events=N + 2)
    fed.append([(cr, sp, op)])
    for x, streams in ((hb, [None, bad, None]), (fed, [bad])):
        with pytest.raises(pkg.SwirldHipError) as ei:
            x.append(streams)
        assert ei.value.code == EINVAL and "self-parent is by another member" in str(ei.value)
    assert hb.synth_stats().mirror_refreshes == 1   # (hashgraph 1's mirror was current)
    assert [s.events for s in hb.summary()] == [N, N + 1, N]
    with pytest.raises(pkg.SwirldHipError) as ei:
        hb.synth([0, 1, 0])
    assert ei.value.code == EINVAL and "host append" in str(ei.value)
    assert hb.synth([1, 0, 2]) == 3                 # the others go on generating
    assert_events(hb, 2, host(n, N + 2, 13))
    hb.close(), fed.close()


# ---- 7. many ---------------------------------------------------------------------------------------------------------
def test_ten_thousand_hashgraphs_in_one_call(pkg):
    B, n, N = 10000, 4, 40
    seed, mode, p0, p1 = params(B, 1)
    hb = pkg.HashgraphBatch(B, n, cap_events=N, cap_rounds=N + 3)
    hb.synth_begin(seed, mode, p0, p1)
    assert hb.synth(N) == B * N
    e = hb.export_events()
    assert np.array_equal(e["off"], np.arange(B + 1) * N)
    for b in range(B):
        cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, int(seed[b]), int(mode[b]), p0[b], p1[b])
        got = hb.events(b, 0, N)
        assert np.array_equal(got[0], cr) and np.array_equal(got[1], sp) and np.array_equal(got[2], op), b
        assert np.array_equal(got[3].view(np.uint64), t.view(np.uint64)) and np.array_equal(got[4], sig), b
        ht, spl, opl = [0] * N, sp.tolist(), op.tolist()
        for i in range(n, N):
            ht[i] = max(ht[spl[i]], ht[opl[i]]) + 1
        assert np.array_equal(e["height"][b * N:(b + 1) * N], ht), b
    hb.close()


# ---- 8. sw_get_batch_events on a host-fed batch ------------------------------------------------------------------------
def test_get_events_returns_what_was_appended(pkg):
    n, N = 5, 60
    a, b = host(n, N, 3, 3, 0.3), host(n, 45, 4)
    hb = pkg.HashgraphBatch(2, n, cap_events=N)
    hb.append([a[:5], b[:5]])
    assert_events(hb, 0, a)
    assert_events(hb, 1, b)
    got = hb.events(0, 17, 9)
    assert np.array_equal(got[1], a[1][17:26]) and np.array_equal(got[4], a[4][17:26])
    assert np.array_equal(got[3].view(np.uint64), a[3][17:26].view(np.uint64))
    for args in ((1, 0, 46), (1, 40, 6), (0, -1, 2), (2, 0, 1), (-1, 0, 1)):
        with pytest.raises(pkg.SwirldHipError) as ei:
            hb.events(*args)
        assert ei.value.code == ERANGE
    assert len(hb.events(1, 45, 0)[0]) == 0
    hb.close()
