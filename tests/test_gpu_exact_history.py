"""GPU (-m gpu): what a context keeps after its first forked event when sw_set_exact_history is on (csrc/exact_history.hip.h;
Hashgraph.set_exact_history, votes_by_event, vote_entries) — round received, consensus time and the ordered stream against
the fixtures of tests/golden/consensus_forked (bit for bit, both timestamp variants), the votes keyed by event against the
reference's complete `votes` dict of the four forked goldens and against the CPU oracle; the hand-over from the fast path
in the middle of a stream, more than 64 members, a tiny store and a low ceiling, a fork that arrives behind an unseen
divide_rounds or behind sw_commit_fame, the switch off, and the call protocols.

No torch here (see tests/test_gpu_export.py): device buffers come through ctypes from the HIP runtime the library is linked
against."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from oracle.oracle import Oracle
from test_exact_history_host import FORKED, load_forked_consensus, same_bits
from test_exact_host import add_forks
from test_gpu_export import Hip
from test_oracle_vs_reference_random import load_case

pytestmark = pytest.mark.gpu

RANDOM_ORDERED = [2, 3, 4, 11, 13, 14]


@pytest.fixture
def hip(pkg):
    h = Hip(pkg)
    yield h
    h.free()


def entries_dict(h):
    y, x, v = h.vote_entries()
    d = {(int(a), int(b)): int(c) for a, b, c in zip(y, x, v)}
    assert len(d) == len(y), "a key twice in the store"
    assert set(v.tolist()) <= {0, 1}
    return d


def run_stream(h, n, stream, chunk, stop_call=None, oracle=None):
    """append / divide / decide_fame / find_order per chunk on `h` (and on `oracle`, compared call by call).  Returns the call
    at which the context was first seen on the exact path, and the events ordered on the fast path before that."""
    cr, sp, op, t, sig = stream
    N = len(cr)
    chunk = chunk or N
    flipped_at, ordered_fast = None, 0
    for i, a in enumerate(range(0, N, chunk)):
        if stop_call is not None and i >= stop_call:
            break
        b = min(N, a + chunk)
        for d in (h, oracle):
            if d is not None:
                d.append_events(cr[a:b], sp[a:b], op[a:b], t[a:b], sig[a:b])
                d.divide_rounds(a, b - a)
        if flipped_at is None and h.exact:
            flipped_at, ordered_fast = i, h.num_ordered
        nc = h.decide_fame()
        tx = h.find_order(nc)
        if oracle is not None:
            nco = oracle.decide_fame()
            assert list(nc) == list(nco)
            assert list(tx) == list(oracle.find_order(nco))
    return flipped_at, ordered_fast


def check_consensus(h, hip, N, tx, rr_fix, cts_fix, creator):
    rr, cts = h.round_received(), h.consensus_time()
    assert np.array_equal(rr, rr_fix[:N])
    assert same_bits(cts_fix[:N], cts)
    # a range in the middle of the stream
    lo, k = N // 3, N // 2
    assert np.array_equal(h.round_received(lo, k), rr_fix[lo:lo + k]) and same_bits(cts_fix[lo:lo + k], h.consensus_time(lo, k))
    K = len(tx)
    assert h.num_ordered == K and np.array_equal(h.transactions(), tx)
    o = h.export_ordered(ids=False)
    assert np.array_equal(o["event"], tx) and np.array_equal(o["creator"], creator[tx])
    assert np.array_equal(o["round_received"], rr_fix[tx]) and same_bits(cts_fix[tx], o["time"])
    if K:
        bufs = dict(event=hip.alloc(4 * K), creator=hip.alloc(4 * K), round_received=hip.alloc(4 * K), time=hip.alloc(8 * K))
        assert h.export_ordered_device(0, K, **bufs) == K
        h.synchronize()
        assert np.array_equal(hip.down(bufs["event"], K, np.int32), tx)
        assert np.array_equal(hip.down(bufs["round_received"], K, np.int32), rr_fix[tx])
        assert same_bits(cts_fix[tx], hip.down(bufs["time"], K, np.float64))
        part = h.export_ordered(K // 2, K - K // 2, ids=False)
        assert np.array_equal(part["event"], tx[K // 2:])


def check_lookups(h, ref, N, seed):
    keys = list(ref)
    y, x = np.array([k[0] for k in keys], np.int32), np.array([k[1] for k in keys], np.int32)
    assert np.array_equal(h.votes_by_event(y, x), np.array([ref[k] for k in keys], np.int8))
    rng = np.random.default_rng(seed)
    ay, ax = rng.integers(-2, N + 2, 500), rng.integers(-2, N + 2, 500)
    exp = np.array([ref.get((int(a), int(b)), -1) for a, b in zip(ay, ax)], np.int8)
    assert (exp == -1).sum() > 400
    assert np.array_equal(h.votes_by_event(ay, ax), exp)
    if keys:
        assert h.votes_by_event(*keys[0]) == ref[keys[0]]


# ---- 1. the forked goldens of the reference, their recorded schedules ---------------------------------------------------------
@pytest.mark.parametrize("variant", ["asis", "wallclock"])
@pytest.mark.parametrize("name", FORKED)
def test_forked_golden_with_history(pkg, hip, name, variant):
    g, f = load_golden(name), load_forked_consensus(name)
    t = g["t"] if variant == "asis" else f["wallclock_t"]
    tx_fix = g["transactions"] if variant == "asis" else f["wallclock_transactions"]
    h = pkg.Hashgraph(g["n"], g["stake"])
    h.set_exact_history()
    assert h.exact_history and h.votes_available
    stream = (g["creator"], g["self_parent"], g["other_parent"], t, g["sig"])
    flipped_at, ordered_fast = run_stream(h, g["n"], stream, g["chunk"])
    assert h.exact
    if "chunk" in name:   # the chunked ones cross from the fast path to the exact path in the middle of the stream ...
        assert flipped_at is not None and flipped_at > 0, "fast-path calls ran before the first fork"
        # ... but in all three the first fork arrives (calls 6, 31 and 2) before the fast path has ordered anything or cast a
        # vote: the hand-over of ordered events and of the votes table is test_crossing_with_ordered_events_and_votes' business
        assert ordered_fast == 0
    N = len(g["creator"])
    check_consensus(h, hip, N, tx_fix, f[variant + "_round_received"], f[variant + "_consensus_time"], g["creator"])
    assert h.votes_available
    ref = {(int(y), int(x)): int(v) for y, x, v in g["votes"]}
    got = entries_dict(h)
    assert got.keys() == ref.keys()
    assert got == ref
    assert np.array_equal(np.array(sorted(map(tuple, h.votes_triples().tolist()))), np.array(sorted((y, x, v) for (y, x), v in ref.items())))
    if name == "n5_s13_forks_chunk1":
        in_table = set(int(w) for w in h.witnesses().ravel() if w >= 0)
        assert any(y not in in_table for y, _ in got), "the case must hold a replaced-sibling voter"
    check_lookups(h, ref, N, 3)
    st = h.vote_store_stats()
    assert st["entries"] == len(ref) and st["capacity"] >= len(ref)
    # the (round, member) forms stay refused on a forked hashgraph
    for call in (lambda: h.vote(1, 0, 0, 0), lambda: h.export_votes()):
        with pytest.raises(pkg.SwirldHipError) as ei:
            call()
        assert ei.value.code == -95 and "exact" in str(ei.value)
    h.close()


@pytest.mark.parametrize("seed", RANDOM_ORDERED)
def test_random_forked_fixture_with_history(pkg, hip, seed):
    n, stream, stake, chunk, calls, index_error_call, ex = load_case("forked", seed)
    f = load_forked_consensus("random_forked_%02d" % seed)
    st = None if stake is None else stake.astype(np.uint64)
    h, o = pkg.Hashgraph(n, st), Oracle(n, st)
    h.set_exact_history()
    run_stream(h, n, stream, chunk, stop_call=index_error_call if index_error_call >= 0 else None, oracle=o)
    assert h.exact
    N = h.num_events
    check_consensus(h, hip, N, np.asarray(o.transactions, np.int32), f["asis_round_received"], f["asis_consensus_time"], stream[0])
    got = entries_dict(h)
    assert len(got) == o.num_votes
    assert all(o.vote(y, x) == v for (y, x), v in got.items())
    check_lookups(h, got, N, seed)
    if index_error_call >= 0:   # the call the reference dies in: an error, and nothing of it is recorded
        cr, sp, op, t, sig = stream
        a, b = index_error_call * chunk, min(len(cr), (index_error_call + 1) * chunk)
        h.append_events(cr[a:b], sp[a:b], op[a:b], t[a:b], sig[a:b])
        h.divide_rounds(a, b - a)
        nc = h.decide_fame()
        before = (h.round_received(0, N).tobytes(), h.consensus_time(0, N).tobytes(), h.num_ordered)
        with pytest.raises(pkg.SwirldHipError):
            h.find_order(nc)
        assert (h.round_received(0, N).tobytes(), h.consensus_time(0, N).tobytes(), h.num_ordered) == before
        assert (h.round_received(N) == -1).all()
    h.close()


@pytest.mark.parametrize("variant", ["asis", "wallclock"])
def test_crossing_with_ordered_events_and_votes(pkg, hip, variant):
    """The first fork arrives after fast-path find_order calls have ordered events and decide_fame calls have cast votes: the
    normalise step keeps what was recorded, the votes table is expanded into the store.  Round received, consensus time and
    the order bit for bit against what the unmodified reference computed for this stream and schedule
    (tests/golden/consensus_forked/crossing_n8_s12_chunk50.npz), the votes against the oracle."""
    from test_exact_history_host import crossing_stream
    n, chunk, (cr, sp, op, t, sig) = crossing_stream()
    f = load_forked_consensus("crossing_n8_s12_chunk50")
    if variant == "wallclock":
        t = f["wallclock_t"]
    stream = (cr, sp, op, t, sig)
    h, o = pkg.Hashgraph(n), Oracle(n)
    h.set_exact_history()
    flipped_at, ordered_fast = run_stream(h, n, stream, chunk, oracle=o)
    assert h.exact and flipped_at is not None and flipped_at * chunk >= 450
    assert 0 < ordered_fast < h.num_ordered, "the fast path ordered events, and so did the exact path"
    assert 0 < h.vote_store_stats()["imported"] < o.num_votes, "votes came from the table, and more were cast behind the fork"
    check_consensus(h, hip, len(cr), f[variant + "_transactions"], f[variant + "_round_received"], f[variant + "_consensus_time"], cr)
    got = entries_dict(h)
    assert len(got) == o.num_votes and all(o.vote(y, xx) == v for (y, xx), v in got.items())
    check_lookups(h, got, len(cr), 8)
    assert h.votes_available
    h.close()


# ---- 2. more than 64 members: the lanes of the one wavefront stride ------------------------------------------------------------
def wide_case(pkg):
    n = 70
    return n, add_forks(pkg.synth_hashgraph(n, 4000, 5), n, 5, 8), 1000


def test_wide_member_count_against_the_oracle(pkg):
    n, stream, chunk = wide_case(pkg)
    h, o = pkg.Hashgraph(n), Oracle(n)
    h.set_exact_history()
    run_stream(h, n, stream, chunk, oracle=o)
    assert h.exact
    assert o.consensus().sum() >= 1 and o.counters()["max_vote_distance"] >= 2
    got = entries_dict(h)
    assert len(got) == o.num_votes > 0
    assert all(o.vote(y, x) == v for (y, x), v in got.items())
    rnd = o.round
    assert any(rnd[y] - rnd[x] >= 2 for y, x in got), "a vote at distance >= 2"
    rr = h.round_received()
    ordered = np.zeros(len(rr), bool)
    ordered[o.transactions] = True
    assert np.array_equal(rr >= 0, ordered) and np.array_equal(~np.isnan(h.consensus_time()), ordered)
    h.close()


# ---- 3. a tiny store grows; a low ceiling loses the votes and nothing else ------------------------------------------------------
def consensus_snapshot(h):
    return (h.rounds().tobytes(), h.witnesses().tobytes(), h.famous().tobytes(), h.famous_events().tobytes(), h.consensus().tobytes(),
            h.transactions().tobytes(), h.round_received().tobytes(), h.consensus_time().tobytes())


def test_tiny_store_and_low_ceiling(pkg, monkeypatch):
    g = load_golden("n8_s12_forks_chunk9")
    stream = (g["creator"], g["self_parent"], g["other_parent"], g["t"], g["sig"])

    def run(**env):
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        h = pkg.Hashgraph(g["n"], g["stake"])
        for k in env:
            monkeypatch.delenv(k)
        h.set_exact_history()
        run_stream(h, g["n"], stream, g["chunk"])
        return h

    base = run()
    want, snap = base.vote_entries(), consensus_snapshot(base)
    tiny = run(SW_VOTE_STORE_INIT=4)
    assert consensus_snapshot(tiny) == snap
    assert tiny.vote_store_stats()["grows"] >= 5 > base.vote_store_stats()["grows"]
    for a, b in zip(want, tiny.vote_entries()):
        assert np.array_equal(a, b)
    low = run(SW_VOTE_STORE_INIT=4, SW_VOTE_STORE_MAX=50)
    assert consensus_snapshot(low) == snap
    assert low.exact_history and not low.votes_available
    for call in (lambda: low.vote_entries(), lambda: low.votes_by_event(5, 1)):
        with pytest.raises(pkg.SwirldHipError) as ei:
            call()
        assert ei.value.code == -95 and "unavailable" in str(ei.value)
    assert low.vote_store_stats()["entries"] <= 50
    assert np.array_equal(low.round_received(), base.round_received())   # only the two vote calls are refused
    assert len(low.export_ordered(ids=False)["event"]) == base.num_ordered
    # a rewind empties the store, and reads the knobs again: the re-run under the normal ceiling holds every vote of its schedule
    low.rewind()
    assert low.votes_available and len(low.vote_entries()[0]) == 0 and (low.round_received() == -1).all() and low.num_ordered == 0
    low.divide_rounds(0, low.num_events)
    low.find_order(low.decide_fame())
    o = Oracle(g["n"], g["stake"])
    o.append_events(*stream)
    o.divide_rounds(0, len(stream[0]))
    o.find_order(o.decide_fame())
    assert np.array_equal(low.transactions(), o.transactions)
    got = entries_dict(low)
    assert len(got) == o.num_votes > 50 and all(o.vote(y, x) == v for (y, x), v in got.items())
    for h in (base, tiny, low):
        h.close()


# ---- 4. a fork that arrives when the fast path's votes are not current ----------------------------------------------------------
def test_late_fork_votes_equal_the_oracle_or_are_refused(pkg):
    n = 8
    base = pkg.synth_hashgraph(n, 700, 9)
    cut = 400
    stream = add_forks(base, n, 9, 5, start=cut + 40)
    cr, sp, op, t, sig = stream
    first_fork = next(i for i in range(len(cr)) if sp[i] >= 0 and any(cr[j] == cr[i] and sp[j] == sp[i] for j in range(i)))
    assert first_fork > cut + 40
    h, o = pkg.Hashgraph(n), Oracle(n)
    h.set_exact_history()
    mid = first_fork - 10
    for d in (h, o):
        d.append_events(cr[:cut], sp[:cut], op[:cut], t[:cut], sig[:cut])
        d.divide_rounds(0, cut)
        d.find_order(d.decide_fame())
        # rounds divided that decide_fame does not see before the fork arrives
        d.append_events(cr[cut:mid], sp[cut:mid], op[cut:mid], t[cut:mid], sig[cut:mid])
        d.divide_rounds(cut, mid - cut)
        d.append_events(cr[mid:], sp[mid:], op[mid:], t[mid:], sig[mid:])
        d.divide_rounds(mid, len(cr) - mid)
    assert h.exact
    assert list(h.decide_fame()) == list((nc := o.decide_fame()))
    assert list(h.find_order(nc)) == list(o.find_order(nc))
    if h.votes_available:
        got = entries_dict(h)
        assert len(got) == o.num_votes and all(o.vote(y, x) == v for (y, x), v in got.items())
    else:
        with pytest.raises(pkg.SwirldHipError) as ei:
            h.vote_entries()
        assert ei.value.code == -95 and "unavailable" in str(ei.value)
    ordered = np.zeros(len(cr), bool)
    ordered[o.transactions] = True
    assert np.array_equal(h.round_received() >= 0, ordered)
    h.close()


def test_fork_after_commit_fame_reports_votes_unavailable(pkg):
    n = 8
    cut = 400
    stream = add_forks(pkg.synth_hashgraph(n, 700, 9), n, 9, 5, start=cut + 40)
    cr, sp, op, t, sig = stream
    h, o = pkg.Hashgraph(n), Oracle(n)
    h.set_exact_history()
    for d in (h, o):
        d.append_events(cr[:cut], sp[:cut], op[:cut], t[:cut], sig[:cut])
        d.divide_rounds(0, cut)
    fam, dec = h.decide_fame_partial(0, 1)
    nc = h.commit_fame(fam, dec)
    assert list(nc) == list(o.decide_fame())
    assert list(h.find_order(nc)) == list(o.find_order(nc))
    rr0 = h.round_received()
    for d in (h, o):
        d.append_events(cr[cut:], sp[cut:], op[cut:], t[cut:], sig[cut:])
        d.divide_rounds(cut, len(cr) - cut)
    assert h.exact and h.exact_history and not h.votes_available
    nc = o.decide_fame()
    assert list(h.decide_fame()) == list(nc)
    assert list(h.find_order(nc)) == list(o.find_order(nc))
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.vote_entries()
    assert ei.value.code == -95 and "unavailable" in str(ei.value)
    rr = h.round_received()
    keep = rr0 >= 0
    assert keep.any() and np.array_equal(rr[:cut][keep], rr0[keep])   # what the fast path recorded stays
    ordered = np.zeros(len(cr), bool)
    ordered[o.transactions] = True
    assert np.array_equal(rr >= 0, ordered)
    h.close()


# ---- 5. the switch off: every answer and every launch as without it -------------------------------------------------------------
def test_switch_off_is_the_parent_behaviour(pkg):
    g = load_golden("n8_s11_forks")
    stream = (g["creator"], g["self_parent"], g["other_parent"], g["t"], g["sig"])
    plain, off = pkg.Hashgraph(g["n"], g["stake"]), pkg.Hashgraph(g["n"], g["stake"])
    off.set_exact_history(False)
    for h in (plain, off):
        run_stream(h, g["n"], stream, g["chunk"])
        assert h.exact and not h.exact_history and not h.votes_available
    assert off.counters()["kernel_launches"] == plain.counters()["kernel_launches"]
    assert np.array_equal(off.transactions(), g["transactions"])
    for call in (lambda: off.vote_entries(), lambda: off.votes_by_event(5, 1), lambda: off.vote_store_stats(),
                 lambda: off.vote_entries_device(0, 0), lambda: off.round_received(), lambda: off.consensus_time(),
                 lambda: off.export_ordered(ids=False), lambda: off.votes_triples()):
        with pytest.raises(pkg.SwirldHipError) as ei:
            call()
        assert ei.value.code == -95
    for h in (plain, off):
        h.close()


# ---- 6. protocols ---------------------------------------------------------------------------------------------------------------
def test_switch_only_before_the_first_event_and_kept_by_reset(pkg):
    g = load_golden("n8_s11_forks")
    h = pkg.Hashgraph(g["n"], g["stake"])
    h.append_events(g["creator"][:8], g["self_parent"][:8], g["other_parent"][:8], g["t"][:8], g["sig"][:8])
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.set_exact_history()
    assert ei.value.code == -22 and not h.exact_history
    h.reset()
    h.set_exact_history()
    h.reset()
    assert h.exact_history
    run_stream(h, g["n"], (g["creator"], g["self_parent"], g["other_parent"], g["t"], g["sig"]), 0)
    assert h.exact and len(entries_dict(h)) == len(g["votes"])
    h.reset()
    assert h.exact_history and not h.exact
    h.close()


def test_capacity_device_form_streams_and_read_only(pkg, hip):
    name = "n12_s14_forks_stake_chunk40"
    g, f = load_golden(name), load_forked_consensus(name)
    h = pkg.Hashgraph(g["n"], g["stake"])
    h.set_exact_history()
    run_stream(h, g["n"], (g["creator"], g["self_parent"], g["other_parent"], g["t"], g["sig"]), g["chunk"])
    L, ctx = h._L, h._h
    K = len(g["votes"])
    y, x, v = h.vote_entries()

    def snapshot():
        c = h.counters()
        c.pop("kernel_launches")
        st = h.vote_store_stats()
        return consensus_snapshot(h) + (c, h.num_events, h.max_round, h.num_ordered, st["entries"], st["capacity"], st["grows"], h.votes_available)

    before = snapshot()
    # size query; too small a capacity writes nothing
    n_total = C.c_int64(-1)
    assert L.sw_export_vote_entries(ctx, 0, 0, None, None, None, C.byref(n_total)) == -34 and n_total.value == K
    small = [np.full(K, 77, np.int32), np.full(K, 77, np.int32), np.full(K, 77, np.int8)]
    assert L.sw_export_vote_entries(ctx, 0, K - 1, *[a.ctypes.data_as(C.c_void_p) for a in small], C.byref(n_total)) == -34
    assert n_total.value == K and all((a == 77).all() for a in small)
    assert L.sw_export_vote_entries(ctx, K, 0, None, None, None, C.byref(n_total)) == 0      # nothing behind the end
    ty, tx_, tv = h.vote_entries(K - 7)
    assert np.array_equal(ty, y[K - 7:]) and np.array_equal(tx_, x[K - 7:]) and np.array_equal(tv, v[K - 7:])
    # the device form: size query, SW_ERANGE, a host pointer, a caller's stream
    assert h.vote_entries_device(0, 0) == K
    d = [hip.alloc(4 * K), hip.alloc(4 * K), hip.alloc(K)]
    for p, nb in zip(d, (4 * K, 4 * K, K)):
        hip.fill(p, 0x4d, nb)
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.vote_entries_device(0, K - 1, *d)
    assert ei.value.code == -34
    assert (hip.down(d[0], K, np.int32) == 0x4d4d4d4d).all() and (hip.down(d[2], K, np.int8) == 0x4d).all()
    launches = h.counters()["kernel_launches"]
    host = np.zeros(K, np.int32)
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.vote_entries_device(0, K, host.ctypes.data, d[1], d[2])
    assert ei.value.code == -22 and h.counters()["kernel_launches"] == launches
    stream = C.c_void_p()
    assert hip.L.hipStreamCreate(C.byref(stream)) == 0
    try:
        assert h.vote_entries_device(0, K, *d, stream=stream.value) == K
        assert hip.L.hipStreamSynchronize(stream) == 0      # the caller's stream waits for the arrays
        assert np.array_equal(hip.down(d[0], K, np.int32), y) and np.array_equal(hip.down(d[1], K, np.int32), x)
        assert np.array_equal(hip.down(d[2], K, np.int8), v)
    finally:
        hip.L.hipStreamDestroy(stream)
    for _ in range(2):
        h.votes_by_event(y[:50], x[:50])
        h.round_received(), h.consensus_time(), h.export_ordered(ids=False)
    assert snapshot() == before
    h.close()


def test_fork_free_context_answers_the_same_entries_from_the_table(pkg):
    """A caller need not know which path it is on: the entries of a fork-free context are those of its votes table."""
    g = load_golden("n7_s2_chunk13")
    h = pkg.Hashgraph(g["n"], g["stake"])
    h.set_exact_history()
    run_stream(h, g["n"], (g["creator"], g["self_parent"], g["other_parent"], g["t"], g["sig"]), g["chunk"])
    assert not h.exact and h.votes_available
    ref = {(int(y), int(x)): int(v) for y, x, v in g["votes"]}
    assert entries_dict(h) == ref
    check_lookups(h, ref, len(g["creator"]), 1)
    assert {(int(y), int(x)): int(v) for y, x, v in h.votes_triples().tolist()} == ref
    h.close()


def test_fork_free_table_over_the_ceiling_is_refused_on_every_read(pkg, monkeypatch):
    """A fork-free context whose votes table holds more entries than SW_VOTE_STORE_MAX: every read is refused as
    unavailable — the first, which fills the store, and the later ones, which find the fill current — never answered
    with an empty store; the consensus getters are unaffected, and the next decide_fame is a new fill."""
    g = load_golden("n7_s2_chunk13")
    assert len(g["votes"]) > 40
    monkeypatch.setenv("SW_VOTE_STORE_MAX", "40")
    h = pkg.Hashgraph(g["n"], g["stake"])
    monkeypatch.delenv("SW_VOTE_STORE_MAX")
    h.set_exact_history()
    stream = (g["creator"], g["self_parent"], g["other_parent"], g["t"], g["sig"])
    cut = len(g["batches"]) // 2
    N_half = g["batches"][cut - 1][1]
    run_stream(h, g["n"], tuple(a[:N_half] for a in stream), g["chunk"])
    assert not h.exact
    for _ in range(3):
        for call in (lambda: h.vote_entries(), lambda: h.votes_by_event(5, 1), lambda: h.votes_by_event([5, 6], [1, 2]),
                     lambda: h.vote_entries_device(0, 0)):
            with pytest.raises(pkg.SwirldHipError) as ei:
                call()
            assert ei.value.code == -95 and "unavailable" in str(ei.value)
        assert not h.votes_available
    assert (h.round_received() >= 0).sum() == h.num_ordered
    # the schedule moves on: filled anew, refused anew
    a, b = g["batches"][cut]
    h.append_events(*(x[a:b] for x in stream))
    h.divide_rounds(a, b - a)
    h.find_order(h.decide_fame())
    for _ in range(2):
        with pytest.raises(pkg.SwirldHipError) as ei:
            h.vote_entries()
        assert ei.value.code == -95 and "unavailable" in str(ei.value)
    h.close()
