"""GPU (-m gpu): batches of small hashgraphs through the C-ABI (sw_batch_*, csrc/batch.hip.h) — B independent hashgraphs,
one wavefront each, one launch per step.  The reference's golden fixtures grouped by member count, each on its own
recorded schedule inside one batch; random forked hashgraphs against the oracle under per-hashgraph chunk sizes; a batch
against single contexts fed the same calls; more workgroups than the machine holds; a batch above 4 GiB; a hashgraph that
ends in the reference's IndexError among healthy ones; the refusals; and what destroy leaves behind.
The same step function on the CPU: tests/test_batch_host.py."""
import functools
import gc
import importlib

import numpy as np
import pytest

import batch_cases
from conftest import golden_names, load_golden
from test_batch_host import consensus_fixture, same_bits

pytestmark = pytest.mark.gpu


# ---- goldens, grouped by member count ------------------------------------------------------------------------------
def run_goldens(pkg, names):
    """One batch for the fixtures `names` (a name may occur several times): every fixture follows its own schedule, a
    finished one sits out.  Per call new_c and transactions, at the end the tables."""
    gs = [load_golden(nm) for nm in names]
    n = gs[0]["n"]
    assert all(g["n"] == n for g in gs)
    B = len(gs)
    hb = pkg.HashgraphBatch(B, n, np.stack([g["stake"] for g in gs]), cap_events=max(len(g["creator"]) for g in gs))
    calls = max(len(g["batches"]) for g in gs)
    for call in range(calls):
        streams, K = [None] * B, np.zeros(B, np.int64)
        for b, g in enumerate(gs):
            if call < len(g["batches"]):
                a, e = g["batches"][call]
                streams[b] = tuple(g[k][a:e] for k in ("creator", "self_parent", "other_parent", "t", "sig"))
                K[b] = e - a
        hb.append(streams)
        out = hb.step(K)
        assert hb.n_failed == 0
        for b, g in enumerate(gs):
            if call >= len(g["batches"]):
                assert out[b] is None, "a finished hashgraph sits out"
                continue
            nc, tx = out[b]
            assert list(nc) == list(g["new_c_flat"][g["new_c_off"][call]:g["new_c_off"][call + 1]]), (names[b], call)
            assert list(tx) == list(g["transactions"][g["tx_off"][call]:g["tx_off"][call + 1]]), (names[b], call)
    for b, (nm, g) in enumerate(zip(names, gs)):
        N = len(g["creator"])
        s = hb.summary(b)
        assert (s.events, s.divided, s.stage) == (N, N, 0), nm
        assert np.array_equal(hb.heights(b), g["height"]), nm
        assert np.array_equal(hb.rounds(b), g["round"]), nm
        assert np.array_equal(hb.can_see(b), g["can_see"]), nm
        wit = hb.witnesses(b)
        assert np.array_equal(wit, g["witnesses"]), nm
        for r, order in enumerate(g["wit_order"]):
            assert np.array_equal(hb.witness_order(b, r), order), "%s: dict order of witnesses[%d]" % (nm, r)
        fam = hb.famous(b)
        m = wit >= 0
        assert np.array_equal(fam[m], g["famous"][wit[m]]) and (fam[~m] == -1).all(), nm
        assert np.array_equal(hb.famous_events(b), g["famous"]), nm
        assert np.array_equal(hb.consensus(b), g["consensus"]), nm
        ev, rr, ts = hb.ordered(b)
        assert np.array_equal(ev, g["transactions"]), nm
        f = consensus_fixture(nm)
        if f is not None:
            assert np.array_equal(rr, f["asis_round_received"][ev]), nm
            assert same_bits(ts, f["asis_consensus_time"][ev]), nm
            assert len(ev) == int((f["asis_round_received"][:N] >= 0).sum())
    return hb


def group(prefix, forks=None):
    return [nm for nm in golden_names() if nm.startswith(prefix) and (forks is None or ("forks" in nm) == forks)]


@pytest.mark.parametrize("prefix,count,forks", [("n4_", 6, None), ("n8_", 2, True), ("n16_", 6, None)])
def test_goldens_grouped_by_member_count(pkg, prefix, count, forks):
    names = group(prefix, forks)
    assert len(names) == count and ("n4_mainloop_node0" in names) == (prefix == "n4_"), names
    run_goldens(pkg, names).close()


@pytest.mark.parametrize("name", [nm for nm in golden_names() if "stake" in nm])
def test_stake_goldens_three_copies_agree_bit_for_bit(pkg, name):
    assert len([nm for nm in golden_names() if "stake" in nm]) == 4
    hb = run_goldens(pkg, [name] * 3)
    ref = None
    for b in range(3):
        got = [hb.rounds(b), hb.can_see(b), hb.witnesses(b), hb.famous(b), hb.famous_events(b), hb.consensus(b)] + list(hb.ordered(b))
        got = [a.tobytes() for a in got] + [tuple(hb.summary(b))]
        if ref is None:
            ref = got
        assert got == ref, "copy %d" % b
    hb.close()


# ---- against the oracle --------------------------------------------------------------------------------------------
def assert_same(o, hb, b):
    """What assert_same of tests/test_gpu_forks.py compares, without the counters."""
    assert np.array_equal(hb.rounds(b), o.round)
    assert np.array_equal(hb.can_see(b), o.can_see)
    assert np.array_equal(hb.witnesses(b), o.witnesses())
    for r in range(o.max_round + 1):
        assert np.array_equal(hb.witness_order(b, r), o.witness_order(r)), "dict order of witnesses[%d]" % r
    assert np.array_equal(hb.famous(b), o.famous_table())
    assert np.array_equal(hb.consensus(b), o.consensus())
    assert np.array_equal(hb.transactions(b), o.transactions)


def run_schedules(hb, streams, scheds, records, frozen_ok=()):
    """Every hashgraph b follows scheds[b] over streams[b]; per call its (new_c, transactions) against records[b]."""
    B = len(streams)
    pos, call = [0] * B, [0] * B
    failed = []
    while any(call[b] < len(scheds[b]) for b in range(B)):
        parts, K = [None] * B, np.zeros(B, np.int64)
        for b in range(B):
            if call[b] < len(scheds[b]):
                k = scheds[b][call[b]]
                parts[b] = tuple(x[pos[b]:pos[b] + k] for x in streams[b])
                K[b] = k
        hb.append(parts)
        out = hb.step(K)
        failed.append(hb.n_failed)
        for b in range(B):
            if not K[b]:
                assert out[b] is None
                continue
            if b in frozen_ok and (records[b].failed_call is not None and call[b] >= records[b].failed_call):
                assert out[b] is None
            else:
                assert out[b] is not None, (b, call[b], hb.summary(b))
                assert (list(out[b][0]), list(out[b][1])) == records[b].calls[call[b]], "hashgraph %d, call %d" % (b, call[b])
            pos[b] += int(K[b])
            call[b] += 1
    return failed


CHUNKS = [1, 600, 5, 37, 9, 150, 13, 60, 299, 100, 23, 450]


@functools.lru_cache(maxsize=None)
def random_case(b):
    forks = 0 if b % 4 == 0 else 3 + b % 13
    stream = batch_cases.forked_stream(8, 600, 100 + b, forks)
    N = len(stream[0])
    chunk = CHUNKS[b % len(CHUNKS)]
    sched = [min(chunk, N - a) for a in range(0, N, chunk)]
    return stream, sched, batch_cases.Record(8, stream, sched)


def test_random_forked_hashgraphs_match_the_oracle(pkg):
    B = 48
    cases = [random_case(b) for b in range(B)]
    assert all(c[2].failed_call is None and c[2].o.max_round >= 3 for c in cases)
    assert sum(len(c[0][0]) == 600 for c in cases) == 12, "some hashgraphs have no fork"
    hb = pkg.HashgraphBatch(B, 8, cap_events=max(len(c[0][0]) for c in cases))
    failed = run_schedules(hb, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    assert not any(failed)
    for b in range(B):
        assert_same(cases[b][2].o, hb, b)
    hb.close()


def test_batch_against_single_contexts(pkg):
    """70 members: rows wider than a wave (a stride of 80 in the batch, 128 in a context)."""
    B, n, N0, chunk = 8, 70, 1500, 500
    streams = [batch_cases.forked_stream(n, N0, 40 + b, 6 if b % 2 else 0) for b in range(B)]
    hb = pkg.HashgraphBatch(B, n, cap_events=max(len(s[0]) for s in streams), cap_rounds=200)
    assert hb.npad == 80
    hs = [pkg.Hashgraph(n) for _ in range(B)]
    for h in hs:
        h.set_exact_history(True)
    for a in range(0, max(len(s[0]) for s in streams), chunk):
        parts = [tuple(x[a:a + chunk] for x in s) if a < len(s[0]) else None for s in streams]
        hb.append(parts)
        out = hb.step()
        for b, h in enumerate(hs):
            if parts[b] is None:
                assert out[b] is None
                continue
            h.append_events(*parts[b])
            h.divide_rounds(a, len(parts[b][0]))
            nc = h.decide_fame()
            tx = h.find_order(nc)
            assert list(out[b][0]) == list(nc) and list(out[b][1]) == list(tx), (b, a)
    for b, h in enumerate(hs):
        assert h.exact == bool(b % 2)
        R = h.max_round + 1
        s = hb.summary(b)
        assert (s.events, s.divided, s.rounds, s.ordered) == (h.num_events, h.num_events, R, h.num_ordered)
        assert np.array_equal(hb.heights(b), h.heights())
        assert np.array_equal(hb.rounds(b), h.rounds())
        assert np.array_equal(hb.can_see(b), h.can_see())
        assert np.array_equal(hb.witnesses(b), h.witnesses())
        for r in range(R):
            assert np.array_equal(hb.witness_order(b, r), h.witness_order(r))
        assert np.array_equal(hb.famous(b), h.famous())
        assert np.array_equal(hb.famous_events(b), h.famous_events())
        assert np.array_equal(hb.consensus(b), h.consensus())
        ev, rr, ts = hb.ordered(b)
        assert np.array_equal(ev, h.transactions())
        assert np.array_equal(rr, h.round_received()[ev]) and same_bits(ts, h.consensus_time()[ev])
        k = min(7, len(ev))   # (a slice of the log, and one of the rounds)
        assert np.array_equal(hb.ordered(b, len(ev) - k, k)[0], ev[len(ev) - k:]) and np.array_equal(hb.rounds(b, 3, 4), h.rounds()[3:7])
        h.close()
    hb.close()


@functools.lru_cache(maxsize=None)
def tiny_case(seed):
    stream = batch_cases.synth(4, 40, seed)
    return stream, batch_cases.Record(4, stream, [40])


def test_more_workgroups_than_the_machine_holds(pkg):
    """10 000 workgroups of one wave against 8192 wave slots: the grid runs in turns, nobody waits for anybody."""
    B, seeds = 10000, 200
    hb = pkg.HashgraphBatch(B, 4, cap_events=40)
    cases = [tiny_case(s) for s in range(seeds)]
    assert all(c[1].failed_call is None for c in cases) and any(len(c[1].calls[0][0]) for c in cases)
    off = np.arange(B + 1, dtype=np.int64) * 40
    cat = [np.concatenate([cases[b % seeds][0][i] for b in range(B)]) for i in range(5)]
    hb.append(off=off, creator=cat[0], self_parent=cat[1], other_parent=cat[2], t=cat[3], sig=cat[4])
    assert hb.step(collect=False) == 0
    summ = hb.summary_array()
    for b in range(B):
        rec = cases[b % seeds][1]
        nc, tx = rec.calls[0]
        assert summ[b].tolist() == [40, 40, rec.o.max_round + 1, len(tx), len(nc), len(tx), 0, 0, 0], b
        assert np.array_equal(hb.rounds(b, 0, 40), rec.o.round), b
        assert np.array_equal(hb.transactions(b, 0, len(tx)), tx), b
    for b in (0, 1, 4999, 8191, 8192, 9999):
        assert_same(cases[b % seeds][1].o, hb, b)
        assert list(hb.new_rounds(b)) == cases[b % seeds][1].calls[0][0]
    hb.close()


def test_a_batch_above_4_gib(pkg):
    """2048 hashgraphs of 8192 events at a row stride of 64: the can_see rows alone take 4 GiB, so the slab of hashgraph
    2047 lies beyond 32-bit offsets.  64 members of which four hold the stake, so that 64 events make rounds."""
    B, n, E = 2048, 64, 8192
    stake = np.zeros(n, np.uint64)
    stake[:4] = 1
    stream = batch_cases.synth(4, 64, 7)
    rec = batch_cases.Record(n, stream, [64], stake)
    assert rec.failed_call is None and rec.o.max_round >= 3
    need = pkg.HashgraphBatch.bytes_needed(B, n, E, 64)
    assert need > 4 << 30
    hb = pkg.HashgraphBatch(B, n, stake, cap_events=E, cap_rounds=64)
    assert hb.npad == 64 and hb.device_bytes == need
    parts = [None] * B
    parts[0] = parts[B - 1] = stream
    hb.append(parts)
    out = hb.step()
    assert [b for b in range(B) if out[b] is not None] == [0, B - 1]
    for b in (0, B - 1):
        assert (list(out[b][0]), list(out[b][1])) == rec.calls[0]
        assert_same(rec.o, hb, b)
    a, z = ([x.tobytes() for x in (hb.rounds(b), hb.can_see(b), hb.witnesses(b), hb.famous(b)) + hb.ordered(b)] for b in (0, B - 1))
    assert a == z
    s = hb.summary_array()
    assert (s[1:B - 1, :8] == 0).all(), "the empty hashgraphs sat out"
    hb.close()


# ---- a frozen hashgraph ----------------------------------------------------------------------------------------------
def test_frozen_hashgraph_among_healthy_ones(pkg):
    B, n, ch, W = 8, batch_cases.WHALE_N, batch_cases.WHALE_CHUNK, 3
    stake = np.ones((B, n), np.uint64)
    stake[W] = batch_cases.whale_stake()
    streams = [batch_cases.whale_stream() if b == W else batch_cases.forked_stream(n, 300, 70 + b, b % 3 * 4) for b in range(B)]
    scheds = [[min(ch, len(s[0]) - a) for a in range(0, len(s[0]), ch)] for s in streams]
    records = [batch_cases.Record(n, s, sc, stake[b]) for b, (s, sc) in enumerate(zip(streams, scheds))]
    at = batch_cases.WHALE_FAILS_AT
    assert records[W].failed_call == at and all(r.failed_call is None for b, r in enumerate(records) if b != W)
    hb = pkg.HashgraphBatch(B, n, stake, cap_events=max(len(s[0]) for s in streams))
    failed = run_schedules(hb, streams, scheds, records, frozen_ok=(W,))
    assert failed[at] == 1 and sum(failed) == 1, failed
    s = hb.summary(W)
    o = records[W].o
    assert (s.stage, s.code) == (3, -3) and 0 <= s.event < (at + 1) * ch
    assert importlib.import_module("py-swirld_amd.engine").BATCH_STAGES[s.stage] == "order"
    # what its earlier calls left is readable; later steps skipped it (events were appended, none was divided)
    assert s.events == len(streams[W][0]) and s.divided == (at + 1) * ch == o.N
    assert np.array_equal(hb.transactions(W), o.transactions), "the log holds what the reference had ordered when it raised"
    assert np.array_equal(hb.rounds(W, 0, s.divided), o.round)
    assert np.array_equal(hb.witnesses(W), o.witnesses())
    assert np.array_equal(hb.rounds(W, s.divided, 10), np.full(10, -1, np.int32))
    K = np.zeros(B, np.int64)
    K[W] = 5
    assert hb.step(K, collect=False) == 0 and hb.summary(W) == s, "a K for a frozen hashgraph is ignored"
    for b in range(B):
        if b != W:
            assert_same(records[b].o, hb, b)
    hb.close()


def test_a_call_that_raises_in_a_later_round_has_logged_the_rounds_before_it(pkg):
    """The reference appends a round's events before it turns to the next round of new_c: a frozen hashgraph's log equals
    the oracle's transactions at the exception, beside a healthy hashgraph fed the same stream with unit stake."""
    n, ch = batch_cases.WHALE_N, batch_cases.LATE_WHALE_CHUNK
    stream = batch_cases.late_whale_stream()
    stake = np.stack([batch_cases.late_whale_stake(), np.ones(n, np.uint64)])
    recs = [batch_cases.Record(n, stream, [ch, ch], stake[b]) for b in range(2)]
    assert recs[0].failed_call == batch_cases.LATE_WHALE_FAILS_AT and recs[1].failed_call is None
    hb = pkg.HashgraphBatch(2, n, stake, cap_events=len(stream[0]))
    failed = run_schedules(hb, [stream, stream], [[ch, ch]] * 2, recs, frozen_ok=(0,))
    assert failed == [0, 1]
    s = hb.summary(0)
    assert (s.stage, s.code, s.n_ordered) == (3, -3, batch_cases.LATE_WHALE_ORDERED_BY_THE_FAILING_CALL)
    assert s.ordered == len(recs[0].o.transactions) and np.array_equal(hb.transactions(0), recs[0].o.transactions)
    assert np.array_equal(hb.consensus(0), recs[0].o.consensus()) and np.array_equal(hb.famous_events(0), recs[0].o.famous_by_event)
    assert_same(recs[1].o, hb, 1)
    hb.close()


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    B, n = 8, 4
    stream = batch_cases.synth(n, 60, 3)
    hb = pkg.HashgraphBatch(B, n, cap_events=60, cap_rounds=48)
    first = [tuple(x[:30] for x in stream)] * B
    hb.append(first)
    hb.step()
    before = hb.summary_array()
    state = [(hb.rounds(b).tobytes(), hb.transactions(b).tobytes()) for b in range(B)]
    # one invalid event in hashgraph 5: its event 33 names a self-parent by another member
    parts = [tuple(np.array(x[30:40]) for x in stream) for _ in range(B)]
    cr, sp = parts[5][0], parts[5][1]
    other = next(e for e in range(30) if stream[0][e] != cr[3])
    sp[3] = other
    with pytest.raises(pkg.SwirldHipError) as ei:
        hb.append(parts)
    assert ei.value.code == -22 and "hashgraph 5" in str(ei.value) and "event 33" in str(ei.value)
    assert np.array_equal(hb.summary_array(), before), "nothing stored anywhere"
    for bad, word in (((n, -1, -1), "creator"), ((0, 2, -1), "0 or 2 parents"), ((0, 45, 1), "not earlier")):
        p2 = [None] * B
        p2[2] = tuple(np.array([v], np.int32) for v in bad)
        with pytest.raises(pkg.SwirldHipError) as ei:
            hb.append(p2)
        assert ei.value.code == -22 and "hashgraph 2" in str(ei.value) and "event 30" in str(ei.value) and word in str(ei.value)
    # beyond cap_events
    p3 = [None] * B
    p3[1] = tuple(x[30:61] if len(x) > 60 else np.concatenate([x[30:60], x[59:60]]) for x in stream)
    with pytest.raises(pkg.SwirldHipError) as ei:
        hb.append(p3)
    assert ei.value.code == -34 and "cap_events" in str(ei.value)
    # beyond cap_rounds: a chain of two members whose height reaches 18 needs 21 rounds
    hc = pkg.HashgraphBatch(2, 2, cap_events=60, cap_rounds=20)
    k = 18
    ccr = np.array([0, 1] + [i % 2 for i in range(k)], np.int32)
    csp = np.array([-1, -1] + [0, 1] + list(range(2, k)), np.int32)
    cop = np.array([-1, -1] + [1] + list(range(2, k + 1)), np.int32)
    with pytest.raises(pkg.SwirldHipError) as ei:
        hc.append([None, (ccr, csp, cop)])
    assert ei.value.code == -34 and "cap_rounds" in str(ei.value) and hc.summary(1).events == 0
    hc.append([None, (ccr[:-1], csp[:-1], cop[:-1])])   # height 17: fits
    assert hc.summary(1).events == k + 1 and hc.heights(1)[-1] == 17
    hc.close()
    # a K beyond the undivided events
    hb.append([tuple(x[30:40] for x in stream)] * B)
    K = np.full(B, 10, np.int64)
    K[6] = 11
    with pytest.raises(pkg.SwirldHipError) as ei:
        hb.step(K)
    assert ei.value.code == -34 and "K[6]" in str(ei.value)
    assert np.array_equal(hb.summary_array()[:, 1:], before[:, 1:]), "nothing ran"
    assert state == [(hb.rounds(b, 0, 30).tobytes(), hb.transactions(b).tobytes()) for b in range(B)]
    with pytest.raises(pkg.SwirldHipError) as ei:
        hb.rounds(B, 0, 0)
    assert ei.value.code == -34
    hb.close()
    with pytest.raises(pkg.SwirldHipError) as ei:
        pkg.HashgraphBatch(2, 4, np.full(4, 1 << 29, np.uint64))
    assert ei.value.code == -75


# ---- destroy -------------------------------------------------------------------------------------------------------
def test_destroy_frees_everything(pkg):
    live = importlib.import_module("py-swirld_amd.engine").live_resources
    stream = batch_cases.forked_stream(4, 200, 5, 3)
    gc.collect()
    for run in range(2):
        before = live()
        hb = pkg.HashgraphBatch(16, 4, cap_events=len(stream[0]))
        now = live()
        assert now.streams == before.streams + 1 and now.pinned_bytes > before.pinned_bytes
        assert now.device_bytes - before.device_bytes >= pkg.HashgraphBatch.bytes_needed(16, 4, len(stream[0])) == hb.device_bytes
        hb.append([stream] * 16)
        out = hb.step()
        assert all(len(o[1]) > 0 for o in out)
        hb.close()
        assert live() == before, "run %d" % run
