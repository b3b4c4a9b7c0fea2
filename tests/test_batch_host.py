"""CPU: swb::step (py-swirld_amd/csrc/batch.hip.h) — one wavefront's whole main-loop step for one hashgraph of a batch —
compiled for the HOST (tests/batch_host.cpp: one lane, and 16 cooperative fibers that hand over at every sync) over a
batch laid out by batch_layout.h in host memory, AT THE ROW STRIDE THE BATCH USES (a multiple of 16, not of 64).

Every golden fixture of the unmodified reference (all 26, the 64- and 130-member ones included) with its recorded schedule,
fork-free and forked: new_c and the
transactions of every call, the final tables, and round received / consensus time of the log against
tests/golden/consensus/ and tests/golden/consensus_forked/.  Random forked streams under ragged schedules against the
oracle, with launches of a few events so that the divide-only launches in front of a step's last one run too.  The
hashgraph that ends in the reference's IndexError freezes, keeps what its earlier calls left, and is skipped afterwards.
The fixture sits in the MIDDLE of a batch of three whose memory starts as garbage: its neighbours must stay as created.
The GPU run of the same cases is tests/test_gpu_batch.py."""
import os

import numpy as np
import pytest

import batch_cases
from batch_hostlib import BatchHost
from conftest import GOLDEN_DIR, golden_names, load_golden


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def consensus_fixture(name):
    for sub in ("consensus", "consensus_forked"):
        p = os.path.join(GOLDEN_DIR, sub, name + ".npz")
        if os.path.exists(p):
            with np.load(p) as z:
                return {k: z[k] for k in z.files}
    return None


def check_log_against_fixture(log, f, N):
    ev, rr, ts = log
    assert np.array_equal(rr, f["asis_round_received"][ev])
    assert same_bits(ts, f["asis_consensus_time"][ev])
    assert len(ev) == int((f["asis_round_received"][:N] >= 0).sum()) == len(set(ev.tolist()))


def _golden_cases():
    """EVERY golden with the 1-lane build — the three wide ones included (64 and 130 members: strides of 64 and 144, a row of
    more than two waves); the 16-fiber build, which pays a fiber switch per lane and sync, on the fixtures of at most 4000
    events and 60 calls."""
    return [pytest.param(name, lanes, id="%s-%s" % (name, "16lanes" if lanes else "1lane"))
            for name in golden_names() for lanes in (False, True)
            if not (lanes and (len(load_golden(name)["batches"]) > 60 or len(load_golden(name)["creator"]) > 4000))]


@pytest.mark.parametrize("name,lanes", _golden_cases())
def test_step_matches_reference_golden(name, lanes):
    g = load_golden(name)
    n, N = g["n"], len(g["creator"])
    stake = np.ones((3, n), np.uint64)
    stake[1] = g["stake"]
    x = BatchHost(3, n, stake, cap_events=N, lanes=lanes)
    assert x.npad == (n + 15) // 16 * 16
    for call, (a, b) in enumerate(g["batches"]):
        x.append(1, g["creator"][a:b], g["self_parent"][a:b], g["other_parent"][a:b], g["t"][a:b], g["sig"][a:b])
        nc, tx = x.step(1, b - a)
        assert list(nc) == list(g["new_c_flat"][g["new_c_off"][call]:g["new_c_off"][call + 1]]), call
        assert list(tx) == list(g["transactions"][g["tx_off"][call]:g["tx_off"][call + 1]]), call
    st = x.state(1)
    assert np.array_equal(st["height"], g["height"])
    assert np.array_equal(st["round"], g["round"])
    assert np.array_equal(st["can_see"], g["can_see"])
    assert np.array_equal(st["wit"], g["witnesses"])
    for r, order in enumerate(g["wit_order"]):
        assert np.array_equal(st["worder"][r], order)
    assert np.array_equal(st["fam"], g["famous"])
    assert np.array_equal(st["cons"], g["consensus"])
    assert np.array_equal(st["tbd"], g["tbd"])
    assert np.array_equal(x.log(1)[0], g["transactions"])
    assert x.visited_clear(1)
    f = consensus_fixture(name)
    if f is not None:
        check_log_against_fixture(x.log(1), f, N)
    for b in (0, 2):   # the neighbours: as created
        assert x.summary(b) == dict(divided=0, rounds=0, ordered=0, n_new=0, n_out=0, stage=0, code=0, event=0)


def test_every_golden_runs_and_all_but_the_main_loop_have_a_consensus_fixture():
    ran = [p.values[0] for p in _golden_cases() if not p.values[1]]
    assert ran == golden_names() and len(ran) == 26 and {"n64_s1_batch", "n64_s2_slow_chunk1000", "n130_s4_batch"} <= set(ran)
    assert [nm for nm in ran if consensus_fixture(nm) is None] == ["n4_mainloop_node0"]
    assert sum("forks" in nm for nm in ran) == 4


def assert_same(o, x, b):
    st = x.state(b)
    assert np.array_equal(st["round"], o.round)
    assert np.array_equal(st["can_see"], o.can_see)
    assert np.array_equal(st["wit"], o.witnesses())
    for r, order in enumerate(st["worder"]):
        assert np.array_equal(order, o.witness_order(r)), "dict order of witnesses[%d]" % r
    assert np.array_equal(st["fam"], o.famous_by_event)
    assert np.array_equal(st["fam_slot"], o.famous_table())
    assert np.array_equal(st["cons"], o.consensus())
    assert np.array_equal(st["tbd"], o.tbd)
    assert np.array_equal(x.log(b)[0], o.transactions)
    assert np.array_equal(st["height"], o.height)


# n, N, seed, forks, (lo, hi) of the ragged call sizes, events per launch (0: the product's 8192), stake, lanes
RANDOM_CASES = [
    (8, 600, 1, 10, (1, 600), 0, None, False), (8, 600, 2, 10, (1, 60), 0, None, True), (5, 400, 3, 25, (1, 4), 0, None, False),
    (16, 900, 4, 20, (50, 300), 64, None, False), (4, 500, 6, 30, (1, 30), 5, None, False), (17, 700, 7, 12, (100, 400), 33, None, True),
    (9, 800, 21, 15, (20, 120), 0, [1, 1, 2, 1, 1, 1, 2, 1, 1], False), (70, 3000, 5, 8, (500, 1500), 400, None, True),
    (8, 600, 9, 0, (1, 100), 0, None, False),
]


@pytest.mark.parametrize("n,N,seed,forks,sizes,per_launch,stake,lanes", RANDOM_CASES)
def test_step_matches_oracle_on_forked_streams_under_ragged_schedules(n, N, seed, forks, sizes, per_launch, stake, lanes):
    stream = batch_cases.forked_stream(n, N, seed, forks)
    cr, sp, op, t, sig = stream
    sched = batch_cases.ragged_schedule(len(cr), seed, *sizes)
    st = None if stake is None else np.array(stake, np.uint64)
    rec = batch_cases.Record(n, stream, sched, st)
    assert rec.failed_call is None and rec.o.max_round >= 3
    x = BatchHost(1, n, None if st is None else st[None, :], cap_events=len(cr), lanes=lanes)
    a = 0
    for call, k in enumerate(sched):
        x.append(0, cr[a:a + k], sp[a:a + k], op[a:a + k], t[a:a + k], sig[a:a + k])
        nc, tx = x.step(0, k, per_launch)
        assert (list(nc), list(tx)) == rec.calls[call], "call %d" % call
        a += k
    assert_same(rec.o, x, 0)
    assert x.visited_clear(0)


def test_the_oracle_raises_on_the_whale_case_and_at_which_call():
    rec = batch_cases.Record(batch_cases.WHALE_N, batch_cases.whale_stream(), [batch_cases.WHALE_CHUNK] * 6, batch_cases.whale_stake())
    assert rec.failed_call == batch_cases.WHALE_FAILS_AT and "IndexError" in rec.error
    st = batch_cases.whale_stake()
    assert 2 * int(st.max()) > int(st.sum()) and (st == 0).sum() == batch_cases.WHALE_N // 2


@pytest.mark.parametrize("lanes", [False, True], ids=["1lane", "16lanes"])
def test_whale_hashgraph_freezes_where_the_oracle_raises(lanes):
    n, ch = batch_cases.WHALE_N, batch_cases.WHALE_CHUNK
    cr, sp, op, t, sig = batch_cases.whale_stream()
    rec = batch_cases.Record(n, (cr, sp, op, t, sig), [ch] * 6, batch_cases.whale_stake())
    x = BatchHost(1, n, batch_cases.whale_stake()[None, :], cap_events=len(cr), lanes=lanes)
    kept = None
    for call in range(4):
        a = call * ch
        x.append(0, cr[a:a + ch], sp[a:a + ch], op[a:a + ch], t[a:a + ch], sig[a:a + ch])
        got = x.step(0, ch)
        if call < rec.failed_call:
            assert (list(got[0]), list(got[1])) == rec.calls[call]
        elif call == rec.failed_call:
            s = x.summary(0)
            assert got is None and (s["stage"], s["code"]) == (3, -3) and 0 <= s["event"] < a + ch
            # the reference appends a round's events before it turns to the next round of new_c (swirld.py:307-309), so what the
            # failing call ordered before it raised is in the log, exactly as in the oracle's transactions
            assert s["ordered"] == len(rec.o.transactions) >= sum(len(c[1]) for c in rec.calls)
            kept = (s, x.state(0))
        else:   # frozen: the step returns at once
            assert got is None and x.summary(0) == kept[0]
            now = x.state(0)
            assert all(np.array_equal(now[k][:len(kept[1][k])], kept[1][k]) for k in ("round", "fam", "tbd", "wit", "cons"))
    assert np.array_equal(x.log(0)[0], rec.o.transactions)
    assert np.array_equal(kept[1]["round"][:rec.o.N], rec.o.round)


@pytest.mark.parametrize("lanes", [False, True], ids=["1lane", "16lanes"])
def test_a_call_that_raises_in_a_later_round_has_logged_the_rounds_before_it(lanes):
    n, ch = batch_cases.WHALE_N, batch_cases.LATE_WHALE_CHUNK
    cr, sp, op, t, sig = batch_cases.late_whale_stream()
    st = batch_cases.late_whale_stake()
    rec = batch_cases.Record(n, (cr, sp, op, t, sig), [ch, ch], st)
    before = sum(len(c[1]) for c in rec.calls)
    assert rec.failed_call == batch_cases.LATE_WHALE_FAILS_AT and "IndexError" in rec.error
    assert len(rec.o.transactions) - before == batch_cases.LATE_WHALE_ORDERED_BY_THE_FAILING_CALL
    x = BatchHost(1, n, st[None, :], cap_events=len(cr), lanes=lanes)
    for call in range(2):
        a = call * ch
        x.append(0, cr[a:a + ch], sp[a:a + ch], op[a:a + ch], t[a:a + ch], sig[a:a + ch])
        got = x.step(0, ch)
        if call < rec.failed_call:
            assert (list(got[0]), list(got[1])) == rec.calls[call]
    s = x.summary(0)
    assert got is None and (s["stage"], s["code"]) == (3, -3)
    assert s["ordered"] == len(rec.o.transactions) and s["n_out"] == batch_cases.LATE_WHALE_ORDERED_BY_THE_FAILING_CALL
    assert np.array_equal(x.log(0)[0], rec.o.transactions)
    state = x.state(0)
    assert np.array_equal(state["tbd"], rec.o.tbd) and np.array_equal(state["cons"], rec.o.consensus()) and np.array_equal(state["fam"], rec.o.famous_by_event)
