"""GPU (-m gpu): the results of a whole batch in one call (sw_export_batch_*, csrc/batch_export.hip.h) — ragged arrays, one
launch, at most one synchronisation.  Expected values are those of the per-hashgraph getters (pinned to the goldens and the
oracle by tests/test_gpu_batch.py) and the goldens themselves; timestamps are compared as bytes.  The per-chunk function on
the CPU, under the sanitizers: tests/test_batch_export_host.py."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

import batch_cases
from conftest import load_golden
from test_batch_host import same_bits

try:
    import torch
except Exception:   # pragma: no cover
    torch = None

pytestmark = pytest.mark.gpu


def seg(d, key, b):
    return d[key][d["off"][b]:d["off"][b + 1]]


def check_against_getters(hb, bs, creators=None, o=None, e=None, r=None):
    """All four exports (taken here unless given) against the getters, for the hashgraphs bs."""
    o = hb.export_ordered() if o is None else o
    e = hb.export_events() if e is None else e
    r = hb.export_rounds() if r is None else r
    nr = hb.export_new_rounds()
    summ = hb.summary_array()
    assert o["off"][-1] == summ[:, 3].sum() and e["off"][-1] == summ[:, 0].sum() and r["off"][-1] == summ[:, 2].sum()
    assert np.array_equal(np.diff(o["off"]), summ[:, 3]) and np.array_equal(np.diff(r["off"]), summ[:, 2])
    assert r["witnesses"].shape == (r["off"][-1], hb.n) and r["famous"].shape == (r["off"][-1], hb.n)
    for b in bs:
        ev, rr, ts = hb.ordered(b)
        assert np.array_equal(seg(o, "event", b), ev) and np.array_equal(seg(o, "round_received", b), rr), b
        assert same_bits(seg(o, "time", b), ts), b
        assert np.array_equal(seg(e, "height", b), hb.heights(b)) and np.array_equal(seg(e, "round", b), hb.rounds(b)), b
        assert np.array_equal(seg(e, "famous", b), hb.famous_events(b)), b
        if creators is not None:
            assert np.array_equal(seg(e, "creator", b), creators[b]), b
        assert np.array_equal(seg(r, "witnesses", b), hb.witnesses(b)) and np.array_equal(seg(r, "famous", b), hb.famous(b)), b
        assert np.array_equal(seg(r, "consensus", b), hb.consensus(b)), b
        if summ[b, 6] == 0:
            assert np.array_equal(seg(nr, "rounds", b), hb.new_rounds(b)), b
    return o, e, r


# ---- 1. goldens ------------------------------------------------------------------------------------------------------
def run_goldens(pkg, names, scheds=None):
    """One batch of the fixtures `names`, fixture b on scheds[b] (None: the schedule it was recorded on, and then every call
    is compared with the recording too).  After every step, step_arrays() against new_rounds(b) and the log's new entries."""
    gs = [load_golden(nm) for nm in names]
    B, n = len(gs), gs[0]["n"]
    assert all(g["n"] == n for g in gs)
    own = [s is None for s in (scheds or [None] * B)]
    scheds = [[e - a for a, e in g["batches"]] if own[b] else scheds[b] for b, g in enumerate(gs)]
    assert all(sum(s) == len(g["creator"]) for s, g in zip(scheds, gs))
    hb = pkg.HashgraphBatch(B, n, np.stack([g["stake"] for g in gs]), cap_events=max(len(g["creator"]) for g in gs))
    pos, call = [0] * B, [0] * B
    while any(call[b] < len(scheds[b]) for b in range(B)):
        streams, K = [None] * B, np.zeros(B, np.int64)
        for b, g in enumerate(gs):
            if call[b] < len(scheds[b]):
                K[b] = scheds[b][call[b]]
                streams[b] = tuple(g[k][pos[b]:pos[b] + K[b]] for k in ("creator", "self_parent", "other_parent", "t", "sig"))
        hb.append(streams)
        calls0 = hb.export_stats().calls
        sa = hb.step_arrays(K)
        assert hb.export_stats().calls == calls0 + 2, "two export calls per step, whatever B"
        now = hb.summary_array()
        assert sa.n_failed == 0 and np.array_equal(sa.took, K > 0)
        assert sa.rounds_off.shape == sa.tx_off.shape == (B + 1,)
        for b, g in enumerate(gs):
            nc = sa.rounds[sa.rounds_off[b]:sa.rounds_off[b + 1]]
            sl = slice(sa.tx_off[b], sa.tx_off[b + 1])
            if not K[b]:
                assert len(nc) == 0 and sl.start == sl.stop, "a finished hashgraph sits out"
                continue
            n_out = int(now[b, 5])
            ev, rr, ts = hb.ordered(b, int(now[b, 3]) - n_out, n_out)
            assert np.array_equal(nc, hb.new_rounds(b)), (names[b], call[b])
            assert np.array_equal(sa.event[sl], ev) and np.array_equal(sa.round_received[sl], rr) and same_bits(sa.time[sl], ts), (names[b], call[b])
            if own[b]:
                c = call[b]
                assert list(nc) == list(g["new_c_flat"][g["new_c_off"][c]:g["new_c_off"][c + 1]]), (names[b], c)
                assert list(sa.event[sl]) == list(g["transactions"][g["tx_off"][c]:g["tx_off"][c + 1]]), (names[b], c)
            pos[b] += int(K[b])
            call[b] += 1
    o, e, r = check_against_getters(hb, range(B), creators=[g["creator"] for g in gs])
    for b, g in enumerate(gs):
        if own[b]:
            assert np.array_equal(seg(o, "event", b), g["transactions"]), names[b]
            assert np.array_equal(seg(e, "round", b), g["round"]) and np.array_equal(seg(e, "height", b), g["height"]), names[b]
            assert np.array_equal(seg(e, "famous", b), g["famous"]) and np.array_equal(seg(r, "witnesses", b), g["witnesses"]), names[b]
            assert np.array_equal(seg(r, "consensus", b), g["consensus"]), names[b]
    hb.close()


@pytest.mark.parametrize("names", [
    ["n4_mainloop_node0", "n4_s1_batch", "n4_s2_batch", "n4_s3_batch", "n4_s5_chunk1", "n4_s6_chunk7"],
    ["n16_s3_batch", "n16_s4_chunk250", "n16_s4_chunk50", "n16_s7_cliques", "n16_s8_slow", "n16_s9_stale"],
], ids=["n4", "n16"])
def test_goldens_on_their_own_schedules(pkg, names):
    run_goldens(pkg, names)


@pytest.mark.parametrize("name,chunk", [("n5_s1_batch", 37), ("n7_s2_chunk13", 700), ("n33_s5_batch", 1000)])
def test_three_copies_on_three_schedules(pkg, name, chunk):
    """Rows of n columns that are no multiple of four out of rows of 16 (n = 5, 7) and of 48 (n = 33).  Copy 0 follows the
    recorded schedule and is compared with the recording; copies 1 and 2 (equal chunks, ragged chunks) with the getters,
    since the reference's results depend on the schedule of its calls."""
    N = len(load_golden(name)["creator"])
    run_goldens(pkg, [name] * 3, [None, [min(chunk, N - a) for a in range(0, N, chunk)], batch_cases.ragged_schedule(N, 5, lo=N // 12, hi=N // 3)])


# ---- 2. ragged edges -------------------------------------------------------------------------------------------------
TINY_N, TINY_EVENTS, TINY_SCHED = 4, 120, (70, 50)


@functools.lru_cache(maxsize=None)
def tiny(seed):
    return batch_cases.synth(TINY_N, TINY_EVENTS, seed)


def tiny_batch(pkg, seeds):
    hb = pkg.HashgraphBatch(len(seeds), TINY_N, cap_events=TINY_EVENTS)
    pos = 0
    for k in TINY_SCHED:
        hb.append([tuple(x[pos:pos + k] for x in tiny(s)) for s in seeds])
        assert hb.step(collect=False) == 0
        pos += k
    return hb


RAGGED_SEEDS = [0, 1, 2, 5, 6, 1, 2]   # (each orders 11 to 66 of its 120 events)


def test_ragged_ranges(pkg):
    hb = tiny_batch(pkg, RAGGED_SEEDS)
    B = len(RAGGED_SEEDS)
    summ = hb.summary_array()
    assert (summ[:, 3] >= 11).all() and (summ[:, 2] >= 7).all()
    check_against_getters(hb, range(B), creators=[tiny(s)[0] for s in RAGGED_SEEDS])
    counts = np.array([0, 1, 0, 0, 2, 3, 1], np.int64)
    for cnt, first in ((counts, np.array([0, 2, 11, 1, 3, 0, 5], np.int64)), (counts[::-1].copy(), np.array([4, 0, 7, 9, 0, 1, 0], np.int64))):
        o, e = hb.export_ordered(first, cnt), hb.export_events(first + 50, cnt)
        assert np.array_equal(np.diff(o["off"]), cnt) and np.array_equal(np.diff(e["off"]), cnt)
        for b in range(B):
            ev, rr, ts = hb.ordered(b, int(first[b]), int(cnt[b]))
            assert np.array_equal(seg(o, "event", b), ev) and np.array_equal(seg(o, "round_received", b), rr) and same_bits(seg(o, "time", b), ts)
            assert np.array_equal(seg(e, "round", b), hb.rounds(b, int(first[b]) + 50, int(cnt[b])))
            assert np.array_equal(seg(e, "famous", b), hb.famous_events(b, int(first[b]) + 50, int(cnt[b])))
            assert np.array_equal(seg(e, "creator", b), tiny(RAGGED_SEEDS[b])[0][first[b] + 50:first[b] + 50 + cnt[b]])
        # first alone: up to the end
        o = hb.export_ordered(first)
        assert np.array_equal(np.diff(o["off"]), summ[:, 3] - first)
        assert all(np.array_equal(seg(o, "event", b), hb.transactions(b)[first[b]:]) for b in range(B))
    # one round per hashgraph: four hashgraphs' famous rows in one 16-byte chunk, all seven consensus bytes in one
    r0 = np.array([b % 5 for b in range(B)], np.int32)
    r = hb.export_rounds(r0, r0 + 1)
    assert list(r["off"]) == list(range(B + 1)) and r["famous"].shape == (B, 4) and r["consensus"].shape == (B,)
    for b in range(B):
        assert np.array_equal(r["witnesses"][b], hb.witnesses(b, int(r0[b]), int(r0[b]) + 1)[0])
        assert np.array_equal(r["famous"][b], hb.famous(b, int(r0[b]), int(r0[b]) + 1)[0])
        assert r["consensus"][b] == hb.consensus(b, int(r0[b]), int(r0[b]) + 1)[0]
    hb.close()


def test_all_counts_zero_launch_nothing(pkg):
    hb = tiny_batch(pkg, RAGGED_SEEDS)
    zero = np.zeros(len(RAGGED_SEEDS), np.int64)
    before = hb.export_stats()
    o = hb.export_ordered(zero, zero)
    e = hb.export_events(None, zero)
    r = hb.export_rounds(np.ones(len(RAGGED_SEEDS), np.int32), np.ones(len(RAGGED_SEEDS), np.int32))
    nr = hb.export_new_rounds(zero)
    for d in (o, e, r, nr):
        assert not d["off"].any() and all(len(v) == 0 for k, v in d.items() if k != "off")
    after = hb.export_stats()
    assert after.calls == before.calls + 8, "a sizing call and an export each"
    assert (after.launches, after.entries, after.d2h_copies) == (before.launches, before.entries, before.d2h_copies)
    hb.close()


def test_a_batch_of_one(pkg):
    hb = tiny_batch(pkg, [5])
    o, e, r = check_against_getters(hb, [0], creators=[tiny(5)[0]])
    assert list(o["off"]) == [0, 66] and list(e["off"]) == [0, TINY_EVENTS]
    part = hb.export_ordered([60], [6])
    assert np.array_equal(part["event"], o["event"][60:]) and same_bits(part["time"], o["time"][60:])
    hb.close()


# ---- 3. many hashgraphs ----------------------------------------------------------------------------------------------
def test_ten_thousand_hashgraphs(pkg):
    B, seeds = 10000, [0, 1, 2, 3, 5, 6, 4]   # (seeds 3 and 4 order nothing: empty segments all along the batch)
    hb = tiny_batch(pkg, [seeds[b % len(seeds)] for b in range(B)])
    stats0 = hb.export_stats()
    o, e, r = hb.export_ordered(), hb.export_events(), hb.export_rounds()
    stats = hb.export_stats()
    assert (stats.calls - stats0.calls, stats.launches - stats0.launches, stats.d2h_copies - stats0.d2h_copies) == (6, 3, 10)
    summ = hb.summary_array()
    assert o["off"][B] == summ[:, 3].sum() > 0 and (np.diff(o["off"]) == 0).sum() >= 2 * (B // len(seeds))
    for d, keys in ((o, ("event", "round_received", "time")), (e, ("creator", "height", "round", "famous")), (r, ("witnesses", "famous", "consensus"))):
        for key in keys:
            ref = [seg(d, key, b).tobytes() for b in range(len(seeds))]
            assert all(seg(d, key, b).tobytes() == ref[b % len(seeds)] for b in range(B)), key
    sample = sorted(set(np.random.default_rng(3).integers(0, B, 60).tolist()) | {0, 1, B - 2, B - 1})[:64]
    check_against_getters(hb, sample, creators={b: tiny(seeds[b % len(seeds)])[0] for b in sample}, o=o, e=e, r=r)
    hb.close()


# ---- 4. the device form ----------------------------------------------------------------------------------------------
def need_torch(pkg, what):
    if torch is None or not torch.cuda.is_available():
        pytest.fail("torch with a GPU is needed for the device form")
    pkg._lib.require_single_hip_runtime(what)
    return torch.device("cuda", 0)


def test_device_form_into_torch_tensors(pkg):
    dev = need_torch(pkg, "test_device_form_into_torch_tensors")
    hb = tiny_batch(pkg, RAGGED_SEEDS)
    B, n, PAD = len(RAGGED_SEEDS), TINY_N, 64
    host_o, host_e, host_r, host_n = hb.export_ordered(), hb.export_events(), hb.export_rounds(), hb.export_new_rounds()
    st = torch.cuda.Stream(device=dev)

    def full(shape, dtype, v):
        return torch.full(shape, v, dtype=dtype, device=dev)

    with torch.cuda.stream(st):
        To, Te, Tr, Tn = (int(d["off"][-1]) for d in (host_o, host_e, host_r, host_n))
        d_o = dict(event=full((To + PAD,), torch.int32, -7), round_received=full((To + PAD,), torch.int32, -7), time=full((To + PAD,), torch.float64, -7.0))
        d_e = dict(creator=full((Te + PAD,), torch.int32, -7), height=full((Te + PAD,), torch.int32, -7), round=full((Te + PAD,), torch.int32, -7),
                   famous=full((Te + PAD,), torch.int8, -7))
        d_r = dict(witnesses=full((Tr + PAD, n), torch.int32, -7), famous=full((Tr + PAD, n), torch.int8, -7), consensus=full((Tr + PAD,), torch.uint8, 0xA5))
        d_n = dict(rounds=full((Tn + PAD,), torch.int32, -7))
        launches0 = hb.export_stats().launches
        off_o, tot_o = hb.export_ordered_device(stream=st.cuda_stream, **d_o)
        off_e, tot_e = hb.export_events_device(stream=st.cuda_stream, **d_e)
        off_r, tot_r = hb.export_rounds_device(stream=st.cuda_stream, **d_r)
        off_n, tot_n = hb.export_new_rounds_device(stream=st.cuda_stream, **d_n)
        # two more with other ranges at once: nothing has been synchronised since the first call
        first, cnt = np.array([0, 2, 11, 1, 3, 0, 5], np.int64), np.array([0, 1, 0, 0, 2, 3, 1], np.int64)
        a = dict(event=full((16,), torch.int32, -7), time=full((16,), torch.float64, -7.0))
        b_ = dict(event=full((16,), torch.int32, -7), time=full((16,), torch.float64, -7.0))
        off_a, tot_a = hb.export_ordered_device(first, cnt, stream=st.cuda_stream, **a)
        off_b, tot_b = hb.export_ordered_device(first[::-1].copy(), cnt[::-1].copy(), stream=st.cuda_stream, **b_)
        assert hb.export_stats().launches == launches0 + 6 and hb.export_stats().d2h_copies == 4 + 3 + 3 + 1, "no copy back in the device form"
        copies = [{k: v.clone() for k, v in d.items()} for d in (d_o, d_e, d_r, d_n, a, b_)]   # readers on the caller's stream
    st.synchronize()
    for host, got, off, tot in ((host_o, copies[0], off_o, tot_o), (host_e, copies[1], off_e, tot_e), (host_r, copies[2], off_r, tot_r),
                                (host_n, copies[3], off_n, tot_n)):
        assert np.array_equal(off, host["off"]) and tot == host["off"][-1]
        for key, t in got.items():
            arr = t.cpu().numpy()
            assert arr[:tot].tobytes() == host[key].tobytes(), key
            rest = arr[tot:]
            assert len(rest) == PAD and (rest == (0xA5 if key == "consensus" else -7)).all(), "%s: written beyond total" % key
    for (f, c), got, off, tot in (((first, cnt), copies[4], off_a, tot_a), ((first[::-1].copy(), cnt[::-1].copy()), copies[5], off_b, tot_b)):
        want = hb.export_ordered(f, c)
        assert tot == 7 and np.array_equal(off, want["off"])
        assert np.array_equal(got["event"].cpu().numpy()[:7], want["event"]) and same_bits(got["time"].cpu().numpy()[:7], want["time"])
        assert (got["event"].cpu().numpy()[7:] == -7).all() and (got["time"].cpu().numpy()[7:] == -7.0).all()
    # a view one element into a tensor is not 16-byte aligned
    with pytest.raises(pkg.SwirldHipError) as ei:
        hb.export_ordered_device(event=d_o["event"][1:], stream=st.cuda_stream)
    assert ei.value.code == -22
    with pytest.raises(pkg.SwirldHipError) as ei:
        hb.export_rounds_device(consensus=d_r["consensus"][1:], stream=st.cuda_stream)
    assert ei.value.code == -22
    st.synchronize()
    assert (d_o["event"].cpu().numpy()[To:] == -7).all() and np.array_equal(d_o["event"].cpu().numpy()[:To], host_o["event"]), "a refused call writes nothing"
    hb.close()


# ---- 5. a frozen hashgraph -------------------------------------------------------------------------------------------
def test_frozen_hashgraph_is_exported_with_what_it_holds(pkg):
    n, ch, W = batch_cases.WHALE_N, batch_cases.LATE_WHALE_CHUNK, 1
    stream = batch_cases.late_whale_stream()
    stake = np.ones((3, n), np.uint64)
    stake[W] = batch_cases.late_whale_stake()
    hb = pkg.HashgraphBatch(3, n, stake, cap_events=len(stream[0]))
    for call, a in enumerate(range(0, len(stream[0]), ch)):
        hb.append([tuple(x[a:a + ch] for x in stream)] * 3)
        sa = hb.step_arrays()
        froze = call == batch_cases.LATE_WHALE_FAILS_AT
        assert sa.n_failed == int(froze) and list(sa.took) == [True, not froze, True]
        if froze:
            assert sa.rounds_off[W] == sa.rounds_off[W + 1] and sa.tx_off[W] == sa.tx_off[W + 1], "a frozen hashgraph's segments are empty"
            assert sa.rounds_off[1] > 0 and sa.tx_off[1] > 0 and sa.tx_off[3] > sa.tx_off[2]
    s = hb.summary(W)
    late = batch_cases.LATE_WHALE_ORDERED_BY_THE_FAILING_CALL
    assert (s.stage, s.code, s.n_ordered) == (3, -3, late) and s.ordered >= late
    o, e, r = check_against_getters(hb, range(3), creators=[stream[0]] * 3)
    assert len(seg(o, "event", W)) == s.ordered
    part = hb.export_ordered([0, s.ordered - late, 0], [0, late, 0])
    assert list(part["off"]) == [0, 0, late, late] and np.array_equal(part["event"], hb.transactions(W, s.ordered - late, late))
    nr = hb.export_new_rounds()
    assert len(seg(nr, "rounds", W)) == 0 and len(seg(nr, "rounds", 0)) > 0
    for d, keys in ((o, ("event", "round_received", "time")), (e, ("round", "famous")), (r, ("witnesses", "famous", "consensus")), (nr, ("rounds",))):
        for key in keys:
            assert seg(d, key, 0).tobytes() == seg(d, key, 2).tobytes(), "the healthy hashgraphs are unaffected (%s)" % key
    hb.close()


# ---- 6. above 4 GiB --------------------------------------------------------------------------------------------------
def test_exports_of_a_batch_above_4_gib(pkg):
    """The shape of test_a_batch_above_4_gib (tests/test_gpu_batch.py): the slab of hashgraph 2047 lies beyond 32-bit offsets.
    (120 events where that test has 64, which order nothing: here the log must hold something to export; their greatest
    height is 66, so 80 rounds of capacity where that test has 64.)"""
    B, n, E = 2048, 64, 8192
    stake = np.zeros(n, np.uint64)
    stake[:4] = 1
    stream = tiny(5)
    assert pkg.HashgraphBatch.bytes_needed(B, n, E, 80) > 4 << 30
    hb = pkg.HashgraphBatch(B, n, stake, cap_events=E, cap_rounds=80)
    parts = [None] * B
    parts[0] = parts[B - 1] = stream
    hb.append(parts)
    sa = hb.step_arrays()
    assert sa.n_failed == 0 and list(np.nonzero(sa.took)[0]) == [0, B - 1]
    assert np.array_equal(sa.rounds[:sa.rounds_off[1]], hb.new_rounds(0)) and np.array_equal(sa.rounds[sa.rounds_off[B - 1]:], hb.new_rounds(B - 1))
    o, e, r = check_against_getters(hb, [0, 1, B - 2, B - 1], creators={0: stream[0], 1: stream[0][:0], B - 2: stream[0][:0], B - 1: stream[0]})
    assert list(e["off"][[1, B - 1, B]]) == [120, 120, 240] and r["off"][1] >= 4 and r["off"][B] == 2 * r["off"][1]
    assert list(o["off"][[1, B - 1, B]]) == [66, 66, 132] and sa.tx_off[B] == 132 and sa.rounds_off[B] == 10
    for d, keys in ((o, ("event", "round_received", "time")), (e, ("creator", "height", "round", "famous")), (r, ("witnesses", "famous", "consensus"))):
        for key in keys:
            assert seg(d, key, 0).tobytes() == seg(d, key, B - 1).tobytes() and len(seg(d, key, 0)) > 0, key
    hb.close()


# ---- 7. refusals and bookkeeping -------------------------------------------------------------------------------------
def test_refusals_write_nothing(pkg):
    hb = tiny_batch(pkg, RAGGED_SEEDS)
    L, B = pkg._lib.load(), len(RAGGED_SEEDS)
    summ = hb.summary_array()
    T = int(summ[:, 3].sum())
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ev, rr, ts = np.full(T + 8, -7, np.int32), np.full(T + 8, -7, np.int32), np.full(T + 8, -7.0)
    off, total = np.full(B + 1, -1, np.int64), C.c_int64(-1)
    stats0 = hb.export_stats()
    assert L.sw_export_batch_ordered(hb._h, None, None, T - 1, p(off), p(ev), p(rr), p(ts), C.byref(total)) == -34
    assert total.value == T and np.array_equal(off, np.concatenate([[0], np.cumsum(summ[:, 3])])), "off and total are filled: size and retry"
    assert (ev == -7).all() and (rr == -7).all() and (ts == -7.0).all()
    assert b"nothing written" in L.sw_batch_last_error(hb._h)
    assert L.sw_export_batch_ordered(hb._h, None, None, T, None, p(ev), p(rr), p(ts), C.byref(total)) == -22, "off is NULL"
    wit = np.full((int(summ[:, 2].sum()), TINY_N), -7, np.int32)
    assert L.sw_export_batch_rounds(hb._h, None, None, len(wit) - 1, p(off), p(wit), None, None, None) == -34 and (wit == -7).all()
    one, zero = np.ones(B, np.int64), np.zeros(B, np.int64)
    for first, count in ((summ[:, 3] + one, None), (summ[:, 3], one), (-one, None), (zero, -one), (None, summ[:, 3] + one), (None, -one)):
        with pytest.raises(pkg.SwirldHipError) as ei:
            hb.export_ordered(first, count)
        assert ei.value.code == -34
    for first, count in ((summ[:, 0] + one, None), (zero, summ[:, 0] + one), (None, -one)):
        with pytest.raises(pkg.SwirldHipError) as ei:
            hb.export_events(first, count)
        assert ei.value.code == -34
    R = summ[:, 2].astype(np.int32)
    i1 = np.ones(B, np.int32)
    for r0, r1 in ((None, R + i1), (R + i1, None), (-i1, None), (2 * i1, i1)):
        with pytest.raises(pkg.SwirldHipError) as ei:
            hb.export_rounds(r0, r1)
        assert ei.value.code == -34
    only_last = zero.copy()
    only_last[B - 1] = summ[B - 1, 3] + 1   # one bad range among good ones
    with pytest.raises(pkg.SwirldHipError):
        hb.export_ordered(only_last)
    stats = hb.export_stats()
    assert (stats.launches, stats.entries, stats.d2h_copies) == (stats0.launches, stats0.entries, stats0.d2h_copies), "refused before any device work"
    # exactly one launch per export call that has something to bring
    o = hb.export_ordered()
    s1 = hb.export_stats()
    assert (s1.calls, s1.launches, s1.entries, s1.d2h_copies) == (stats.calls + 2, stats.launches + 1, stats.entries + T, stats.d2h_copies + 3)
    hb.export_events()
    hb.export_rounds()
    hb.export_new_rounds()
    s2 = hb.export_stats()
    assert (s2.calls, s2.launches, s2.d2h_copies) == (s1.calls + 6, s1.launches + 3, s1.d2h_copies + 4 + 3 + 1)
    assert L.sw_export_batch_ordered(hb._h, None, None, T, p(off), p(ev), None, None, None) == 0 and np.array_equal(ev[:T], o["event"]) and (ev[T:] == -7).all()
    assert hb.export_stats().d2h_copies == s2.d2h_copies + 1, "one copy per REQUESTED array"
    hb.close()


def test_destroy_gives_everything_back(pkg):
    gc.collect()
    before = pkg.engine.live_resources()
    hb = tiny_batch(pkg, RAGGED_SEEDS)
    hb.export_ordered()
    hb.export_rounds()
    if torch is not None and torch.cuda.is_available():
        out = torch.zeros(int(hb.summary_array()[:, 3].sum()), dtype=torch.int32, device="cuda:0")
        hb.export_ordered_device(event=out, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    during = pkg.engine.live_resources()
    assert during.device_bytes > before.device_bytes and during.pinned_bytes > before.pinned_bytes and during.events > before.events
    hb.close()
    assert pkg.engine.live_resources() == before
