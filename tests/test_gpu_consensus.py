"""GPU (-m gpu): round received and consensus timestamp kept on the device (sw_get_round_received, sw_get_consensus_time,
sw_export_ordered[_device], sw_get_consensus_stats; csrc/consensus.hip.h) against the reference's own values
(tests/golden/consensus: every fork-free golden, its stored timestamps and wall-clock-like ones, three settings of the
find_order path), against tests/model_consensus.py where no fixture exists (300, 600 and 256 members), on the host-sorted
rounds, across rewind / reset, as a read-only call, in its refusals, and into torch tensors on a stream of the caller's.

Timestamps are compared bit for bit: both sides evaluate .5 * (a + b) on the same two doubles.

torch is imported here, at collection, BEFORE the library is loaded (one HIP runtime for both: tests/conftest.py), and used
by the last test only; every other device buffer comes through ctypes from the runtime the library is linked against."""
import numpy as np
import pytest

try:
    import torch
except ImportError:      # (the device-consumer test reports it)
    torch = None

import model_consensus as mc
from test_gpu_export import Hip, stream_ids
from test_model_consensus import NAMES, VARIANTS, load_consensus, same_bits, variant
from conftest import load_golden

pytestmark = pytest.mark.gpu

EINVAL, ERANGE, ENOTSUP = -22, -34, -95


@pytest.fixture
def hip(pkg):
    h = Hip(pkg)
    yield h
    h.free()


def wallclock(N, seed):
    return 1.7e9 + 0.013 * np.arange(N) + np.random.default_rng(seed).uniform(0.0, 0.0129, N)


def check_against(h, N, tx, rr_fix, cts_fix, creator, ids=None):
    """the getters over events [0, N) and the exported stream equal the fixture restricted to the order so far"""
    ordered = np.zeros(N, bool)
    ordered[tx] = True
    rr, ct = h.round_received(), h.consensus_time()
    assert rr.shape == (N,) and ct.shape == (N,)
    assert np.array_equal(rr, np.where(ordered, rr_fix[:N], -1))
    assert np.array_equal(np.isnan(ct), ~ordered) and same_bits(ct[ordered], cts_fix[:N][ordered])
    d = h.export_ordered()
    assert np.array_equal(h.transactions(), tx) and np.array_equal(d["event"], tx)
    assert np.array_equal(d["round_received"], rr_fix[tx]) and same_bits(d["time"], cts_fix[tx])
    assert np.array_equal(d["creator"], creator[tx])
    assert ("ids" in d) == (ids is not None)
    if ids is not None:
        assert np.array_equal(d["ids"], ids[tx])
    if len(tx) > 2:       # a range inside the order, through the same call
        a, k = len(tx) // 3, len(tx) // 2
        p = h.export_ordered(a, k)
        assert np.array_equal(p["event"], tx[a:a + k]) and same_bits(p["time"], cts_fix[tx[a:a + k]])


def run_schedule(h, g, t, ids=None, after=None):
    calls = 0
    for a, b in g["batches"]:
        h.append_events(g["creator"][a:b], g["self_parent"][a:b], g["other_parent"][a:b], t[a:b], g["sig"][a:b])
        if ids is not None:
            h.set_event_ids(a, ids[a:b])
        h.divide_rounds(a, b - a)
        h.find_order(h.decide_fame())
        calls += 1
        if after:
            after(calls, b)


# ---- 1. the reference's own values ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bulk", ["default", "1", "0"])   # default threshold, always the table, always the searches
@pytest.mark.parametrize("v", VARIANTS)
@pytest.mark.parametrize("name", NAMES)
def test_golden_parity(pkg, name, v, bulk, monkeypatch):
    if bulk != "default":
        monkeypatch.setenv("SW_ORDER_BULK", bulk)
    g, f = load_golden(name), load_consensus(name)
    t, tx, tx_off, rr_fix, cts_fix = variant(g, f, v)
    N = len(g["creator"])
    ids = stream_ids(N) if v == "wallclock" else None       # (half of the cases with an id index)
    h = pkg.Hashgraph(g["n"], g["stake"])
    ncalls = len(g["batches"])
    checked = []

    def after(calls, n_now):
        if calls == ncalls or (ncalls > 1 and calls == (ncalls + 1) // 2):      # chunked cases: also after a middle call
            check_against(h, n_now, tx[:tx_off[calls]], rr_fix, cts_fix, g["creator"], ids)
            checked.append(calls)

    run_schedule(h, g, t, ids, after)
    assert checked[-1] == ncalls and len(checked) == (2 if ncalls > 1 else 1)
    st = h.consensus_stats()
    assert st["recorded_events"] == len(tx) and st["record_calls"] == int((np.diff(tx_off) > 0).sum())
    h.close()


# ---- 2. rounds the host sorts: their part of the device copy of the order is patched from the host --------------------------
@pytest.mark.parametrize("name,v", [("n16_s4_chunk250", "wallclock"), ("n64_s1_batch", "asis"), ("n4_s6_chunk7", "wallclock")])
def test_host_sorted_rounds_golden(pkg, name, v, monkeypatch):
    monkeypatch.setenv("SW_ORDER_HOST", "1")
    g, f = load_golden(name), load_consensus(name)
    t, tx, tx_off, rr_fix, cts_fix = variant(g, f, v)
    h = pkg.Hashgraph(g["n"], g["stake"])
    run_schedule(h, g, t)
    assert h.counters()["order_rounds_host_sorted"] > 0
    check_against(h, len(g["creator"]), tx, rr_fix, cts_fix, g["creator"])
    h.close()


def model_check(h, n, stream, new_c, seed, want_rounds=3):
    """No fixture: the model on a seeded sample of 256 ordered events plus the first and last event of every received round;
    (round received, consensus time) non-decreasing along the order of this ONE call, on all ordered events."""
    cr, sp, op, t, sig = stream
    tx = h.transactions()
    rr, ct = h.round_received(), h.consensus_time()
    ordered = np.zeros(len(cr), bool)
    ordered[tx] = True
    assert np.array_equal(rr >= 0, ordered) and np.array_equal(np.isnan(ct), ~ordered)
    assert mc.order_key_ok(tx, rr, ct)
    rounds = np.unique(rr[tx])
    assert len(rounds) >= want_rounds and set(rounds) <= set(int(r) for r in new_c)      # (coverage: a condition, not a measurement)
    sample = np.random.default_rng(seed).choice(tx, 256, replace=False)
    assert len(set(sample.tolist())) == 256
    edges = []
    for r in rounds:
        of_r = tx[rr[tx] == r]
        edges += [of_r[0], of_r[-1]]
    ev = np.unique(np.concatenate([sample, np.array(edges, tx.dtype)]))
    m_rr, m_ct = mc.consensus_values(ev, sorted(int(r) for r in new_c), h.can_see(), h.witnesses(), h.famous(), cr, sp, h.heights(), t,
                                     np.ones(n, np.int64))
    assert np.array_equal(m_rr, rr[ev]) and same_bits(m_ct, ct[ev])
    d = h.export_ordered(ids=False)
    assert np.array_equal(d["event"], tx) and np.array_equal(d["round_received"], rr[tx]) and same_bits(d["time"], ct[tx])
    assert np.array_equal(d["creator"], cr[tx])


def one_call(pkg, n, N, seed, mode=0, p0=0.0, p1=0.0):
    cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, seed, mode, p0, p1)
    stream = (cr, sp, op, wallclock(N, seed), sig)
    h = pkg.Hashgraph(n)
    h.append_events(*stream)
    h.divide_rounds(0, N)
    nc = list(h.decide_fame())
    h.find_order(nc)
    return h, stream, nc


def test_host_sorted_oversize_rounds(pkg, monkeypatch):
    """the shape of test_rounds_larger_than_the_lds_sort with SW_ORDER_BIG_HOST=1: rounds of more than 4096 events go to the host"""
    monkeypatch.setenv("SW_ORDER_BIG_HOST", "1")
    h, stream, nc = one_call(pkg, 256, 70000, 87, 2, 0.35, 0.02)
    assert h.counters()["order_rounds_host_sorted"] > 0
    model_check(h, 256, stream, nc, 87)
    h.close()


# ---- 3. beyond 130 members no fixture exists: the model -----------------------------------------------------------------------
@pytest.mark.parametrize("n,N,seed,bulk", [(300, 60000, 95, None), (600, 90000, 93, None), (256, 120000, 91, "0")])
def test_wide_hashgraphs_against_the_model(pkg, n, N, seed, bulk, monkeypatch):
    """8 and 16 mask words on the table path (k_order_median writes the timestamps), 256 members on the search path
    (k_order_times)"""
    if bulk is not None:
        monkeypatch.setenv("SW_ORDER_BULK", bulk)
    h, stream, nc = one_call(pkg, n, N, seed)
    model_check(h, n, stream, nc, seed)
    h.close()


# ---- 4. state -------------------------------------------------------------------------------------------------------------
def assert_nothing_ordered(h, N):
    rr, ct = h.round_received(), h.consensus_time()
    assert rr.shape == (N,) and np.all(rr == -1) and np.all(np.isnan(ct))
    d = h.export_ordered(0, 0)
    assert all(len(a) == 0 for a in d.values()) and h.num_ordered == 0
    with pytest.raises(pkg_error()) as e:
        h.export_ordered(0, 1)
    assert e.value.code == ERANGE


def pkg_error():
    import importlib
    return importlib.import_module("py-swirld_amd").SwirldHipError


@pytest.mark.parametrize("name", ["n16_s4_chunk50", "n10_s1_stake"])
def test_rewind_and_reset(pkg, name):
    g, f = load_golden(name), load_consensus(name)
    t, tx, tx_off, rr_fix, cts_fix = variant(g, f, "wallclock")
    N = len(g["creator"])
    h = pkg.Hashgraph(g["n"], g["stake"])
    run_schedule(h, g, t)
    check_against(h, N, tx, rr_fix, cts_fix, g["creator"])
    h.rewind()
    assert_nothing_ordered(h, N)              # after the rewind and before any find_order
    # the same schedule again over the resident events
    for call, (a, b) in enumerate(g["batches"]):
        h.divide_rounds(a, b - a)
        h.find_order(h.decide_fame())
    # (all events were resident from the start: round received may differ from the incremental run only through the
    # schedule, Q10, and the schedule is the same)
    check_against(h, N, tx, rr_fix, cts_fix, g["creator"])
    h.reset()
    assert h.num_events == 0 and h.num_ordered == 0 and len(h.round_received()) == 0
    a, b = g["batches"][0]
    h.append_events(g["creator"][a:b], g["self_parent"][a:b], g["other_parent"][a:b], t[a:b], g["sig"][a:b])
    h.divide_rounds(a, b - a)
    assert_nothing_ordered(h, b - a)
    h.reset()
    run_schedule(h, g, t)
    check_against(h, N, tx, rr_fix, cts_fix, g["creator"])
    h.close()


def test_getters_and_exports_change_nothing(pkg, hip):
    name = "n16_s4_chunk250"
    g, f = load_golden(name), load_consensus(name)
    t, tx, tx_off, rr_fix, cts_fix = variant(g, f, "wallclock")
    N = len(g["creator"])
    ids = stream_ids(N)
    h = pkg.Hashgraph(g["n"], g["stake"])
    half = len(g["batches"]) // 2
    first_half = dict(g, batches=g["batches"][:half])
    run_schedule(h, first_half, t, ids)
    n_now = g["batches"][half - 1][1]
    assert 0 < tx_off[half] < len(tx)

    def snapshot():
        c = h.counters()
        c.pop("kernel_launches")
        st = h.consensus_stats()
        return (h.rounds().tobytes(), h.witnesses().tobytes(), h.famous().tobytes(), h.consensus().tobytes(), h.transactions().tobytes(),
                h.heights().tobytes(), h.event_ids().tobytes(), h.payload_stats(), h.export_stats(), c, h.num_events, h.max_round, h.num_ordered,
                st["record_calls"], st["recorded_events"])

    before = snapshot()
    K = int(tx_off[half])
    bufs = dict(event=hip.alloc(4 * K), ids=hip.alloc(32 * K), creator=hip.alloc(4 * K), round_received=hip.alloc(4 * K), time=hip.alloc(8 * K))
    for _ in range(3):
        check_against(h, n_now, tx[:K], rr_fix, cts_fix, g["creator"], ids)
        assert h.export_ordered_device(0, K, **bufs) == K
        assert h.export_ordered_device(K // 2, K - K // 2, time=bufs["time"]) == K - K // 2
    h.synchronize()
    assert np.array_equal(hip.down(bufs["event"], K, np.int32), tx[:K])
    assert snapshot() == before
    assert h.consensus_stats()["export_calls"] >= 12
    # ... and the voting goes on to the fixture as if nothing had happened
    run_schedule(h, dict(g, batches=g["batches"][half:]), t, ids)
    check_against(h, N, tx, rr_fix, cts_fix, g["creator"], ids)
    h.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(pkg, hip):
    Err = pkg.SwirldHipError
    name = "n16_s3_batch"
    g, f = load_golden(name), load_consensus(name)
    t, tx, tx_off, rr_fix, cts_fix = variant(g, f, "asis")
    N, K = len(g["creator"]), len(tx)
    h = pkg.Hashgraph(g["n"], g["stake"])
    run_schedule(h, g, t)
    d_ev, d_id = hip.alloc(4 * (K + 8)), hip.alloc(32 * (K + 8) + 16)
    hip.fill(d_ev, 0x5A, 4 * (K + 8))
    hip.fill(d_id, 0x5A, 32 * (K + 8) + 16)

    def untouched():
        h.synchronize()
        return bool(np.all(hip.down(d_ev, K + 8, np.int32) == 0x5A5A5A5A) and np.all(hip.down(d_id, 32 * (K + 8) + 16, np.uint8) == 0x5A))

    # a range beyond the ordered events
    for first, k in ((0, K + 1), (K, 1), (-1, 2), (1, -1)):
        with pytest.raises(Err) as e:
            h.export_ordered_device(first, k, event=d_ev)
        assert e.value.code == ERANGE and untouched()
        with pytest.raises(Err) as e:
            h.export_ordered(first, k)
        assert e.value.code == ERANGE
    for fn in (h.round_received, h.consensus_time):
        with pytest.raises(Err) as e:
            fn(N - 1, 2)
        assert e.value.code == ERANGE
    # ids wanted without a complete id index; the same call without ids succeeds
    with pytest.raises(Err) as e:
        h.export_ordered_device(0, K, event=d_ev, ids=d_id)
    assert e.value.code == ENOTSUP and untouched()
    with pytest.raises(Err) as e:
        h.export_ordered(ids=True)
    assert e.value.code == ENOTSUP
    assert "ids" not in h.export_ordered() and h.export_ordered_device(0, K, event=d_ev) == K
    h.synchronize()
    assert np.array_equal(hip.down(d_ev, K, np.int32), tx)
    hip.fill(d_ev, 0x5A, 4 * (K + 8))
    h.set_event_ids(0, stream_ids(N))
    # misaligned ids; a host array where a device array belongs
    with pytest.raises(Err) as e:
        h.export_ordered_device(0, K, event=d_ev, ids=d_id + 8)
    assert e.value.code == EINVAL and untouched()
    host = np.full(K, 0x5A5A5A5A, np.int32)
    for kw in (dict(event=host.ctypes.data), dict(event=d_ev, creator=host.ctypes.data), dict(time=host.ctypes.data, event=d_ev)):
        with pytest.raises(Err) as e:
            h.export_ordered_device(0, K // 2, **kw)
        assert e.value.code == EINVAL and untouched() and np.all(host == 0x5A5A5A5A)
    # ... and the context still answers
    assert h.export_ordered_device(0, K, event=d_ev, ids=d_id) == K
    h.synchronize()
    assert np.array_equal(hip.down(d_id, 32 * K, np.uint8).reshape(K, 32), stream_ids(N)[tx])
    check_against(h, N, tx, rr_fix, cts_fix, g["creator"], stream_ids(N))
    h.close()


def test_exact_path_is_refused(pkg, hip):
    Err = pkg.SwirldHipError
    g = load_golden("n4_s1_batch")
    h = pkg.Hashgraph(g["n"], g["stake"])
    run_schedule(h, g, g["t"])
    K = h.num_ordered
    assert K > 0 and not h.exact and len(h.export_ordered()["event"]) == K
    # a forked event: member c's second event on the self-parent of its newest one
    cr, sp = g["creator"], g["self_parent"]
    c = 0
    newest = int(np.flatnonzero(cr == c)[-1])
    other = int(np.flatnonzero(cr == 1)[-1])
    h.append_events(np.array([c], np.int32), np.array([sp[newest]], np.int32), np.array([other], np.int32),
                    np.array([1e6]), np.zeros((1, 64), np.uint8))
    assert h.exact
    d_ev = hip.alloc(4 * K)
    for call in (lambda: h.round_received(), lambda: h.consensus_time(0, 1), lambda: h.export_ordered(0, 1), lambda: h.export_ordered(0, 0),
                 lambda: h.export_ordered_device(0, 1, event=d_ev)):
        with pytest.raises(Err) as e:
            call()
        assert e.value.code == ENOTSUP and "exact" in str(e.value)
    h.close()


# ---- 6. a consumer on the device ----------------------------------------------------------------------------------------------
def test_export_into_torch_tensors_on_a_stream(pkg):
    if torch is None or not torch.cuda.is_available():
        pytest.fail("torch with a GPU is needed for the device consumer")
    pkg._lib.require_single_hip_runtime("test_export_into_torch_tensors_on_a_stream")
    name = "n64_s1_batch"
    g, f = load_golden(name), load_consensus(name)
    t, tx, tx_off, rr_fix, cts_fix = variant(g, f, "wallclock")
    N, K = len(g["creator"]), len(tx)
    ids = stream_ids(N)
    h = pkg.Hashgraph(g["n"], g["stake"])
    run_schedule(h, g, t, ids)
    host = h.export_ordered()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    first, k = 5, K - 9
    with torch.cuda.stream(st):
        out = dict(event=torch.full((k,), -7, dtype=torch.int32, device=dev), ids=torch.full((k, 32), 0x5A, dtype=torch.uint8, device=dev),
                   creator=torch.full((k,), -7, dtype=torch.int32, device=dev), round_received=torch.full((k,), -7, dtype=torch.int32, device=dev),
                   time=torch.zeros(k, dtype=torch.float64, device=dev))
        assert h.export_ordered_device(first, k, stream=st.cuda_stream, **out) == k
        # ops enqueued on the caller's stream behind the call read complete arrays
        total = out["time"].sum() + out["round_received"].sum()
        copies = {key: a.clone() for key, a in out.items()}
    st.synchronize()
    sl = slice(first, first + k)
    assert np.array_equal(copies["event"].cpu().numpy(), host["event"][sl]) and np.array_equal(copies["ids"].cpu().numpy(), host["ids"][sl])
    assert np.array_equal(copies["creator"].cpu().numpy(), host["creator"][sl])
    assert np.array_equal(copies["round_received"].cpu().numpy(), host["round_received"][sl])
    assert same_bits(copies["time"].cpu().numpy(), host["time"][sl])
    assert same_bits(host["time"], cts_fix[tx]) and np.array_equal(host["event"], tx)
    exp_total = torch.from_numpy(host["time"][sl].copy()).sum().item() + int(host["round_received"][sl].sum())
    assert abs(total.item() - exp_total) <= 1e-9 * abs(exp_total)      # (a sum in another order: not a bit-exact quantity)
    h.close()
