"""GPU (-m gpu): find_order's final sort (swirld.py:306) where consensus timestamp AND the first 8 key bytes tie — the cases
of tests/order_tie_cases.py, which tests/test_order_tie_cases.py proves (oracle alone) to be ordered by key bytes 8..63.

The device sorts (k_order_sort, k_order_sort_big; csrc/order.hip.h) carry 8 key bytes and flag a round with two events
equal in (timestamp, those bytes); host_sort_rounds re-sorts the flagged rounds on all 64 bytes, fetches the signatures it
needs (ensure_sig_h), repeats an early copy to the caller and patches the device's copy of the order (consensus_record).
Every case is compared with the oracle on the same stream — find_order's return value call by call, transactions() and
export_ordered()["event"] at the end — and, on the fast path, counters()["order_rounds_host_sorted"] must rise in every call
by exactly the number of received rounds that hold two events equal in consensus_time() and in bytes 0..7 of the
signature (the whitening key is common to a round).  Nothing here sets SW_ORDER_HOST except test_forced_host_sort.

Orders are integer arrays and timestamps are compared by bit pattern: no tolerance anywhere.

No torch here (see tests/test_gpu_ingest_device.py): device buffers come through ctypes from the HIP runtime the library is
linked against."""
import ctypes as C
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import model_consensus as mc
import model_payload as mp
import order_tie_cases as T
from test_gpu_export import Hip
from test_model_consensus import same_bits
from test_order_tie_cases import median_conditions

pytestmark = pytest.mark.gpu

ERANGE = -34
SLOW = ("n256_big_window", "n300_q16", "n300_q64", "n100_groups_window")      # oracle runs of 1 to 8 seconds
_EX = ThreadPoolExecutor(max_workers=4)
_pending, _oracle = {}, {}


def _oracle_of(name):
    case = T.BY_NAME[name]
    stream, stake, crafted, deep = T.build(case)
    t0 = time.time()
    run, o = T.oracle_run(case, stream, stake)
    return case, stream, stake, crafted, run, o, time.time() - t0


@pytest.fixture(scope="module", autouse=True)
def slow_oracles(pkg):
    """the oracle runs of the large cases, once per module, side by side on threads from the module's first test on (the
    oracle's C calls release the GIL)"""
    from oracle import oracle as _o
    _o.lib()
    for nm in SLOW:
        if nm not in _oracle and nm not in _pending:
            _pending[nm] = _EX.submit(_oracle_of, nm)
    yield
    for f in _pending.values():
        f.cancel()


def oracle_of(name):
    """(case, stream, stake, crafted mask, oracle run, oracle, oracle seconds), once per case"""
    if name not in _oracle:
        _oracle[name] = _pending.pop(name).result() if name in _pending else _oracle_of(name)
    return _oracle[name]


@pytest.fixture
def hip(pkg):
    h = Hip(pkg)
    yield h
    h.free()


def host_append(h, stream, a, b):
    h.append_events(*[x[a:b] for x in stream])


def drive(h, calls, stream, run, append=host_append, count=True, dense_of=None):
    """`h` through the call schedule against the oracle's run: new_c and find_order's return value of every call, and (with
    `count`) the rise of order_rounds_host_sorted against the tied rounds of the call.  `dense_of`: stream index -> dense
    index, where the context numbers the events itself.  Returns (rounds ordered, rounds tied, events per received round)."""
    sig = stream[4]
    ordered_rounds, tied_rounds, sizes = [], [], {}
    for i, (a, b) in enumerate(calls):
        append(h, stream, a, b)
        h.divide_rounds(a, b - a)
        nc = [int(r) for r in h.decide_fame()]
        assert nc == run.new_c[i], "new_c of call %d" % i
        before = h.counters()["order_rounds_host_sorted"]
        tx = np.array(h.find_order(nc))
        exp = run.orders[i] if dense_of is None else dense_of[run.orders[i]]
        assert np.array_equal(tx, exp), "find_order of call %d" % i
        if count:
            rr, ct = h.round_received(), h.consensus_time()
            sig_dense = sig[:b] if dense_of is None else sig[np.argsort(dense_of[:b])]
            tied = T.tied_rounds(tx, rr, ct, sig_dense)
            rise = h.counters()["order_rounds_host_sorted"] - before
            assert rise == len(tied), "call %d: %d rounds went to the host sort, %d hold a (time, 8-byte key) tie: %s" % (i, rise, len(tied), tied.tolist())
            for r in np.unique(rr[tx]):
                sizes[int(r)] = int((rr[tx] == r).sum())
            ordered_rounds += np.unique(rr[tx]).tolist()
            tied_rounds += tied.tolist()
    assert len(set(ordered_rounds)) == len(ordered_rounds), "a round receives events in one call only"
    return ordered_rounds, tied_rounds, sizes


def check_end(h, run, dense_of=None):
    exp = run.transactions if dense_of is None else dense_of[run.transactions]
    assert h.num_ordered == len(exp) and np.array_equal(h.transactions(), exp), "transactions()"
    assert np.array_equal(h.export_ordered()["event"], exp), 'export_ordered()["event"]'


def check_export_agrees(h, tx):
    """the device's copy of the order (patched where the host re-sorted) against the getters, bit for bit"""
    d = h.export_ordered()
    rr, ct = h.round_received(), h.consensus_time()
    assert np.array_equal(d["event"], tx) and np.array_equal(d["round_received"], rr[tx]) and same_bits(d["time"], ct[tx])
    ordered = np.zeros(len(rr), bool)
    ordered[tx] = True
    assert np.array_equal(rr >= 0, ordered) and np.array_equal(np.isnan(ct), ~ordered)


def set_bulk(monkeypatch, bulk):
    if bulk != "default":
        monkeypatch.setenv("SW_ORDER_BULK", bulk)


# ---- 1. what the reference itself computed -----------------------------------------------------------------------------------
@pytest.mark.parametrize("bulk", ["default", "1", "0"])   # default threshold, always the table, always the searches
@pytest.mark.parametrize("name", T.RECORDED)
def test_recorded_reference(pkg, name, bulk, monkeypatch):
    set_bulk(monkeypatch, bulk)
    case = T.BY_NAME[name]
    g = T.load_recorded(name)
    stream = (g["creator"], g["self_parent"], g["other_parent"], g["t"], g["sig"])
    ends = np.cumsum(g["sched"])
    calls = [(int(e - k), int(e)) for k, e in zip(g["sched"], ends)]
    run = T.Run([[int(r) for r in g["new_c_flat"][g["new_c_off"][i]:g["new_c_off"][i + 1]]] for i in range(len(calls))],
                [g["tx_flat"][g["tx_off"][i]:g["tx_off"][i + 1]] for i in range(len(calls))], g["tx_flat"])
    h = pkg.Hashgraph(case.n, None if (g["stake"] == 1).all() else g["stake"].astype(np.uint64))
    ordered, tied, _ = drive(h, calls, stream, run)
    check_end(h, run)
    check_export_agrees(h, run.transactions)
    assert len(tied) > 0 and (len(tied) == len(ordered) if case.window is T.ALL else len(tied) < len(ordered))
    assert h.counters()["order_rounds_host_sorted"] == len(tied)
    h.close()


# ---- 2. the tie flag of k_order_sort is exact ----------------------------------------------------------------------------------
@pytest.mark.parametrize("bulk", ["default", "1", "0"])
@pytest.mark.parametrize("name", ["n33_window", "n130_window"])
def test_tie_detection_is_exact(pkg, name, bulk, monkeypatch):
    set_bulk(monkeypatch, bulk)
    case, stream, stake, crafted, run, o, sec = oracle_of(name)
    h = pkg.Hashgraph(case.n, stake)
    t0 = time.time()
    ordered, tied, sizes = drive(h, T.calls_of(case), stream, run)
    print("\n[%s bulk=%s] %d rounds ordered, %d tied %s, oracle %.2f s, device pass %.2f s" % (name, bulk, len(ordered), len(tied), tied, sec, time.time() - t0))
    assert 0 < len(tied) < len(ordered), "rounds with and without ties in one call"
    assert h.counters()["order_rounds_host_sorted"] == len(tied) > 0
    check_end(h, run)
    check_export_agrees(h, run.transactions)
    h.close()


# ---- 3. ... and so is k_order_sort_big's -------------------------------------------------------------------------------------
def test_big_sort_flags_exactly_the_tied_rounds(pkg):
    """the shape of test_rounds_larger_than_the_lds_sort (256 members, slow members, rounds of more than 4096 events) with
    ties crafted in a window: oversize rounds with and without a tie, sorted by k_order_sort_big"""
    case, stream, stake, crafted, run, o, sec = oracle_of("n256_big_window")
    h = pkg.Hashgraph(case.n, stake)
    t0 = time.time()
    ordered, tied, sizes = drive(h, T.calls_of(case), stream, run)
    print("\n[n256_big_window] events per round %s, tied %s, oracle %.2f s, device pass %.2f s" % (sizes, tied, sec, time.time() - t0))
    tx = run.transactions
    assert len(run.new_c[0]) >= 4 and len(tx) > 4096 * 3 and len(tx) / len(run.new_c[0]) > 4096      # (the rounds really are that large)
    big = {r for r, k in sizes.items() if k > 4096}
    assert big & set(tied), "an oversize round with a tie"
    assert big - set(tied), "an oversize round without one"
    assert 0 < len(tied) < len(ordered) and h.counters()["order_rounds_host_sorted"] == len(tied)
    check_end(h, run)
    check_export_agrees(h, tx)
    h.close()


# ---- 4. the early copy to the caller, redone -----------------------------------------------------------------------------------
@pytest.mark.parametrize("one_stream", [False, True])
def test_early_copy_is_redone_after_a_host_sort(pkg, one_stream, monkeypatch):
    """several groups (SW_ORDER_SLAB_MB=1 on test_find_order_table_path_under_its_knobs' smallest shape): the caller's array is
    filled group by group as the device sorted it, and again once the host has re-sorted the tied rounds"""
    monkeypatch.setenv("SW_ORDER_BULK", "1")
    monkeypatch.setenv("SW_ORDER_SLAB_MB", "1")
    if one_stream:
        monkeypatch.setenv("SW_ORDER_ONE_STREAM", "1")
    case, stream, stake, crafted, run, o, sec = oracle_of("n100_groups_window")
    h = pkg.Hashgraph(case.n, stake)
    t0 = time.time()
    ordered, tied, sizes = drive(h, T.calls_of(case), stream, run)       # (the array find_order RETURNS equals the oracle's)
    print("\n[n100_groups_window one_stream=%s] %d rounds ordered, %d tied, oracle %.2f s, device pass %.2f s" % (one_stream, len(ordered), len(tied), sec, time.time() - t0))
    assert len(run.transactions) > 20000 and max(sizes.values()) <= 4096      # (no oversize round: those keep the copy for the end)
    assert 0 < len(tied) < len(ordered) and h.counters()["order_rounds_host_sorted"] == len(tied)
    check_end(h, run)
    check_export_agrees(h, run.orders[0])
    h.close()


# ---- 5. an out_events shorter than the order -----------------------------------------------------------------------------------
@pytest.mark.parametrize("bulk", ["1", "0"])   # the table / the searches
def test_short_out_events_keeps_the_tied_order(pkg, monkeypatch, bulk):
    """test_short_out_events_keeps_the_order's scenario on a case in which every round is re-sorted by the host"""
    monkeypatch.setenv("SW_ORDER_BULK", bulk)
    case, stream, stake, crafted, _, _, _ = oracle_of("n16_all")
    N, N2 = 4000, case.N
    two_calls = case._replace(chunk=N)
    assert T.calls_of(two_calls) == [(0, N), (N, N2)]
    run, o = T.oracle_run(two_calls, stream, stake)
    h = pkg.Hashgraph(case.n, stake)
    host_append(h, stream, 0, N)
    h.divide_rounds(0, N)
    nc = [int(r) for r in h.decide_fame()]
    assert nc == run.new_c[0]
    exp = run.orders[0]
    cap = len(exp) // 2
    assert cap > 100
    rounds = np.ascontiguousarray(sorted(nc), np.int32)
    out, n_out = np.full(cap, -1, np.int32), C.c_int64(-1)
    rc = h._L.sw_find_order(h._h, rounds.ctypes.data_as(C.c_void_p), len(rounds), out.ctypes.data_as(C.c_void_p), cap, C.byref(n_out))
    assert rc == ERANGE and n_out.value == len(exp)
    assert np.array_equal(out, exp[:cap]), "the part that fits is the oracle's"
    assert h.num_ordered == len(exp) and np.array_equal(h.transactions(), exp)
    tied = T.tied_rounds(exp, h.round_received(), h.consensus_time(), stream[4][:N])
    assert h.counters()["order_rounds_host_sorted"] == len(tied) > 0
    check_export_agrees(h, exp)
    host_append(h, stream, N, N2)
    h.divide_rounds(N, N2 - N)
    nc = [int(r) for r in h.decide_fame()]
    assert nc == run.new_c[1] and len(nc) > 0
    assert np.array_equal(h.find_order(nc), run.orders[1])
    check_end(h, run)
    check_export_agrees(h, run.transactions)
    h.close()


# ---- 6. signatures that never passed through the host ----------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["append_events_device", "ingest_payload_device"])
def test_events_entered_from_device_memory(pkg, hip, route):
    """sig_h is incomplete: ensure_sig_h fetches what host_sort_rounds compares, and a later call extends the part it has"""
    case, stream, stake, crafted, run, o, sec = oracle_of("n16_all")
    cr, sp, op, t, sig = stream
    h = pkg.Hashgraph(case.n, stake)
    dense_of = np.full(case.N, -1, np.int64)

    def append(h, stream, a, b):
        if route == "append_events_device":
            h.append_events_device(hip.up(cr[a:b], np.int32), hip.up(sp[a:b], np.int32), hip.up(op[a:b], np.int32), hip.up(t[a:b], np.float64),
                                   hip.up(sig[a:b], np.uint8), count=b - a)
            dense_of[a:b] = np.arange(a, b)
        else:
            ids, spi, opi, ar, crr, ok = mp.to_arrays(mp.from_stream(cr, sp, op, list(range(a, b))))
            d_out = hip.alloc(4 * (b - a))
            _, n_stored = h.ingest_payload_device(hip.up(ids, np.uint8), hip.up(spi, np.uint8), hip.up(opi, np.uint8), hip.up(ar, np.uint8),
                                                  hip.up(crr, np.int32), None, hip.up(t[a:b], np.float64), hip.up(sig[a:b], np.uint8),
                                                  index_out=d_out, count=b - a)
            assert n_stored == b - a
            dense_of[a:b] = hip.down(d_out, b - a, np.int32)
        h.synchronize()
        hip.free()
        assert sorted(dense_of[:b].tolist()) == list(range(b))

    calls = T.calls_of(case)
    assert len(calls) >= 3
    ordered, tied, _ = drive(h, calls, stream, run, append=append, dense_of=dense_of)
    assert len(tied) == len(ordered) > 0 and h.counters()["order_rounds_host_sorted"] == len(tied)
    assert sum(len(x) > 0 for x in run.orders) >= 3, "several calls that order (and tie): sig_h grows call by call"
    if route == "append_events_device":
        assert h.ingest_stats()["device_batches"] == len(calls), "no batch fell back to the host path"
    check_end(h, run, dense_of)
    check_export_agrees(h, dense_of[run.transactions])
    h.close()


# ---- 7. the forced host sort on real ties --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n16_all", "ref_n10_stake_all"])
def test_forced_host_sort_on_real_ties(pkg, name, monkeypatch):
    """SW_ORDER_HOST=1 (the hook of test_host_sort_fallback_matches) where every round holds ties behind byte 8"""
    monkeypatch.setenv("SW_ORDER_HOST", "1")
    case, stream, stake, crafted, run, o, sec = oracle_of(name)
    h = pkg.Hashgraph(case.n, stake)
    drive(h, T.calls_of(case), stream, run, count=False)
    assert h.counters()["order_rounds_host_sorted"] > 0
    check_end(h, run)
    check_export_agrees(h, run.transactions)
    h.close()


# ---- 8. the exact path: item_less and the heap sort of csrc/exact.hip.h --------------------------------------------------------
@pytest.mark.parametrize("history", [False, True])
@pytest.mark.parametrize("name", ["forks_n8_all", "forks_n12_stake_chunk40_all"])
def test_exact_path_on_tied_keys(pkg, name, history):
    case, stream, stake, crafted, run, o, sec = oracle_of(name)
    h = pkg.Hashgraph(case.n, stake)
    if history:
        h.set_exact_history()
    drive(h, T.calls_of(case), stream, run, count=False)
    assert h.exact
    assert np.array_equal(h.transactions(), run.transactions) and h.num_ordered == len(run.transactions)
    assert np.array_equal(h.rounds(), o.round) and np.array_equal(h.famous(), o.famous_table())
    if history:
        check_export_agrees(h, run.transactions)
        rr, ct = h.round_received(), h.consensus_time()
        tx = run.transactions
        assert len(T.tied_rounds(tx, rr, ct, stream[4])) == len(np.unique(rr[tx])), "every round holds a (time, 8-byte key) tie"
    h.close()


# ---- 9. medians over duplicate-heavy samples -----------------------------------------------------------------------------------
_model = {}


def model_of(name):
    """(round received, consensus time, sample lists) of every ordered event from tests/model_consensus.py on the oracle's
    tables, once per case — a superset of model_check's sample (tests/test_gpu_consensus.py) and of the events whose consensus
    time equals another's in their round"""
    if name not in _model:
        case, stream, stake, crafted, run, o, sec = oracle_of(name)
        cr, sp, op, t, sig = stream
        lists = {}
        tx = run.transactions
        rr, ct = mc.consensus_values(tx, sorted(run.new_c[0]), o.can_see, o.witnesses(), o.famous_table(), cr, sp, o.height, t,
                                     np.ones(case.n, np.int64), lists)
        _model[name] = (rr, ct, lists)
    return _model[name]


@pytest.mark.parametrize("bulk", ["default", "1", "0"])   # k_order_median (default / always the table), k_order_times (the searches)
@pytest.mark.parametrize("name", ["n130_q16", "n130_q64", "n300_q16", "n300_q64"])
def test_medians_over_duplicate_heavy_samples(pkg, name, bulk, monkeypatch):
    """more than 64 samples per event (4 and 8 mask words) with runs of q equal values: wave_pseudo_median's selection loop,
    its branch k1 < c_le with the second value taken from the pivot's successor, runs that straddle the two middle positions"""
    set_bulk(monkeypatch, bulk)
    case, stream, stake, crafted, run, o, sec = oracle_of(name)
    m_rr, m_ct, lists = model_of(name)
    tx = run.transactions
    # conditions on the input, from the model's own sample lists
    long_dup, split = median_conditions(lists, tx.tolist())
    assert len(long_dup) >= 1 and len(split) >= 1 and max(len(s) for s in lists.values()) > 64
    key = np.stack([m_rr.astype(np.float64), m_ct], 1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    shared = cnt[inv.reshape(-1)] > 1
    assert shared.sum() >= 256, "events whose consensus time equals another's in their round"
    h = pkg.Hashgraph(case.n, stake)
    t0 = time.time()
    ordered, tied, sizes = drive(h, T.calls_of(case), stream, run)
    print("\n[%s bulk=%s] %d ordered, %d share their time inside the round, %d rounds ordered, %d tied, oracle %.2f s, device pass %.2f s"
          % (name, bulk, len(tx), int(shared.sum()), len(ordered), len(tied), sec, time.time() - t0))
    rr, ct = h.round_received(), h.consensus_time()
    assert np.array_equal(rr[tx], m_rr), "round received"
    bad = np.flatnonzero(ct[tx].view(np.uint64) != m_ct.view(np.uint64))
    assert len(bad) == 0, "consensus time of %d events, first: event %d, %r for %r over %d samples" % (
        len(bad), tx[bad[0]], ct[tx[bad[0]]], m_ct[bad[0]], len(lists[int(tx[bad[0]])]))
    assert len(tied) == len(ordered) > 0
    check_end(h, run)
    check_export_agrees(h, tx)
    h.close()
