"""GPU (-m gpu): what a context leaves behind.  The owning types of csrc/owned.h count what the library holds in this process
(Hashgraph-independent: engine.live_resources() — bytes of device memory, bytes of pinned host memory, events, streams);
every case below reads the counts, makes its contexts, uses one subsystem, closes them and reads the counts again: they
must be equal.  Every case runs twice in one process, so that nothing made on first use hides a leak of the second run.
(The device's free memory is no measure here: other processes share it.)

4 members and a few hundred events wherever the path under test runs at that size; two cases need more: the bulk
find_order makes its side streams only for a call of more than one group (more than 1024 ordered events at the smallest
slab), and the windowed table evicts whole chunks of the address range (megabytes of 256-byte rows).

No torch here (see tests/test_gpu_export.py): device buffers come through ctypes from the HIP runtime the library is linked
against."""
import gc
import importlib

import numpy as np
import pytest

from test_exact_host import add_forks
from test_gpu_ingest_device import Hip
from test_gpu_turn import golden_universe, split
from test_gpu_walk import holder

pytestmark = pytest.mark.gpu

N_MEMBERS = 4


def live(pkg):
    return importlib.import_module("py-swirld_amd.engine").live_resources()


def leaves_nothing(pkg, body):
    gc.collect()   # (a context an earlier test dropped without close() goes now, not between two readings)
    for run in range(2):
        before = live(pkg)
        body()
        assert live(pkg) == before, "run %d" % run


def test_create_and_close(pkg):
    def body():
        before = live(pkg)
        h = pkg.Hashgraph(N_MEMBERS)
        now = live(pkg)
        # the counts see a context: its four streams, its events, its tables and read-back slots
        assert now.streams == before.streams + 4 and now.events > before.events
        assert now.device_bytes > before.device_bytes and now.pinned_bytes > before.pinned_bytes
        h.close()
    leaves_nothing(pkg, body)


def test_chunked_divide(pkg, monkeypatch):
    monkeypatch.setenv("SW_CHUNKS", "4")
    monkeypatch.setenv("SW_CHUNK_MIN", "64")
    monkeypatch.setenv("SW_HALO", "0")
    N = 600
    stream = pkg.synth_hashgraph(N_MEMBERS, N, 1)

    def body():
        h = pkg.Hashgraph(N_MEMBERS)
        h.append_events(*stream)
        h.divide_rounds(0, N)
        assert h.counters()["chunk_sweeps"] > 0, "the call was not swept in chunks: the cut tables were never made"
        h.decide_fame()
        h.close()
    leaves_nothing(pkg, body)


def test_appends_from_host_and_device(pkg):
    N = 700
    cr, sp, op, t, sig = pkg.synth_hashgraph(N_MEMBERS, N, 2)
    hip = Hip(pkg)

    def body():
        h = pkg.Hashgraph(N_MEMBERS)
        h.append_events(cr[:300], sp[:300], op[:300], t[:300], sig[:300])          # bulk (the first of a context), staged payload
        for a in range(300, 320, 5):                                                # small: one packed record per event
            h.append_events(cr[a:a + 5], sp[a:a + 5], op[a:a + 5], t[a:a + 5], sig[a:a + 5])
        try:
            args = [hip.up(x[320:], dt) for x, dt in ((cr, np.int32), (sp, np.int32), (op, np.int32), (t, np.float64), (sig, np.uint8))]
            h.append_events_device(*args, count=N - 320)
        finally:
            hip.free()
        st = h.ingest_stats()
        assert st["device_batches"] == 1 and st["fallback_batches"] == 0, st
        h.divide_rounds(0, N)
        assert h.num_events == N and h.max_round > 3
        h.close()
    leaves_nothing(pkg, body)


def test_decide_fame_and_bulk_find_order(pkg, monkeypatch):
    monkeypatch.setenv("SW_ORDER_BULK", "1")       # every call takes the first-descendant table ...
    monkeypatch.setenv("SW_ORDER_SLAB_MB", "0")    # ... in groups of the smallest slab: more than one, so on the side streams
    N = 3000
    stream = pkg.synth_hashgraph(N_MEMBERS, N, 3)

    def body():
        before = live(pkg)
        h = pkg.Hashgraph(N_MEMBERS)
        h.append_events(*stream)
        h.divide_rounds(0, N)
        new_c = h.decide_fame()
        tx = h.find_order(new_c)
        assert len(new_c) > 50 and len(tx) > 2048
        assert live(pkg).streams == before.streams + 7, "the bulk find_order did not make its three side streams"
        h.close()
    leaves_nothing(pkg, body)


def test_windowed_table_with_evictions(pkg):
    N, step = 40000, 4000
    cr, sp, op, t, sig = pkg.synth_hashgraph(N_MEMBERS, N, 4)

    def body():
        h = pkg.Hashgraph(N_MEMBERS)
        h.set_window(True, chunk_mb=1)
        for a in range(0, N, step):
            b = a + step
            h.append_events(cr[a:b], sp[a:b], op[a:b], t[a:b], sig[a:b])
            h.divide_rounds(a, step)
            h.find_order(h.decide_fame())
        first, _, evictions = h.window()
        assert evictions >= 1 and first > 0, (first, evictions)
        h.close()
    leaves_nothing(pkg, body)


def test_forked_hashgraph_with_exact_history(pkg):
    stream = add_forks(pkg.synth_hashgraph(N_MEMBERS, 400, 5), N_MEMBERS, 5, 3, start=150)
    cr, sp, op, t, sig = stream
    N = len(cr)

    def body():
        h = pkg.Hashgraph(N_MEMBERS)
        h.set_exact_history(True)
        for a in range(0, N, 100):   # (the first calls on the fast path: its votes are handed over at the first fork)
            b = min(N, a + 100)
            h.append_events(cr[a:b], sp[a:b], op[a:b], t[a:b], sig[a:b])
            h.divide_rounds(a, b - a)
            h.find_order(h.decide_fame())
        assert h.exact and h.votes_available and h.num_ordered > 0
        assert len(h.vote_entries()[0]) > 0 and len(h.round_received()) == N
        h.close()
    leaves_nothing(pkg, body)


def test_ids_data_keys_messages_and_a_gossip_turn(pkg):
    u = golden_universe(pkg, "n4_s1_batch", 43)
    assert u["n"] == N_MEMBERS
    member, dst_head, events, src_head = split(u, 200, 300)

    def body():
        # (a holder has member keys and signing keys and CREATES its events: ids, signatures and data on the device)
        src, _, _ = holder(pkg, u, events)
        a, _, _ = holder(pkg, u, list(range(200)))
        b, _, _ = holder(pkg, u, list(range(200)))
        msg = src.export_message(src_head, a.known_heights(dst_head), data=True)
        got = a.ingest_message(msg, validate=True, data=True)
        assert got is not None and got["n_stored"] >= 5 and got["n_valid"] == got["n_events"]
        r = b.gossip_turn(src, member, dst_head, src_head, 5e8, b"payload", validate=True, data_store=True)
        assert r.stage == 5 and r.n_stored >= 5 and r.new_head == 200 + r.n_stored and r.n_ordered > 0
        assert b.unpack_data(*b.get_event_data())[-1] == b"payload"
        for h in (src, a, b):
            h.close()
    leaves_nothing(pkg, body)


def test_refused_knob_leaves_nothing(pkg, monkeypatch):
    monkeypatch.setenv("SW_SKIP", "33")

    def body():
        with pytest.raises(pkg.SwirldHipError) as ei:
            pkg.Hashgraph(N_MEMBERS)
        assert ei.value.code == -22 and "SW_SKIP" in str(ei.value)
    leaves_nothing(pkg, body)
