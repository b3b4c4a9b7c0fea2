"""GPU (-m gpu): the id index and the payload ingest by event id (sw_set_event_ids, sw_lookup_event_ids,
sw_ingest_payload[_device]; csrc/resolve.hip.h).  A payload arrives shuffled, with ids the context knows and invalid
events among it: index_out and n_stored must equal tests/model_payload.py exactly, and the context afterwards —
mapped through the ids — the oracle's on the original order.

No torch here (see tests/test_gpu_ingest_device.py): device buffers come through ctypes from the HIP runtime the
library is linked against."""
import ctypes as C

import numpy as np
import pytest

import model_payload as mp

pytestmark = pytest.mark.gpu

H2D, D2H = 1, 2


class Hip:
    def __init__(self, pkg):
        L = C.CDLL(pkg.LIB_PATH)
        self.L = L
        L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.hipFree.argtypes = [C.c_void_p]
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.bufs = []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.L.hipMalloc(C.byref(p), max(int(nbytes), 16)) == 0
        self.bufs.append(p)
        return p.value

    def up(self, a, dtype, offset=0):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype)
        p = self.alloc(a.nbytes + offset) + offset
        assert self.L.hipMemcpy(C.c_void_p(p), a.ctypes.data_as(C.c_void_p), a.nbytes, H2D) == 0
        return p

    def down(self, p, n, dtype):
        out = np.empty(n, dtype)
        assert self.L.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.nbytes, D2H) == 0
        return out

    def free(self):
        for p in self.bufs:
            self.L.hipFree(p)
        self.bufs = []


@pytest.fixture
def hip(pkg):
    h = Hip(pkg)
    yield h
    h.free()


def dev_ingest(h, hip, events, t=None, sig=None, with_ok=True):
    """events (model tuples) through ingest_payload_device; returns (index_out, n_stored)."""
    ids, spi, opi, ar, cr, ok = mp.to_arrays(events)
    K = len(events)
    d_out = hip.alloc(4 * K)
    try:
        _, n_stored = h.ingest_payload_device(hip.up(ids, np.uint8), hip.up(spi, np.uint8), hip.up(opi, np.uint8), hip.up(ar, np.uint8),
                                              hip.up(cr, np.int32), hip.up(ok, np.uint8) if with_ok else None, hip.up(t, np.float64),
                                              hip.up(sig, np.uint8), index_out=d_out, count=K)
        return hip.down(d_out, K, np.int32), n_stored
    finally:
        hip.free()


def host_ingest(h, hip, events, t=None, sig=None, with_ok=True):
    ids, spi, opi, ar, cr, ok = mp.to_arrays(events)
    return h.ingest_payload(ids, spi, opi, ar, cr, ok if with_ok else None, t, sig)


def ids_array(keys):
    return np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), 32)


def _oracle_run(n, stream):
    from oracle.oracle import Oracle
    o = Oracle(n)
    o.append_events(*stream)
    N = len(stream[0])
    o.divide_rounds(0, N)
    nco = list(o.decide_fame())
    return o, nco, list(o.find_order(nco))


def finish(h, N):
    h.divide_rounds(0, N)
    nc = list(h.decide_fame())
    return nc, list(h.find_order(nc))


def assert_equals_oracle(h, n, stream, dense_of, rows=None):
    """Every view of `h`, whose event k of the stream has dense index dense_of[k], equals the oracle's on the stream."""
    N = len(stream[0])
    o, nco, txo = _oracle_run(n, stream)
    nc, tx = finish(h, N)
    assert nc == nco
    assert tx == [int(dense_of[k]) for k in txo], "transaction order"
    relabel = lambda a: np.where(a >= 0, dense_of[np.maximum(a, 0)], -1)
    assert np.array_equal(h.rounds()[dense_of], o.round), "rounds"
    assert np.array_equal(h.heights()[dense_of], o.height), "heights"
    wit = h.witnesses()
    ow = o.witnesses()
    assert np.array_equal(wit, relabel(ow)), "witnesses"
    m = ow >= 0
    assert np.array_equal(h.famous()[m], o.famous_by_event[ow[m]]), "famous"
    assert np.array_equal(h.consensus(), np.isin(np.arange(wit.shape[0]), nco).astype(np.uint8)), "consensus"
    rows = np.arange(0, N, max(1, N // 400)) if rows is None else rows
    ocs = o.can_see
    for k in rows:
        assert np.array_equal(h.can_see(int(dense_of[k]), 1)[0], relabel(ocs[k])), "can_see row of event %d" % k


def ingest_chunks(pkg, hip, n, stream, cuts, seed, route, extra_known=0):
    """The stream cut at `cuts`, every chunk shuffled (plus `extra_known` ids the context has already), through `route`;
    index_out and n_stored are checked against the model.  Returns (context, dense_of, waves per chunk)."""
    cr, sp, op, t, sig = stream
    N = len(cr)
    rng = np.random.default_rng(seed)
    h = pkg.Hashgraph(n)
    index = mp.Index(n)
    dense_of = np.full(N, -1, np.int64)
    waves = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        extra = rng.choice(a, min(a, extra_known), replace=False).tolist() if a else []
        idx = rng.permutation(np.array(list(range(a, b)) + extra, np.int64))
        events = mp.from_stream(cr, sp, op, idx.tolist())
        exp_out, order, w, _ = mp.ingest(index, events)
        out, n_stored = route(h, hip, events, t[idx], sig[idx])
        assert n_stored == len(order) == b - a
        assert np.array_equal(out, exp_out), "index_out of chunk [%d, %d)" % (a, b)
        assert h.payload_stats()["waves"] == w and h.num_events == b
        dense_of[idx] = out
        waves.append(w)
    assert sorted(dense_of.tolist()) == list(range(N))
    # the ids the context holds are the stream's, in dense order
    got = h.event_ids()
    assert got.shape == (N, 32) and bytes(got[int(dense_of[N - 1])]) == mp.event_id(N - 1) and bytes(got[int(dense_of[0])]) == mp.event_id(0)
    return h, dense_of, waves


def test_permutation_invariance_against_the_oracle(pkg, hip):
    """Four prefix-closed chunks, each permuted.  The 2 000-event chunk comes LAST: only behind 38 000 stored events is a
    chunk not bulk-sized (8 K < events stored), and one chunk must take the append's host fallback."""
    n, N = 64, 40_000
    stream = pkg.synth_hashgraph(n, N, 611)
    cuts = [0, 9_000, 21_000, 38_000, N]
    h, dense_of, waves = ingest_chunks(pkg, hip, n, stream, cuts, 1, dev_ingest, extra_known=50)
    st = h.ingest_stats()
    assert st["device_batches"] == 3 and st["fallback_batches"] == 1, st   # a run that fell back throughout proves nothing
    assert h.payload_stats()["table_rebuilds"] >= 3                       # 2 x 9 000, 2 x 21 000, 2 x 38 000 slots needed
    assert_equals_oracle(h, n, stream, dense_of)
    h.close()


def test_deep_payload_needs_a_second_sort_pass(pkg, hip):
    n, K = 4, 8192
    stream = pkg.synth_hashgraph(n, K, 612)
    h, dense_of, waves = ingest_chunks(pkg, hip, n, stream, [0, K], 2, dev_ingest)
    assert waves[0] > 1024, waves          # the wave key does not fit the 10 bits of one pass
    assert h.ingest_stats()["device_batches"] == 1
    assert_equals_oracle(h, n, stream, dense_of)
    h.close()


def test_members_not_a_multiple_of_64_through_the_host_wrapper(pkg, hip):
    n, N = 300, 20_000
    stream = pkg.synth_hashgraph(n, N, 613)
    h, dense_of, _ = ingest_chunks(pkg, hip, n, stream, [0, 8_500, N], 3, host_ingest, extra_known=30)
    assert h.ingest_stats()["device_batches"] == 2
    ref = pkg.Hashgraph(n)
    ref.append_events(*stream)
    assert finish(ref, N)[0] == finish(h, N)[0]
    assert np.array_equal(h.rounds()[dense_of], ref.rounds()) and np.array_equal(h.heights()[dense_of], ref.heights())
    rw = ref.witnesses()
    assert np.array_equal(h.witnesses(), np.where(rw >= 0, dense_of[np.maximum(rw, 0)], -1))
    assert np.array_equal(h.famous(), ref.famous()) and np.array_equal(h.consensus(), ref.consensus())
    assert [int(x) for x in h.transactions()] == [int(dense_of[k]) for k in ref.transactions()]
    for k in range(0, N, 997):
        row = ref.can_see(k, 1)[0]
        assert np.array_equal(h.can_see(int(dense_of[k]), 1)[0], np.where(row >= 0, dense_of[np.maximum(row, 0)], -1))
    h.close()
    ref.close()


def _with_known_prefix(pkg, n, stream, known):
    cr, sp, op, t, sig = stream
    h = pkg.Hashgraph(n)
    h.append_events(cr[:known], sp[:known], op[:known], t[:known], sig[:known])
    index = mp.Index(n)
    for k in range(known):
        index.add(mp.event_id(k), cr[k])
    return h, index


def test_rejects(pkg, hip):
    n, N, known = 8, 300, 60
    stream = cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, 614)
    h, index = _with_known_prefix(pkg, n, stream, known)
    h.set_event_ids(0, ids_array(index.ids))
    events, expect = mp.reject_payload(cr, sp, op, n, known, 4)
    assert set(expect.values()) == {-2, -3, -4, -5, -6, -7, -8}
    exp_out, order, _, parents = mp.ingest(index, events)
    K = len(events)
    tt, ss = np.arange(K, dtype=np.float64) + 1000.0, np.random.default_rng(9).integers(0, 256, (K, 64), dtype=np.uint8)
    out, n_stored = dev_ingest(h, hip, events, tt, ss)
    assert np.array_equal(out, exp_out), [(i, int(out[i]), int(exp_out[i])) for i in np.flatnonzero(out != exp_out)]
    for pos, code in expect.items():
        assert out[pos] == code
    assert n_stored == len(order) == N - known and h.num_events == N
    # the context equals one fed only the accepted events, in dense order, through sw_append_events
    ref = pkg.Hashgraph(n)
    ref.append_events(cr[:known], sp[:known], op[:known], t[:known], sig[:known])
    ref.append_events(np.array([events[i][2] for i in order], np.int32), np.array([parents[i][0] for i in order], np.int32),
                      np.array([parents[i][1] for i in order], np.int32), tt[order], ss[order])
    assert finish(h, N) == finish(ref, N)
    assert np.array_equal(h.heights(), ref.heights()) and np.array_equal(h.rounds(), ref.rounds())
    assert np.array_equal(h.can_see(), ref.can_see()) and np.array_equal(h.witnesses(), ref.witnesses())
    assert np.array_equal(h.famous(), ref.famous())
    assert [bytes(x) for x in h.event_ids()] == index.ids
    h.close()
    ref.close()


def test_ids_that_share_their_hash_word(pkg, hip):
    """200 stored and 100 arriving events whose ids come in groups of 8 with the same first 8 bytes (the word the table
    hashes): every one resolves."""
    n, N, known = 8, 300, 200
    stream = cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, 615)
    crafted = lambda k: mp.event_id(k // 8)[:8] + mp.event_id(1_000_000 + k)[8:]
    assert len({crafted(k) for k in range(N)}) == N and len({crafted(k)[:8] for k in range(N)}) == (N + 7) // 8
    h, _ = _with_known_prefix(pkg, n, stream, known)
    index = mp.Index(n)
    for k in range(known):
        index.add(crafted(k), cr[k])
    h.set_event_ids(0, ids_array(index.ids))
    rng = np.random.default_rng(6)
    probe = rng.permutation(N)
    got = h.lookup_event_ids(ids_array([crafted(int(k)) for k in probe]))
    assert np.array_equal(got, np.where(probe < known, probe, -1))
    idx = rng.permutation(np.arange(known, N)).tolist()
    events = mp.from_stream(cr, sp, op, idx, id_of=crafted)
    exp_out, order, _, _ = mp.ingest(index, events)
    out, n_stored = dev_ingest(h, hip, events, with_ok=False)
    assert np.array_equal(out, exp_out) and n_stored == N - known == len(order)
    assert np.array_equal(h.lookup_event_ids(ids_array(index.ids)), np.arange(N))
    h.close()


def test_index_rules(pkg, hip):
    n, N, known = 8, 400, 100
    stream = cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, 616)
    h, index = _with_known_prefix(pkg, n, stream, known)
    events = mp.from_stream(cr, sp, op, list(range(N - 1, known - 1, -1)))
    # events but no ids: the index is not complete
    with pytest.raises(pkg.SwirldHipError) as ei:
        dev_ingest(h, hip, events)
    assert ei.value.code == -95 and h.num_events == known
    with pytest.raises(pkg.SwirldHipError) as ei:
        host_ingest(h, hip, events)
    assert ei.value.code == -95 and h.num_events == known
    # a duplicate inside the call, nothing stored; ids must continue where they end
    ids = ids_array(index.ids)
    bad = ids.copy()
    bad[70] = bad[3]
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.set_event_ids(0, bad)
    assert ei.value.code == -22
    assert np.array_equal(h.lookup_event_ids(ids[:10]), np.full(10, -1))
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.set_event_ids(5, ids[5:])
    assert ei.value.code == -22
    h.set_event_ids(0, ids[:40])
    with pytest.raises(pkg.SwirldHipError) as ei:      # an id that is present already
        h.set_event_ids(40, np.concatenate([ids[40:99], ids[7:8]]))
    assert ei.value.code == -22
    assert np.array_equal(h.lookup_event_ids(ids), np.where(np.arange(known) < 40, np.arange(known), -1))
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.event_ids(0, 41)
    assert ei.value.code == -34
    with pytest.raises(pkg.SwirldHipError) as ei:      # beyond the stored events
        h.set_event_ids(40, np.concatenate([ids[40:], ids_array([mp.event_id(known)])]))
    assert ei.value.code == -34
    h.set_event_ids(40, ids[40:])
    assert np.array_equal(h.event_ids(), ids)
    # pointer checks of the device call: a misaligned id array, a host pointer
    a_ids, a_sp, a_op, a_ar, a_cr, a_ok = mp.to_arrays(events)
    K = len(events)
    d = dict(ids=hip.up(a_ids, np.uint8), sp=hip.up(a_sp, np.uint8), op=hip.up(a_op, np.uint8), ar=hip.up(a_ar, np.uint8), cr=hip.up(a_cr, np.int32))
    d_out = hip.alloc(4 * K)
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.ingest_payload_device(hip.up(a_ids, np.uint8, offset=4), d["sp"], d["op"], d["ar"], d["cr"], index_out=d_out, count=K)
    assert ei.value.code == -22 and "aligned" in str(ei.value)
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.ingest_payload_device(d["ids"], d["sp"], a_op.ctypes.data, d["ar"], d["cr"], index_out=d_out, count=K)
    assert ei.value.code == -22 and h.num_events == known
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.ingest_payload_device(d["ids"], d["sp"], d["op"], d["ar"], d["cr"], index_out=np.empty(K, np.int32).ctypes.data, count=K)
    assert ei.value.code == -22 and h.num_events == known
    # now it works (the payload in reverse order: one event per wave at the worst)
    exp_out, order, _, _ = mp.ingest(index, events)
    _, n_stored = h.ingest_payload_device(d["ids"], d["sp"], d["op"], d["ar"], d["cr"], index_out=d_out, count=K)
    assert n_stored == N - known and np.array_equal(hip.down(d_out, K, np.int32), exp_out)
    all_ids = ids_array(index.ids)
    # events appended by index afterwards have no id: the index is incomplete until they get one
    m_cr, m_sp, m_op, m_t, m_sig = (x[N:] for x in pkg.synth_hashgraph(n, N + 50, 616))    # (the same stream, 50 events longer)
    dense_of = np.arange(N + 50)
    dense_of[np.arange(N - 1, known - 1, -1)] = exp_out
    h.append_events(m_cr, dense_of[m_sp], dense_of[m_op], m_t, m_sig)
    with pytest.raises(pkg.SwirldHipError) as ei:
        host_ingest(h, hip, events)
    assert ei.value.code == -95
    h.set_event_ids(N, ids_array([mp.event_id(k) for k in range(N, N + 50)]))
    out, n_stored = host_ingest(h, hip, events)
    assert n_stored == 0 and np.array_equal(out, exp_out)   # every id known: the index it got then
    # rewind keeps the ids, reset forgets them
    h.divide_rounds(0, N + 50)
    h.rewind()
    assert np.array_equal(h.event_ids(0, N), all_ids) and np.array_equal(h.lookup_event_ids(all_ids), np.arange(N))
    h.reset()
    assert h.num_events == 0
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.event_ids(0, 1)
    assert ei.value.code == -34
    assert np.array_equal(h.lookup_event_ids(all_ids[:50]), np.full(50, -1))
    # ... and an empty context counts as complete
    whole = mp.from_stream(cr, sp, op, np.random.default_rng(1).permutation(N).tolist())
    exp_out, order, _, _ = mp.ingest(mp.Index(n), whole)
    out, n_stored = host_ingest(h, hip, whole)
    assert n_stored == N and np.array_equal(out, exp_out)
    h.close()


def test_forks(pkg, hip):
    n, N = 8, 400
    cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, 617)
    f_sp = sp.copy()
    known = 50
    j = int(np.nonzero(cr[known:] == cr[n + 5])[0][3]) + known    # an event of the payload, deep enough in its creator's chain
    assert sp[sp[j]] >= 0
    f_sp[j] = sp[sp[j]]                       # event j forks: its self-parent is its creator's event before the last
    idx = np.random.default_rng(2).permutation(np.arange(known, N)).tolist()
    events = mp.from_stream(cr, f_sp, op, idx)
    h = pkg.Hashgraph(n)
    h.append_events(cr[:known], sp[:known], op[:known], t[:known], sig[:known])
    index = mp.Index(n)
    for k in range(known):
        index.add(mp.event_id(k), cr[k])
    h.set_event_ids(0, ids_array(index.ids))
    h.set_forks(False)
    with pytest.raises(pkg.SwirldHipError) as ei:
        dev_ingest(h, hip, events)
    assert ei.value.code == -95 and h.num_events == known
    assert np.array_equal(h.event_ids(), ids_array(index.ids))
    assert np.array_equal(h.lookup_event_ids(ids_array([e[0] for e in events])), np.full(len(events), -1))
    h.set_forks(True)
    exp_out, order, _, parents = mp.ingest(index, events)
    out, n_stored = dev_ingest(h, hip, events)
    assert n_stored == N - known and np.array_equal(out, exp_out) and h.exact
    ref = pkg.Hashgraph(n)
    ref.append_events(cr[:known], sp[:known], op[:known], t[:known], sig[:known])
    ref.append_events(np.array([events[i][2] for i in order], np.int32), np.array([parents[i][0] for i in order], np.int32),
                      np.array([parents[i][1] for i in order], np.int32))
    assert ref.exact
    assert finish(h, N) == finish(ref, N)
    assert np.array_equal(h.heights(), ref.heights()) and np.array_equal(h.rounds(), ref.rounds())
    h.close()
    ref.close()


def _gossip(pkg, threshold, turns=300, n_nodes=4):
    """One seeded gossip simulation (deterministic clock, keys and partner choice) with Node.device_payload_threshold set."""
    import contextlib
    import io
    import random
    from test_node_host import _run_simulation
    node_mod = pkg.node
    rng = random.Random(20261018)
    saved = (node_mod.crypto.randombytes, node_mod.time, node_mod.randrange, node_mod.Node.device_payload_threshold)
    clock = iter(range(1, 1 << 30))
    node_mod.crypto.randombytes = lambda k: bytes(rng.getrandbits(8) for _ in range(k))
    node_mod.time = lambda: 1.0e9 + 0.001 * next(clock)
    node_mod.randrange = lambda k: rng.randrange(k)
    node_mod.Node.device_payload_threshold = threshold
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return _run_simulation(pkg, n_nodes, turns, rng)
    finally:
        node_mod.crypto.randombytes, node_mod.time, node_mod.randrange, node_mod.Node.device_payload_threshold = saved


def test_node_takes_the_device_route(pkg):
    a = _gossip(pkg, 1)
    b = _gossip(pkg, None)
    assert any(nd._device_payloads > 0 for nd in a) and all(nd._device_payloads == 0 for nd in b)
    for x, y in zip(a, b):
        assert x.pk == y.pk and set(x.hg) == set(y.hg) and len(x.hg) > 100
        assert x.transactions == y.transactions and len(x.transactions) > 30
        assert {h: x.round[h] for h in x.hg} == {h: y.round[h] for h in y.hg}
        assert dict(x.famous) == dict(y.famous) and x.consensus == y.consensus
        assert x.height == y.height and x.tbd == y.tbd and x.head == y.head
        # (the node's own newest events get their ids with the next payload)
        assert x._dev_ids > 50 and [bytes(i) for i in x._dev.event_ids(0, x._dev_ids)] == x._ids[:x._dev_ids]
