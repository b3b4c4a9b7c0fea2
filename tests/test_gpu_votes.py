"""GPU (-m gpu): Node.votes read out in bulk (sw_export_votes[_device], csrc/votes.hip.h; Hashgraph.export_votes /
votes_triples, Node.votes, DeviceNetwork.votes) against the reference's complete `votes` dict of every fork-free golden,
against the CPU oracle on wide masks and on a windowed context, and against sw_get_vote on the same context; the range and
capacity protocol, the device form, the refusals, and the C-ABI from plain C.

No torch here (see tests/test_gpu_export.py): device buffers come through ctypes from the HIP runtime the library is linked
against."""
import contextlib
import ctypes as C
import io
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_names, load_golden
from test_gpu_export import Hip
from test_gpu_parity import hip_run, oracle_run, run_schedule

pytestmark = pytest.mark.gpu

FORKFREE = [n for n in golden_names() if "forks" not in n]


@pytest.fixture
def hip(pkg):
    h = Hip(pkg)
    yield h
    h.free()


def as_set(tr):
    return set(map(tuple, np.asarray(tr).tolist()))


def check_table(h, table):
    """rows sorted by (round(y), y, rc), one row per key, value inside exists, no empty row"""
    row_voter, row_cand, exists, value = table
    assert not (value & ~exists).any()
    assert exists.any(axis=1).all(), "a row has at least one entry"
    rnd = h.rounds()
    keys = list(zip(rnd[row_voter].tolist(), row_voter.tolist(), row_cand.tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert (row_cand < rnd[row_voter]).all()


def entries(table):
    return int(np.unpackbits(np.ascontiguousarray(table[2]).view(np.uint8)).sum())


# ---- 1. every fork-free golden with its recorded schedule, exhaustively -----------------------------------------------------
@pytest.mark.parametrize("name", FORKFREE)
def test_votes_table_equals_the_reference_golden(pkg, name):
    g = load_golden(name)
    h = pkg.Hashgraph(g["n"], g["stake"])
    run_schedule(h, g)
    table = h.export_votes()
    check_table(h, table)
    tr = h.votes_triples()
    exp = as_set(g["votes"])
    assert len(tr) == len(exp) == len(g["votes"]) == entries(table)
    assert as_set(tr) == exp
    st = h.votes_stats()
    assert st["entries"] == 2 * len(exp) and (st["calls"] == 2 and st["levels"] > 0 or not len(exp))
    h.close()


# ---- 2. wide masks against the oracle, and against sw_get_vote on the same context ------------------------------------------
def lookup(h, table):
    """(y, x) -> -1 / 0 / 1 from the table"""
    row_voter, row_cand, exists, value = table
    rows = {(int(y), int(rc)): i for i, (y, rc) in enumerate(zip(row_voter, row_cand))}
    rnd, cr = h.rounds(), None

    def at(y, x, creator):
        i = rows.get((int(y), int(rnd[x])))
        if i is None:
            return -1
        mc = int(creator[x])
        if not (int(exists[i, mc >> 6]) >> (mc & 63)) & 1:
            return -1
        return (int(value[i, mc >> 6]) >> (mc & 63)) & 1
    return at


def sample_pairs(wit, triples, rng, n_random, n_present, rv_from=1):
    R, n = wit.shape
    pairs = []
    while len(pairs) < n_random:
        rv = int(rng.integers(rv_from, R)); rc = int(rng.integers(0, rv))
        y, x = wit[rv, int(rng.integers(0, n))], wit[rc, int(rng.integers(0, n))]
        if y >= 0 and x >= 0:
            pairs.append((int(y), int(x)))
    if len(triples):
        pick = rng.choice(len(triples), min(n_present, len(triples)), replace=False)
        pairs += [(int(y), int(x)) for y, x, _ in triples[pick]]
    return pairs


@pytest.mark.parametrize("n,N,seed,mode,p0,p1,chunk", [(256, 40000, 3, 0, 0, 0, None), (300, 40000, 45, 2, 0.35, 0.02, 9000),
                                                      (520, 40000, 46, 2, 0.4, 0.02, None)])
def test_wide_masks_against_the_oracle(pkg, n, N, seed, mode, p0, p1, chunk):
    stream = pkg.synth_hashgraph(n, N, seed, mode, p0, p1)
    o, _ = oracle_run(n, stream, chunk=chunk)
    h, _ = hip_run(pkg, n, stream, chunk=chunk)
    table = h.export_votes()
    check_table(h, table)
    tr = h.votes_triples()
    assert len(tr) == o.num_votes == entries(table)
    at = lookup(h, table)
    cr, rnd, wit = stream[0], h.rounds(), h.witnesses()
    rng = np.random.default_rng(seed)
    pairs = sample_pairs(wit, tr, rng, 20000, 5000)
    present = 0
    for y, x in pairs:
        got = at(y, x, cr)
        assert got == o.vote(y, x), "votes[%d][%d]" % (y, x)
        present += got >= 0
    assert present >= min(5000, len(tr))
    for y, x in pairs[:1000] + pairs[-1000:]:
        assert at(y, x, cr) == h.vote(int(rnd[y]), int(cr[y]), int(rnd[x]), int(cr[x]))
    h.close()


# ---- 3. ranges and capacity ---------------------------------------------------------------------------------------------------
def test_ranges_and_capacity(pkg):
    g = load_golden("n16_s4_chunk50")
    h = pkg.Hashgraph(g["n"], g["stake"])
    run_schedule(h, g)
    R = h.max_round + 1
    whole = h.export_votes(1, R)
    assert len(whole[0]) > 100
    parts = [h.export_votes(r, r + 1) for r in range(R)]
    for k in range(4):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k])
    assert np.array_equal(h.export_votes(0, R)[2], whole[2]), "round 0 holds no voter"
    K, nwo = len(whole[0]), whole[2].shape[1]
    n_rows, n_entries = C.c_int64(-1), C.c_int64(-1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    arrays = [np.full(K, 0x5A5A5A5A, np.int32), np.full(K, 0x5A5A5A5A, np.int32), np.full((K, nwo), 0x5A5A5A5A5A5A5A5A, np.uint64),
              np.full((K, nwo), 0x5A5A5A5A5A5A5A5A, np.uint64)]
    before = [a.copy() for a in arrays]
    rc = h._L.sw_export_votes(h._h, 1, R, K - 1, *[p(a) for a in arrays], C.byref(n_rows), C.byref(n_entries))
    assert rc == -34 and n_rows.value == K and n_entries.value == len(g["votes"])
    assert all(np.array_equal(a, b) for a, b in zip(arrays, before)), "a refused call writes no array"
    rc = h._L.sw_export_votes(h._h, 1, R, 0, None, None, None, None, C.byref(n_rows), C.byref(n_entries))
    assert rc == -34 and n_rows.value == K, "capacity 0 is the size query"
    assert h._L.sw_export_votes(h._h, 1, R, K, *[p(a) for a in arrays], C.byref(n_rows), C.byref(n_entries)) == 0
    assert all(np.array_equal(a, b) for a, b in zip(arrays, whole))
    for a, b in ((3, 3), (5, 2), (R, R)):
        t = h.export_votes(a, b)
        assert len(t[0]) == 0 and t[2].shape == (0, nwo)
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.export_votes(1, R + 1)
    assert ei.value.code == -34
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.export_votes(-1, R)
    assert ei.value.code == -34
    assert np.array_equal(h.export_votes(1, R)[3], whole[3])
    h.close()


# ---- 4. the device form -------------------------------------------------------------------------------------------------------
def test_device_form_equals_the_host_form(pkg, hip):
    g = load_golden("n70_s3_batch")
    h = pkg.Hashgraph(g["n"], g["stake"])
    run_schedule(h, g)
    whole = h.export_votes()
    K, nwo = len(whole[0]), whole[2].shape[1]
    assert nwo == 2 and K > 0
    assert h.export_votes_device(1, h.max_round + 1, 0) == (K, len(g["votes"]))
    cap = K + 3
    d = [hip.alloc(cap * 4), hip.alloc(cap * 4), hip.alloc(cap * nwo * 8), hip.alloc(cap * nwo * 8)]
    for q, nb in zip(d, (cap * 4, cap * 4, cap * nwo * 8, cap * nwo * 8)):
        hip.fill(q, 0x5A, nb)
    stream = C.c_void_p()
    hip.L.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.L.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.L.hipStreamDestroy.argtypes = [C.c_void_p]
    assert hip.L.hipStreamCreate(C.byref(stream)) == 0
    try:
        assert h.export_votes_device(1, h.max_round + 1, cap, *d, stream=stream.value) == (K, len(g["votes"]))
        assert hip.L.hipStreamSynchronize(stream) == 0, "the caller's stream waits for the table"
        got = [hip.down(d[0], cap, np.int32), hip.down(d[1], cap, np.int32), hip.down(d[2], cap * nwo, np.uint64).reshape(cap, nwo),
               hip.down(d[3], cap * nwo, np.uint64).reshape(cap, nwo)]
        for a, b in zip(got, whole):
            assert np.array_equal(a[:K], b)
            assert (a[K:].view(np.uint8) == 0x5A).all(), "nothing behind the rows"
        # too small: refused, nothing written
        hip.fill(d[2], 0x33, cap * nwo * 8)
        with pytest.raises(pkg.SwirldHipError) as ei:
            h.export_votes_device(1, h.max_round + 1, K - 1, *d, stream=stream.value)
        assert ei.value.code == -34
        assert hip.L.hipStreamSynchronize(stream) == 0
        assert (hip.down(d[2], cap * nwo, np.uint64).view(np.uint8) == 0x33).all()
        # a misaligned mask array, a host pointer
        with pytest.raises(pkg.SwirldHipError) as ei:
            h.export_votes_device(1, h.max_round + 1, K, d[0], d[1], d[2] + 8, d[3], stream=stream.value)
        assert ei.value.code == -22
        host = np.zeros((cap, nwo), np.uint64)
        with pytest.raises(pkg.SwirldHipError) as ei:
            h.export_votes_device(1, h.max_round + 1, K, d[0], d[1], host.ctypes.data, d[3], stream=stream.value)
        assert ei.value.code == -22
        assert np.array_equal(h.export_votes()[3], whole[3])
    finally:
        hip.L.hipStreamDestroy(stream)
    h.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(pkg):
    g = load_golden("n8_s11_forks")
    h = pkg.Hashgraph(g["n"])
    run_schedule(h, g)
    assert h.exact
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.export_votes()
    assert ei.value.code == -95
    assert np.array_equal(h.rounds(), g["round"])
    h.close()
    # after sw_commit_fame
    n, N = 16, 4000
    stream = pkg.synth_hashgraph(n, N, 9)
    h = pkg.Hashgraph(n)
    h.append_events(*stream)
    h.divide_rounds(0, N)
    fam, dec = h.decide_fame_partial(0, 1)
    h.commit_fame(fam, dec)
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.export_votes()
    assert ei.value.code == -95
    ref, _ = hip_run(pkg, n, stream)
    assert np.array_equal(h.famous(), ref.famous())
    h.close()
    # rounds decide_fame has not seen
    h = pkg.Hashgraph(n)
    half = N // 2
    cr, sp, op, t, sig = stream
    h.append_events(cr[:half], sp[:half], op[:half], t[:half], sig[:half])
    h.divide_rounds(0, half)
    with pytest.raises(pkg.SwirldHipError) as ei:     # no decide_fame yet
        h.export_votes()
    assert ei.value.code == -22
    h.decide_fame()
    seen = h.max_round + 1
    first = h.export_votes(1, seen)
    h.append_events(cr[half:], sp[half:], op[half:], t[half:], sig[half:])
    h.divide_rounds(half, N - half)
    assert h.max_round + 1 > seen
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.export_votes()
    assert ei.value.code == -22
    again = h.export_votes(1, seen)
    assert all(np.array_equal(a, b) for a, b in zip(first, again)), "the rounds it has seen are served, unchanged"
    before = as_set(h.votes_triples(1, seen))
    h.decide_fame()
    after = as_set(h.votes_triples())
    assert after > before, "a later call adds entries and removes none"
    h.close()
    ref.close()


# ---- 6. a windowed context ------------------------------------------------------------------------------------------------------
def test_windowed_context_is_served(pkg):
    from oracle.oracle import Oracle
    n, N, chunk = 24, 150_000, 3_000
    cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, 701, 2, 0.25, 0.2)
    o, h = Oracle(n), pkg.Hashgraph(n)
    h.set_window(True, chunk_mb=2)
    for a in range(0, N, chunk):
        b = min(N, a + chunk)
        for d in (o, h):
            d.append_events(cr[a:b], sp[a:b], op[a:b], t[a:b], sig[a:b])
            d.divide_rounds(a, b - a)
        nco, nch = list(o.decide_fame()), list(h.decide_fame())
        assert nco == nch
        assert list(h.find_order(nch)) == list(o.find_order(nco))   # (rows are evicted behind the ordered events)
    first, _, evictions = h.window()
    assert evictions > 3 and first > N // 2, "most can_see rows are evicted"
    R = h.max_round + 1
    table = h.export_votes(R - 6, R)
    check_table(h, table)
    tr = h.votes_triples(R - 6, R)
    assert len(tr) > 0
    at = lookup(h, table)
    wit = h.witnesses()
    rng = np.random.default_rng(6)
    for y, x in sample_pairs(wit, tr, rng, 20000, 5000, rv_from=R - 6):
        assert at(y, x, cr) == o.vote(y, x), "votes[%d][%d]" % (y, x)
    h.close()


# ---- 7. Node and DeviceNetwork ----------------------------------------------------------------------------------------------------
def seeded_nodes(pkg, n, turns, seed):
    """pkg.test(n, turns) with seeded keys and a deterministic clock; -> (nodes, {id(node): batch sizes})"""
    node_mod = pkg.node
    sched = {}
    orig = node_mod.Node.divide_rounds

    def recording(self, events):
        events = tuple(events)
        sched.setdefault(id(self), []).append(len(events))
        return orig(self, events)

    rng = random.Random(seed)
    clock = iter(range(1, 1 << 30))
    saved = (node_mod.crypto.randombytes, node_mod.time)
    node_mod.crypto.randombytes = lambda k: bytes(rng.getrandbits(8) for _ in range(k))
    node_mod.time = lambda: 1.0e9 + 0.001 * next(clock)
    node_mod.Node.divide_rounds = recording
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            nodes = pkg.test(n, turns)
    finally:
        node_mod.Node.divide_rounds = orig
        node_mod.crypto.randombytes, node_mod.time = saved
    return nodes, sched


def test_node_votes_take_the_bulk_route(pkg):
    """The simulation of tests/golden/node/sim_4_250_11 (4 nodes, 250 turns, seed 11) with the voting on the GPU.  The node
    goldens record no votes, so the truth is the CPU oracle fed each node's own call schedule, as tests/test_gpu_node.py
    does — here for EVERY (voter, candidate) pair."""
    from oracle.oracle import Oracle
    nodes, sched = seeded_nodes(pkg, 4, 250, 11)
    total = 0
    for nd in nodes:
        ids, N, index = nd._ids, len(nd._ids), nd._index
        cr = np.array([nd._mindex[nd.hg[h].c] for h in ids], np.int32)
        sp = np.array([index[nd.hg[h].p[0]] if nd.hg[h].p else -1 for h in ids], np.int32)
        op = np.array([index[nd.hg[h].p[1]] if nd.hg[h].p else -1 for h in ids], np.int32)
        t = np.array([nd.hg[h].t for h in ids], np.float64)
        sig = np.frombuffer(b"".join(nd.hg[h].s for h in ids), np.uint8).reshape(N, 64)
        o, a = Oracle(4), 0
        for i, k in enumerate(sched[id(nd)]):
            o.append_events(cr[a:a + k], sp[a:a + k], op[a:a + k], t[a:a + k], sig[a:a + k])
            o.divide_rounds(a, k)
            if i > 0:
                o.decide_fame()
            a += k
        wit = o.witnesses()
        slots = [int(e) for e in wit[wit >= 0]]
        exp = {}
        for y in slots:
            d = {ids[x]: bool(v) for x in slots if o.round[x] < o.round[y] for v in [o.vote(y, x)] if v >= 0}
            if o.round[y] >= 1:
                exp[ids[y]] = d
        calls0 = nd._dev.votes_stats()["calls"]
        got = {y: dict(nd.votes[y]) for y in nd.votes}
        assert got == exp
        assert sum(len(d) for d in got.values()) == o.num_votes
        voter_rounds = wit.shape[0] - 1
        assert 0 < nd._dev.votes_stats()["calls"] - calls0 <= voter_rounds, "at most one export per voter round"
        # the order of one voter's keys: candidate rounds ascending, registration order inside a round
        y = max(got, key=lambda k: len(got[k]))
        keys = [index[x] for x in nd.votes[y]]
        assert keys == sorted(keys, key=lambda e: (o.round[e], e)) and len(nd.votes[y]) == len(keys)
        x = ids[keys[0]]
        assert nd.votes[y][x] == got[y][x]
        total += o.num_votes
    assert total > 100   # (which simulation runs depends on the process's hash seed: swirld.py:323 walks a set of keys)


def test_device_network_votes_equal_the_node_simulation(pkg):
    from test_gpu_turn import node_simulation
    n, turns = 4, 60
    seeds = [bytes([70 + n, m]) + bytes(30) for m in range(n)]
    payloads = lambda k: None if k % 2 == 0 else b"tx %d" % k   # noqa: E731
    nodes = node_simulation(pkg, seeds, turns, 20261020, payloads)
    rng = random.Random(20261020)
    clock = iter(range(1, 1 << 30))
    tick = lambda: 1.0e9 + 0.001 * next(clock)   # noqa: E731
    ev = pkg.node.Event
    net = pkg.DeviceNetwork(seeds, event_class=(ev.__module__, ev.__qualname__), clock=tick)
    net.run(turns, rng.randrange, tick, payloads)
    entries = 0
    for i, nd in enumerate(nodes):   # (node 0 is the one the feature names; the others come for free)
        assert net.event_ids(i) == set(nd.hg)
        exp = {y: dict(nd.votes[y]) for y in nd.votes}
        exp = {y: d for y, d in exp.items() if d}
        assert net.votes(i) == exp
        entries += sum(len(d) for d in exp.values())
    assert entries > 0
    net.close()


# ---- 8. the C-ABI from plain C ------------------------------------------------------------------------------------------------
def test_plain_c_client(pkg, tmp_path):
    exe = str(tmp_path / "c_abi_votes")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi_votes.c"),
                           "-L", libdir, "-lswirld_hip", "-Wl,-rpath," + libdir, "-o", exe])
    n, N = 70, 12000
    out = subprocess.check_output([exe, str(n), str(N)], text=True).split()
    h = pkg.Hashgraph(n)
    h.append_events(*pkg.synth_hashgraph(n, N, 11))
    h.divide_rounds(0, N)
    h.decide_fame()
    table = h.export_votes()
    x = 1469598103934665603
    for a in table:
        for v in a.ravel().tolist():
            x = ((x ^ (int(v) & 0xFFFFFFFFFFFFFFFF)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert (int(out[0]), int(out[1]), int(out[2])) == (len(table[0]), entries(table), x)
    h.close()
