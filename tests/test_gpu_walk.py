"""GPU (-m gpu): answering a sync by the pruned walk (sw_sync_walk, sw_export_walk[_device], sw_sync_pull_walk,
sw_get_fork_trunks; csrc/walk.hip.h), on contexts that hold forks (the exact path) and on fork-free ones (the fast path).
Every result is an integer or a byte string and must equal tests/model_walk.py exactly: the ascending list without
duplicates, the slot contents, the trunk heights; the capacity protocol and the refusals leave the context usable; with
real can_see heights the walk names the events sw_sync_diff names; two contexts that hold different siblings of one fork
exchange them through pull_from(walk=True, trunks=True) and not without the trunks; a Node simulation with an equivocator
answers every sync by the walk as its host BFS would.

No torch here (see tests/test_gpu_ingest_device.py): device buffers come through ctypes from the HIP runtime the library
is linked against."""
import contextlib
import ctypes as C
import io
import random

import numpy as np
import pytest

import model_walk as mw
from test_exact_host import add_forks
from test_gpu_export import FIELDS, WIDTH, Hip, Out, same, stream_ids

pytestmark = pytest.mark.gpu

INT32_MAX = 2**31 - 1
SHAPES = {5: 301, 33: 1203, 70: 1501, 130: 2001}      # members -> events of the base stream (no multiple of 32)


@pytest.fixture
def hip(pkg):
    h = Hip(pkg)
    yield h
    h.free()


def refused(pkg, code, fn):
    with pytest.raises(pkg.SwirldHipError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)


def context(pkg, n, stream, ids=True, divided=None):
    h = pkg.Hashgraph(n)
    h.append_events(*stream)
    N = len(stream[0])
    if ids:
        h.set_event_ids(0, stream_ids(N))
    h.divide_rounds(0, N if divided is None else divided)
    return h


_cache = {}


def graph(pkg, n, forked):
    """(stream, model graph) per shape, built once: forked = add_forks + a second root of member 1."""
    key = (n, forked)
    if key not in _cache:
        stream = pkg.synth_hashgraph(n, SHAPES[n], 900 + n)
        if forked:
            stream = mw.with_second_root(add_forks(stream, n, 950 + n, 6), 1, n)
        if len(stream[0]) % 32 == 0:
            stream = tuple(a[:-1] for a in stream)
        _cache[key] = (stream, mw.WalkGraph(n, *stream))
    return _cache[key]


def check_walk(h, g, head, known=None, cap=None):
    exp = g.walk(head, known, cap)
    got = h.sync_walk(head, known, cap)
    assert got.dtype == np.int32 and np.all(np.diff(got) > 0), "strictly ascending: no event twice"
    assert len(got) == len(exp) and np.array_equal(got, exp)
    same(h.export_walk(head, known, cap), g.slots(exp), "export_walk")
    return got


# ---- 1. the walk and the export against the model ---------------------------------------------------------------------------
@pytest.mark.parametrize("forked", [True, False])
@pytest.mark.parametrize("n", [5, 33, 70, 130])
def test_walk_and_export_equal_the_model(pkg, hip, n, forked):
    stream, g = graph(pkg, n, forked)
    N = g.N
    assert N % 32 != 0
    h = context(pkg, n, stream)
    assert h.exact == forked
    head, mid = N - 1, N // 2 + 3
    everything = check_walk(h, g, head)                                              # nobody known: every ancestor of the head
    assert len(everything) > N // 2
    assert check_walk(h, g, head, np.full(n, INT32_MAX, np.int32)).tolist() == [head]   # everything known: the head alone
    got = check_walk(h, g, mid, h.known_heights(N // 5))                             # a head in the middle, a real can_see row
    assert got[-1] == mid and len(got) > 1
    assert check_walk(h, g, 2).tolist() == [2]                                       # the head a root
    check_walk(h, g, head, h.known_heights(mid))
    check_walk(h, g, head, mw.arbitrary_heights(g, head, n))
    trunk = h.fork_trunks()
    assert np.array_equal(trunk, g.trunks())
    if forked:
        assert trunk[1] == -1 and (trunk != INT32_MAX).sum() >= 2
        known = h.known_heights(mid)
        assert len(check_walk(h, g, head, known, trunk)) > len(g.walk(head, known))
    else:
        assert (trunk == INT32_MAX).all()
        check_walk(h, g, head, h.known_heights(mid), trunk)
    # the device form: heights and cap in device memory, the arrays poisoned first
    known = mw.arbitrary_heights(g, mid, n + 1)
    exp = g.export_walk(mid, known, trunk)
    K = len(exp["event"])
    out = Out(hip, K)
    out.fill(0xA5)
    p = out.p
    dk, dc = hip.up(known, np.int32), hip.up(trunk, np.int32)
    assert h.walk_size(mid, dk, dc) == K
    assert h.export_walk_device(mid, dk, dc, K, p["ids"], p["sp_ids"], p["op_ids"], p["arity"], p["creator"], p["t"], p["sig"], p["event"]) == K
    same(out.read(K), exp, "export_walk_device")
    st = h.walk_stats()
    assert st["calls"] > 10 and st["levels"] == len(g.levels(mid, known, trunk))
    h.close()


def test_the_strict_subset_case_and_the_fast_path_cross_check(pkg):
    n, N, seed, head, hseed = mw.STRICT_CASE
    stream = pkg.synth_hashgraph(n, N, seed)
    g = mw.WalkGraph(n, *stream)
    h = context(pkg, n, stream, ids=False)          # (sync_walk needs no id index)

    def diff_set(head, known):
        first, end, tot = h.sync_diff(head, known)
        ev = [int(e) for m in range(n) for e in h.chain_events(m, int(first[m]), int(end[m]))]
        assert len(ev) == tot
        return set(ev)

    known = mw.arbitrary_heights(g, head, hseed)
    got = h.sync_walk(head, known)
    assert np.array_equal(got, g.walk(head, known))
    assert set(got.tolist()) < diff_set(head, known), "arbitrary heights: fewer events than the chain ranges"
    rng = np.random.default_rng(seed)
    for hd, asker in [(int(rng.integers(n, N)), int(rng.integers(0, N))) for _ in range(6)] + [(N - 1, 0), (N - 1, N - 1)]:
        known = h.known_heights(asker)
        got = h.sync_walk(hd, known)
        assert np.array_equal(got, g.walk(hd, known)) and set(got.tolist()) == diff_set(hd, known)
    h.close()


def test_equal_height_siblings_and_the_cap(pkg):
    """An asker height EQUAL to the height of two fork siblings: neither is sent without the cap, both with it."""
    cr = np.array([0, 1, 2, 0, 1, 1, 2, 0, 2], np.int32)
    sp = np.array([-1, -1, -1, 0, 1, 1, 2, 3, 6], np.int32)
    op = np.array([-1, -1, -1, 1, 3, 3, 4, 5, 7], np.int32)
    stream = (cr, sp, op, np.arange(9.0), (np.arange(9 * 64) % 251).astype(np.uint8).reshape(9, 64))
    g = mw.WalkGraph(3, *stream)
    h = context(pkg, 3, stream)
    assert h.exact and g.height[4] == g.height[5] == 2
    trunk = h.fork_trunks()
    assert trunk.tolist() == [INT32_MAX, 0, INT32_MAX]
    known = np.array([1, 2, 0], np.int32)
    assert check_walk(h, g, 8, known).tolist() == [6, 7, 8]
    assert check_walk(h, g, 8, known, trunk).tolist() == [4, 5, 6, 7, 8]
    h.close()


def test_a_workgroup_narrower_than_a_level(pkg, monkeypatch):
    stream, g = graph(pkg, 130, True)
    head = g.N - 1
    assert max(len(l) for l in g.levels(head)) > 64, "some level takes the stride loop"
    wide = context(pkg, 130, stream)
    a = check_walk(wide, g, head)
    monkeypatch.setenv("SW_WALK_THREADS", "64")
    narrow = context(pkg, 130, stream)
    monkeypatch.delenv("SW_WALK_THREADS")
    b = check_walk(narrow, g, head)
    assert np.array_equal(a, b)
    check_walk(narrow, g, head, mw.arbitrary_heights(g, head, 7), g.trunks())
    assert narrow.walk_stats()["levels"] == len(g.levels(head, mw.arbitrary_heights(g, head, 7), g.trunks()))
    wide.close()
    narrow.close()


def test_slot_contents_with_data(pkg):
    stream, g = graph(pkg, 33, True)
    N = g.N
    h = context(pkg, 33, stream)
    rng = np.random.default_rng(5)
    datas = [None if e % 3 == 0 else rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes() for e in range(N)]
    h.set_event_data(0, datas)
    known = h.known_heights(N // 3)
    x = h.export_walk(N - 1, known, h.fork_trunks(), data=True)
    exp = g.export_walk(N - 1, known, g.trunks())
    same({k: x[k] for k in FIELDS}, exp, "export_walk(data=True)")
    roots = x["arity"] == 0
    assert roots.any() and not x["sp_ids"][roots].any() and not x["op_ids"][roots].any()
    d, off, none = h.gather_event_data(exp["event"])
    assert x["data"].tobytes() == d.tobytes() and np.array_equal(x["data_off"], off) and np.array_equal(x["data_none"], none)
    assert h.unpack_data(x["data"], x["data_off"], x["data_none"]) == [datas[e] for e in exp["event"]]
    h.close()


# ---- 2. capacity protocol and refusals, each leaving the context usable -----------------------------------------------------
def test_capacity_protocol_and_refusals(pkg, hip):
    stream, g = graph(pkg, 33, True)
    n, N = 33, g.N
    h = context(pkg, n, stream, ids=False, divided=N - 10)
    head = N - 20
    exp = g.export_walk(head)
    total = len(exp["event"])
    out = Out(hip, total)
    p = out.p
    args = [C.c_void_p(p[k]) for k in FIELDS]

    def dev(hd=head, cap_events=total, known=None, **repl):
        a = dict(p, **repl)
        return h.export_walk_device(hd, known, None, cap_events, a["ids"], a["sp_ids"], a["op_ids"], a["arity"], a["creator"], a["t"], a["sig"], a["event"])

    # an incomplete id index refuses the export forms, not sync_walk
    refused(pkg, -95, dev)
    refused(pkg, -95, lambda: h.export_walk(head))
    assert np.array_equal(h.sync_walk(head), exp["event"])
    h.set_event_ids(0, stream_ids(N)[:N - 1])
    refused(pkg, -95, dev)
    h.set_event_ids(N - 1, stream_ids(N)[N - 1:])
    # the size query, and a capacity one too small: nothing written
    out.fill(0xA5)
    n_out = C.c_int64(-1)
    assert h._L.sw_export_walk_device(h._h, head, None, None, 0, *([None] * 8), None, C.byref(n_out)) == -34 and n_out.value == total
    n_out = C.c_int64(-1)
    assert h._L.sw_export_walk(h._h, head, None, None, 0, *([None] * 8), C.byref(n_out)) == -34 and n_out.value == total
    n_out = C.c_int64(-1)
    assert h._L.sw_sync_walk(h._h, head, None, None, 0, None, C.byref(n_out)) == -34 and n_out.value == total
    assert h.walk_size(head) == total
    n_out = C.c_int64(-1)
    assert h._L.sw_export_walk_device(h._h, head, None, None, total - 1, *args, None, C.byref(n_out)) == -34 and n_out.value == total
    for k in FIELDS:
        assert np.all(hip.down(p[k], total * WIDTH[k], np.uint8) == 0xA5), "%s was written" % k
    small = np.full(total, -7, np.int32)
    n_out = C.c_int64(-1)
    assert h._L.sw_sync_walk(h._h, head, None, None, total - 1, small.ctypes.data_as(C.c_void_p), C.byref(n_out)) == -34 and n_out.value == total
    assert (small == -7).all()
    # an undivided head, a head that is no event
    for bad in (N - 5, -1, N + 3):
        refused(pkg, -34, lambda: dev(bad))
        refused(pkg, -34, lambda: h.export_walk(bad))
        refused(pkg, -34, lambda: h.sync_walk(bad))
    # a host pointer for an output array or the heights; an id array at offset 8
    host = np.empty(N * 64, np.uint8)
    for k in FIELDS:
        refused(pkg, -22, lambda: dev(**{k: host.ctypes.data}))
    refused(pkg, -22, lambda: dev(known=np.zeros(n, np.int32).ctypes.data))
    for k in ("ids", "sp_ids", "op_ids", "sig"):
        refused(pkg, -22, lambda: dev(**{k: hip.alloc(N * 64 + 16) + 8}))
    # ... and the call that is in order works
    assert dev() == total
    same(out.read(total), exp, "after the refusals")
    same(h.export_walk(head), exp, "after the refusals (host)")
    h.close()
    # a windowed context is out of scope: refused
    w_stream, _ = graph(pkg, 5, False)
    w = pkg.Hashgraph(5)
    w.set_window(True)
    w.append_events(*w_stream)
    w.set_event_ids(0, stream_ids(len(w_stream[0])))
    w.divide_rounds(0, len(w_stream[0]))
    last = len(w_stream[0]) - 1
    refused(pkg, -95, lambda: w.sync_walk(last))
    refused(pkg, -95, lambda: w.export_walk(last))
    refused(pkg, -95, lambda: w.fork_trunks())
    refused(pkg, -95, lambda: w.walk_size(last))
    assert w.known_heights(last).shape == (5,)
    w.close()


# ---- 3. two contexts that hold different siblings of one fork ----------------------------------------------------------------
@pytest.fixture(scope="module")
def universe(pkg):
    """A trunk of 80 really signed events of 5 members, then member 4 forks: siblings sA and sB on its newest event, equal in
    everything but the timestamp (so their heights are equal); a1 is built on sA by member 0, b1 on sB by member 1.
    Context A holds the trunk, BOTH siblings and a1; context B the trunk, sB and b1."""
    from test_gpu_sign import keypairs
    n, M = 5, 80
    cr, sp, op, t, _ = pkg.synth_hashgraph(n, M, 77)
    last = {m: int(np.flatnonzero(cr == m)[-1]) for m in range(n)}
    sA, sB, a1, b1 = M, M + 1, M + 2, M + 3
    cr = np.concatenate([cr, [4, 4, 0, 1]]).astype(np.int32)
    sp = np.concatenate([sp, [last[4], last[4], last[0], last[1]]]).astype(np.int32)
    op = np.concatenate([op, [last[2], last[2], sA, sB]]).astype(np.int32)
    t = np.concatenate([t, [t[-1] + 1, t[-1] + 2, t[-1] + 3, t[-1] + 4]])
    rng = np.random.default_rng(77)
    d = [None if e % 4 == 0 else rng.integers(0, 256, int(rng.integers(0, 30)), dtype=np.uint8).tobytes() for e in range(M + 4)]
    seeds, kps = keypairs(pkg, n, 77)
    return dict(n=n, M=M, cr=cr, sp=sp, op=op, t=t, d=d, seeds=seeds, kps=kps, sA=sA, sB=sB, a1=a1, b1=b1,
                A=list(range(M)) + [sA, sB, a1], B=list(range(M)) + [sB, b1])


def holder(pkg, u, events, with_data=True):
    """A context that created `events` (indices into the universe, topological) itself; returns it with the model's graph
    of what it holds (dense indices = positions in `events`, ids = the device's).  with_data=False: every event is signed
    with data None, which is what a validated pull WITHOUT data rebuilds."""
    from test_gpu_sign import signer
    loc = {e: i for i, e in enumerate(events)}
    ev = np.array(events)
    cr = u["cr"][ev]
    sp = np.array([loc[p] if p >= 0 else -1 for p in u["sp"][ev]], np.int32)
    op = np.array([loc[p] if p >= 0 else -1 for p in u["op"][ev]], np.int32)
    h = signer(pkg, u["n"], u["seeds"], u["kps"])
    first, ids, sig = h.create_events(cr, sp, op, u["t"][ev], [u["d"][e] if with_data else None for e in events], want_ids=True)
    assert first == 0
    h.divide_rounds(0, len(events))
    return h, mw.WalkGraph(u["n"], cr, sp, op, u["t"][ev], sig, ids), loc


def id_set(h):
    return set(bytes(i) for i in h.event_ids())


def storable(g, events, have):
    """The ids a receiver holding `have` stores out of `events` of g (ascending): an event whose parents it holds by then."""
    have = set(have)
    for e in sorted(events):
        if g.sp[e] < 0 or (bytes(g.ids[g.sp[e]]) in have and bytes(g.ids[g.op[e]]) in have):
            have.add(bytes(g.ids[e]))
    return have


@pytest.mark.parametrize("validate,data", [(False, False), (True, False), (False, True), (True, True)])
def test_pull_by_the_walk_exchanges_fork_siblings_only_with_the_trunks(pkg, universe, validate, data):
    u = universe
    A, gA, locA = holder(pkg, u, u["A"], with_data=data)
    B, gB, locB = holder(pkg, u, u["B"], with_data=data)
    assert A.exact and not B.exact
    headA, headB = locA[u["a1"]], locB[u["b1"]]
    id_sA = bytes(gA.ids[locA[u["sA"]]])
    known = B.known_heights(headB)
    assert known[4] == gA.height[locA[u["sA"]]] == gA.height[locA[u["sB"]]], "B reports the height both siblings have"
    before = id_set(B)
    assert id_sA not in before
    # without the trunks A's sibling stays behind, and so does a1, whose parent B lacks (node.py, ask_sync)
    walk = gA.walk(headA, known)
    assert locA[u["sA"]] not in walk.tolist()
    res = B.pull_from(A, headA, headB, validate, data=data, walk=True)
    assert res[0] == len(walk) and (not validate or res[1] == len(walk))
    assert id_set(B) == storable(gA, walk.tolist(), before) == before and res[-1] == 0
    # with them it arrives
    trunk = gA.trunks()
    assert np.array_equal(A.fork_trunks(), trunk) and trunk[4] == gA.height[gA.sp[locA[u["sA"]]]] < known[4]
    walk = gA.walk(headA, known, trunk)
    assert locA[u["sA"]] in walk.tolist()
    res = B.pull_from(A, headA, headB, validate, data=data, walk=True, trunks=True)
    assert res[0] == len(walk) and (not validate or res[1] == len(walk))
    after = id_set(B)
    assert after == storable(gA, walk.tolist(), before) == before | {id_sA, bytes(gA.ids[headA])}
    assert res[-1] == 2 and B.exact
    if data:
        held = {bytes(i): x for i, x in zip(B.event_ids(), B.unpack_data(*B.get_event_data()))}
        assert held[id_sA] == u["d"][u["sA"]] and held[bytes(gA.ids[headA])] == u["d"][u["a1"]]
    A.close()
    B.close()


def test_pull_by_the_walk_between_forkfree_contexts_equals_the_plain_pull(pkg, universe):
    u = universe
    src, g, _ = holder(pkg, u, list(range(u["M"])))
    got = []
    for walk in (True, False):
        dst, _, _ = holder(pkg, u, list(range(20)))
        n_sent, n_stored = dst.pull_from(src, u["M"] - 1, 19, walk=walk)
        assert n_stored > 20 and n_sent >= n_stored
        got.append((n_sent, n_stored, id_set(dst)))
        dst.close()
    assert got[0] == got[1] and not src.exact
    src.close()


# ---- 4. Node.ask_sync by the walk, in a gossip with an equivocator ----------------------------------------------------------
def equivocator_run(pkg, monkeypatch, walk):
    """Seven nodes; B equivocates, A holds both siblings, C one; then random syncs among the honest nodes.  Deterministic keys
    and clock, so two runs create the same events.  Returns (transactions per honest node, ask_sync calls checked)."""
    from test_node_host import _build_on, _seven_nodes
    crypto, loads = pkg.node.crypto, pkg.node.loads
    seeds = iter(range(1, 1 << 20))
    monkeypatch.setattr(crypto, "sign_keypair", lambda: crypto.sign_seed_keypair(next(seeds).to_bytes(32, "little")))
    clock = iter(range(1, 1 << 30))
    monkeypatch.setattr(pkg.node, "time", lambda: 1.0e9 + 0.001 * next(clock))
    checked = []

    def answer(nd):
        def ask(pk, info):
            nd.device_sync_walk = False
            host = nd.ask_sync(pk, info)
            if not walk:
                return host
            nd.device_sync_walk = True
            dev = nd.ask_sync(pk, info)
            (h0, s0), (h1, s1) = loads(crypto.sign_open(host, nd.pk)), loads(crypto.sign_open(dev, nd.pk))
            assert h0 == h1 and set(s0) == set(s1)
            checked.append((len(s1), bool(nd._dev.exact)))
            return dev
        return ask

    with contextlib.redirect_stdout(io.StringIO()):
        a, b, c, rest = _seven_nodes(pkg)
        for nd in [a, b, c] + rest:
            nd.network[nd.pk] = answer(nd)
        hb = b.head
        h1, e1 = b.new_event(b"one", (hb, b._chain_head[a.pk]))
        h2, e2 = b.new_event(b"two", (hb, b._chain_head[c.pk]))
        a.add_event(h1, e1)
        a.add_event(h2, e2)
        ha = _build_on(a, h1, b"on-one")
        a.divide_rounds((h1, h2, ha))
        c.add_event(h2, e2)
        hc = _build_on(c, h2, b"on-two")
        c.divide_rounds((h2, hc))
        new = c.sync(a.pk, b"after-fork")
        assert h1 in c.hg and ha in c.hg
        c.divide_rounds(new)
        c.find_order(c.decide_fame())
        rng = random.Random(11)
        honest = [a, c] + rest
        for _ in range(120):
            x, y = rng.sample(honest, 2)
            x.divide_rounds(x.sync(y.pk, b"more"))
            x.find_order(x.decide_fame())
    tx = [(list(nd.transactions), set(nd.hg)) for nd in honest]
    exact = [bool(nd._dev.exact) for nd in honest]
    for nd in [a, b, c] + rest:
        nd._dev.close()
    return tx, exact, checked


def test_node_answers_by_the_walk_as_its_host_bfs_would(pkg, monkeypatch):
    tx0, exact0, _ = equivocator_run(pkg, monkeypatch, walk=False)
    tx1, exact1, checked = equivocator_run(pkg, monkeypatch, walk=True)
    assert len(checked) > 50 and any(e for _, e in checked) and any(k > 1 for k, _ in checked)
    assert any(exact1) and exact0 == exact1
    assert tx0 == tx1, "the same events and the same order, whichever route answered"
