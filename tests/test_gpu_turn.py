"""GPU (-m gpu): one event signed by one wavefront and the gossip turn around it (sw_create_event, sw_gossip_turn,
sw_get_turn_stats; csrc/turn.hip.h).  create_event's id and signature are those of sign_events (the one-lane kernel) and of
the host route — pickle.dumps, libsodium, hashlib — for every data shape, roots and two-parent events, and the context then
equals one that took create_events.  A turn leaves what the composed calls leave (pull by the walk, id lookup, create,
divide_rounds, decide_fame, find_order), with and without validation, data and consensus, and from a forked peer with the
trunks.  A simulation of whole networks equals the drop-in Node's, by event id.  Refusals store nothing."""
import random
import struct

import numpy as np
import pytest

from conftest import load_golden
from test_gpu_sign import host_sign, keypairs, signer
from test_gpu_walk import holder

pytestmark = pytest.mark.gpu

ENOTSUP, EINVAL = -95, -22
SHAPES = [None, 0, 1, 255, 256, 257, 60000]


def refused(pkg, code, fn):
    with pytest.raises(pkg.SwirldHipError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    return ei.value


def payload_of(rng, dl):
    return None if dl is None else rng.integers(0, 256, dl, dtype=np.uint8).tobytes()


# ---- 1. create_event against sign_events, the host route and create_events ---------------------------------------------------
@pytest.mark.parametrize("dl", SHAPES, ids=lambda d: "data%s" % d)
def test_create_event_is_sign_events_and_the_host_route(pkg, dl):
    n = 3
    seeds, kps = keypairs(pkg, n, 41)
    h, ref = signer(pkg, n, seeds, kps), signer(pkg, n, seeds, kps)
    rng = np.random.default_rng(41 + (dl or 0))
    # two roots and a two-parent event of two members each, every one with data of this shape; member 2's root first
    cr = [2, 0, 1, 0, 1]
    sp = [-1, -1, -1, 1, 2]
    op = [-1, -1, -1, 2, 3]
    t = [1.5, 2.5, -0.0, 1e300, 4.25]
    d = [None] + [payload_of(rng, dl) for _ in range(4)]
    ids = []
    exp_ids, exp_sig = host_sign(pkg, kps, cr, sp, op, t, d, ids)
    for e in range(len(cr)):
        one_lane = h.sign_events([cr[e]], [sp[e]], [op[e]], [t[e]], [d[e]])
        idx, eid, sig = h.create_event(cr[e], sp[e], op[e], t[e], d[e], want_ids=True)
        assert idx == e == h.num_events - 1
        assert eid == bytes(one_lane["ids"][0]) and sig == bytes(one_lane["sig"][0]), "against the one-lane kernel (event %d)" % e
        assert eid == bytes(exp_ids[e]) and sig == bytes(exp_sig[e]), "against pickle, libsodium and hashlib (event %d)" % e
    assert ref.create_events(cr, sp, op, t, d) == 0
    for x in (h, ref):
        x.divide_rounds(0, len(cr))
    assert np.array_equal(h.event_ids(), ref.event_ids())
    assert h.unpack_data(*h.get_event_data()) == ref.unpack_data(*ref.get_event_data()) == d
    assert np.array_equal(h.heights(), ref.heights()) and np.array_equal(h.rounds(), ref.rounds())
    assert np.array_equal(h.can_see(), ref.can_see())
    st = h.turn_stats()
    assert st["create_calls"] == st["events"] == len(cr) and st["turns"] == 0
    h.close()
    ref.close()


def test_create_event_refuses_as_create_events_does(pkg):
    n = 3
    seeds, kps = keypairs(pkg, n, 42)
    h = signer(pkg, n, seeds, kps, members=[0, 1])
    for m in (0, 1):
        h.create_event(m, -1, -1, float(m))
    before = (h.num_events, h.event_ids().tobytes(), h.data_stats()["events"])
    for args in ((0, 0, -1, 1.0), (0, 1, 0, 1.0), (0, 0, 0, 1.0), (0, 0, 7, 1.0), (2, -1, -1, 1.0), (5, -1, -1, 1.0)):
        one = refused(pkg, EINVAL, lambda: h.create_event(*args))
        many = refused(pkg, EINVAL, lambda: h.create_events([args[0]], [args[1]], [args[2]], [args[3]]))
        assert one.code == many.code
    refused(pkg, EINVAL, lambda: h.create_event(0, 0, 1, 1.0, bytes(60001)))
    refused(pkg, EINVAL, lambda: h.create_event(0, -1, -1, 0.0))      # the stored root again: equal events have equal ids
    assert (h.num_events, h.event_ids().tobytes(), h.data_stats()["events"]) == before
    assert h.create_event(0, 0, 1, 9.0, b"fine") == 2
    bare = pkg.Hashgraph(n)
    refused(pkg, ENOTSUP, lambda: bare.create_event(0, -1, -1, 0.0))
    bare.close()
    h.close()


# ---- 2. a turn against the composed calls ---------------------------------------------------------------------------------
def golden_universe(pkg, name, tag):
    g = load_golden(name)
    n, N = g["n"], len(g["creator"])
    rng = np.random.default_rng(tag)
    d = [None if e % 3 == 0 else rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes() for e in range(N)]
    seeds, kps = keypairs(pkg, n, tag)
    return dict(n=n, N=N, cr=g["creator"].astype(np.int32), sp=g["self_parent"].astype(np.int32), op=g["other_parent"].astype(np.int32),
                t=g["t"].astype(np.float64), d=d, seeds=seeds, kps=kps)


@pytest.fixture(scope="module")
def plain(pkg):
    return golden_universe(pkg, "n4_s1_batch", 43)


@pytest.fixture(scope="module")
def forked(pkg):
    return golden_universe(pkg, "n5_s13_forks_chunk1", 44)


def split(u, n_dst, n_src):
    """dst holds the prefix [0, n_dst) and its head is the newest event of it; src holds the events below n_src that are not
    built on a LATER event of dst's member (a node's own newer events exist nowhere else).  Returns the member, dst's head,
    src's events (indices into the universe) and src's head as an index of src's context: its newest event by another member."""
    dst_head = n_dst - 1
    member = int(u["cr"][dst_head])
    late = set()
    for e in range(n_dst, n_src):
        if u["cr"][e] == member or int(u["sp"][e]) in late or int(u["op"][e]) in late:
            late.add(e)
    events = [e for e in range(n_src) if e not in late]
    src_head = max(i for i, e in enumerate(events) if u["cr"][e] != member)
    return member, dst_head, events, src_head


def new_to_prefix(u, tops, n_dst):
    """How many ancestors (themselves included) of the universe's events `tops` lie outside the prefix [0, n_dst): what a
    pull from a head with those ancestors stores in a context that holds the prefix."""
    seen, todo = set(), [int(e) for e in tops]
    while todo:
        e = todo.pop()
        if e < n_dst or e in seen:
            continue
        seen.add(e)
        todo += [int(u["sp"][e]), int(u["op"][e])]
    return len(seen)


def snapshot(h, divided=None):
    """Every getter of a context whose id index is complete, as comparable values (divided: how many events have a round;
    default all of them)."""
    N = h.num_events
    divided = N if divided is None else divided
    rounds = h.rounds(0, divided)
    s = dict(N=N, ids=h.event_ids().tobytes(), heights=h.heights().tobytes(), rounds=rounds.tobytes(), can_see=h.can_see(0, divided).tobytes(),
             max_round=h.max_round, witnesses=h.witnesses().tobytes(), famous=h.famous().tobytes(), tx=h.transactions().tobytes(),
             n_data=h.data_stats()["events"], exact=h.exact)
    if not s["exact"]:          # (the exact path keeps neither)
        s.update(rr=h.round_received(0, divided).tobytes(), ct=h.consensus_time(0, divided).tobytes())
    if s["n_data"]:
        s["data"] = h.unpack_data(*h.get_event_data())
    by_id = [bytes(i) for i in h.event_ids()]
    s["round_by_id"] = dict(zip(by_id, rounds.tolist()))
    s["order_by_id"] = [by_id[e] for e in h.transactions()]
    return s


def composed(dst, src, member, dst_head, src_head, t, payload, validate, data, trunks, consensus):
    """The sequence of calls a turn is defined by."""
    N0 = dst.num_events
    res = dst.pull_from(src, src_head, dst_head, validate, data=data, walk=True, trunks=trunks)
    idx = int(dst.lookup_event_ids(src.event_ids(src_head, 1))[0])
    new_head = -1
    if idx >= 0:
        new_head = dst.create_events([member], [dst_head], [idx], [t], [payload])
    new_c = np.zeros(0, np.int32)
    n_ord = 0
    if consensus:
        dst.divide_rounds(N0, dst.num_events - N0)
        new_c = dst.decide_fame()
        n_ord = len(dst.find_order(new_c))
    return res, new_head, new_c, n_ord


def run_both(pkg, u, n_dst, n_src, validate, data, trunks, consensus, payload=b"turn payload"):
    member, dst_head, events, src_head = split(u, n_dst, n_src)
    src, _, _ = holder(pkg, u, events, with_data=data)
    got = []
    for turn in (True, False):
        dst, _, _ = holder(pkg, u, list(range(n_dst)), with_data=data)
        src_before = snapshot(src)
        if turn:
            r = dst.gossip_turn(src, member, dst_head, src_head, 5e8, payload, validate=validate, data_store=data, trunks=trunks, consensus=consensus)
            out = (r.n_sent, r.n_valid if validate else None, r.n_stored, r.new_head, r.new_rounds.tolist(), r.n_ordered)
            assert r.stage == (5 if consensus else 2) and r.n_new_rounds == len(r.new_rounds)
            assert dst.turn_stats()["turns"] == 1
        else:
            res, new_head, new_c, n_ord = composed(dst, src, member, dst_head, src_head, 5e8, payload, validate, data, trunks, consensus)
            out = (res[0], res[1] if validate else None, res[-1], new_head, new_c.tolist(), n_ord)
        assert snapshot(src) == src_before, "src untouched"
        got.append((out, snapshot(dst, None if consensus else n_dst)))
        dst.close()
    src.close()
    (out_t, snap_t), (out_c, snap_c) = got
    assert out_t == out_c
    for k in snap_c:
        assert snap_t[k] == snap_c[k], k
    return out_t, snap_t


@pytest.mark.parametrize("validate,data,consensus", [(True, True, True), (False, True, True), (True, False, True), (False, False, True), (True, True, False)])
def test_turn_equals_the_composed_calls(pkg, plain, validate, data, consensus):
    n_dst = 200
    out, snap = run_both(pkg, plain, n_dst, 300, validate, data, False, consensus)
    n_sent, _, n_stored, new_head, new_rounds, n_ordered = out
    _, _, events, src_head = split(plain, n_dst, 300)
    missing = new_to_prefix(plain, [events[src_head]], n_dst)
    assert missing >= 5 and n_stored == missing and new_head == n_dst + n_stored and snap["N"] == new_head + 1
    if consensus:   # (dst never decided anything before: the turn decides and orders what 200 events of 4 members allow)
        assert len(new_rounds) > 0 and n_ordered > 0 and snap["max_round"] > 3 and len(snap["order_by_id"]) == n_ordered
    else:
        assert snap["max_round"] > 3 and snap["order_by_id"] == [] and len(snap["round_by_id"]) == n_dst
    if data:
        assert snap["data"][-1] == b"turn payload"


def test_turn_from_a_forked_peer_with_the_trunks(pkg, forked):
    n_dst = 200
    out, snap = run_both(pkg, forked, n_dst, forked["N"], True, True, True, True, payload=None)
    _, _, events, src_head = split(forked, n_dst, forked["N"])
    assert out[2] == new_to_prefix(forked, [events[src_head]], n_dst) >= 5 and out[3] == n_dst + out[2] and snap["exact"]


# ---- 3. whole networks against the drop-in Node ------------------------------------------------------------------------------
def node_simulation(pkg, seeds, n_turns, seed, payloads):
    node_mod = pkg.node
    crypto = node_mod.crypto
    rng = random.Random(seed)
    clock = iter(range(1, 1 << 30))
    saved = (crypto.randombytes, node_mod.time, node_mod.randrange)
    crypto.randombytes = lambda k: bytes(rng.getrandbits(8) for _ in range(k))
    node_mod.time = lambda: 1.0e9 + 0.001 * next(clock)
    node_mod.randrange = lambda k: rng.randrange(k)
    try:
        kps = [crypto.sign_seed_keypair(s) for s in seeds]
        network = {}
        stake = {kp[0]: 1 for kp in kps}
        nodes = [pkg.Node(kp, network, len(kps), stake) for kp in kps]
        for nd in nodes:
            network[nd.pk] = nd.ask_sync
        mains = [nd.main() for nd in nodes]
        for m in mains:
            next(m)
        for k in range(n_turns):
            mains[rng.randrange(len(kps))].send(payloads(k))
        return nodes
    finally:
        crypto.randombytes, node_mod.time, node_mod.randrange = saved


@pytest.mark.parametrize("n,turns", [(4, 150), (5, 300)])
def test_device_network_equals_the_node_simulation(pkg, n, turns):
    seeds = [bytes([50 + n, m]) + bytes(30) for m in range(n)]
    payloads = lambda k: None if k % 2 == 0 else b"tx %d" % k
    nodes = node_simulation(pkg, seeds, turns, 20261019 + n, payloads)
    rng = random.Random(20261019 + n)
    clock = iter(range(1, 1 << 30))
    tick = lambda: 1.0e9 + 0.001 * next(clock)
    ev = pkg.node.Event
    net = pkg.DeviceNetwork(seeds, event_class=(ev.__module__, ev.__qualname__), clock=tick)
    net.run(turns, rng.randrange, tick, payloads)
    assert all(r.new_head >= 0 and r.stage == 5 for r in net.results) and len(net.results) == turns
    bits = lambda x: struct.pack("<d", x)
    # (the partner choice of swirld.py:323 walks a set of keys: which simulation runs depends on the process's hash seed, and
    # with four members some of them order nothing in 150 turns — no bound on the ordered events here)
    for i, nd in enumerate(nodes):
        assert net.pks[i] == nd.pk
        assert net.event_ids(i) == set(nd.hg) and len(nd.hg) > turns // n
        assert net.head(i) == nd.head
        assert net.round(i) == {h: nd.round[h] for h in nd.hg}
        assert net.transactions(i) == list(nd.transactions)
        assert net.round_received(i) == {h: nd.round_received[h] for h in nd.transactions}
        assert {h: bits(x) for h, x in net.consensus_time(i).items()} == {h: bits(nd.consensus_time[h]) for h in nd.transactions}
        assert net.ordered_data(i) == [nd.hg[h].d for h in nd.transactions]
    assert sum(len(nd.hg) for nd in nodes) > turns
    net.close()


# ---- 4. refusals: the code, nothing stored, src untouched, and the context still answers -------------------------------------
def counts(h):
    try:
        n_ids = len(h.event_ids())
    except Exception:   # (an incomplete id index has no "all ids")
        n_ids = None
    return h.num_events, n_ids, h.data_stats()["events"], h.data_stats()["bytes"]


def test_a_refused_turn_leaves_both_contexts_as_they_were(pkg, plain):
    u = plain
    n = u["n"]
    member, dst_head, events, src_head = split(u, 60, 150)
    dst, _, _ = holder(pkg, u, list(range(60)))
    src, _, _ = holder(pkg, u, events)
    other = next(e for e in range(59, -1, -1) if u["cr"][e] != member)          # dst: an event that is not member's
    own_in_src = max(i for i, e in enumerate(events) if u["cr"][e] == member)    # src: an event that is member's

    def turn(d=dst, s=src, m=member, dh=dst_head, sh=src_head, data=None, **kw):
        return d.gossip_turn(s, m, dh, sh, 1.0, data, **kw)

    few = pkg.Hashgraph(n + 1)
    bare = pkg.Hashgraph(n)                                                       # no member keys
    windowed = pkg.Hashgraph(n)
    windowed.set_window(True)
    seeds, kps = u["seeds"], u["kps"]
    nokey = signer(pkg, n, seeds, kps, members=[m for m in range(n) if m != member])
    raw = signer(pkg, n, seeds, kps)                                              # events without ids
    raw.append_events(u["cr"][:60], u["sp"][:60], u["op"][:60], u["t"][:60])
    raw.divide_rounds(0, 60)
    nodata = signer(pkg, n, seeds, kps)                                           # ids, and no data store
    nodata.append_events(u["cr"][:60], u["sp"][:60], u["op"][:60], u["t"][:60])
    nodata.set_event_ids(0, dst.event_ids())
    nodata.divide_rounds(0, 60)
    undivided, _, _ = holder(pkg, u, list(range(60)))
    undivided.create_event(member, dst_head, other, 2.0)
    cases = [
        (EINVAL, lambda: turn(s=dst)),
        (EINVAL, lambda: turn(s=few)),
        (EINVAL, lambda: turn(dh=other)),
        (EINVAL, lambda: turn(sh=own_in_src)),
        (EINVAL, lambda: turn(d=undivided)),
        (EINVAL, lambda: turn(data=bytes(60001))),
        (ENOTSUP, lambda: turn(d=nokey)),
        (ENOTSUP, lambda: turn(d=bare)),
        (ENOTSUP, lambda: turn(d=raw)),
        (ENOTSUP, lambda: turn(s=raw)),
        (ENOTSUP, lambda: turn(d=nodata, data_store=True)),
        (ENOTSUP, lambda: turn(s=nodata, data_store=True)),
        (ENOTSUP, lambda: turn(d=windowed)),
        (ENOTSUP, lambda: turn(s=windowed)),
    ]
    everyone = [dst, src, few, bare, windowed, nokey, raw, nodata, undivided]
    before = [counts(x) for x in everyone]
    src_snap = snapshot(src)
    for code, fn in cases:
        refused(pkg, code, fn)
        assert [counts(x) for x in everyone] == before
    assert snapshot(src) == src_snap
    assert len(dst.rounds()) == 60 and len(raw.rounds()) == 60 and len(nodata.rounds()) == 60 and len(undivided.rounds(0, 60)) == 60
    r = turn(data=b"after the refusals", data_store=True)
    assert r.stage == 5 and r.new_head == dst.num_events - 1 and r.n_stored == new_to_prefix(u, [events[src_head]], 60) > 0
    for x in everyone:
        x.close()


def test_absent_head_is_no_event_and_no_error(pkg, plain):
    """src stored, unchecked, a head whose signature is not its creator's; under validate dst rejects it: no event."""
    u = plain
    member, dst_head, events, _ = split(u, 60, 150)
    dst, _, _ = holder(pkg, u, list(range(60)))
    src, _, _ = holder(pkg, u, events)
    M = len(events)
    c = (member + 1) % u["n"]
    sp = max(i for i, e in enumerate(events) if u["cr"][e] == c)
    op = max(i for i, e in enumerate(events) if u["cr"][e] != c)
    src.append_events([c], [sp], [op], [7.0], np.full((1, 64), 9, np.uint8))
    src.set_event_ids(M, np.full((1, 32), 0xAB, np.uint8))
    src.set_event_data(M, [None])
    src.divide_rounds(M, 1)
    r = dst.gossip_turn(src, member, dst_head, M, 8.0, b"never stored", validate=True, data_store=True)
    assert r.new_head == -1 and r.stage == 5
    # (the walk is pruned by what dst's HEAD sees: an event dst holds beside it travels again, is valid, and is not stored twice)
    assert r.n_sent == r.n_valid + 1 > r.n_stored and r.n_stored == new_to_prefix(u, [events[sp], events[op]], 60) > 0
    assert dst.num_events == 60 + r.n_stored == len(dst.event_ids()) == dst.data_stats()["events"]
    assert int(dst.lookup_event_ids(np.full((1, 32), 0xAB, np.uint8))[0]) == -1
    assert (dst.rounds() >= 0).all()
    # without validation the same head is stored, and the event exists
    dst2, _, _ = holder(pkg, u, list(range(60)))
    r2 = dst2.gossip_turn(src, member, dst_head, M, 8.0, None, validate=False, data_store=True)
    assert r2.new_head == dst2.num_events - 1 and r2.n_stored == r.n_stored + 1
    for x in (dst, dst2, src):
        x.close()


# ---- 5. the stamps -----------------------------------------------------------------------------------------------------------
def test_stamps_are_monotonic_and_counted(pkg):
    n = 3
    seeds, kps = keypairs(pkg, n, 45)
    h = signer(pkg, n, seeds, kps)
    h.create_event(0, -1, -1, 0.5)
    st = h.turn_stats()
    assert (st["create_calls"], st["events"], st["stamped"]) == (1, 1, 0) and st["stamps"] == [0] * 8
    h.set_profiling(True)
    h.create_event(1, -1, -1, 1.5, b"x" * 300)
    h.create_event(0, 0, 1, 2.5)
    st = h.turn_stats()
    assert (st["create_calls"], st["events"], st["stamped"]) == (3, 3, 2)
    s = st["stamps"]
    assert all(b >= a for a, b in zip(s, s[1:])) and s[-1] > s[0] > 0, s
    assert 0 < st["tick_ns"] <= 1000 and sum(st["phase_us"].values()) < 1e5
    h.set_profiling(False)
    h.create_event(1, 1, 2, 3.5)
    st2 = h.turn_stats()
    assert (st2["create_calls"], st2["events"], st2["stamped"]) == (4, 4, 2) and st2["stamps"] == s
    h.close()
