"""GPU (-m gpu): signed events created on the device (sw_set_signing_keys, sw_sign_events[_device],
sw_create_events[_device]; csrc/sign.hip.h).  Every id and signature must be bit for bit what the host route gives —
pickle.dumps, libsodium, hashlib — whether an event's parents are stored, in the batch, or one of each; at the wavefront
edges of a level; and create_events must leave the state ingest_payload(..., data=...) of the same host-signed events
leaves.  The pipeline accepts its own output (pack, validate, a validated pull with data); refusals change nothing; forks
are signed like anything else; signing is read-only.

No torch here (see tests/test_gpu_ingest_device.py): device buffers come through ctypes from the HIP runtime the library
is linked against."""
import pickle

import numpy as np
import pytest

import model_pack as mpk
from test_gpu_payload import Hip

pytestmark = pytest.mark.gpu

ENOTSUP, EINVAL = -95, -22


@pytest.fixture
def hip(pkg):
    h = Hip(pkg)
    yield h
    h.free()


def member_seeds(n, tag):
    return [bytes([tag & 255, m & 255, m >> 8]) + bytes(29) for m in range(n)]


def keypairs(pkg, n, tag):
    seeds = member_seeds(n, tag)
    return seeds, [pkg.node.crypto.sign_seed_keypair(s) for s in seeds]


def host_sign(pkg, kps, cr, sp, op, t, d, ids, mod="swirld", qual="Event"):
    """The host route for events whose parents are ABSOLUTE dense indices into `ids` (a list of the ids so far, extended in
    place): per event two pickle.dumps, crypto_sign_detached, BLAKE2b.  Returns (ids, sigs) of the new events as arrays."""
    crypto = pkg.node.crypto
    new_ids, sigs = [], []
    with mpk.event_class(mod, qual) as Event:
        for e in range(len(cr)):
            p = () if sp[e] < 0 else (ids[sp[e]], ids[op[e]])
            body = (d[e], p, float(t[e]), kps[cr[e]][0])
            s = crypto.sign_detached(pickle.dumps(body, protocol=4), kps[cr[e]][1])
            i = crypto.generichash(pickle.dumps(Event(*body, s), protocol=4))
            ids.append(i)
            new_ids.append(i)
            sigs.append(s)
    arr = lambda rows, w: np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), w).copy()
    return arr(new_ids, 32), arr(sigs, 64)


def signer(pkg, n, seeds, kps, members=None):
    h = pkg.Hashgraph(n)
    assert h.set_member_keys([pk for pk, _ in kps]) == 0
    members = list(range(n)) if members is None else members
    h.set_signing_seeds(members, [seeds[m] for m in members])
    return h


def dev_sign(h, hip, cr, sp, op, t, d):
    """sign_events_device between device arrays; returns the same dict sign_events returns."""
    K = len(cr)
    data, off, none = h.pack_data(d)
    outs = dict(ids=hip.alloc(32 * K), sp_ids=hip.alloc(32 * K), op_ids=hip.alloc(32 * K), arity=hip.alloc(K), sig=hip.alloc(64 * K))
    h.sign_events_device(hip.up(cr, np.int32), hip.up(sp, np.int32), hip.up(op, np.int32), hip.up(t, np.float64), outs["ids"], outs["sp_ids"],
                         outs["op_ids"], outs["arity"], outs["sig"], data=hip.up(data, np.uint8, offset=3) if len(data) else None,
                         data_off=hip.up(off, np.int64), data_bytes=len(data), data_none=hip.up(none, np.uint8), count=K)
    width = dict(ids=32, sp_ids=32, op_ids=32, arity=1, sig=64)
    return {k: hip.down(p, K * width[k], np.uint8).reshape((K, width[k]) if width[k] > 1 else (K,)) for k, p in outs.items()}


def check_signed(out, ids, sigs, sp, all_ids):
    assert np.array_equal(out["ids"], ids), "ids against pickle + BLAKE2b"
    assert np.array_equal(out["sig"], sigs), "signatures against libsodium"
    assert np.array_equal(out["arity"], np.where(np.asarray(sp) < 0, 0, 2))
    return out


def test_bit_exact_against_the_host_route(pkg, hip):
    n, N = 4, 60
    cr, sp, op, t, _ = pkg.synth_hashgraph(n, N, 31)
    rng = np.random.default_rng(31)
    d = [None] * N
    for e in rng.choice(N, N // 3, replace=False):
        d[e] = rng.integers(0, 256, int(rng.integers(1, 300)), dtype=np.uint8).tobytes()
    with_data = [e for e in range(N) if d[e] is not None]
    d[with_data[0]] = b""
    d[with_data[-1]] = rng.integers(0, 256, 60000, dtype=np.uint8).tobytes()
    seeds, kps = keypairs(pkg, n, 31)
    h = signer(pkg, n, seeds, kps)
    ids = []
    kinds = set()
    for a, b in ((0, 1), (1, 8), (8, N)):
        s = slice(a, b)
        exp_ids, exp_sig = host_sign(pkg, kps, cr[s], sp[s], op[s], t[s], d[s], ids)
        for e in range(a, b):
            if sp[e] >= 0:
                kinds.add((bool(sp[e] >= a), bool(op[e] >= a)))
        host = check_signed(h.sign_events(cr[s], sp[s], op[s], t[s], d[s]), exp_ids, exp_sig, sp[s], ids)
        dev = dev_sign(h, hip, cr[s], sp[s], op[s], t[s], d[s])
        for k in host:
            assert np.array_equal(host[k], dev[k]), k
        first, got_ids, got_sig = h.create_events(cr[s], sp[s], op[s], t[s], d[s], want_ids=True)
        assert first == a and h.num_events == b
        assert np.array_equal(got_ids, exp_ids) and np.array_equal(got_sig, exp_sig)
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}, "stored, in-batch and mixed parents"
    assert np.array_equal(h.event_ids(), np.frombuffer(b"".join(ids), np.uint8).reshape(N, 32))
    assert h.unpack_data(*h.get_event_data()) == d
    assert h.sign_stats()["calls"] == 9
    h.close()


def test_wavefront_edges(pkg):
    n = 65
    seeds, kps = keypairs(pkg, n, 32)
    h = signer(pkg, n, seeds, kps)
    ids = []
    root = np.full(n, -1, np.int32)
    t = np.arange(n, dtype=np.float64)
    exp = host_sign(pkg, kps, np.arange(n), root, root, t, [None] * n, ids)
    first, got_ids, got_sig = h.create_events(np.arange(n, dtype=np.int32), root, root, t, want_ids=True)
    assert first == 0 and np.array_equal(got_ids, exp[0]) and np.array_equal(got_sig, exp[1])
    assert h.sign_stats()["levels"] == 1
    for w in (63, 64, 65):      # one further level of that width on the stored roots (nothing is stored: sign_events)
        cr = np.arange(w, dtype=np.int32)
        sp, op, tt = cr.copy(), ((cr + 1) % n).astype(np.int32), 100.0 + cr
        e_ids, e_sig = host_sign(pkg, kps, cr, sp, op, tt, [None] * w, list(ids))
        check_signed(h.sign_events(cr, sp, op, tt), e_ids, e_sig, sp, ids)
        assert h.sign_stats()["levels"] == 1
    # a chain of 5 events by two members: five levels of width 1
    cr = np.array([0, 1, 0, 1, 0], np.int32)
    sp = np.array([0, 1, n, n + 1, n + 2], np.int32)
    op = np.array([1, n, n + 1, n + 2, n + 3], np.int32)
    tt = 200.0 + np.arange(5)
    e_ids, e_sig = host_sign(pkg, kps, cr, sp, op, tt, [b"x"] * 5, list(ids))
    check_signed(h.sign_events(cr, sp, op, tt, [b"x"] * 5), e_ids, e_sig, sp, ids)
    assert h.sign_stats()["levels"] == 5
    h.close()


def test_a_level_of_1024_roots(pkg):
    n = 1024
    seeds, kps = keypairs(pkg, n, 33)
    h = signer(pkg, n, seeds, kps)
    root = np.full(n, -1, np.int32)
    cr = np.arange(n, dtype=np.int32)[::-1].copy()
    t = np.linspace(0.0, 1.0, n)
    e_ids, e_sig = host_sign(pkg, kps, cr, root, root, t, [None] * n, [])
    check_signed(h.sign_events(cr, root, root, t), e_ids, e_sig, root, [])
    assert h.sign_stats()["levels"] == 1
    h.close()


# ---- one really signed history of 5 members, shared by the tests below

@pytest.fixture(scope="module")
def history(pkg):
    n, N, seed = 5, 400, 905      # (with 905, more than 200 of the 400 events get ordered: tests/test_gpu_event_data.py)
    cr, sp, op, t, _ = pkg.synth_hashgraph(n, N, seed)
    rng = np.random.default_rng(seed)
    d = []
    for e in range(N):
        kind = rng.integers(0, 4)
        d.append(None if kind == 0 else b"" if kind == 1 else rng.integers(0, 256, int(rng.integers(1, 40)) if kind == 2 else 300, dtype=np.uint8).tobytes())
    seeds, kps = keypairs(pkg, n, seed)
    ids = []
    arr_ids, arr_sig = host_sign(pkg, kps, cr, sp, op, t, d, ids)
    return dict(n=n, N=N, cr=cr, sp=sp, op=op, t=t, d=d, seeds=seeds, kps=kps, ids=arr_ids, sig=arr_sig)


def created(pkg, g, cuts=(0, 1, 150, 400)):
    h = signer(pkg, g["n"], g["seeds"], g["kps"])
    for a, b in zip(cuts[:-1], cuts[1:]):
        s = slice(a, b)
        assert h.create_events(g["cr"][s], g["sp"][s], g["op"][s], g["t"][s], g["d"][s]) == a
    return h


def ingested(pkg, g, cuts=(0, 1, 150, 400)):
    h = pkg.Hashgraph(g["n"])
    zero = np.zeros((g["N"], 32), np.uint8)
    sp_ids = np.where((g["sp"] >= 0)[:, None], g["ids"][np.maximum(g["sp"], 0)], zero)
    op_ids = np.where((g["op"] >= 0)[:, None], g["ids"][np.maximum(g["op"], 0)], zero)
    arity = np.where(g["sp"] < 0, 0, 2).astype(np.uint8)
    for a, b in zip(cuts[:-1], cuts[1:]):
        s = slice(a, b)
        _, stored = h.ingest_payload(g["ids"][s], sp_ids[s], op_ids[s], arity[s], g["cr"][s], t=g["t"][s], sig=g["sig"][s], data=g["d"][s])
        assert stored == b - a
    return h


def consensus_by_id(h):
    """Everything the issue lists, keyed by event id (the payload ingest numbers a batch by acceptance wave, create_events
    in the order given: the dense indices of the two contexts differ, what is known about every event may not)."""
    N = h.num_events
    ids = [bytes(i) for i in h.event_ids()]
    h.divide_rounds(0, N)
    new_c = list(h.decide_fame())
    order = [ids[e] for e in h.find_order(new_c)]
    data = h.unpack_data(*h.get_event_data())
    wit = h.witnesses()
    fam = h.famous()
    x = h.export_payload(N - 1, data=True)
    o = h.export_ordered()
    return dict(
        data=dict(zip(ids, data)), heights=dict(zip(ids, h.heights().tolist())), rounds=dict(zip(ids, h.rounds().tolist())),
        witnesses=sorted((r, m, ids[wit[r, m]], int(fam[r, m])) for r in range(wit.shape[0]) for m in range(wit.shape[1]) if wit[r, m] >= 0),
        new_c=new_c, order=order,
        seen=sorted((bytes(i), bytes(s), float(tt), int(c)) for i, s, tt, c in zip(x["ids"], x["sig"], x["t"], x["creator"])),
        ordered=[(bytes(i), int(c), int(r), float(tt)) for i, c, r, tt in zip(o["ids"], o["creator"], o["round_received"], o["time"])])


def test_create_events_leaves_the_state_of_the_payload_ingest(pkg, history):
    g = history
    a, b = created(pkg, g), ingested(pkg, g)
    assert np.array_equal(a.event_ids(), g["ids"]), "create_events numbers the events in the order given"
    assert a.num_events == b.num_events == g["N"] and a.data_stats()["events"] == b.data_stats()["events"] == g["N"]
    ca, cb = consensus_by_id(a), consensus_by_id(b)
    for k in ca:
        assert ca[k] == cb[k], k
    assert len(ca["order"]) > 200 and len(ca["new_c"]) >= 3, "several rounds decide"
    assert ca["data"] == dict(zip((bytes(i) for i in g["ids"]), g["d"]))
    a.close()
    b.close()


def test_the_pipeline_accepts_its_own_output(pkg, history):
    g = history
    N = g["N"]
    h = signer(pkg, g["n"], g["seeds"], g["kps"])
    s = h.sign_events(g["cr"], g["sp"], g["op"], g["t"], g["d"])
    assert np.array_equal(s["ids"], g["ids"]) and np.array_equal(s["sig"], g["sig"])
    data, off, none = h.pack_data(g["d"])
    msgs, moff, whole, woff, enc = h.pack_events(s["sp_ids"], s["op_ids"], s["arity"], g["cr"], g["t"], s["sig"], data, off, none)
    assert enc.all()
    assert h.validate_payload((msgs, moff), s["sig"], g["cr"], (whole, woff), s["ids"]).all()
    t2 = g["t"].copy()
    t2[137] += 1.0
    msgs, moff, whole, woff, enc = h.pack_events(s["sp_ids"], s["op_ids"], s["arity"], g["cr"], t2, s["sig"], data, off, none)
    ok = h.validate_payload((msgs, moff), s["sig"], g["cr"], (whole, woff), s["ids"])
    assert np.flatnonzero(~ok).tolist() == [137]
    h.close()
    # a validated pull with data from a context built by create_events into a context that holds only the first event
    src = created(pkg, g)
    src.divide_rounds(0, N)
    dst = signer(pkg, g["n"], g["seeds"], g["kps"], members=[int(g["cr"][0])])
    assert dst.create_events(g["cr"][:1], g["sp"][:1], g["op"][:1], g["t"][:1], g["d"][:1]) == 0
    dst.divide_rounds(0, 1)
    anc = {N - 1}
    for e in range(N - 1, -1, -1):
        if e in anc and g["sp"][e] >= 0:
            anc.update((int(g["sp"][e]), int(g["op"][e])))
    new = sorted(anc - {0})
    n_sent, n_valid, n_stored = dst.pull_from(src, N - 1, 0, validate=True, data=True)
    assert n_sent == n_valid and n_stored == len(new) > 300
    by_id = {bytes(i): e for e, i in enumerate(g["ids"])}
    held = [by_id[bytes(i)] for i in dst.event_ids()]
    assert sorted(held) == [0] + new
    assert dst.unpack_data(*dst.get_event_data()) == [g["d"][e] for e in held]
    src.close()
    dst.close()


def refused(pkg, code, fn, *args, **kw):
    with pytest.raises(pkg.SwirldHipError) as ei:
        fn(*args, **kw)
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


def counts(h):
    """events, events that have an id, events that have data"""
    with_ids = h.num_events
    while with_ids:
        try:
            h.event_ids(0, with_ids)
            break
        except Exception:      # (beyond the events that have ids)
            with_ids -= 1
    return h.num_events, with_ids, h.data_stats()["events"]


def test_errors_change_nothing(pkg, hip, history):
    g = history
    n = g["n"]
    keys = [pk for pk, _ in g["kps"]]
    K = 8
    ev = lambda s=slice(0, K): (g["cr"][s], g["sp"][s], g["op"][s], g["t"][s])
    # ---- what must be set first
    h = pkg.Hashgraph(n)
    refused(pkg, ENOTSUP, h.sign_events, *ev())                      # no member keys
    refused(pkg, ENOTSUP, h.set_signing_seeds, [0], [g["seeds"][0]])
    h.set_member_keys(keys)
    refused(pkg, ENOTSUP, h.sign_events, *ev())                      # no signing keys
    refused(pkg, ENOTSUP, h.create_events, *ev())
    refused(pkg, EINVAL, h.set_signing_seeds, [0, 1], [g["seeds"][0], g["seeds"][2]])     # a wrong seed: nothing changed
    refused(pkg, EINVAL, h.set_signing_seeds, [1, 1], [g["seeds"][1], g["seeds"][1]])     # twice
    refused(pkg, EINVAL, h.set_signing_seeds, [n], [g["seeds"][0]])                       # out of range
    assert not h.signing_members().any()
    some = [m for m in range(n) if m != int(g["cr"][3])]
    h.set_signing_seeds(some, [g["seeds"][m] for m in some])
    assert h.signing_members().tolist() == [m in some for m in range(n)]
    assert int(np.flatnonzero(g["cr"] == g["cr"][3])[0]) == 3
    assert "event 3" in refused(pkg, EINVAL, h.sign_events, *ev())   # a creator without a key
    refused(pkg, EINVAL, h.create_events, *ev())
    h.set_signing_seeds([int(g["cr"][3])], [g["seeds"][int(g["cr"][3])]])
    assert h.signing_members().all() and h.sign_stats()["key_sets"] == 2
    assert counts(h) == (0, 0, 0)
    assert h.create_events(*ev(), g["d"][:K]) == 0                   # K stored events with ids and data
    base = counts(h)
    assert base == (K, K, K)
    # ---- K = 0
    none = np.zeros(0, np.int32)
    assert h.create_events(none, none, none, np.zeros(0)) == K and counts(h) == base
    assert h.sign_events(none, none, none, np.zeros(0))["ids"].shape == (0, 32)
    # ---- structural defects: the append's verdict on the same arrays, lowest offender first
    nxt = slice(K, K + 6)
    cr, sp, op, t = (x.copy() for x in ev(nxt))
    assert sp[4] >= 0 and sp[5] >= 0
    own = lambda m: int(np.flatnonzero(g["cr"][:K] == m)[-1])        # a stored event of member m
    cases = []
    for name, edit in (("creator", lambda c, s, o: c.__setitem__(4, n)), ("arity", lambda c, s, o: s.__setitem__(4, -1)),
                       ("order", lambda c, s, o: o.__setitem__(4, K + 4)), ("self", lambda c, s, o: s.__setitem__(4, own((c[4] + 1) % n))),
                       ("other", lambda c, s, o: o.__setitem__(4, own(c[4])))):
        c2, s2, o2 = cr.copy(), sp.copy(), op.copy()
        edit(c2, s2, o2)
        c2[5] = -1                                                   # a later event with the lowest code: it must not win
        cases.append((name, c2, s2, o2))
    for name, c2, s2, o2 in cases:
        msg = refused(pkg, EINVAL, h.sign_events, c2, s2, o2, t)
        want = refused(pkg, EINVAL, h.append_events_device, hip.up(c2, np.int32), hip.up(s2, np.int32), hip.up(o2, np.int32), count=6)
        assert msg == want and ("event %d" % (K + 4)) in msg, name
        assert refused(pkg, EINVAL, h.create_events, c2, s2, o2, t) == want
        assert counts(h) == base
    # ---- data that cannot be signed
    bad_off = np.array([0, 1, 2, 1, 2, 3, 4], np.int64)
    assert "event %d" % (K + 2) in refused(pkg, EINVAL, h.sign_events, cr, sp, op, t, np.zeros(8, np.uint8), bad_off)
    long_off = np.array([0, 60001, 60001, 60001, 60001, 60001, 60001], np.int64)
    assert "event %d" % K in refused(pkg, EINVAL, h.create_events, cr, sp, op, t, np.zeros(60001, np.uint8), long_off)
    assert counts(h) == base
    # ---- the device forms: a host pointer, a misaligned id array
    d = {k: hip.up(v, dt) for k, v, dt in (("cr", cr, np.int32), ("sp", sp, np.int32), ("op", op, np.int32), ("t", t, np.float64))}
    out = [hip.alloc(64 * 6 + 16) for _ in range(5)]
    refused(pkg, EINVAL, h.sign_events_device, cr.ctypes.data, d["sp"], d["op"], d["t"], *out, count=6)
    refused(pkg, EINVAL, h.sign_events_device, d["cr"], d["sp"], d["op"], d["t"], out[0] + 8, *out[1:], count=6)
    refused(pkg, EINVAL, h.create_events_device, d["cr"], d["sp"], d["op"], t.ctypes.data, count=6)
    refused(pkg, EINVAL, h.create_events_device, d["cr"], d["sp"], d["op"], d["t"], ids=out[0] + 8, count=6)
    h.sign_events_device(d["cr"], d["sp"], d["op"], d["t"], *out, count=6)
    e_ids, e_sig = host_sign(pkg, g["kps"], cr, sp, op, t, [None] * 6, [bytes(i) for i in g["ids"][:K]])
    assert np.array_equal(hip.down(out[0], 6 * 32, np.uint8).reshape(6, 32), e_ids)
    assert np.array_equal(hip.down(out[4], 6 * 64, np.uint8).reshape(6, 64), e_sig)
    assert counts(h) == base
    # ---- an incomplete id index
    h.append_events(cr, sp, op, t)
    refused(pkg, ENOTSUP, h.sign_events, *ev(slice(K + 6, K + 8)))
    refused(pkg, ENOTSUP, h.create_events, *ev(slice(K + 6, K + 8)))
    assert counts(h) == (K + 6, K, K)
    # ---- cleared keys; member keys set again drop them too
    g2 = signer(pkg, n, g["seeds"], g["kps"])
    g2.clear_signing_seeds()
    assert not g2.signing_members().any()
    refused(pkg, ENOTSUP, g2.sign_events, *ev())
    g2.set_signing_seeds(list(range(n)), g["seeds"])
    g2.sign_events(*ev())
    g2.set_member_keys(keys)
    refused(pkg, ENOTSUP, g2.sign_events, *ev())
    assert counts(g2) == (0, 0, 0)
    h.close()
    g2.close()


def test_a_fork_is_signed_and_stored_on_the_exact_path(pkg, history):
    g = history
    n, K = g["n"], 40
    s = slice(0, K)
    m = int(g["cr"][K - 1])
    last = int(np.flatnonzero(g["cr"][:K] == m)[-1])
    other = int(np.flatnonzero(g["cr"][:K] != m)[-1])
    sp_last = int(g["sp"][last])
    assert sp_last >= 0
    # two more events of member m: one on its latest event, one on that event's self-parent again — a fork
    cr = np.array([m, m], np.int32)
    sp = np.array([last, sp_last], np.int32)
    op = np.array([other, other], np.int32)
    t = np.array([1e6, 1e6 + 1])
    for accept in (True, False):
        h = created(pkg, g, (0, K))
        h.set_forks(accept)
        ids = [bytes(i) for i in g["ids"][:K]]
        e_ids, e_sig = host_sign(pkg, g["kps"], cr, sp, op, t, [None, b"fork"], ids)
        check_signed(h.sign_events(cr, sp, op, t, [None, b"fork"]), e_ids, e_sig, sp, ids)
        if accept:
            assert h.create_events(cr, sp, op, t, [None, b"fork"]) == K
            assert h.exact and h.num_events == K + 2
            assert np.array_equal(h.event_ids(K), e_ids) and h.unpack_data(*h.get_event_data(K)) == [None, b"fork"]
        else:
            refused(pkg, ENOTSUP, h.create_events, cr, sp, op, t, [None, b"fork"])
            assert counts(h) == (K, K, K) and not h.exact
            assert h.create_events(cr[:1], sp[:1], op[:1], t[:1]) == K      # the id index is as it was: the first event alone goes in
        h.close()


def test_sign_events_is_read_only(pkg, history):
    g = history
    K = 300
    h = created(pkg, g, (0, K))
    h.divide_rounds(0, K)
    new_c = list(h.decide_fame())
    h.find_order(new_c)

    def snapshot():
        c = h.counters()
        c.pop("kernel_launches")
        return (h.rounds().tobytes(), h.witnesses().tobytes(), h.famous().tobytes(), h.heights().tobytes(), h.num_events, h.max_round, h.num_ordered,
                h.event_ids().tobytes(), tuple(a.tobytes() for a in h.get_event_data()), h.data_stats(), h.payload_stats(), h.ingest_stats(),
                h.export_stats(), c, h.signing_members().tobytes(), h.transactions().tobytes())

    before = snapshot()
    s = slice(K, g["N"])
    out = h.sign_events(g["cr"][s], g["sp"][s], g["op"][s], g["t"][s], g["d"][s])
    assert np.array_equal(out["ids"], g["ids"][s]) and np.array_equal(out["sig"], g["sig"][s])
    assert snapshot() == before
    h.close()
