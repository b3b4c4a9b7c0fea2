"""GPU (-m gpu): validation of payloads against the member key table (sw_set_member_keys, sw_validate_payload[_device];
csrc/validate.hip.h).  The verdicts — through the host-array form and through the device form — must be libsodium
1.0.18's and hashlib's on the case sets of tests/test_validate_host.py (adversarial encodings, keys of mixed order, the
padding edges of both hashes), for every batch size around a wavefront, for 1, 4 and 1 024 members; events whose creator
or offsets are out of range are invalid and nothing outside the buffers is read; the verdicts left on the device feed
sw_ingest_payload_device on the same stream; the call changes nothing of the hashgraph; and a Node simulation validated
this way reproduces the host-validated one.

No torch here (see tests/test_gpu_ingest_device.py): device buffers come through ctypes from the HIP runtime the library
is linked against."""
import contextlib
import hashlib
import io
import random
from pickle import dumps

import numpy as np
import pytest

from test_crypto_host import signed_cases, sodium_verify
from test_gpu_payload import Hip
from test_validate_host import MSG_EDGES, WHOLE_EDGES, _signed, members_of, mixed_order_cases, pack, sodium

pytestmark = pytest.mark.gpu


@pytest.fixture
def hip(pkg):
    h = Hip(pkg)
    yield h
    h.free()


def dev_validate(h, hip, msgs, sigs, creator, whole=None, ids=None, msg_bytes=None, msg_off=None, slack=0):
    """The verdicts of validate_payload_device as a bool array.  `slack`: bytes the message buffer is allocated beyond the
    msg_bytes the call is told about."""
    data, off = pack(msgs)
    if msg_off is not None:
        off = np.ascontiguousarray(msg_off, np.int64)
    K = len(off) - 1
    nbytes = len(data) - 1 if msg_bytes is None else msg_bytes
    d_ok = hip.alloc(K)
    kw = {}
    if whole is not None:
        wdata, woff = pack(whole)
        kw = dict(whole=hip.up(wdata, np.uint8), whole_off=hip.up(woff, np.int64), whole_bytes=len(wdata) - 1,
                  ids=hip.up(np.frombuffer(b"".join(ids) + bytes(8), np.uint8), np.uint8))
    buf = np.concatenate([data, np.zeros(slack, np.uint8)])
    h.validate_payload_device(hip.up(buf, np.uint8), hip.up(off, np.int64), nbytes, hip.up(np.frombuffer(b"".join(sigs) + bytes(8), np.uint8), np.uint8),
                              hip.up(np.ascontiguousarray(creator, np.int32) if K else np.zeros(1, np.int32), np.int32), d_ok, count=K, **kw)
    return hip.down(d_ok, K, np.uint8).astype(bool)


def both_routes(h, hip, msgs, sigs, creator, whole=None, ids=None):
    a = h.validate_payload(msgs, np.frombuffer(b"".join(sigs), np.uint8), creator, whole=whole,
                           ids=None if ids is None else np.frombuffer(b"".join(ids), np.uint8))
    b = dev_validate(h, hip, msgs, sigs, creator, whole, ids)
    assert np.array_equal(a, b), "host-array form and device form disagree"
    return a


@pytest.fixture(scope="module")
def sod():
    return sodium()


@pytest.fixture(scope="module")
def adversarial(sod):
    cases = signed_cases(sod, random.Random(3), 40)
    return cases, np.array([sodium_verify(sod, s, m, p) for s, m, p in cases])


@pytest.fixture(scope="module")
def mixed(sod):
    cases = mixed_order_cases(random.Random(5))
    return cases, np.array([sodium_verify(sod, s, m, p) for s, m, p in cases])


@pytest.fixture(scope="module")
def pool(sod):
    """257 signed events of 4 members with ids, every 9th tampered (signature, message or id in turn); expected verdicts."""
    rng = random.Random(21)
    keys, msgs, sigs, creator = _signed(sod, rng, 4, [rng.randrange(150, 250) for _ in range(257)])
    whole = [m + s for m, s in zip(msgs, sigs)]
    ids = [hashlib.blake2b(w, digest_size=32).digest() for w in whole]
    for i in range(0, 257, 9):
        if (i // 9) % 3 == 0:
            sigs[i] = bytes([sigs[i][0] ^ 4]) + sigs[i][1:]
        elif (i // 9) % 3 == 1:
            msgs[i] = msgs[i][:-1] + bytes([msgs[i][-1] ^ 1])
        else:
            ids[i] = ids[i][:31] + bytes([ids[i][31] ^ 0x80])
    exp = np.array([sodium_verify(sod, s, m, keys[c]) and hashlib.blake2b(w, digest_size=32).digest() == i
                    for s, m, c, w, i in zip(sigs, msgs, creator, whole, ids)])
    assert 20 < (~exp).sum() < 40
    return keys, msgs, sigs, creator, whole, ids, exp


def test_verdicts_on_the_adversarial_set(pkg, hip, adversarial):
    cases, exp = adversarial
    keys, creator = members_of(cases)
    h = pkg.Hashgraph(len(keys))
    bad = h.set_member_keys(keys)
    k2, usable = h.member_keys()
    assert 0 < bad < len(keys) and bad == (~usable).sum() and [bytes(k) for k in k2] == keys
    got = both_routes(h, hip, [m for _, m, _ in cases], [s for s, _, _ in cases], creator)
    assert np.array_equal(got, exp) and exp.sum() >= 40 and (~exp).sum() > 300
    st = h.validate_stats()
    assert st["calls"] == 2 and st["events"] == 2 * len(cases) and st["accepted"] == exp.sum() and st["table_builds"] == 1
    h.close()


def test_verdicts_on_keys_of_mixed_order(pkg, hip, mixed):
    cases, exp = mixed
    keys, creator = members_of(cases)
    assert exp.sum() >= 8 and (~exp).sum() >= 8
    h = pkg.Hashgraph(len(keys))
    assert h.set_member_keys(keys) == 0
    assert np.array_equal(both_routes(h, hip, [m for _, m, _ in cases], [s for s, _, _ in cases], creator), exp)
    h.close()


def test_length_boundaries_of_both_hashes(pkg, hip, sod):
    rng = random.Random(7)
    lengths = [a for a in MSG_EDGES for _ in WHOLE_EDGES]
    keys, msgs, sigs, creator = _signed(sod, rng, 3, lengths)
    whole = [bytes(rng.getrandbits(8) for _ in range(w)) for _ in MSG_EDGES for w in WHOLE_EDGES]
    ids = [hashlib.blake2b(w, digest_size=32).digest() for w in whole]
    h = pkg.Hashgraph(3)
    h.set_member_keys(keys)
    assert both_routes(h, hip, msgs, sigs, creator, whole, ids).all()
    assert not both_routes(h, hip, [m + b"\0" for m in msgs], sigs, creator, whole, ids).any()
    h.close()


@pytest.mark.parametrize("K", [0, 1, 63, 64, 65, 257])
def test_batch_sizes(pkg, hip, pool, K):
    keys, msgs, sigs, creator, whole, ids, exp = pool
    h = pkg.Hashgraph(4)
    h.set_member_keys(keys)
    got = both_routes(h, hip, msgs[:K], sigs[:K], creator[:K], whole[:K], ids[:K])
    assert got.shape == (K,) and np.array_equal(got, exp[:K])
    h.close()


def test_id_check(pkg, hip, pool):
    keys, msgs, sigs, creator, whole, ids, exp = pool
    sl = slice(1, 9)   # eight untampered events
    m, s, c, w, i = msgs[sl], sigs[sl], creator[sl], list(whole[sl]), list(ids[sl])
    h = pkg.Hashgraph(4)
    h.set_member_keys(keys)
    assert both_routes(h, hip, m, s, c, w, i).all()
    i2 = list(i)
    i2[3] = i2[3][:7] + bytes([i2[3][7] ^ 0x10]) + i2[3][8:]
    assert both_routes(h, hip, m, s, c, w, i2).tolist() == [True] * 3 + [False] + [True] * 4
    w2 = list(w)
    w2[5] = w2[5][:40] + bytes([w2[5][40] ^ 0xff]) + w2[5][41:]
    assert both_routes(h, hip, m, s, c, w2, i).tolist() == [True] * 5 + [False] + [True] * 2
    assert both_routes(h, hip, m, s, c).all()                       # whole = NULL: no id check ...
    assert both_routes(h, hip, msgs[:20], sigs[:20], creator[:20]).tolist() == \
        [sodium_verify(sodium(), sg, mm, keys[cc]) for sg, mm, cc in zip(sigs[:20], msgs[:20], creator[:20])]   # ... wrong ids and all
    h.close()


def test_rejected_inputs(pkg, hip, sod, pool):
    keys, msgs, sigs, creator, _, _, _ = pool
    m, s = msgs[1:9], sigs[1:9]
    c = np.array(creator[1:9], np.int32)
    h = pkg.Hashgraph(4)
    h.set_member_keys(keys)
    assert both_routes(h, hip, m, s, c).all()
    c2 = c.copy()
    c2[2], c2[6] = -1, 4
    assert both_routes(h, hip, m, s, c2).tolist() == [True, True, False, True, True, True, False, True]
    # offsets: the buffer is 4 KB larger than the msg_bytes the call is told about
    _, off = pack(m)
    total = int(off[-1])
    assert dev_validate(h, hip, m, s, c, slack=4096).all()
    assert dev_validate(h, hip, m, s, c, msg_bytes=total - 1, slack=4096).tolist() == [True] * 7 + [False]
    dec = off.copy()
    dec[3] = dec[2] - 1   # event 2 ends before it starts; event 3 then covers other bytes than were signed
    assert dev_validate(h, hip, m, s, c, msg_off=dec, slack=4096).tolist() == [True, True, False, False, True, True, True, True]
    neg = off.copy()
    neg[0] = -3
    assert dev_validate(h, hip, m, s, c, msg_off=neg, slack=4096).tolist() == [False] + [True] * 7
    far = off.copy()
    far[8] = total + 4000
    assert dev_validate(h, hip, m, s, c, msg_off=far, slack=4096).tolist() == [True] * 7 + [False]
    # a member with an unusable key: its events are invalid, its neighbours' are not
    keys2 = list(keys)
    keys2[1] = (1).to_bytes(32, "little")   # the identity: small order
    assert h.set_member_keys(keys2) == 1
    assert not h.member_keys()[1][1] and h.member_keys()[1].sum() == 3
    assert both_routes(h, hip, m, s, c).tolist() == [cc != 1 for cc in c.tolist()]
    assert h.validate_stats()["table_builds"] == 2
    h.close()


@pytest.mark.parametrize("n", [1, 4])
def test_small_member_counts(pkg, hip, sod, n):
    rng = random.Random(30 + n)
    keys, msgs, sigs, creator = _signed(sod, rng, n, [rng.randrange(0, 300) for _ in range(70)])
    sigs[5] = sigs[5][:40] + bytes([sigs[5][40] ^ 2]) + sigs[5][41:]
    exp = [sodium_verify(sod, s, m, keys[c]) for s, m, c in zip(sigs, msgs, creator)]
    h = pkg.Hashgraph(n)
    h.set_member_keys(keys)
    assert both_routes(h, hip, msgs, sigs, creator).tolist() == exp and exp.count(False) == 1
    h.close()


def test_1024_members(pkg, hip, sod):
    rng = random.Random(41)
    n, K = 1024, 2048
    keys, msgs, sigs, creator = _signed(sod, rng, n, [rng.randrange(20, 120) for _ in range(K)])
    assert sorted(creator) == sorted(list(range(n)) * 2)   # every member twice
    for i in range(0, K, 97):
        sigs[i] = sigs[i][:33] + bytes([sigs[i][33] ^ 1]) + sigs[i][34:]
    for i in range(5, K, 131):
        creator[i] = (creator[i] + 1) % n   # somebody else's signature
    exp = np.array([sodium_verify(sod, s, m, keys[c]) for s, m, c in zip(sigs, msgs, creator)])
    assert 25 < (~exp).sum() < 60
    h = pkg.Hashgraph(n)
    assert h.set_member_keys(keys) == 0
    assert np.array_equal(both_routes(h, hip, msgs, sigs, creator), exp)
    assert h.validate_stats()["table_builds"] == 1
    h.close()


def _seeded_nodes(pkg, turns, **attrs):
    """pkg.test(4, turns) with seeded keys, partners and clock, and the given Node class attributes."""
    node_mod = pkg.node
    rng = random.Random(20261019)
    saved = (node_mod.crypto.randombytes, node_mod.time, {k: getattr(node_mod.Node, k) for k in attrs})
    clock = iter(range(1, 1 << 30))
    node_mod.crypto.randombytes = lambda k: bytes(rng.getrandbits(8) for _ in range(k))
    node_mod.time = lambda: 1.0e9 + 0.001 * next(clock)
    for k, v in attrs.items():
        setattr(node_mod.Node, k, v)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return pkg.test(4, turns)
    finally:
        node_mod.crypto.randombytes, node_mod.time = saved[0], saved[1]
        for k, v in saved[2].items():
            setattr(node_mod.Node, k, v)


def test_verdicts_chain_into_the_ingest_on_one_stream(pkg, hip, sod):
    assert pkg.node.crypto.HAVE_SODIUM
    nodes = _seeded_nodes(pkg, 60)
    nd = max(nodes, key=lambda x: len(x._ids))
    eids = list(nd._ids)
    K = len(eids)
    assert K >= 30, K   # (about 60; the exact count follows the iteration order of Python sets in Node.sync)
    events = [nd.hg[e] for e in eids]
    members = list(nd._members)
    rng = random.Random(4)
    perm = list(range(K))
    rng.shuffle(perm)
    eids, events = [eids[i] for i in perm], [events[i] for i in perm]
    msgs, whole = [dumps(ev[:-1]) for ev in events], [dumps(ev) for ev in events]
    sigs, ids = [bytes(ev.s) for ev in events], [bytes(e) for e in eids]
    creator = np.array([members.index(ev.c) for ev in events], np.int32)
    for k, i in enumerate(rng.sample(range(K), 5)):   # signature, message, id, signature, message
        if k % 3 == 0:
            sigs[i] = sigs[i][:10] + bytes([sigs[i][10] ^ 8]) + sigs[i][11:]
        elif k % 3 == 1:
            msgs[i] = msgs[i][:-2] + bytes([msgs[i][-2] ^ 1]) + msgs[i][-1:]
        else:
            whole[i] = whole[i][:-3] + bytes([whole[i][-3] ^ 1]) + whole[i][-2:]
    ok_host = np.array([sodium_verify(sod, s, m, members[c]) and hashlib.blake2b(w, digest_size=32).digest() == i
                        for s, m, c, w, i in zip(sigs, msgs, creator, whole, ids)], np.uint8)
    assert (ok_host == 0).sum() == 5
    ida = np.frombuffer(b"".join(ids), np.uint8).reshape(K, 32)
    par = np.zeros((2, K, 32), np.uint8)
    arity = np.zeros(K, np.uint8)
    for i, ev in enumerate(events):
        arity[i] = len(ev.p)
        for q in range(len(ev.p)):
            par[q, i] = np.frombuffer(bytes(ev.p[q]), np.uint8)
    t = np.array([float(ev.t) for ev in events])
    sg = np.frombuffer(b"".join(bytes(ev.s) for ev in events), np.uint8).reshape(K, 64)

    ref = pkg.Hashgraph(4)
    out_ref, stored_ref = ref.ingest_payload(ida, par[0], par[1], arity, creator, ok_host, t, sg)

    h = pkg.Hashgraph(4)
    h.set_member_keys(members)
    data, off = pack(msgs)
    wdata, woff = pack(whole)
    d_ids, d_cr, d_ok, d_out = hip.up(ida, np.uint8), hip.up(creator, np.int32), hip.alloc(K), hip.alloc(4 * K)
    h.validate_payload_device(hip.up(data, np.uint8), hip.up(off, np.int64), len(data) - 1, hip.up(np.frombuffer(b"".join(sigs), np.uint8), np.uint8),
                              d_cr, d_ok, whole=hip.up(wdata, np.uint8), whole_off=hip.up(woff, np.int64), whole_bytes=len(wdata) - 1,
                              ids=d_ids, stream=0, count=K)
    _, stored = h.ingest_payload_device(d_ids, hip.up(par[0], np.uint8), hip.up(par[1], np.uint8), hip.up(arity, np.uint8), d_cr, d_ok,
                                        hip.up(t, np.float64), hip.up(sg, np.uint8), index_out=d_out, stream=0, count=K)
    out = hip.down(d_out, K, np.int32)
    assert np.array_equal(hip.down(d_ok, K, np.uint8), ok_host)
    assert stored == stored_ref and np.array_equal(out, out_ref)
    assert (out[ok_host == 0] == -3).all() and 0 < stored < K
    h.close()
    ref.close()


def test_state_errors_and_read_only(pkg, hip, pool):
    keys, msgs, sigs, creator, whole, ids, exp = pool
    sl = slice(0, 40)
    args = (msgs[sl], sigs[sl], creator[sl], whole[sl], ids[sl])
    n, N = 4, 400
    h = pkg.Hashgraph(n)
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.validate_payload(args[0], np.frombuffer(b"".join(args[1]), np.uint8), args[2])
    assert ei.value.code == -95   # SW_ENOTSUP: no keys yet
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.member_keys()
    assert ei.value.code == -95
    stream = pkg.synth_hashgraph(n, N, 3)
    h.append_events(*stream)
    ev_ids = np.random.default_rng(1).integers(0, 256, (N, 32), dtype=np.uint8)
    h.set_event_ids(0, ev_ids)
    h.divide_rounds(0, N)
    h.decide_fame()
    h.set_member_keys(keys)
    before = (h.num_events, h.rounds().copy(), h.lookup_event_ids(ev_ids).copy(), h.witnesses().copy(), h.max_round)
    got = both_routes(h, hip, *args)
    assert np.array_equal(got, exp[sl])
    after = (h.num_events, h.rounds(), h.lookup_event_ids(ev_ids), h.witnesses(), h.max_round)
    assert before[0] == after[0] and before[4] == after[4] and all(np.array_equal(a, b) for a, b in zip(before[1:4], after[1:4]))
    # a host pointer is refused before anything is launched
    host = np.zeros(64, np.uint8)
    d_ok = hip.alloc(8)
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.validate_payload_device(int(host.ctypes.data), hip.up(np.zeros(2, np.int64), np.int64), 8, hip.up(np.zeros(64, np.uint8), np.uint8),
                                  hip.up(np.zeros(1, np.int32), np.int32), d_ok, count=1)
    assert ei.value.code == -22
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.validate_payload_device(hip.up(np.zeros(64, np.uint8), np.uint8), hip.up(np.zeros(2, np.int64), np.int64), 0,
                                  hip.up(np.zeros(64, np.uint8), np.uint8), hip.up(np.zeros(1, np.int32), np.int32), int(host.ctypes.data), count=1)
    assert ei.value.code == -22
    # keys and verdicts survive sw_rewind and sw_reset
    for forget in (h.rewind, h.reset):
        forget()
        assert [bytes(k) for k in h.member_keys()[0]] == keys
        assert np.array_equal(both_routes(h, hip, *args), exp[sl])
    assert h.validate_stats()["table_builds"] == 1
    # other keys, other verdicts: members 0 and 1 swapped
    swapped = [keys[1], keys[0]] + keys[2:]
    h.set_member_keys(swapped)
    assert [bytes(k) for k in h.member_keys()[0]] == swapped
    exp2 = exp[sl] & np.array([c >= 2 for c in creator[sl]])
    assert np.array_equal(both_routes(h, hip, *args), exp2) and exp2.any() and (exp2 != exp[sl]).any()
    assert h.validate_stats()["table_builds"] == 2
    h.close()


def test_exact_path_and_windowed_table(pkg, hip, pool):
    keys, msgs, sigs, creator, whole, ids, exp = pool
    sl = slice(0, 30)
    h = pkg.Hashgraph(4)
    h.set_forks(True)
    h.set_member_keys(keys)
    h.append_events(np.array([0, 1, 2, 3, 0, 0], np.int32), np.array([-1, -1, -1, -1, 0, 0], np.int32), np.array([-1, -1, -1, -1, 1, 2], np.int32))
    h.divide_rounds(0, 6)
    assert h.exact   # a fork: the context is on the exact path
    assert np.array_equal(both_routes(h, hip, msgs[sl], sigs[sl], creator[sl], whole[sl], ids[sl]), exp[sl])
    h.close()
    w = pkg.Hashgraph(4)
    w.set_window(True)
    w.set_member_keys(keys)
    assert np.array_equal(both_routes(w, hip, msgs[sl], sigs[sl], creator[sl], whole[sl], ids[sl]), exp[sl])
    w.close()


def test_node_simulation_with_device_validation(pkg):
    """Every sync payload validated against the member table (threshold 1), on the host loop's route and on the device
    payload route: the simulation must run as with libsodium on the host, and a tampered event must be rejected."""
    assert pkg.node.crypto.HAVE_SODIUM
    view = lambda nodes: [(len(nd._ids), sorted(nd.consensus), len(nd.transactions)) for nd in nodes]
    host = _seeded_nodes(pkg, 120, device_validate_threshold=None)
    dev = _seeded_nodes(pkg, 120, device_validate_threshold=1)
    assert view(host) == view(dev), "device-validated gossip reproduces host-validated gossip"
    assert all(nd._dev.validate_stats()["calls"] == 0 for nd in host)
    assert any(nd._dev.validate_stats()["calls"] > 0 for nd in dev) and all(nd._dev.validate_stats()["table_builds"] <= 1 for nd in dev)
    p_host = _seeded_nodes(pkg, 120, device_validate_threshold=None, device_payload_threshold=1)
    p_dev = _seeded_nodes(pkg, 120, device_validate_threshold=1, device_payload_threshold=1)
    assert view(p_host) == view(p_dev)
    assert any(nd._dev.validate_stats()["calls"] > 0 and nd._device_payloads > 0 for nd in p_dev)
    nd, other = dev[0], dev[1]
    h = other._ids[-1]
    ev = other.hg[h]
    saved = pkg.node.Node.device_validate_threshold
    try:
        pkg.node.Node.device_validate_threshold = 1
        assert nd._batch_validate([h], {h: ev})[h] == (True, h)
        bad = ev._replace(s=bytes([ev.s[0] ^ 1]) + ev.s[1:])
        assert nd._batch_validate([h], {h: bad})[h][0] is False
        assert nd._batch_validate([h], {h: ev._replace(t=ev.t + 1.0)})[h][0] is False        # another message under the signature
        wrong = hashlib.blake2b(h, digest_size=32).digest()
        assert nd._batch_validate([wrong], {wrong: ev})[wrong][0] is False                   # the id is not the event's hash
        assert nd._batch_validate([h], {h: ev._replace(s=b"short")})[h][0] is False          # malformed: invalid on the host side
    finally:
        pkg.node.Node.device_validate_threshold = saved
