"""GPU (-m gpu): the signed bytes of events built on the device (sw_pack_events[_device], sw_sync_pull_validated;
csrc/pack.hip.h).  Both forms must write exactly what tests/model_pack.py writes — offsets, both streams, flags — and
nothing behind off[K]; the refusals come before any launch; the packed streams, fed to validate_payload_device, give the
verdicts validate_payload gives on the same events pickled on the host; pull_from(validate=True) stores what the
unvalidated pull stores when everything is valid, and what ingest_payload stores under the host route's verdicts when
some signatures are corrupt; and packing changes nothing of the hashgraph.

No torch here (see tests/test_gpu_ingest_device.py): device buffers come through ctypes from the HIP runtime the library
is linked against."""
import pickle

import numpy as np
import pytest

import model_pack as mp
from test_gpu_payload import Hip
from test_pack_kernels_host import events, with_data

pytestmark = pytest.mark.gpu

LONG = ("m" * 255, "é" * 127 + "Q")      # 255 bytes of UTF-8 each
SHORT = ("m", "Q")


@pytest.fixture
def hip(pkg):
    h = Hip(pkg)
    yield h
    h.free()


def dev_pack(h, hip, a, slack=48, enc=True):
    """pack_events_device on uploaded arrays; returns (msgs, msg_off, whole, whole_off, flags) with the WHOLE buffers,
    canary included (0xA5 where nothing was written)."""
    K = len(a["arity"])
    has = "data_off" in a
    nbytes = len(a["data"]) if has else 0
    bm, bw = h.pack_bound(K, nbytes)
    d_m, d_w = hip.up(np.full(bm + slack, 0xA5, np.uint8), np.uint8), hip.up(np.full(bw + slack, 0xA5, np.uint8), np.uint8)
    d_mo, d_wo, d_enc = hip.alloc(8 * (K + 1)), hip.alloc(8 * (K + 1)), hip.alloc(K) if enc else None
    kw = {}
    if has:
        kw = dict(data=hip.up(a["data"], np.uint8) if nbytes else None, data_off=hip.up(a["data_off"], np.int64), data_bytes=nbytes,
                  data_none=hip.up(a["data_none"], np.uint8) if "data_none" in a else None)
    h.pack_events_device(hip.up(a["sp"], np.uint8), hip.up(a["op"], np.uint8), hip.up(a["arity"], np.uint8), hip.up(a["creator"], np.int32),
                         hip.up(a["t"], np.float64), hip.up(a["sig"], np.uint8), d_m, d_mo, bm, d_w, d_wo, bw, encodable=d_enc, count=K, **kw)
    return (hip.down(d_m, bm + slack, np.uint8), hip.down(d_mo, K + 1, np.int64), hip.down(d_w, bw + slack, np.uint8),
            hip.down(d_wo, K + 1, np.int64), hip.down(d_enc, K, np.uint8) if enc else None)


def model_of(a, mod, qual):
    return mp.pack(a["keys"], a["sp"], a["op"], a["arity"], a["creator"], a["t"], a["sig"], a.get("data"), a.get("data_off"),
                   a.get("data_none"), mod, qual)


def assert_device_equals_model(got, exp):
    msgs, moff, whole, woff, enc = got
    e_msgs, e_moff, e_whole, e_woff, e_enc = exp
    assert np.array_equal(moff, e_moff) and np.array_equal(woff, e_woff), "offsets"
    assert np.array_equal(enc, e_enc), "flags"
    for g, e, what in ((msgs, e_msgs, "msgs"), (whole, e_whole, "whole")):
        bad = np.flatnonzero(g[:len(e)] != e)
        assert bad.size == 0, "%s: first differing byte at %d of %d" % (what, bad[0], len(e))
        assert (g[len(e):] == 0xA5).all(), "%s: bytes at or beyond off[K] were written" % what


@pytest.mark.parametrize("n", [5, 70])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 1000])
def test_both_forms_equal_the_model(pkg, hip, K, n):
    h = pkg.Hashgraph(n)
    rng = np.random.default_rng(K * 100 + n)
    plain = events(K, n, 900 + K + n, 0.3)
    bad = plain["creator"].copy()
    if K > 8:
        plain["arity"][[2, 5]] = [1, 255]
        bad[[3, 7]] = [-1, n]
    plain["creator"] = bad
    lens = rng.choice([0, 1, 31, 32, 255, 256, 257, 700], K)
    rich = with_data(events(K, n, 950 + K + n, 0.5), lens, 7, rng.random(K) < 0.2)
    h.set_member_keys(plain["keys"])
    for a in (plain, rich):
        a["keys"] = plain["keys"]
        for mod, qual in (SHORT, LONG):
            h.set_event_class(mod, qual)
            assert h.event_class() == (mod, qual)
            exp = model_of(a, mod, qual)
            assert_device_equals_model(dev_pack(h, hip, a), exp)
            hip.free()
            kw = {k: a[k] for k in ("data", "data_off", "data_none") if k in a}
            msgs, moff, whole, woff, enc = h.pack_events(a["sp"], a["op"], a["arity"], a["creator"], a["t"], a["sig"], **kw)
            assert np.array_equal(moff, exp[1]) and np.array_equal(woff, exp[3]) and np.array_equal(enc, exp[4].astype(bool))
            assert msgs.tobytes() == exp[0].tobytes() and whole.tobytes() == exp[2].tobytes()
            assert mp.bound(K, len(a["data"]) if "data" in a else 0, mod, qual) == h.pack_bound(K, len(a["data"]) if "data" in a else 0)
    st = h.pack_stats()
    assert st["calls"] == 8 and st["events"] == 8 * K and st["bytes"] > 0
    h.close()


def test_one_event_of_60001_bytes_and_one_of_60000(pkg, hip):
    h = pkg.Hashgraph(5)
    a = with_data(events(4, 5, 31, 0.5), [60000, 60001, 0, 4095], 8)
    h.set_member_keys(a["keys"])
    exp = model_of(a, "swirld", "Event")
    assert exp[4].tolist() == [1, 0, 1, 1]
    assert_device_equals_model(dev_pack(h, hip, a), exp)
    h.close()


def test_refusals_come_before_any_launch(pkg, hip):
    n, K = 5, 40
    a = events(K, n, 41)
    h = pkg.Hashgraph(n)
    up = lambda: (hip.up(a["sp"], np.uint8), hip.up(a["op"], np.uint8), hip.up(a["arity"], np.uint8), hip.up(a["creator"], np.int32),
                  hip.up(a["t"], np.float64), hip.up(a["sig"], np.uint8))
    bm, bw = h.pack_bound(K)
    assert (bm, bw) == mp.bound(K, 0)
    d_m, d_w = hip.up(np.full(bm + 32, 0xA5, np.uint8), np.uint8), hip.up(np.full(bw + 32, 0xA5, np.uint8), np.uint8)
    d_mo, d_wo = hip.up(np.full(K + 1, -7, np.int64), np.int64), hip.up(np.full(K + 1, -7, np.int64), np.int64)

    def refused(code, *args, **kw):
        launches = h.counters()["kernel_launches"]
        with pytest.raises(pkg.SwirldHipError) as ei:
            h.pack_events_device(*args, count=K, **kw)
        assert ei.value.code == code, ei.value
        assert h.counters()["kernel_launches"] == launches
    ins = up()
    refused(-95, *ins, d_m, d_mo, bm, d_w, d_wo, bw)                  # SW_ENOTSUP: no member keys
    with pytest.raises(pkg.SwirldHipError) as ei:
        h.pack_events(a["sp"], a["op"], a["arity"], a["creator"], a["t"], a["sig"])
    assert ei.value.code == -95
    h.set_member_keys(a["keys"])
    refused(-34, *ins, d_m, d_mo, bm - 1, d_w, d_wo, bw)              # SW_ERANGE: one byte short of the bound
    refused(-34, *ins, d_m, d_mo, bm, d_w, d_wo, bw - 1)
    refused(-22, *ins, d_m + 8, d_mo, bm, d_w, d_wo, bw)              # SW_EINVAL: a stream that is not 16-byte aligned
    refused(-22, *ins, d_m, d_mo, bm, d_w + 1, d_wo, bw)
    refused(-22, *ins, d_m, d_mo + 4, bm, d_w, d_wo, bw)              # ... offsets that are not 8-byte aligned
    refused(-22, ins[0], ins[1], ins[2], ins[3], ins[4], ins[5] + 8, d_m, d_mo, bm, d_w, d_wo, bw)   # ... signatures
    refused(-22, ins[0] + 4, *ins[1:], d_m, d_mo, bm, d_w, d_wo, bw)                                  # ... ids
    host = np.zeros(bm + 64, np.uint8)
    host_p = (int(host.ctypes.data) + 15) & ~15
    refused(-22, *ins, host_p, d_mo, bm, d_w, d_wo, bw)               # a host pointer
    refused(-22, ins[0], ins[1], int(host.ctypes.data), *ins[3:], d_m, d_mo, bm, d_w, d_wo, bw)
    for name in ("a" * 256, "", "caf\xe9".encode("latin-1")):
        rc = h._L.sw_set_event_class(h._h, name if isinstance(name, bytes) else name.encode(), b"Event")
        assert rc == -22, name
    assert h.event_class() == ("swirld", "Event")
    # nothing was written by any of the refused calls
    assert (hip.down(d_m, bm + 32, np.uint8) == 0xA5).all() and (hip.down(d_mo, K + 1, np.int64) == -7).all()
    # K = 0 writes off[0] = 0 and nothing else
    h.pack_events_device(None, None, None, None, None, None, None, d_mo, 0, None, d_wo, 0, count=0)
    assert hip.down(d_mo, 2, np.int64).tolist() == [0, -7] and hip.down(d_wo, 2, np.int64).tolist() == [0, -7]
    # the class survives rewind and reset
    h.set_event_class(*SHORT)
    h.rewind()
    h.reset()
    assert h.event_class() == SHORT
    h.close()


def signed_graph(pkg, n, N, seed, mod="swirld", qual="Event"):
    """A synthetic hashgraph whose events are really signed and really named: per event the id BLAKE2b(dumps(ev)), the
    signature over dumps(ev[:-1]) by its creator's key, and both pickles (by pickle itself)."""
    crypto = pkg.node.crypto
    cr, sp, op, t, _ = pkg.synth_hashgraph(n, N, seed)
    kps = [crypto.sign_seed_keypair(bytes([seed & 255, m & 255, m >> 8]) + bytes(29)) for m in range(n)]
    ids, sigs, msgs, wholes = [], [], [], []
    with mp.event_class(mod, qual) as Event:
        for e in range(N):
            p = () if sp[e] < 0 else (ids[sp[e]], ids[op[e]])
            body = (None, p, float(t[e]), kps[cr[e]][0])
            m = pickle.dumps(body, protocol=4)
            s = crypto.sign_detached(m, kps[cr[e]][1])
            w = pickle.dumps(Event(*body, s), protocol=4)
            msgs.append(m)
            sigs.append(s)
            wholes.append(w)
            ids.append(crypto.generichash(w))
    arr = lambda rows, w: np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), w).copy()
    return dict(n=n, N=N, cr=cr, sp=sp, op=op, t=t, keys=[pk for pk, _ in kps], ids=arr(ids, 32), sig=arr(sigs, 64), msgs=msgs, wholes=wholes)


@pytest.fixture(scope="module")
def graphs(pkg):
    return {n: signed_graph(pkg, n, 400, 700 + n) for n in (5, 70)}


def payload_arrays(g, sl):
    """The arrays of events `sl` of a signed graph as sw_export_payload_device would write them."""
    zero = np.zeros(32, np.uint8)
    sp = np.stack([g["ids"][g["sp"][e]] if g["sp"][e] >= 0 else zero for e in sl])
    op = np.stack([g["ids"][g["op"][e]] if g["op"][e] >= 0 else zero for e in sl])
    arity = np.array([2 if g["sp"][e] >= 0 else 0 for e in sl], np.uint8)
    return dict(sp=sp, op=op, arity=arity, creator=g["cr"][sl].astype(np.int32), t=g["t"][sl].copy(), sig=g["sig"][sl].copy(),
                keys=np.frombuffer(b"".join(g["keys"]), np.uint8).reshape(-1, 32))


def test_packed_streams_feed_the_validation(pkg, hip, graphs):
    g = graphs[5]
    sl = np.arange(50, 350)
    a = payload_arrays(g, sl)
    ids = g["ids"][sl].copy()
    msgs, wholes = [g["msgs"][e] for e in sl], [g["wholes"][e] for e in sl]
    # ten events with one flipped bit: signature, id or timestamp in turn.  The host route pickles what the arrays say.
    with mp.event_class("swirld", "Event") as Event:
        for j, i in enumerate(range(7, 300, 30)):
            if j % 3 == 0:
                a["sig"][i, 11] ^= 0x10
            elif j % 3 == 1:
                ids[i, 0] ^= 1
            else:
                a["t"][i:i + 1].view(np.uint64)[0] ^= 1
            p = () if a["arity"][i] == 0 else (a["sp"][i].tobytes(), a["op"][i].tobytes())
            body = (None, p, float(a["t"][i]), g["keys"][a["creator"][i]])
            msgs[i] = pickle.dumps(body, protocol=4)
            wholes[i] = pickle.dumps(Event(*body, a["sig"][i].tobytes()), protocol=4)
    h = pkg.Hashgraph(5)
    h.set_member_keys(g["keys"])
    want = h.validate_payload(msgs, a["sig"], a["creator"], whole=wholes, ids=ids)       # the existing route is the oracle
    assert (~want).sum() == 10 and not want[7] and not want[37] and not want[67]
    K = len(sl)
    bm, bw = h.pack_bound(K)
    d_m, d_w, d_mo, d_wo = hip.alloc(bm), hip.alloc(bw), hip.alloc(8 * (K + 1)), hip.alloc(8 * (K + 1))
    d_sig, d_cr, d_ok = hip.up(a["sig"], np.uint8), hip.up(a["creator"], np.int32), hip.alloc(K)
    h.pack_events_device(hip.up(a["sp"], np.uint8), hip.up(a["op"], np.uint8), hip.up(a["arity"], np.uint8), d_cr, hip.up(a["t"], np.float64),
                         d_sig, d_m, d_mo, bm, d_w, d_wo, bw, count=K)
    h.validate_payload_device(d_m, d_mo, bm, d_sig, d_cr, d_ok, whole=d_w, whole_off=d_wo, whole_bytes=bw, ids=hip.up(ids, np.uint8), count=K)
    got = hip.down(d_ok, K, np.uint8).astype(bool)
    assert np.array_equal(got, want)
    h.close()


def contexts(pkg, g, a, sig=None, count=3):
    """src holding the whole graph (with `sig` in place of the signatures), and `count` - 1 contexts holding its first `a`
    events; ids set, everything divided."""
    out = []
    for k in range(count):
        N = g["N"] if k == 0 else a
        s = (g["sig"] if sig is None or k else sig)[:N]
        h = pkg.Hashgraph(g["n"])
        h.append_events(g["cr"][:N], g["sp"][:N], g["op"][:N], g["t"][:N], s)
        h.set_event_ids(0, g["ids"][:N])
        h.divide_rounds(0, N)
        out.append(h)
    return out


def seen_from(g, head):
    """The events `head` can see (its ancestors and itself), ascending."""
    anc = {head}
    for e in range(head, -1, -1):
        if e in anc and g["sp"][e] >= 0:
            anc.update((int(g["sp"][e]), int(g["op"][e])))
    return sorted(anc)


def finish(h, first):
    h.divide_rounds(first, h.num_events - first)
    nc = list(h.decide_fame())
    return (h.event_ids().tobytes(), h.rounds().tobytes(), h.witnesses().tobytes(), h.famous().tobytes(), nc,
            [int(x) for x in h.find_order(nc)], h.heights().tobytes())


@pytest.mark.parametrize("n", [5, 70])
def test_validated_pull_of_valid_events_equals_the_plain_pull(pkg, graphs, n):
    g = graphs[n]
    a = 100
    new = [e for e in seen_from(g, g["N"] - 1) if e >= a]      # what the peer's head sees and I do not hold
    assert len(new) >= 60
    src, dst, twin = contexts(pkg, g, a)
    with pytest.raises(pkg.SwirldHipError) as ei:
        dst.pull_from(src, g["N"] - 1, a - 1, validate=True)
    assert ei.value.code == -95 and dst.num_events == a            # SW_ENOTSUP without keys, nothing stored
    dst.set_member_keys(g["keys"])
    n_sent, n_valid, n_stored = dst.pull_from(src, g["N"] - 1, a - 1, validate=True)
    t_sent, t_stored = twin.pull_from(src, g["N"] - 1, a - 1)
    assert (n_sent, n_stored) == (t_sent, t_stored) and n_valid == n_sent and n_stored == len(new)
    assert finish(dst, a) == finish(twin, a)
    # another event class: every id check fails, nothing is stored
    dst2 = contexts(pkg, g, a, count=2)[1]
    dst2.set_member_keys(g["keys"])
    dst2.set_event_class("swirld", "Evenu")
    assert dst2.pull_from(src, g["N"] - 1, a - 1, validate=True) == (n_sent, 0, 0) and dst2.num_events == a
    for h in (src, dst, twin, dst2):
        h.close()


@pytest.mark.parametrize("n", [5, 70])
def test_validated_pull_drops_corrupt_signatures_and_what_is_built_on_them(pkg, graphs, n):
    g = graphs[n]
    a, N = 100, g["N"]
    sig = g["sig"].copy()
    # seven of the later events the peer's head can see
    cand = [e for e in seen_from(g, N - 1) if e >= a]
    cand = cand[len(cand) // 2:-1]
    victims = cand[::max(1, len(cand) // 7)][:7]
    assert len(victims) == 7
    for v in victims:
        sig[v, v % 64] ^= 0x04
    src, dst, ref = contexts(pkg, g, a, sig=sig)
    for h in (dst, ref):
        h.set_member_keys(g["keys"])
    # the host route: src's payload on the host, pickled by pickle, judged by validate_payload; its verdicts are the `ok`
    sent = src.export_payload(N - 1, dst.known_heights(a - 1))
    K = len(sent["arity"])
    msgs, wholes = [], []
    with mp.event_class("swirld", "Event") as Event:
        for i in range(K):
            p = () if sent["arity"][i] == 0 else (sent["sp_ids"][i].tobytes(), sent["op_ids"][i].tobytes())
            body = (None, p, float(sent["t"][i]), g["keys"][sent["creator"][i]])
            msgs.append(pickle.dumps(body, protocol=4))
            wholes.append(pickle.dumps(Event(*body, sent["sig"][i].tobytes()), protocol=4))
    ok = ref.validate_payload(msgs, sent["sig"], sent["creator"], whole=wholes, ids=sent["ids"])
    in_payload = sum(1 for v in victims if v in sent["event"].tolist())
    assert in_payload == 7 and (~ok).sum() == 7
    _, r_stored = ref.ingest_payload(sent["ids"], sent["sp_ids"], sent["op_ids"], sent["arity"], sent["creator"], ok.astype(np.uint8),
                                     sent["t"], sent["sig"])
    n_sent, n_valid, n_stored = dst.pull_from(src, N - 1, a - 1, validate=True)
    assert (n_sent, n_valid, n_stored) == (K, int(ok.sum()), r_stored) and 0 < n_stored <= n_valid
    assert finish(dst, a) == finish(ref, a)
    # invalid events and their descendants are absent, everything else of the payload is there
    tainted = set(victims)
    for e in range(a, N):
        if g["sp"][e] in tainted or g["op"][e] in tainted:
            tainted.add(e)
    held = {bytes(i) for i in dst.event_ids()}
    for e in sent["event"].tolist():
        assert (bytes(g["ids"][e]) in held) == (e not in tainted or e < a), e
    for h in (src, dst, ref):
        h.close()


def test_packing_changes_nothing(pkg, hip):
    from oracle.oracle import Oracle
    n, N, N1 = 16, 3000, 2400
    cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, 861)
    ids = np.random.default_rng(2).integers(0, 256, (N, 32), dtype=np.uint8)
    o, h = Oracle(n), pkg.Hashgraph(n)
    for d in (o, h):
        d.append_events(cr[:N1], sp[:N1], op[:N1], t[:N1], sig[:N1])
        d.divide_rounds(0, N1)
    nco = list(o.decide_fame())
    nc = list(h.decide_fame())
    assert nc == nco and list(h.find_order(nc)) == list(o.find_order(nco))
    h.set_event_ids(0, ids[:N1])
    a = with_data(events(500, n, 77), np.random.default_rng(3).integers(0, 400, 500), 9)
    h.set_member_keys(a["keys"])

    def snapshot():
        c = h.counters()
        c.pop("kernel_launches")
        return (h.rounds().tobytes(), h.witnesses().tobytes(), h.famous().tobytes(), h.consensus().tobytes(), h.transactions().tobytes(),
                h.heights().tobytes(), h.payload_stats(), h.export_stats(), h.validate_stats(), h.ingest_stats(), c, h.num_events, h.max_round,
                h.event_ids().tobytes(), h.known_heights(N1 - 1).tobytes(), h.member_keys()[0].tobytes())

    before = snapshot()
    exp = model_of(a, "swirld", "Event")
    for _ in range(3):
        assert_device_equals_model(dev_pack(h, hip, a), exp)
        got = h.pack_events(a["sp"], a["op"], a["arity"], a["creator"], a["t"], a["sig"], data=a["data"], data_off=a["data_off"])
        assert got[0].tobytes() == exp[0].tobytes() and got[2].tobytes() == exp[2].tobytes()
    assert snapshot() == before and h.pack_stats()["calls"] == 6
    # ... and the voting goes on as if nothing had happened
    for d in (o, h):
        d.append_events(cr[N1:], sp[N1:], op[N1:], t[N1:], sig[N1:])
        d.divide_rounds(N1, N - N1)
    nco = list(o.decide_fame())
    nc = list(h.decide_fame())
    assert nc == nco and list(h.find_order(nc)) == list(o.find_order(nco))
    assert np.array_equal(h.rounds(), o.round) and np.array_equal(h.heights(), o.height)
    h.close()
    # the exact (forked) path and the windowed table: the same bytes
    f = pkg.Hashgraph(n)
    f.set_forks(True)
    f.set_member_keys(a["keys"])
    f.append_events(np.array([0, 1, 2, 3, 0, 0], np.int32), np.array([-1, -1, -1, -1, 0, 0], np.int32), np.array([-1, -1, -1, -1, 1, 2], np.int32))
    f.divide_rounds(0, 6)
    assert f.exact
    assert_device_equals_model(dev_pack(f, hip, a), exp)
    f.close()
    w = pkg.Hashgraph(n)
    w.set_window(True)
    w.set_member_keys(a["keys"])
    assert_device_equals_model(dev_pack(w, hip, a), exp)
    w.close()
