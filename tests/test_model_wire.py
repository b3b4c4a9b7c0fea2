"""CPU: tests/model_wire.py (the canonical wire form of a sync answer) against pickle itself: the C unpickler and the
Python one turn pack_message's bytes into (head, {id: Event}) equal in value and in key order to what Node.ask_sync pickles
today; unpack_message returns the arrays, and refuses what is not canonical."""
import pickle
import struct

import numpy as np
import pytest

import model_pack as mp
import model_wire as mw

DATA_LENS = [None, 0, 1, 255, 256, 257, 60000]


def arrays(K, n, seed, lens=None):
    rng = np.random.default_rng(seed)
    a = dict(head=rng.integers(0, 256, 32, dtype=np.uint8), keys=rng.integers(0, 256, (n, 32), dtype=np.uint8),
             ids=rng.integers(0, 256, (K, 32), dtype=np.uint8), sp=rng.integers(0, 256, (K, 32), dtype=np.uint8),
             op=rng.integers(0, 256, (K, 32), dtype=np.uint8), sig=rng.integers(0, 256, (K, 64), dtype=np.uint8),
             arity=np.where(rng.random(K) < 0.3, 0, 2).astype(np.uint8), creator=rng.integers(0, n, K).astype(np.int32),
             t=1.7e9 + rng.random(K))
    for i, v in enumerate((-0.0, np.inf)):
        if i < K:
            a["t"][i] = v
    if lens is None:
        lens = [DATA_LENS[i % len(DATA_LENS)] if i < 2 * len(DATA_LENS) else (None if i % 5 == 0 else i % 300) for i in range(K)]
    if K >= 2 * len(DATA_LENS):      # every data shape on a root and on a non-root
        a["arity"][:len(DATA_LENS)] = 0
        a["arity"][len(DATA_LENS):2 * len(DATA_LENS)] = 2
    a["data_none"] = np.array([x is None for x in lens], np.uint8)
    a["data_off"] = np.concatenate([[0], np.cumsum([x or 0 for x in lens])]).astype(np.int64)
    a["data"] = rng.integers(0, 256, int(a["data_off"][-1]), dtype=np.uint8)
    return a


def message(a, mod="swirld", qual="Event"):
    return mw.pack_message(a["head"], a["keys"], a["ids"], a["sp"], a["op"], a["arity"], a["creator"], a["t"], a["sig"], a["data"],
                           a["data_off"], a["data_none"], mod, qual)


def expected(a, cls):
    """(head, {id: Event}) the way Node.ask_sync builds it."""
    sub = {}
    for i in range(len(a["arity"])):
        d = None if a["data_none"][i] else a["data"][a["data_off"][i]:a["data_off"][i + 1]].tobytes()
        p = () if a["arity"][i] == 0 else (a["sp"][i].tobytes(), a["op"][i].tobytes())
        sub[a["ids"][i].tobytes()] = cls(d, p, float(a["t"][i]), a["keys"][a["creator"][i]].tobytes(), a["sig"][i].tobytes())
    return a["head"].tobytes(), sub


def same(got, want):
    assert got[0] == want[0] and list(got[1]) == list(want[1])
    for k, ev in want[1].items():
        g = got[1][k]
        assert type(g) is type(ev) and g[:2] == ev[:2] and g[3:] == ev[3:]
        assert struct.pack("<d", g.t) == struct.pack("<d", ev.t)        # -0.0 stays -0.0


@pytest.mark.parametrize("mod,qual", [("swirld", "Event"), ("py-swirld_amd.node", "Event")])
@pytest.mark.parametrize("K", [0, 1, 2, 1000])
def test_any_unpickler_reads_the_message(K, mod, qual):
    a = arrays(K, 5, 3 + K)
    if K == 2:
        a["arity"][:] = [0, 2]
    msg = message(a, mod, qual)
    assert len(msg) <= mw.bound(K, len(a["data"]), mod, qual)
    with mp.event_class(mod, qual) as cls:
        want = expected(a, cls)
        same(pickle.loads(msg), want)
        same(pickle._loads(msg), want)
        assert pickle.loads(msg) == pickle.loads(pickle.dumps(want, protocol=4))
    if K == 0:
        with mp.event_class(mod, qual):
            assert pickle.loads(msg) == (a["head"].tobytes(), {})


def test_every_data_shape_on_roots_and_non_roots():
    a = arrays(2 * len(DATA_LENS), 4, 9)
    msg = message(a)
    with mp.event_class("swirld", "Event") as cls:
        same(pickle.loads(msg), expected(a, cls))
    off = np.frombuffer(msg, "<u8", len(a["arity"]) + 1, len(mw.prefix("swirld", "Event")) + 8)
    lens = np.diff(off.astype(np.int64))
    assert lens[0] == 150 and lens[len(DATA_LENS)] == 218 and lens[6] == 150 + 4 + 60000
    assert msg[int(off[-1]):] == b"u\x86."


@pytest.mark.parametrize("K", [0, 1, 2, 1000])
def test_round_trip_through_the_strict_reader(K):
    a = arrays(K, 5, 20 + K)
    a["keys"][3] = a["keys"][1]          # equal keys: the lowest index is reported
    msg = message(a, "m", "Q")
    u = mw.unpack_message(msg, a["keys"], "m", "Q")
    assert u is not None
    root = a["arity"] == 0
    for name in ("ids", "arity", "sig", "data_off", "data_none", "data"):
        assert np.array_equal(u[name], a[name]), name
    assert np.array_equal(u["head"], a["head"])
    assert np.array_equal(u["t"].view(np.uint64), a["t"].view(np.uint64))
    assert np.array_equal(u["creator"], np.where(a["creator"] == 3, 1, a["creator"]))
    assert np.array_equal(u["sp"][~root], a["sp"][~root]) and not u["sp"][root].any() and not u["op"][root].any()
    assert np.array_equal(u["op"][~root], a["op"][~root])
    other = a["keys"].copy()
    other[2] ^= 1
    assert (mw.unpack_message(msg, other, "m", "Q")["creator"][a["creator"] == 2] == -1).all()


def test_unencodable_events_are_named():
    a = arrays(20, 5, 30, lens=[3] * 20)
    for field, idx, val in (("arity", 7, 1), ("creator", 4, 5), ("creator", 0, -1)):
        b = {k: v.copy() for k, v in a.items()}
        b[field][idx] = val
        assert message(b) == -(idx + 1)
    b = {k: v.copy() for k, v in a.items()}
    b["data_off"][10] = 10 ** 9
    assert message(b) == -(9 + 1)


def test_the_strict_reader_refuses():
    a = arrays(6, 5, 40, lens=[None, 0, 5, 256, None, 300])
    a["arity"][:] = [0, 2, 0, 2, 2, 0]
    msg = message(a)
    keys = a["keys"]
    assert mw.unpack_message(msg, keys) is not None
    assert mw.unpack_message(msg, keys, "swirld", "Evenu") is None and mw.unpack_message(msg, keys, "swirle", "Event") is None
    with mp.event_class("swirld", "Event") as cls:
        assert mw.unpack_message(pickle.dumps(expected(a, cls), protocol=4), keys) is None
    for cut in range(0, len(msg), 97):
        assert mw.unpack_message(msg[:cut], keys) is None
    assert mw.unpack_message(msg + b".", keys) is None
    # every byte that is not a field's content is a constant: flipping it must be noticed
    u = mw.unpack_message(msg, keys)
    content = np.zeros(len(msg), bool)
    t0 = len(mw.prefix("swirld", "Event")) + 8
    off = np.frombuffer(msg, "<u8", 7, t0).astype(np.int64)
    q = t0 + 8 * 7
    content[q + 3:q + 35] = True          # the head
    for i in range(6):
        s = int(off[i])
        content[s + 2:s + 34] = True
        dl = int(u["data_off"][i + 1] - u["data_off"][i])
        dsz = 1 if u["data_none"][i] else (2 + dl if dl < 256 else 5 + dl)
        d0 = s + 37 + dsz - dl
        content[d0:d0 + dl] = True
        p = s + 37 + dsz
        if u["arity"][i]:
            content[p + 2:p + 34] = True
            content[p + 36:p + 68] = True
            p += 69
        else:
            p += 1
        content[p + 1:p + 9] = True
        content[p + 11:p + 43] = True
        content[p + 45:p + 109] = True
    for pos in np.flatnonzero(~content):
        bad = bytearray(msg)
        bad[pos] ^= 0x01
        assert mw.unpack_message(bytes(bad), keys) is None, "a flipped constant at %d was accepted" % pos
    for pos in np.flatnonzero(content)[::7]:
        bad = bytearray(msg)
        bad[pos] ^= 0x80
        assert mw.unpack_message(bytes(bad), keys) is not None
