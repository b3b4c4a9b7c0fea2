"""CPU: the template of tests/model_pack.py (what csrc/pack.hip.h writes) against pickle.dumps(protocol=4) of a namedtuple
Event, byte for byte: two (module, qualified name) pairs, data None and of every length at which the encoding changes, roots
and non-roots, timestamps whose bit pattern matters."""
import os
import pickle

import numpy as np
import pytest

import model_pack as mp

CLASSES = (("swirld", "Event"), ("py-swirld_amd.node", "Event"))
DATA = (None, 0, 1, 255, 256, 257, 60000)
TIMES = (0.0, -0.0, 1.5, float("inf"), 1e300)


def rnd(n):
    return os.urandom(n)     # a fresh object every time: no two fields of an event share one (no memo reads)


@pytest.mark.parametrize("mod,qual", CLASSES)
def test_template_equals_pickle(mod, qual):
    with mp.event_class(mod, qual) as Event:
        for dl in DATA:
            for root in (True, False):
                for t in TIMES:
                    d = None if dl is None else rnd(dl)
                    p = () if root else (rnd(32), rnd(32))
                    ev = Event(d, p, t, rnd(32), rnd(64))
                    assert mp.msg(ev.d, ev.p, ev.t, ev.c) == pickle.dumps(ev[:-1], protocol=4), (dl, root, t)
                    assert mp.whole(ev.d, ev.p, ev.t, ev.c, ev.s, mod, qual) == pickle.dumps(ev, protocol=4), (dl, root, t)


def test_sizes_that_follow_from_the_template():
    c, s = rnd(32), rnd(64)
    assert len(mp.msg(None, (), 1.0, c)) == 61
    assert len(mp.msg(None, (rnd(32), rnd(32)), 1.0, c)) == 132
    for mod, qual in CLASSES + (("m", "Q" * 255),):
        for d in (None, b"", rnd(300)):
            for p in ((), (rnd(32), rnd(32))):
                m, w = mp.msg(d, p, 2.5, c), mp.whole(d, p, 2.5, c, s, mod, qual)
                assert len(w) == len(m) + 77 + len(mod.encode()) + len(qual.encode())
                bm, bw = mp.bound(1, 0 if d is None else len(d), mod, qual)
                assert len(m) <= bm and len(w) <= bw
    # the bound is reached: a non-root with 256 bytes of data
    m, w = mp.msg(rnd(256), (rnd(32), rnd(32)), 0.0, c), mp.whole(rnd(256), (rnd(32), rnd(32)), 0.0, c, s)
    assert (len(m), len(w)) == mp.bound(1, 256)


def test_negative_zero_and_infinity_keep_their_bits():
    c = rnd(32)
    assert mp.msg(None, (), 0.0, c) != mp.msg(None, (), -0.0, c)
    assert mp.msg(None, (), -0.0, c)[14:23] == b"G\x80" + b"\0" * 7
    assert mp.msg(None, (), float("inf"), c)[14:23] == b"G\x7f\xf0" + b"\0" * 6


def test_array_form_matches_the_event_form_and_flags_what_cannot_be_encoded():
    rng = np.random.default_rng(5)
    n, K = 7, 40
    keys = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sp, op = rng.integers(0, 256, (K, 32), dtype=np.uint8), rng.integers(0, 256, (K, 32), dtype=np.uint8)
    sig = rng.integers(0, 256, (K, 64), dtype=np.uint8)
    arity = np.where(rng.random(K) < 0.3, 0, 2).astype(np.uint8)
    creator = rng.integers(0, n, K).astype(np.int32)
    t = rng.random(K)
    arity[3], creator[5], creator[6] = 1, -1, n
    lens = rng.integers(0, 300, K)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    data = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    none = (rng.random(K) < 0.2).astype(np.uint8)
    msgs, moff, wh, woff, enc = mp.pack(keys, sp, op, arity, creator, t, sig, data, off, none)
    assert enc.tolist() == [0 if i in (3, 5, 6) else 1 for i in range(K)]
    with mp.event_class("swirld", "Event") as Event:
        for i in range(K):
            m, w = msgs[moff[i]:moff[i + 1]].tobytes(), wh[woff[i]:woff[i + 1]].tobytes()
            if not enc[i]:
                assert m == b"" and w == b""
                continue
            d = None if none[i] else data[off[i]:off[i + 1]].tobytes()
            p = () if arity[i] == 0 else (sp[i].tobytes(), op[i].tobytes())
            ev = Event(d, p, float(t[i]), keys[creator[i]].tobytes(), sig[i].tobytes())
            assert m == pickle.dumps(ev[:-1], protocol=4) and w == pickle.dumps(ev, protocol=4), i
