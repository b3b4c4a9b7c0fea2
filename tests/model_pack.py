"""The signed bytes of an event as a fixed template (csrc/pack.hip.h), in Python: what
pickle.dumps(ev[:-1], protocol=4) and pickle.dumps(ev, protocol=4) write for a namedtuple Event(d, p, t, c, s) whose data is
None or a bytes object of at most MAX_DATA bytes, whose parents are () or two 32-byte ids, whose timestamp is a float and
whose creator key and signature are bytes of 32 and 64 — one frame, no memo reads.  tests/test_model_pack.py holds it against
pickle itself; the kernels and the library are held against this file.  Also the array form: pack() takes the arrays
sw_pack_events takes and returns the two streams, the offsets and the flags."""
import collections
import contextlib
import importlib
import struct
import sys
import types

import numpy as np

MAX_DATA = 60000
MSG_MAX = 137        # per event without its data: sw_pack_bound
WHOLE_MAX = 206      # ... and without the class header


def frame(x):
    return b"\x80\x04\x95" + struct.pack("<Q", len(x)) + x


def class_header(mod, qual):
    m, q = mod.encode("utf-8"), qual.encode("utf-8")
    assert 1 <= len(m) <= 255 and 1 <= len(q) <= 255
    return b"\x8c" + bytes([len(m)]) + m + b"\x94\x8c" + bytes([len(q)]) + q + b"\x94\x93\x94"


def _data(d):
    if d is None:
        return b"N"
    assert len(d) <= MAX_DATA
    if len(d) < 256:
        return b"C" + bytes([len(d)]) + d + b"\x94"
    return b"B" + struct.pack("<I", len(d)) + d + b"\x94"


def _parents(p):
    if len(p) == 0:
        return b")"
    sp, op = p
    assert len(sp) == 32 and len(op) == 32
    return b"C\x20" + sp + b"\x94C\x20" + op + b"\x94\x86\x94"


def _head(d, p, t, c):
    assert len(c) == 32
    return b"(" + _data(d) + _parents(p) + b"G" + struct.pack(">d", t) + b"C\x20" + c + b"\x94"


def msg(d, p, t, c):
    """dumps(ev[:-1])"""
    return frame(_head(d, p, t, c) + b"t\x94.")


def whole(d, p, t, c, s, mod="swirld", qual="Event"):
    """dumps(ev)"""
    assert len(s) == 64
    return frame(class_header(mod, qual) + _head(d, p, t, c) + b"C\x40" + s + b"\x94t\x94\x81\x94.")


@contextlib.contextmanager
def event_class(mod, qual):
    """A namedtuple Event(d, p, t, c, s) that pickles as mod.qual: registered under sys.modules[mod] for the length of the
    `with` block, so that pickle finds it; a module of that name that is loaded already is put back afterwards."""
    cls = collections.namedtuple(qual, "d p t c s")
    cls.__module__ = mod
    cls.__qualname__ = qual
    m = types.ModuleType(mod)
    setattr(m, qual, cls)
    missing = object()
    if "." in mod:      # pickle imports the name, parents first: a real parent package must be loaded before its child is shadowed
        importlib.import_module(mod.rpartition(".")[0])
    before = sys.modules.get(mod, missing)
    sys.modules[mod] = m
    try:
        yield cls
    finally:
        if before is missing:
            del sys.modules[mod]
        else:
            sys.modules[mod] = before


def pack(keys, sp_id, op_id, arity, creator, t, sig, data=None, data_off=None, data_none=None, mod="swirld", qual="Event"):
    """The array form.  keys: n x 32 uint8.  Returns (msgs uint8, msg_off int64, whole uint8, whole_off int64, encodable uint8)."""
    keys = np.asarray(keys, np.uint8).reshape(-1, 32)
    n, K = keys.shape[0], len(arity)
    sp_id, op_id = np.asarray(sp_id, np.uint8).reshape(K, 32), np.asarray(op_id, np.uint8).reshape(K, 32)
    sig = np.asarray(sig, np.uint8).reshape(K, 64)
    t = np.asarray(t, np.float64)
    nbytes = 0 if data is None else len(data)
    ms, ws, enc = [], [], np.zeros(K, np.uint8)
    for i in range(K):
        ok = int(arity[i]) in (0, 2) and 0 <= int(creator[i]) < n
        d = None
        if ok and data_off is not None:
            a, b = int(data_off[i]), int(data_off[i + 1])
            ok = 0 <= a <= b <= nbytes and b - a <= MAX_DATA
            if ok and not (data_none is not None and data_none[i]):
                d = bytes(bytearray(data[a:b]))
        if not ok:
            ms.append(b"")
            ws.append(b"")
            continue
        enc[i] = 1
        p = () if int(arity[i]) == 0 else (sp_id[i].tobytes(), op_id[i].tobytes())
        tt = struct.unpack("<d", t[i:i + 1].tobytes())[0]
        c = keys[int(creator[i])].tobytes()
        ms.append(msg(d, p, tt, c))
        ws.append(whole(d, p, tt, c, sig[i].tobytes(), mod, qual))
    out = []
    for lst in (ms, ws):
        off = np.zeros(K + 1, np.int64)
        if K:
            np.cumsum([len(x) for x in lst], out=off[1:])
        out += [np.frombuffer(b"".join(lst), np.uint8), off]
    return out[0], out[1], out[2], out[3], enc


def bound(K, data_bytes, mod="swirld", qual="Event"):
    h = len(class_header(mod, qual))
    return K * MSG_MAX + data_bytes, K * (WHOLE_MAX + h) + data_bytes
