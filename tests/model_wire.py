"""The canonical wire form of a sync answer (csrc/wire.hip.h), in Python: a protocol-4 pickle without
frames that any pickle.loads turns into (head, {id: Event(d, p, t, c, s)}), with a layout fixed enough for one lane to own
one record:

  message = 0x80 0x04
            0x8c u8(len mod) mod 0x8c u8(len qual) qual 0x93 0x94 '0'   the class: STACK_GLOBAL, MEMOIZE (memo 0), POP
            0x8e u64le(8*(K+1)) off[0..K] as u64le '0'                  BINBYTES8: the record-offset table, POPped again
            'C' 0x20 head32  '}' '('
            record_0 ... record_{K-1}
            'u' 0x86 '.'
  record  = 'C' 0x20 id32  'h' 0x00  '(' D P 'G' t_be64 'C' 0x20 pk32 'C' 0x40 sig64 't' 0x81
  D = 'N' | 'C' u8(len) data (len < 256) | 'B' u32le(len) data (256 <= len <= 60 000)
  P = ')' | 'C' 0x20 sp32 'C' 0x20 op32 0x86

off[i] is the absolute position of record i, off[K] that of 'u'.  tests/test_model_wire.py holds pack_message against
pickle.loads; the kernels and the library are held against this file.  unpack_message is the strict reader: it accepts a
message only if it is byte for byte what pack_message writes for some arrays under the given class."""
import struct

import numpy as np

MAX_DATA = 60000
REC_FIXED = 148      # a record without D and P
REC_MAX = 222        # ... with the longest D (without its data bytes) and P: sw_pack_message_bound
TRAILER = b"u\x86."


def prefix(mod, qual):
    """The bytes in front of the table's length field."""
    m, q = mod.encode("utf-8"), qual.encode("utf-8")
    assert 1 <= len(m) <= 255 and 1 <= len(q) <= 255
    return b"\x80\x04\x8c" + bytes([len(m)]) + m + b"\x8c" + bytes([len(q)]) + q + b"\x93\x940\x8e"


def header_len(K, mod, qual):
    """off[0]: the position of the first record."""
    return len(prefix(mod, qual)) + 8 + 8 * (K + 1) + 1 + 34 + 2


def bound(K, data_bytes, mod="swirld", qual="Event"):
    return header_len(K, mod, qual) + K * REC_MAX + data_bytes + 3


def _data(d):
    if d is None:
        return b"N"
    assert len(d) <= MAX_DATA
    if len(d) < 256:
        return b"C" + bytes([len(d)]) + d
    return b"B" + struct.pack("<I", len(d)) + d


def record(id32, d, p, t_bits, c, s):
    """t_bits: the timestamp as the 64-bit integer that holds its bits."""
    assert len(id32) == 32 and len(c) == 32 and len(s) == 64
    par = b")" if len(p) == 0 else b"C\x20" + p[0] + b"C\x20" + p[1] + b"\x86"
    return (b"C\x20" + id32 + b"h\x00(" + _data(d) + par + b"G" + struct.pack(">Q", t_bits) + b"C\x20" + c + b"C\x40" + s + b"t\x81")


def pack_message(head32, keys, ids, sp_id, op_id, arity, creator, t, sig, data=None, data_off=None, data_none=None, mod="swirld",
                 qual="Event"):
    """The array form (the arrays sw_pack_message takes; keys: n x 32 uint8).  Returns the message as bytes, or the index of
    the first event that cannot be encoded as a negative number -(index + 1)."""
    keys = np.asarray(keys, np.uint8).reshape(-1, 32)
    n, K = keys.shape[0], len(arity)
    ids, sp_id, op_id = (np.asarray(x, np.uint8).reshape(K, 32) for x in (ids, sp_id, op_id))
    sig = np.asarray(sig, np.uint8).reshape(K, 64)
    tb = np.ascontiguousarray(t, np.float64).view(np.uint64)
    nbytes = 0 if data is None else len(data)
    recs = []
    for i in range(K):
        ok = int(arity[i]) in (0, 2) and 0 <= int(creator[i]) < n
        d = None
        if ok and data_off is not None:
            a, b = int(data_off[i]), int(data_off[i + 1])
            ok = 0 <= a <= b <= nbytes and b - a <= MAX_DATA
            if ok and not (data_none is not None and data_none[i]):
                d = bytes(bytearray(data[a:b]))
        if not ok:
            return -(i + 1)
        p = () if int(arity[i]) == 0 else (sp_id[i].tobytes(), op_id[i].tobytes())
        recs.append(record(ids[i].tobytes(), d, p, int(tb[i]), keys[int(creator[i])].tobytes(), sig[i].tobytes()))
    off = np.zeros(K + 1, np.uint64)
    off[0] = header_len(K, mod, qual)
    if K:
        off[1:] = off[0] + np.cumsum([len(r) for r in recs], dtype=np.uint64)
    head = bytes(bytearray(np.asarray(head32, np.uint8)))
    assert len(head) == 32
    return (prefix(mod, qual) + struct.pack("<Q", 8 * (K + 1)) + off.astype("<u8").tobytes() + b"0C\x20" + head + b"}(" + b"".join(recs) + TRAILER)


def unpack_message(msg, keys, mod="swirld", qual="Event"):
    """The strict reader.  None for anything that is not canonical under this class, else a dict of arrays: head (32 uint8),
    ids / sp / op (K x 32; a root's parents are zeros), arity, creator (-1: the key of no member; the lowest index of equal
    keys), t (float64, bit pattern kept), sig (K x 64), data, data_off (K + 1), data_none."""
    msg = bytes(msg)
    keys = np.asarray(keys, np.uint8).reshape(-1, 32)
    pre = prefix(mod, qual)
    if len(msg) < len(pre) + 8 or msg[:len(pre)] != pre:
        return None
    tb = struct.unpack_from("<Q", msg, len(pre))[0]
    if tb % 8 or tb < 8 or tb > len(msg):
        return None
    K = tb // 8 - 1
    base = header_len(K, mod, qual)
    if base + 3 > len(msg):
        return None
    t0 = len(pre) + 8
    off = np.frombuffer(msg, "<u8", K + 1, t0)
    if int(off[0]) != base or int(off[K]) + 3 != len(msg) or (K and not (off[1:] > off[:-1]).all()):
        return None
    q = t0 + 8 * (K + 1)
    if msg[q:q + 3] != b"0C\x20" or msg[q + 35:q + 37] != b"}(" or msg[-3:] != TRAILER:
        return None
    index = {}
    for i in range(keys.shape[0] - 1, -1, -1):
        index[keys[i].tobytes()] = i
    out = dict(head=np.frombuffer(msg, np.uint8, 32, q + 3).copy(), ids=np.zeros((K, 32), np.uint8), sp=np.zeros((K, 32), np.uint8),
               op=np.zeros((K, 32), np.uint8), arity=np.zeros(K, np.uint8), creator=np.zeros(K, np.int32), t=np.zeros(K, np.float64),
               sig=np.zeros((K, 64), np.uint8), data_off=np.zeros(K + 1, np.int64), data_none=np.zeros(K, np.uint8))
    chunks = []
    for i in range(K):
        r = msg[int(off[i]):int(off[i + 1])]
        if len(r) < REC_FIXED + 2 or r[:2] != b"C\x20" or r[34:37] != b"h\x00(":
            return None
        if r[37:38] == b"N":
            d, dsz = None, 1
        elif r[37:38] == b"C":
            d, dsz = r[39:39 + r[38]], 2 + r[38]
        elif r[37:38] == b"B":
            ln = struct.unpack_from("<I", r, 38)[0]
            if not 256 <= ln <= MAX_DATA:
                return None
            d, dsz = r[42:42 + ln], 5 + ln
        else:
            return None
        p = 37 + dsz
        if p >= len(r) or r[p:p + 1] not in (b")", b"C"):
            return None
        root = r[p:p + 1] == b")"
        if len(r) != REC_FIXED + dsz + (1 if root else 69):
            return None
        if not root:
            if r[p:p + 2] != b"C\x20" or r[p + 34:p + 36] != b"C\x20" or r[p + 68:p + 69] != b"\x86":
                return None
            out["sp"][i] = np.frombuffer(r, np.uint8, 32, p + 2)
            out["op"][i] = np.frombuffer(r, np.uint8, 32, p + 36)
            out["arity"][i] = 2
        p += 1 if root else 69
        if r[p:p + 1] != b"G" or r[p + 9:p + 11] != b"C\x20" or r[p + 43:p + 45] != b"C\x40" or r[p + 109:] != b"t\x81":
            return None
        out["ids"][i] = np.frombuffer(r, np.uint8, 32, 2)
        out["t"][i:i + 1] = np.frombuffer(struct.pack("<Q", struct.unpack_from(">Q", r, p + 1)[0]), np.float64)
        out["creator"][i] = index.get(r[p + 11:p + 43], -1)
        out["sig"][i] = np.frombuffer(r, np.uint8, 64, p + 45)
        out["data_none"][i] = d is None
        chunks.append(d or b"")
        out["data_off"][i + 1] = out["data_off"][i] + len(chunks[-1])
    out["data"] = np.frombuffer(b"".join(chunks), np.uint8).copy()
    return out
