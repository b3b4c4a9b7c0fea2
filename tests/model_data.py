"""The data store of a context (csrc/data.hip.h, include/swirld_hip.h "The DATA of events") stated in numpy / Python: the
ragged gather every call is made of, the store, the append an ingest makes, and the rule that folds "data range usable"
into a payload's ok flags.  tests/test_model_data.py holds it against plain Python lists; the host emulation of the kernels
and the GPU tests are held against it."""
import numpy as np

MAX_DATA = 60000        # pack.hip.h's MAX_DATA: nothing longer can be part of an encodable event


def pack(datas):
    """A list of bytes | None as (data uint8, off int64 [K + 1], none uint8 [K])."""
    none = np.array([d is None for d in datas], np.uint8).reshape(len(datas))
    off = np.concatenate([[0], np.cumsum([0 if d is None else len(d) for d in datas])]).astype(np.int64)
    return np.frombuffer(b"".join(d for d in datas if d is not None), np.uint8), off, none


def unpack(data, off, none):
    raw = np.asarray(data, np.uint8).tobytes()
    return [None if none[i] else raw[int(off[i]):int(off[i + 1])] for i in range(len(none))]


def range_ok(off, i, nbytes):
    a, b = int(off[i]), int(off[i + 1])
    return a >= 0 and b >= a and b <= nbytes and b - a <= MAX_DATA


def fold_ok(K, ok, data_off, data_bytes):
    """ok AND "the data range can be used" (the rule of pack's d_encodable); ok None = all valid, data_off None = all None."""
    out = np.ones(K, np.uint8) if ok is None else (np.asarray(ok) != 0).astype(np.uint8)
    if data_off is not None:
        for i in range(K):
            if not range_ok(data_off, i, data_bytes):
                out[i] = 0
    return out


def fold_sum(K, folded, data_off):
    """The bytes of the ranges that stay ok: what an ingest can append at most.  A payload whose sum exceeds its data buffer
    (a peer's ranges overlap) is refused as a whole, SW_EINVAL, before anything is stored."""
    return 0 if data_off is None else sum(int(data_off[i + 1]) - int(data_off[i]) for i in range(K) if folded[i])


def ragged_gather(K, src, src_off, src_none, idx, n_src):
    """K slots; slot k is source entry idx[k] (idx None: k).  Returns (data, off from 0, none, bad): bad counts the slots whose
    index is outside [0, n_src) or whose range cannot be used; with bad != 0 nothing else means anything."""
    nbytes = 0 if src is None else len(src)
    parts, none, bad = [], np.ones(K, np.uint8), 0
    for k in range(K):
        e = k if idx is None else int(idx[k])
        part = b""
        if idx is not None and not 0 <= e < n_src:
            bad += 1
        elif src_off is not None:
            if not range_ok(src_off, e, nbytes):
                bad += 1
            elif not (src_none is not None and src_none[e]):
                none[k] = 0
                part = bytes(bytearray(src[int(src_off[e]):int(src_off[e + 1])]))
        parts.append(part)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return np.frombuffer(b"".join(parts), np.uint8), off, none, bad


def slots(index_out, first_new, A):
    """Dense rank -> payload position of the events an ingest stored (the lowest position where an id occurs twice)."""
    out = np.full(A, 0x7f7f7f7f, np.int64)
    for i, v in enumerate(index_out):
        r = int(v) - first_new
        if 0 <= r < A and i < out[r]:
            out[r] = i
    return out.astype(np.int32)


class Store:
    """The store of one context: arena bytes, absolute offsets (one more than the events that have data), None flags."""

    def __init__(self):
        self.data, self.off, self.none = bytearray(), [0], []

    @property
    def events(self):
        return len(self.none)

    def set(self, first, N, data, off, none, K=None):
        """sw_set_event_data: 0, or the error's name with nothing stored."""
        K = (len(off) - 1 if off is not None else K) if K is None else K
        if first != self.events:
            return "SW_EINVAL"
        if first + K > N:
            return "SW_ERANGE"
        d, o, nn, bad = ragged_gather(K, data, off, none, None, K)
        if bad:
            return "SW_EINVAL"
        self._append(d, o, nn)
        return 0

    def _append(self, d, o, nn):
        base = len(self.data)
        self.data += bytes(bytearray(d))
        self.off += [base + int(x) for x in o[1:]]
        self.none += [int(x) for x in nn]

    def get(self, first, K):
        a = self.off[first]
        return (np.frombuffer(bytes(self.data[a:self.off[first + K]]), np.uint8), np.array(self.off[first:first + K + 1], np.int64) - a,
                np.array(self.none[first:first + K], np.uint8))

    def gather(self, events):
        """sw_gather_event_data: (data, off, none), or "SW_ERANGE"."""
        d, o, nn, bad = ragged_gather(len(events), self.data, self.off, self.none, events, self.events)
        return "SW_ERANGE" if bad else (d, o, nn)

    def ingest_append(self, index_out, first_new, A, data, off, none):
        """What sw_ingest_payload_data appends behind payload_core: the data of the A stored events in dense-index order."""
        K = len(index_out)
        d, o, nn, bad = ragged_gather(A, data, off, none, slots(index_out, first_new, A), K)
        assert bad == 0
        self._append(d, o, nn)

    def as_list(self):
        return unpack(self.data, self.off, self.none)
