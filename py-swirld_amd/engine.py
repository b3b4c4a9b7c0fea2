"""Array-in / array-out front end of the C-ABI: one `Hashgraph` = the voting state of
one Node view, resident in HBM.  Mirrors the reference's hot-path methods
(swirld.py:187-311) on dense event / member indices."""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Counters, SwirldHipError, Timings

# what Hashgraph.gossip_turn returns: sw_turn_result's fields and the rounds decide_fame added to the consensus
TurnResult = collections.namedtuple("TurnResult", "n_sent n_valid n_stored new_head n_new_rounds n_ordered stage new_rounds")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dev_ptr(a):
    """(address, length or None) of an array in device memory: an integer address, an object with data_ptr()
    (a torch tensor) or with __cuda_array_interface__."""
    if a is None:
        return None, None
    if isinstance(a, (int, np.integer)):
        return int(a), None
    if hasattr(a, "data_ptr"):
        ptr = int(a.data_ptr())
    elif hasattr(a, "__cuda_array_interface__"):
        ptr = int(a.__cuda_array_interface__["data"][0])
    else:
        raise TypeError("expected a device address, or an object with data_ptr() / __cuda_array_interface__ "
                        "(got %s; host arrays go through append_events)" % type(a).__name__)
    try:
        return ptr, len(a)
    except TypeError:
        return ptr, None


class Hashgraph:
    def __init__(self, n_members, stake=None, coin_period=6, device=0):
        self._L = _lib.load()
        self.n = int(n_members)
        if stake is None:
            st = np.ones(self.n, np.uint64)
        else:
            raw = np.asarray(stake)
            if raw.shape != (self.n,):
                raise ValueError("stake must have one entry per member")
            # the reference compares sums of stakes with 2*tot/3 in Python arithmetic (swirld.py:41-44); the
            # device tallies are integer: non-integer, negative or non-finite stakes are refused, not truncated
            if raw.dtype.kind not in "iu":
                as_f = raw.astype(np.float64)
                if not np.all(np.isfinite(as_f)) or np.any(as_f != np.floor(as_f)):
                    raise ValueError("stakes must be integers (got %r)" % (raw.tolist(),))
            if np.any(raw.astype(np.float64) < 0):
                raise ValueError("stakes must be non-negative")
            st = np.ascontiguousarray(raw, np.uint64)
        self.stake = st
        self._h = C.c_void_p()
        rc = self._L.sw_create(self.n, _p(st), int(coin_period), int(device), C.byref(self._h))
        if rc != 0:
            raise SwirldHipError(rc, (self._L.sw_last_error(None) or b"").decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.sw_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise SwirldHipError(rc, (self._L.sw_last_error(self._h) or b"").decode())

    # ---- ingest (Node.add_event, swirld.py:114-120) ----
    def reserve(self, n_events):
        self._chk(self._L.sw_reserve(self._h, int(n_events)))

    def append_events(self, creator, self_parent, other_parent, t=None, sig=None):
        creator = np.ascontiguousarray(creator, np.int32)
        sp = np.ascontiguousarray(self_parent, np.int32)
        op = np.ascontiguousarray(other_parent, np.int32)
        K = creator.shape[0]
        if sp.shape != (K,) or op.shape != (K,):
            raise ValueError("creator / parents must have equal length")
        t = None if t is None else np.ascontiguousarray(t, np.float64)
        sig = None if sig is None else np.ascontiguousarray(sig, np.uint8).reshape(K, 64)
        self._chk(self._L.sw_append_events(self._h, K, _p(creator), _p(sp), _p(op), _p(t), _p(sig)))

    def append_events_device(self, creator, self_parent, other_parent, t=None, sig=None, stream=0, count=None):
        """append_events for arrays that lie in DEVICE memory (int32 creator / parents, float64 t, K x 64 uint8 sig):
        each one an integer address or an object with data_ptr() (torch) or __cuda_array_interface__.  K comes from
        `creator`'s length where it has one, else from `count`.  `stream` (a raw hipStream_t) has the arrays' producers
        enqueued; the library waits for them on the device.  Batches outside the bulk fork-free fast path fall back
        to the host path inside the library (ingest_stats() counts them)."""
        ptrs = [_dev_ptr(a) for a in (creator, self_parent, other_parent, t, sig)]
        K = count if count is not None else ptrs[0][1]
        if K is None:
            raise ValueError("the number of events is not known: pass count=")
        K = int(K)
        for (_, ln), what in zip(ptrs[:4], ("creator", "self_parent", "other_parent", "t")):
            if ln is not None and ln != K:
                raise ValueError("%s holds %d entries, expected %d" % (what, ln, K))
        if ptrs[4][1] is not None and ptrs[4][1] not in (K, 64 * K):
            raise ValueError("sig holds %d entries, expected %d x 64 bytes" % (ptrs[4][1], K))
        args = [C.c_void_p(q) if q else None for q, _ in ptrs]
        self._chk(self._L.sw_append_events_device(self._h, K, *args, C.c_void_p(int(stream))))

    def ingest_stats(self):
        """Counters of append_events_device since the context was created: batches and events the device path
        committed, batches that fell back to the host path, events whose height the host loop computed."""
        v = [C.c_int64() for _ in range(4)]
        self._chk(self._L.sw_get_ingest_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("device_batches", "device_events", "fallback_batches", "host_height_events"), (int(x.value) for x in v)))

    # ---- events by id (Node.sync, swirld.py:130-136): the id index and whole payloads addressed by id ----
    @staticmethod
    def _ids(a, K=None):
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32)
        if K is not None and a.shape[0] != K:
            raise ValueError("expected %d ids of 32 bytes, got %d" % (K, a.shape[0]))
        return a

    def set_event_ids(self, first, ids):
        """Attach the 32-byte ids `ids` (K x 32 uint8) to the stored events [first, first + K); `first` must be the number
        of events that have ids already.  SW_EINVAL when an id is already present or occurs twice."""
        ids = self._ids(ids)
        self._chk(self._L.sw_set_event_ids(self._h, int(first), ids.shape[0], _p(ids)))

    def event_ids(self, first=0, K=None):
        """The ids of the events [first, first + K) as a K x 32 uint8 array (K None: every event from `first` on)."""
        if K is None:
            K = self.num_events - first
        out = np.empty((max(int(K), 0), 32), np.uint8)
        self._chk(self._L.sw_get_event_ids(self._h, int(first), int(K), _p(out)))
        return out

    def lookup_event_ids(self, ids):
        """Dense index of every id, -1 where the context does not hold it (looked up on the device)."""
        ids = self._ids(ids)
        out = np.empty(ids.shape[0], np.int32)
        self._chk(self._L.sw_lookup_event_ids(self._h, ids.shape[0], _p(ids), _p(out)))
        return out

    def ingest_payload(self, ids, sp_ids, op_ids, arity, creator, ok=None, t=None, sig=None, *, data=None, data_off=None, data_none=None):
        """A sync payload addressed by id, host arrays in any order (sw_ingest_payload): known ids are recognised, invalid
        events dropped, the rest ordered topologically and appended.  Returns (index_out, n_stored): per event its dense
        index or a reject code -2 .. -8 (include/swirld_hip.h).
        data / data_off / data_none (as pack_events takes them; `data` may also be a list of bytes | None): the events bring
        their data (sw_ingest_payload_data) — the data store must be complete, an event with an unusable range is -3."""
        ids = self._ids(ids)
        K = ids.shape[0]
        sp_ids, op_ids = self._ids(sp_ids, K), self._ids(op_ids, K)
        arity = np.ascontiguousarray(arity, np.uint8)
        creator = np.ascontiguousarray(creator, np.int32)
        if arity.shape != (K,) or creator.shape != (K,):
            raise ValueError("arity / creator must have one entry per event")
        ok = None if ok is None else np.ascontiguousarray(ok, np.uint8).reshape(K)
        t = None if t is None else np.ascontiguousarray(t, np.float64).reshape(K)
        sig = None if sig is None else np.ascontiguousarray(sig, np.uint8).reshape(K, 64)
        out = np.empty(K, np.int32)
        n_stored = C.c_int64()
        if data is not None or data_off is not None or data_none is not None:
            data, data_off, data_none, nbytes = self._data_arrays(K, data, data_off, data_none)
            self._chk(self._L.sw_ingest_payload_data(self._h, K, _p(ids), _p(sp_ids), _p(op_ids), _p(arity), _p(creator), _p(ok), _p(t), _p(sig),
                                                     _p(out), C.byref(n_stored), _p(data), _p(data_off), nbytes, _p(data_none)))
            return out, int(n_stored.value)
        self._chk(self._L.sw_ingest_payload(self._h, K, _p(ids), _p(sp_ids), _p(op_ids), _p(arity), _p(creator), _p(ok), _p(t), _p(sig),
                                            _p(out), C.byref(n_stored)))
        return out, int(n_stored.value)

    def ingest_payload_device(self, ids, sp_ids, op_ids, arity, creator, ok=None, t=None, sig=None, index_out=None, stream=0, count=None,
                              *, data=None, data_off=None, data_bytes=0, data_none=None):
        """ingest_payload for arrays in DEVICE memory (addresses, or objects with data_ptr() / __cuda_array_interface__;
        the id arrays 8-byte aligned).  `index_out` (required): K int32 in device memory, where the answer is left.
        Returns (index_out as given, n_stored).  data_off (K + 1 int64 in device memory) with data / data_bytes / data_none:
        the events bring their data (sw_ingest_payload_data_device)."""
        if index_out is None:
            raise ValueError("index_out (K int32 in device memory) is required")
        ptrs = [_dev_ptr(a) for a in (ids, sp_ids, op_ids, arity, creator, ok, t, sig, index_out)]
        K = count if count is not None else ptrs[3][1]
        if K is None:
            raise ValueError("the number of events is not known: pass count=")
        K = int(K)
        args = [C.c_void_p(q) if q else None for q, _ in ptrs]
        n_stored = C.c_int64()
        if data is not None or data_off is not None or data_none is not None:
            dp = [C.c_void_p(q) if q else None for q in (_dev_ptr(a)[0] for a in (data, data_off, data_none))]
            self._chk(self._L.sw_ingest_payload_data_device(self._h, K, *args[:8], C.c_void_p(int(stream)), args[8], C.byref(n_stored),
                                                            dp[0], dp[1], int(data_bytes), dp[2]))
            return index_out, int(n_stored.value)
        self._chk(self._L.sw_ingest_payload_device(self._h, K, *args[:8], C.c_void_p(int(stream)), args[8], C.byref(n_stored)))
        return index_out, int(n_stored.value)

    def payload_stats(self):
        """Payload calls so far, waves / accepted events of the most recent one, id-table rebuilds, and (under
        set_profiling) the host milliseconds of its phases: resolve, waves, sort, append."""
        v = [C.c_int64() for _ in range(4)]
        ms = (C.c_double * 4)()
        self._chk(self._L.sw_get_payload_stats(self._h, *[C.byref(x) for x in v], ms))
        d = dict(zip(("calls", "waves", "accepted", "table_rebuilds"), (int(x.value) for x in v)))
        d.update(zip(("resolve_ms", "waves_ms", "sort_ms", "append_ms"), (float(x) for x in ms)))
        return d

    # ---- the data of events, Event.d (swirld.py:30, :82-95; csrc/data.hip.h) ----
    @staticmethod
    def pack_data(datas):
        """A list of bytes | None as (data uint8, data_off int64 [K + 1], data_none uint8 [K])."""
        none = np.fromiter((d is None for d in datas), np.uint8, len(datas))
        lens = np.fromiter((0 if d is None else len(d) for d in datas), np.int64, len(datas))
        off = np.zeros(len(datas) + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        data = np.frombuffer(b"".join(d for d in datas if d is not None), np.uint8)
        return data, off, none

    @staticmethod
    def unpack_data(data, data_off, data_none):
        """The inverse: a list of bytes | None."""
        raw = np.ascontiguousarray(data, np.uint8).tobytes()
        return [None if data_none[i] else raw[int(data_off[i]):int(data_off[i + 1])] for i in range(len(data_none))]

    def _data_arrays(self, K, data, data_off, data_none):
        if data_off is None and data is not None and not isinstance(data, np.ndarray):
            if data_none is not None:
                raise ValueError("a list of bytes | None carries its own None flags")
            data, data_off, data_none = self.pack_data(list(data))
        if data_off is None:
            if data is not None:
                raise ValueError("data needs data_off")
            data_off = np.zeros(K + 1, np.int64)       # (only None flags: every range empty)
        data_off = np.ascontiguousarray(data_off, np.int64)
        if data_off.shape != (K + 1,):
            raise ValueError("data_off must have K + 1 entries (got %d for %d events)" % (data_off.shape[0], K))
        data = np.zeros(0, np.uint8) if data is None else np.ascontiguousarray(data, np.uint8).reshape(-1)
        nbytes = data.shape[0]
        if data_none is not None:
            data_none = np.ascontiguousarray(data_none, np.uint8)
            if data_none.shape != (K,):
                raise ValueError("data_none must have one entry per event")
        return (data if nbytes else None), data_off, data_none, nbytes

    def set_event_data(self, first, datas):
        """The data of the stored events [first, first + K) (sw_set_event_data): `datas` is a list of bytes | None, or a
        (data, data_off, data_none) triple as pack_events takes it.  `first` must be the number of events that have data."""
        if isinstance(datas, tuple) and len(datas) == 3 and isinstance(datas[1], np.ndarray):
            K = len(datas[1]) - 1
            data, off, none, nbytes = self._data_arrays(K, *datas)
        else:
            datas = list(datas)
            K = len(datas)
            data, off, none, nbytes = self._data_arrays(K, datas, None, None)
        self._chk(self._L.sw_set_event_data(self._h, int(first), K, _p(data), _p(off), nbytes, _p(none)))

    def set_event_data_device(self, first, K, data=None, data_off=None, data_bytes=0, data_none=None, stream=0):
        """set_event_data from DEVICE memory (sw_set_event_data_device); all of data, data_off, data_none None: every None."""
        dp = [C.c_void_p(q) if q else None for q in (_dev_ptr(a)[0] for a in (data, data_off, data_none))]
        self._chk(self._L.sw_set_event_data_device(self._h, int(first), int(K), dp[0], dp[1], int(data_bytes), dp[2], C.c_void_p(int(stream))))

    def get_event_data(self, first=0, K=None):
        """(data, data_off, data_none) of the events [first, first + K), offsets from 0 (K None: up to the last event that
        has data)."""
        if K is None:
            K = self.data_stats()["events"] - first
        k = max(int(K), 0)
        off, none, nb = np.zeros(k + 1, np.int64), np.zeros(k, np.uint8), C.c_int64()
        data = np.empty(0, np.uint8)
        rc = self._L.sw_get_event_data(self._h, int(first), int(K), 0, None, _p(off), _p(none), C.byref(nb))
        if rc == -34 and nb.value > 0:      # (the size: now with room)
            data = np.empty(int(nb.value), np.uint8)
            rc = self._L.sw_get_event_data(self._h, int(first), int(K), data.shape[0], _p(data), _p(off), _p(none), C.byref(nb))
        self._chk(rc)
        return data, off, none

    def gather_event_data(self, events):
        """(data, data_off, data_none) of the events named by dense index, in the order given, repeats allowed
        (sw_gather_event_data) — e.g. export_ordered()["event"] or export_payload()["event"]."""
        ev = np.ascontiguousarray(events, np.int32).reshape(-1)
        K, nb = ev.shape[0], C.c_int64()
        rc = self._L.sw_gather_event_data(self._h, K, _p(ev), 0, None, None, None, C.byref(nb))
        if not (rc == -34 and nb.value > 0):
            self._chk(rc)
        data, off, none = np.empty(int(nb.value), np.uint8), np.zeros(K + 1, np.int64), np.zeros(K, np.uint8)
        self._chk(self._L.sw_gather_event_data(self._h, K, _p(ev), data.shape[0], _p(data), _p(off), _p(none), C.byref(nb)))
        return data, off, none

    def gather_event_data_device(self, K, events, cap=0, data=None, data_off=None, data_none=None, stream=0):
        """gather_event_data between DEVICE arrays (sw_gather_event_data_device): `events` K int32, data `cap` bytes and
        16-byte aligned, data_off K + 1 int64, data_none K uint8.  Returns the byte total; with cap = 0 and no arrays it
        only asks for it.  A total beyond `cap` raises SwirldHipError -34 and writes nothing."""
        ptrs = [C.c_void_p(q) if q else None for q in (_dev_ptr(a)[0] for a in (events, data, data_off, data_none))]
        nb = C.c_int64()
        rc = self._L.sw_gather_event_data_device(self._h, int(K), ptrs[0], int(cap), ptrs[1], ptrs[2], ptrs[3], C.c_void_p(int(stream)), C.byref(nb))
        if not (rc == -34 and cap == 0 and data is None and data_off is None and data_none is None and nb.value > 0):
            self._chk(rc)
        return int(nb.value)

    def data_stats(self):
        """Events that have data, arena bytes in use, store calls, gather calls, bytes gathered, and (under set_profiling)
        the host milliseconds of the last call's lengths + scan and of its copy."""
        v = [C.c_int64() for _ in range(5)]
        ms = (C.c_double * 2)()
        self._chk(self._L.sw_get_data_stats(self._h, *[C.byref(x) for x in v], ms))
        d = dict(zip(("events", "bytes", "store_calls", "gather_calls", "gather_bytes"), (int(x.value) for x in v)))
        d.update(zip(("scan_ms", "copy_ms"), (float(x) for x in ms)))
        return d

    # ---- validation against the member keys (the crypto of Node.is_valid_event, swirld.py:97-103) ----
    def set_member_keys(self, keys):
        """The members' Ed25519 public keys (n x 32 uint8, or n byte strings): builds the fixed-base table on the device
        (sw_set_member_keys).  Returns the number of keys libsodium would refuse; their members' events are all invalid."""
        if isinstance(keys, (list, tuple)):
            keys = np.frombuffer(b"".join(bytes(k) for k in keys), np.uint8)
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1)
        if keys.shape[0] != 32 * self.n:
            raise ValueError("expected %d keys of 32 bytes" % self.n)
        bad = C.c_int32()
        self._chk(self._L.sw_set_member_keys(self._h, _p(keys), C.byref(bad)))
        return int(bad.value)

    def member_keys(self):
        """(keys n x 32 uint8, usable n bool) as set by set_member_keys."""
        keys, usable = np.empty((self.n, 32), np.uint8), np.empty(self.n, np.uint8)
        self._chk(self._L.sw_get_member_keys(self._h, _p(keys), _p(usable)))
        return keys, usable.astype(bool)

    @staticmethod
    def _pack(items):
        """(bytes as uint8 array, int64 offsets) of a list of byte strings; arrays (data, off) pass through."""
        if isinstance(items, tuple) and len(items) == 2 and isinstance(items[1], np.ndarray):
            return np.ascontiguousarray(items[0], np.uint8).reshape(-1), np.ascontiguousarray(items[1], np.int64)
        off = np.zeros(len(items) + 1, np.int64)
        if len(items):
            np.cumsum([len(m) for m in items], out=off[1:])
        return np.frombuffer(b"".join(items), np.uint8), off

    def validate_payload(self, msgs, sig, creator, whole=None, ids=None):
        """Verdicts of K events, host arrays in and a bool array out (sw_validate_payload).  msgs / whole: lists of byte
        strings, or (uint8 data, int64 offsets of K + 1 entries); msgs[i] is what event i's signature sig[i] (K x 64) by
        member creator[i] covers, whole[i] what its id ids[i] (K x 32) is the BLAKE2b-256 of (whole None: no id check)."""
        data, off = self._pack(msgs)
        K = off.shape[0] - 1
        sig = np.ascontiguousarray(sig, np.uint8).reshape(K, 64)
        creator = np.ascontiguousarray(creator, np.int32)
        if creator.shape != (K,):
            raise ValueError("creator must have one entry per event")
        wdata = woff = None
        wbytes = 0
        if whole is not None:
            wdata, woff = self._pack(whole)
            if woff.shape[0] != K + 1:
                raise ValueError("whole must have one entry per event")
            ids = self._ids(ids, K)
            wbytes = wdata.shape[0]
            if wbytes == 0:
                wdata = np.zeros(1, np.uint8)
        if data.shape[0] == 0:
            data = np.zeros(1, np.uint8)
        ok = np.zeros(K, np.uint8)
        self._chk(self._L.sw_validate_payload(self._h, K, _p(data), _p(off), int(off[-1]) if K else 0, _p(wdata), _p(woff), wbytes,
                                              _p(sig), _p(creator), _p(ids) if whole is not None else None, _p(ok)))
        return ok.astype(bool)

    def validate_payload_device(self, msgs, msg_off, msg_bytes, sig, creator, ok, whole=None, whole_off=None, whole_bytes=0, ids=None,
                                stream=0, count=None):
        """validate_payload for arrays in DEVICE memory (addresses, or objects with data_ptr() / __cuda_array_interface__):
        uint8 msgs of msg_bytes bytes, int64 msg_off (K + 1), K x 64 uint8 sig, int32 creator, and — for the id check —
        whole / whole_off / whole_bytes and K x 32 uint8 ids (8-byte aligned).  `ok` (K uint8 in device memory) receives
        the verdicts, complete for whatever is enqueued on `stream` afterwards — an ingest_payload_device(ok=ok,
        stream=stream) in particular.  K comes from `creator`'s length where it has one, else from `count`.  Returns `ok`."""
        ptrs = [_dev_ptr(a) for a in (msgs, msg_off, whole, whole_off, sig, creator, ids, ok)]
        K = count if count is not None else ptrs[5][1]
        if K is None:
            raise ValueError("the number of events is not known: pass count=")
        a = [C.c_void_p(q) if q else None for q, _ in ptrs]
        self._chk(self._L.sw_validate_payload_device(self._h, int(K), a[0], a[1], int(msg_bytes), a[2], a[3], int(whole_bytes),
                                                     a[4], a[5], a[6], a[7], C.c_void_p(int(stream))))
        return ok

    def validate_stats(self):
        """Validation calls and events judged so far, events accepted (host form only), table builds, and (under
        set_profiling) the host milliseconds of the last table build and of the last validation."""
        v = [C.c_int64() for _ in range(4)]
        ms = (C.c_double * 2)()
        self._chk(self._L.sw_get_validate_stats(self._h, *[C.byref(x) for x in v], ms))
        d = dict(zip(("calls", "events", "accepted", "table_builds"), (int(x.value) for x in v)))
        d.update(zip(("table_ms", "validate_ms"), (float(x) for x in ms)))
        return d

    @property
    def num_events(self):
        return int(self._L.sw_num_events(self._h))

    # ---- hot path ----
    def divide_rounds(self, first, K):
        self._chk(self._L.sw_divide_rounds(self._h, int(first), int(K)))

    def decide_fame(self):
        cap = self.max_round + 2
        out = np.empty(max(cap, 1), np.int32)
        n_new = C.c_int()
        self._chk(self._L.sw_decide_fame(self._h, _p(out), int(out.shape[0]), C.byref(n_new)))
        return out[: n_new.value].copy()

    def decide_fame_partial(self, part, nparts):
        """This part's share of the elections (candidate rounds max_c + part, + nparts, ...):
        (famous[R][n] int8 with -1 = undecided or not owned, decided[R] uint8); nothing committed."""
        R = self.max_round + 1
        fam = np.empty((max(R, 1), self.n), np.int8)
        dec = np.empty(max(R, 1), np.uint8)
        r_out = C.c_int()
        self._chk(self._L.sw_decide_fame_partial(self._h, int(part), int(nparts), _p(fam), _p(dec), R, C.byref(r_out)))
        return fam[:R], dec[:R]

    def commit_fame(self, famous, decided):
        """Commit the element-wise MAX of all parts' tables: the context is then exactly as after
        decide_fame(); returns new_c."""
        fam = np.ascontiguousarray(famous, np.int8)
        dec = np.ascontiguousarray(decided, np.uint8)
        R = dec.shape[0]
        out = np.empty(max(R, 1), np.int32)
        n_new = C.c_int()
        self._chk(self._L.sw_commit_fame(self._h, _p(fam), _p(dec), R, _p(out), int(out.shape[0]), C.byref(n_new)))
        return out[: n_new.value].copy()

    @staticmethod
    def split_link(parts):
        """Link the contexts `parts` (2 .. 8 Hashgraph objects holding the same events, one per GPU or several on one): from now
        on ONE round loop runs over all of them, split inside its iterations (include/swirld_hip.h, part 3).  Every part then
        calls divide_rounds with the same arguments from its own thread: `split_divide_rounds` does that."""
        arr = (C.c_void_p * len(parts))(*[p._h for p in parts])
        rc = parts[0]._L.sw_split_link(arr, len(parts))
        if rc != 0:
            msg = next((m for m in (p._L.sw_last_error(p._h).decode() for p in parts) if m), "") or parts[0]._L.sw_last_error(None).decode()
            raise SwirldHipError(rc, msg)

    def split_unlink(self):
        self._chk(self._L.sw_split_unlink(self._h))

    @staticmethod
    def split_rewind(parts):
        """rewind every linked part and wait for all of them: none may divide again before every one has rewound
        (include/swirld_hip.h, part 3)"""
        for p in parts:
            p.rewind()
        for p in parts:
            p.synchronize()

    @staticmethod
    def split_divide_rounds(parts, first, K):
        """divide_rounds(first, K) on every linked context at once, one host thread per part (the C calls release the GIL and meet
        iteration by iteration on the device); raises the first part's error."""
        import threading
        errs = [None] * len(parts)

        def work(i):
            try:
                parts[i].divide_rounds(first, K)
            except Exception as exc:  # noqa: BLE001
                errs[i] = exc
        ths = [threading.Thread(target=work, args=(i,)) for i in range(len(parts))]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        for e in errs:
            if e is not None:
                raise e

    def find_order(self, rounds):
        rounds = np.ascontiguousarray(sorted(int(r) for r in rounds), np.int32)
        cap = self.num_events
        out = np.empty(max(cap, 1), np.int32)
        n_out = C.c_int64()
        self._chk(self._L.sw_find_order(self._h, _p(rounds), len(rounds), _p(out), cap, C.byref(n_out)))
        return out[: n_out.value].copy()

    # ---- state views ----
    @property
    def max_round(self):
        v = C.c_int()
        self._chk(self._L.sw_max_round(self._h, C.byref(v)))
        return v.value

    def rounds(self, first=0, K=None):
        K = self.num_events - first if K is None else K
        out = np.empty(K, np.int32)
        self._chk(self._L.sw_get_round(self._h, first, K, _p(out)))
        return out

    def heights(self, first=0, K=None):
        K = self.num_events - first if K is None else K
        out = np.empty(K, np.int32)
        self._chk(self._L.sw_get_height(self._h, first, K, _p(out)))
        return out

    def can_see(self, first=0, K=None):
        K = self.num_events - first if K is None else K
        out = np.empty((K, self.n), np.int32)
        self._chk(self._L.sw_get_can_see(self._h, first, K, _p(out)))
        return out

    def sees_masks(self, first=0, K=None):
        K = self.num_events - first if K is None else K
        out = np.empty((K, (self.n + 63) // 64), np.uint64)
        self._chk(self._L.sw_get_sees_mask(self._h, first, K, _p(out)))
        return out

    def witnesses(self, r0=0, r1=None):
        r1 = self.max_round + 1 if r1 is None else r1
        out = np.empty((max(r1 - r0, 0), self.n), np.int32)
        self._chk(self._L.sw_get_witnesses(self._h, r0, r1, _p(out)))
        return out

    def witness_order(self, r):
        """Members of witnesses[r] in dict insertion order (swirld.py:234, 240)."""
        out = np.empty(self.n, np.int32)
        k = C.c_int(0)
        self._chk(self._L.sw_get_witness_order(self._h, int(r), _p(out), C.byref(k)))
        return out[:k.value].copy()

    def famous(self, r0=0, r1=None):
        r1 = self.max_round + 1 if r1 is None else r1
        out = np.empty((max(r1 - r0, 0), self.n), np.int8)
        self._chk(self._L.sw_get_famous(self._h, r0, r1, _p(out)))
        return out

    def famous_events(self, first=0, K=None):
        """Node.famous keyed by event: -1 undecided / not a witness, 0 / 1 (swirld.py:64)."""
        K = self.num_events - first if K is None else K
        out = np.empty(max(K, 0), np.int8)
        self._chk(self._L.sw_get_famous_events(self._h, first, K, _p(out)))
        return out

    def consensus(self, r0=0, r1=None):
        r1 = self.max_round + 1 if r1 is None else r1
        out = np.empty(max(r1 - r0, 0), np.uint8)
        self._chk(self._L.sw_get_consensus(self._h, r0, r1, _p(out)))
        return out

    def vote(self, rv, mv, rc, mc):
        """Node.votes[witness (rv, mv)][witness (rc, mc)]: 0 / 1, or -1 when there is no entry."""
        v = C.c_int8()
        self._chk(self._L.sw_get_vote(self._h, int(rv), int(mv), int(rc), int(mc), C.byref(v)))
        return int(v.value)

    # ---- Node.votes in bulk (swirld.py:60-61, 256-272; csrc/votes.hip.h) ----
    def export_votes_device(self, rv0, rv1, cap_rows, row_voter=None, row_cand_round=None, exists=None, value=None, stream=0):
        """The votes table of the voter rounds [rv0, rv1) written to DEVICE arrays (include/swirld_hip.h): row_voter,
        row_cand_round (int32 per row), exists, value (ceil(n / 64) uint64 per row, 16-byte aligned).  `cap_rows`: rows the
        arrays can take; a larger table raises SwirldHipError with code -34 and writes nothing (cap_rows = 0 with no arrays:
        the size query, which does not raise).  `stream` is made to wait for the arrays.  Returns (n_rows, n_entries)."""
        a = [C.c_void_p(q) if q else None for q in (_dev_ptr(x)[0] for x in (row_voter, row_cand_round, exists, value))]
        n_rows, n_entries = C.c_int64(), C.c_int64()
        rc = self._L.sw_export_votes_device(self._h, int(rv0), int(rv1), int(cap_rows), *a, C.byref(n_rows), C.byref(n_entries), C.c_void_p(int(stream)))
        if not (rc == -34 and int(cap_rows) == 0 and n_rows.value > 0):
            self._chk(rc)
        return int(n_rows.value), int(n_entries.value)

    def export_votes(self, rv0=1, rv1=None):
        """Node.votes of the voter rounds [rv0, rv1) (default: every round) as (row_voter, row_cand_round, exists, value):
        one row per (voter witness y, candidate round rc) with an entry, sorted by (round(y), y, rc); bit mc of
        exists[row] / value[row] (uint64 words, ceil(n / 64) per row): votes[y][witnesses[rc][mc]] exists / is True."""
        rv1 = self.max_round + 1 if rv1 is None else int(rv1)
        nwo = (self.n + 63) // 64
        n_rows, n_entries = C.c_int64(), C.c_int64()
        rc = self._L.sw_export_votes(self._h, int(rv0), rv1, 0, None, None, None, None, C.byref(n_rows), C.byref(n_entries))
        if not (rc == -34 and n_rows.value > 0):
            self._chk(rc)
        K = int(n_rows.value)
        out = (np.empty(K, np.int32), np.empty(K, np.int32), np.empty((K, nwo), np.uint64), np.empty((K, nwo), np.uint64))
        if K:
            self._chk(self._L.sw_export_votes(self._h, int(rv0), rv1, K, *[_p(a) for a in out], C.byref(n_rows), C.byref(n_entries)))
        return out

    def votes_triples(self, rv0=1, rv1=None):
        """export_votes expanded to an int64 [K, 3] array of (y, x, v): voter, candidate (dense indices) and the vote, in row
        order, candidates of a row by member index.  On the exact path with exact_history on: every entry of the store
        (vote_entries(); rv0 and rv1 are not looked at — voters are no longer named by rounds)."""
        if self.exact_history and self.exact:
            y, x, v = self.vote_entries()
            return np.stack([y, x, v], axis=1).astype(np.int64)
        row_voter, row_cand, exists, value = self.export_votes(rv0, rv1)
        rows = len(row_voter)
        bits = lambda w: np.unpackbits(np.ascontiguousarray(w.astype("<u8")).view(np.uint8).reshape(rows, -1), axis=1,  # noqa: E731
                                       bitorder="little")[:, :self.n]
        out = np.empty((0, 3), np.int64)
        if rows:
            ex = bits(exists)
            i, mc = np.nonzero(ex)
            wit = self.witnesses(0, int(row_cand.max()) + 1)
            out = np.empty((len(i), 3), np.int64)
            out[:, 0] = row_voter[i]
            out[:, 1] = wit[row_cand[i], mc]
            out[:, 2] = bits(value)[i, mc]
        return out

    def votes_stats(self):
        """Bulk exports since the context was created: calls, rows and entries exported, election levels replayed, and under
        set_profiling the host time of the most recent call's phases (plan + existence + counts, rows + values)."""
        c = [C.c_int64() for _ in range(4)]
        ms = (C.c_double * 2)()
        self._chk(self._L.sw_get_votes_stats(self._h, *[C.byref(x) for x in c], ms))
        return {"calls": c[0].value, "rows": c[1].value, "entries": c[2].value, "levels": c[3].value, "phase_ms": [ms[0], ms[1]]}

    # ---- gossip side from device state (N4) ----
    def known_heights(self, head_event):
        """{member -> height of the newest event of that member `head_event` sees} as an array, -1 absent
        (what Node.sync reports, swirld.py:125-126)."""
        out = np.empty(self.n, np.int32)
        self._chk(self._L.sw_get_known_heights(self._h, int(head_event), _p(out)))
        return out

    def sync_diff(self, head_event, known_height):
        """Chain position ranges (first[m], end[m]) of the events a peer with these heights is missing
        (what Node.ask_sync sends, swirld.py:154-161)."""
        kn = np.ascontiguousarray(known_height, np.int32)
        first = np.empty(self.n, np.int32)
        end = np.empty(self.n, np.int32)
        tot = C.c_int64()
        self._chk(self._L.sw_sync_diff(self._h, int(head_event), _p(kn), _p(first), _p(end), C.byref(tot)))
        return first, end, int(tot.value)

    def chain_events(self, member, p0, p1):
        out = np.empty(max(p1 - p0, 0), np.int32)
        self._chk(self._L.sw_get_chain_events(self._h, int(member), int(p0), int(p1), _p(out)))
        return out

    # ---- answering a sync on the device (Node.ask_sync, swirld.py:148-161; csrc/gossip.hip.h) ----
    def known_heights_device(self, head, out, stream=0):
        """known_heights(head) left in DEVICE memory: `out` holds n int32 (an address, or an object with data_ptr() /
        __cuda_array_interface__); `stream` (a raw hipStream_t) is made to wait for it.  Returns `out`."""
        ptr, ln = _dev_ptr(out)
        if ln is not None and ln < self.n:
            raise ValueError("out holds %d entries, expected %d" % (ln, self.n))
        self._chk(self._L.sw_get_known_heights_device(self._h, int(head), C.c_void_p(ptr), C.c_void_p(int(stream))))
        return out

    def export_payload_device(self, head, known, cap, ids, sp_ids, op_ids, arity, creator, t=None, sig=None, event=None, stream=0):
        """The events sync_diff(head, known) names, written to DEVICE arrays in the layout ingest_payload_device takes
        (member-major, chain order inside a member; include/swirld_hip.h).  `known`: n int32 in device memory, or None (the
        asker knows nobody).  `cap`: events the arrays can take; a larger diff raises SwirldHipError with code -34 and writes
        nothing (export_size gives the size).  The id arrays and `sig` 16-byte aligned.  `stream` has the producer of `known`
        enqueued and is made to wait for the arrays.  Returns the number of events exported."""
        ptrs = [_dev_ptr(a)[0] for a in (known, ids, sp_ids, op_ids, arity, creator, t, sig, event)]
        a = [C.c_void_p(q) if q else None for q in ptrs]
        n_out = C.c_int64()
        self._chk(self._L.sw_export_payload_device(self._h, int(head), a[0], int(cap), *a[1:], C.c_void_p(int(stream)), C.byref(n_out)))
        return int(n_out.value)

    def export_size(self, head, known=None, stream=0):
        """Number of events export_payload_device(head, known, ...) would write (`known` in device memory, or None)."""
        kp = _dev_ptr(known)[0]
        n_out = C.c_int64()
        rc = self._L.sw_export_payload_device(self._h, int(head), C.c_void_p(kp) if kp else None, 0, *([None] * 8),
                                              C.c_void_p(int(stream)), C.byref(n_out))
        if rc != -34:      # (a diff is never empty — the head is always sent — so the size query answers SW_ERANGE)
            self._chk(rc)
        return int(n_out.value)

    def export_payload(self, head, known=None, *, data=False):
        """The same into fresh numpy arrays: a dict with ids, sp_ids, op_ids (K x 32 uint8), arity (uint8), creator (int32),
        t (float64), sig (K x 64 uint8) and event (int32, the dense indices here).  `known`: n heights (host), None = nobody.
        data=True adds data, data_off, data_none: the events' data, through gather_event_data."""
        kn = None if known is None else np.ascontiguousarray(known, np.int32)
        if kn is not None and kn.shape != (self.n,):
            raise ValueError("known must have one height per member")
        n_out = C.c_int64()
        rc = self._L.sw_export_payload(self._h, int(head), _p(kn), 0, *([None] * 8), C.byref(n_out))
        if rc != -34:
            self._chk(rc)
        K = int(n_out.value)
        d = dict(ids=np.empty((K, 32), np.uint8), sp_ids=np.empty((K, 32), np.uint8), op_ids=np.empty((K, 32), np.uint8),
                 arity=np.empty(K, np.uint8), creator=np.empty(K, np.int32), t=np.empty(K, np.float64),
                 sig=np.empty((K, 64), np.uint8), event=np.empty(K, np.int32))
        self._chk(self._L.sw_export_payload(self._h, int(head), _p(kn), K, *[_p(d[k]) for k in ("ids", "sp_ids", "op_ids", "arity", "creator", "t", "sig", "event")],
                                            C.byref(n_out)))
        if data:
            d["data"], d["data_off"], d["data_none"] = self.gather_event_data(d["event"])
        return d

    # ---- answering a sync by the pruned walk, forked hashgraphs included (swirld.py:154-161; csrc/walk.hip.h) ----
    def _heights_arg(self, a, what):
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.int32)
        if a.shape != (self.n,):
            raise ValueError("%s must have one entry per member" % what)
        return a

    def fork_trunks(self):
        """Per member the height of its earliest fork point (the lowest event that is the self-parent of two stored events),
        -1 for a member with two roots, INT32_MAX for a member that has not forked: what Node.ask_sync caps a forked
        member's reported height with.  Either path."""
        out = np.empty(self.n, np.int32)
        self._chk(self._L.sw_get_fork_trunks(self._h, _p(out)))
        return out

    def sync_walk(self, head, known=None, cap=None):
        """The events Node.ask_sync's BFS reaches from `head` (swirld.py:154-161) as dense indices, ascending: `head` itself,
        and every parent p of a reached event with known[creator(p)] < 0 or height(p) > known[creator(p)].  `known`: n
        heights (host), None = the asker knows nobody; `cap`: n heights, the walk prunes at min(known, cap) (fork_trunks()).
        Fast and exact path; needs no id index."""
        kn, cp = self._heights_arg(known, "known"), self._heights_arg(cap, "cap")
        n_out = C.c_int64()
        out = np.empty(max(int(head) + 1, 1), np.int32)      # (the walk names ancestors of the head: at most head + 1 events, so ONE call)
        self._chk(self._L.sw_sync_walk(self._h, int(head), _p(kn), _p(cp), len(out), _p(out), C.byref(n_out)))
        return out[:int(n_out.value)].copy()

    def export_walk_device(self, head, known, cap, cap_events, ids, sp_ids, op_ids, arity, creator, t=None, sig=None, event=None, stream=0):
        """The events of sync_walk(head, known, cap) written to DEVICE arrays in the layout ingest_payload_device takes, in
        ascending dense index.  `known`, `cap`: n int32 in device memory, or None.  `cap_events`: events the arrays can take; a
        larger set raises SwirldHipError with code -34 and writes nothing (walk_size gives the size).  Alignment and
        streams as for export_payload_device.  Returns the number of events exported."""
        ptrs = [_dev_ptr(a)[0] for a in (known, cap, ids, sp_ids, op_ids, arity, creator, t, sig, event)]
        a = [C.c_void_p(q) if q else None for q in ptrs]
        n_out = C.c_int64()
        self._chk(self._L.sw_export_walk_device(self._h, int(head), a[0], a[1], int(cap_events), *a[2:], C.c_void_p(int(stream)), C.byref(n_out)))
        return int(n_out.value)

    def walk_size(self, head, known=None, cap=None, stream=0):
        """Number of events export_walk_device(head, known, cap, ...) would write (`known`, `cap` in device memory, or None)."""
        kp, cp = _dev_ptr(known)[0], _dev_ptr(cap)[0]
        n_out = C.c_int64()
        rc = self._L.sw_export_walk_device(self._h, int(head), C.c_void_p(kp) if kp else None, C.c_void_p(cp) if cp else None, 0, *([None] * 8),
                                           C.c_void_p(int(stream)), C.byref(n_out))
        if rc != -34:
            self._chk(rc)
        return int(n_out.value)

    def export_walk(self, head, known=None, cap=None, *, data=False):
        """export_payload's dict for the events of sync_walk(head, known, cap), in ascending dense index (host arrays)."""
        kn, cp = self._heights_arg(known, "known"), self._heights_arg(cap, "cap")
        n_out = C.c_int64()
        rc = self._L.sw_export_walk(self._h, int(head), _p(kn), _p(cp), 0, *([None] * 8), C.byref(n_out))
        if rc != -34:
            self._chk(rc)
        K = int(n_out.value)
        d = dict(ids=np.empty((K, 32), np.uint8), sp_ids=np.empty((K, 32), np.uint8), op_ids=np.empty((K, 32), np.uint8),
                 arity=np.empty(K, np.uint8), creator=np.empty(K, np.int32), t=np.empty(K, np.float64),
                 sig=np.empty((K, 64), np.uint8), event=np.empty(K, np.int32))
        self._chk(self._L.sw_export_walk(self._h, int(head), _p(kn), _p(cp), K,
                                         *[_p(d[k]) for k in ("ids", "sp_ids", "op_ids", "arity", "creator", "t", "sig", "event")], C.byref(n_out)))
        if data:
            d["data"], d["data_off"], d["data_none"] = self.gather_event_data(d["event"])
        return d

    def walk_stats(self):
        """Walk calls, events named, levels of the most recent walk, and (under set_profiling) the host milliseconds of the
        most recent call's phases: walk + count, list, gather."""
        a, b, lv = C.c_int64(), C.c_int64(), C.c_int64()
        ms = (C.c_double * 3)()
        self._chk(self._L.sw_get_walk_stats(self._h, C.byref(a), C.byref(b), C.byref(lv), ms))
        return dict(calls=int(a.value), events=int(b.value), levels=int(lv.value), walk_ms=ms[0], list_ms=ms[1], gather_ms=ms[2])

    def pull_from(self, peer, peer_head, my_head, validate=False, *, data=False, walk=False, trunks=False):
        """Node.sync without the new event (swirld.py:125-136) against `peer`, a Hashgraph on the same device: my known
        heights at `my_head` -> the peer's diff at `peer_head` -> my ingest, all in device memory.  Returns (n_sent,
        n_stored); my new events are the last n_stored ones, their ids event_ids(num_events - n_stored).
        validate=True puts is_valid_event's crypto in the middle (sw_sync_pull_validated): the signed bytes of the peer's
        events are built on the device, judged by MY member keys and event class, and only valid events are ingested;
        returns (n_sent, n_valid, n_stored).  Needs set_member_keys; the bytes are built with data None.
        data=True (sw_sync_pull_data): the events travel WITH their data, from the peer's data store into mine, and with
        validate=True the signed bytes are built with it; both data stores must be complete.
        walk=True (sw_sync_pull_walk): the peer answers by the pruned walk instead of the chain ranges, so either side may
        hold forks; trunks=True caps the walk by the PEER's fork_trunks(), which is how two contexts holding different
        siblings of a fork exchange them.  validate and data mean the same."""
        a, b = C.c_int64(), C.c_int64()
        if trunks and not walk:
            raise ValueError("trunks=True needs walk=True")
        if walk:
            v = C.c_int64()
            self._chk(self._L.sw_sync_pull_walk(self._h, int(my_head), peer._h, int(peer_head), 1 if trunks else 0, 1 if validate else 0,
                                                1 if data else 0, C.byref(a), C.byref(v), C.byref(b)))
            return (int(a.value), int(v.value), int(b.value)) if validate else (int(a.value), int(b.value))
        if data:
            v = C.c_int64()
            self._chk(self._L.sw_sync_pull_data(self._h, int(my_head), peer._h, int(peer_head), 1 if validate else 0, C.byref(a), C.byref(v), C.byref(b)))
            return (int(a.value), int(v.value), int(b.value)) if validate else (int(a.value), int(b.value))
        if validate:
            v = C.c_int64()
            self._chk(self._L.sw_sync_pull_validated(self._h, int(my_head), peer._h, int(peer_head), C.byref(a), C.byref(v), C.byref(b)))
            return int(a.value), int(v.value), int(b.value)
        self._chk(self._L.sw_sync_pull(self._h, int(my_head), peer._h, int(peer_head), C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    # ---- the signed bytes of events built on the device (dumps(ev[:-1]), dumps(ev), swirld.py:95-103; csrc/pack.hip.h) ----
    def set_event_class(self, module, qualname):
        """Module and qualified name of the Event class (Event.__module__, Event.__qualname__): part of dumps(ev) and so of
        every id.  1 .. 255 bytes of UTF-8 each; default "swirld", "Event"."""
        self._chk(self._L.sw_set_event_class(self._h, module.encode("utf-8"), qualname.encode("utf-8")))

    def event_class(self):
        m, q = C.create_string_buffer(256), C.create_string_buffer(256)
        self._chk(self._L.sw_get_event_class(self._h, m, q))
        return m.value.decode("utf-8"), q.value.decode("utf-8")

    def pack_bound(self, K, data_bytes=0):
        """(msg_bytes, whole_bytes): upper bounds of the two streams for any K events with data_bytes bytes of data."""
        m, w = C.c_int64(), C.c_int64()
        self._chk(self._L.sw_pack_bound(self._h, int(K), int(data_bytes), C.byref(m), C.byref(w)))
        return int(m.value), int(w.value)

    def pack_events(self, sp_ids, op_ids, arity, creator, t, sig, data=None, data_off=None, data_none=None):
        """dumps(ev[:-1]) and dumps(ev) of K events from host arrays (sw_pack_events): sp_ids / op_ids K x 32 uint8 (read
        where arity is 2), arity uint8, creator int32 (dense member index; the key bytes are set_member_keys'), t float64,
        sig K x 64 uint8; data (uint8) / data_off (K + 1 int64) / data_none (uint8 per event) or None: every data None.
        Returns (msgs, msg_off, whole, whole_off, encodable): uint8 bytes and int64 offsets as validate_payload takes them
        as (data, offsets) pairs, and a bool per event — False: the event has no such bytes and length 0 in both."""
        arity = np.ascontiguousarray(arity, np.uint8)
        K = arity.shape[0]
        sp_ids, op_ids = self._ids(sp_ids, K), self._ids(op_ids, K)
        creator = np.ascontiguousarray(creator, np.int32)
        t = np.ascontiguousarray(t, np.float64)
        sig = np.ascontiguousarray(sig, np.uint8).reshape(K, 64)
        if creator.shape != (K,) or t.shape != (K,):
            raise ValueError("creator and t must have one entry per event")
        nbytes = 0
        if data_off is not None:
            data_off = np.ascontiguousarray(data_off, np.int64)
            if data_off.shape != (K + 1,):
                raise ValueError("data_off must have K + 1 entries")
            data = np.zeros(0, np.uint8) if data is None else np.ascontiguousarray(data, np.uint8).reshape(-1)
            nbytes = data.shape[0]
            if nbytes == 0:
                data = None
            if data_none is not None:
                data_none = np.ascontiguousarray(data_none, np.uint8)
                if data_none.shape != (K,):
                    raise ValueError("data_none must have one entry per event")
        elif data is not None or data_none is not None:
            raise ValueError("data needs data_off")
        bm, bw = self.pack_bound(K, nbytes)
        msgs, whole = np.empty(max(bm, 1), np.uint8), np.empty(max(bw, 1), np.uint8)
        moff, woff = np.empty(K + 1, np.int64), np.empty(K + 1, np.int64)
        enc = np.zeros(K, np.uint8)
        tm, tw = C.c_int64(), C.c_int64()
        self._chk(self._L.sw_pack_events(self._h, K, _p(sp_ids), _p(op_ids), _p(arity), _p(creator), _p(t), _p(sig), _p(data), _p(data_off),
                                         nbytes, _p(data_none), _p(msgs), _p(moff), bm, _p(whole), _p(woff), bw, _p(enc),
                                         C.byref(tm), C.byref(tw)))
        return msgs[:tm.value], moff, whole[:tw.value], woff, enc.astype(bool)

    def pack_events_device(self, sp_ids, op_ids, arity, creator, t, sig, msgs, msg_off, msg_cap, whole, whole_off, whole_cap,
                           encodable=None, data=None, data_off=None, data_bytes=0, data_none=None, stream=0, count=None):
        """pack_events for arrays in DEVICE memory (addresses, or objects with data_ptr() / __cuda_array_interface__), as
        export_payload_device writes them.  msgs / whole (uint8, msg_cap / whole_cap bytes, at least pack_bound's, 16-byte
        aligned) and msg_off / whole_off (K + 1 int64) receive the streams in the form validate_payload_device takes;
        `encodable` (K uint8, optional) the flags.  Complete for whatever is enqueued on `stream` afterwards; nothing is
        read back.  K comes from `creator`'s length where it has one, else from `count`."""
        ptrs = [_dev_ptr(a) for a in (sp_ids, op_ids, arity, creator, t, sig, data, data_off, data_none, msgs, msg_off, whole, whole_off,
                                      encodable)]
        K = count if count is not None else ptrs[3][1]
        if K is None:
            raise ValueError("the number of events is not known: pass count=")
        a = [C.c_void_p(q) if q else None for q, _ in ptrs]
        self._chk(self._L.sw_pack_events_device(self._h, int(K), a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], int(data_bytes), a[8],
                                                a[9], a[10], int(msg_cap), a[11], a[12], int(whole_cap), a[13], C.c_void_p(int(stream))))

    def pack_stats(self):
        """Pack calls and events encoded so far, bytes written (host form only), and (under set_profiling) the host
        milliseconds of the last call's lengths-and-scan and of its two writers."""
        v = [C.c_int64() for _ in range(3)]
        ms = (C.c_double * 2)()
        self._chk(self._L.sw_get_pack_stats(self._h, *[C.byref(x) for x in v], ms))
        d = dict(zip(("calls", "events", "bytes"), (int(x.value) for x in v)))
        d.update(zip(("scan_ms", "write_ms"), (float(x) for x in ms)))
        return d

    # ---- the wire bytes of a sync answer (dumps((head, subset)), swirld.py:166; loads, swirld.py:129; csrc/wire.hip.h) ----
    def pack_message_bound(self, K, data_bytes=0):
        """Upper bound of the message of any K events with data_bytes bytes of data."""
        m = C.c_int64()
        self._chk(self._L.sw_pack_message_bound(self._h, int(K), int(data_bytes), C.byref(m)))
        return int(m.value)

    def pack_message(self, head_id, ids, sp_ids, op_ids, arity, creator, t, sig, data=None, data_off=None, data_none=None):
        """The canonical wire form of (head, {id: Event}) from host arrays (sw_pack_message), as bytes: any pickle.loads reads
        it.  The arrays are pack_events' plus the ids and the head's id (32 bytes).  One event that cannot be encoded makes
        the message unbuildable: SwirldHipError -22 names it."""
        arity = np.ascontiguousarray(arity, np.uint8)
        K = arity.shape[0]
        head = self._ids(head_id, 1)
        ids, sp_ids, op_ids = self._ids(ids, K), self._ids(sp_ids, K), self._ids(op_ids, K)
        creator = np.ascontiguousarray(creator, np.int32)
        t = np.ascontiguousarray(t, np.float64)
        sig = np.ascontiguousarray(sig, np.uint8).reshape(K, 64)
        if creator.shape != (K,) or t.shape != (K,):
            raise ValueError("creator and t must have one entry per event")
        nbytes = 0
        if data_off is not None:
            data_off = np.ascontiguousarray(data_off, np.int64)
            if data_off.shape != (K + 1,):
                raise ValueError("data_off must have K + 1 entries")
            data = np.zeros(0, np.uint8) if data is None else np.ascontiguousarray(data, np.uint8).reshape(-1)
            nbytes = data.shape[0]
            if nbytes == 0:
                data = None
            if data_none is not None:
                data_none = np.ascontiguousarray(data_none, np.uint8)
                if data_none.shape != (K,):
                    raise ValueError("data_none must have one entry per event")
        elif data is not None or data_none is not None:
            raise ValueError("data needs data_off")
        cap = self.pack_message_bound(K, nbytes)
        msg = np.empty(cap, np.uint8)
        n = C.c_int64()
        self._chk(self._L.sw_pack_message(self._h, K, _p(head), _p(ids), _p(sp_ids), _p(op_ids), _p(arity), _p(creator), _p(t), _p(sig), _p(data),
                                          _p(data_off), nbytes, _p(data_none), _p(msg), cap, C.byref(n)))
        return msg[:n.value].tobytes()

    def pack_message_device(self, head_id, ids, sp_ids, op_ids, arity, creator, t, sig, msg, msg_cap, msg_len, data=None, data_off=None,
                            data_bytes=0, data_none=None, stream=0, count=None):
        """pack_message between DEVICE arrays (sw_pack_message_device), as export_walk_device and gather_event_data_device
        leave them.  msg: uint8, msg_cap bytes (at least pack_message_bound's), 16-byte aligned; msg_len: one int64 that
        receives the length, or -1 when an event cannot be encoded (msg is then not written).  Nothing is read back."""
        ptrs = [_dev_ptr(a) for a in (head_id, ids, sp_ids, op_ids, arity, creator, t, sig, data, data_off, data_none, msg, msg_len)]
        K = count if count is not None else ptrs[5][1]
        if K is None:
            raise ValueError("the number of events is not known: pass count=")
        a = [C.c_void_p(q) if q else None for q, _ in ptrs]
        self._chk(self._L.sw_pack_message_device(self._h, int(K), *a[:10], int(data_bytes), a[10], a[11], int(msg_cap), a[12], C.c_void_p(int(stream))))

    def unpack_message(self, msg, cap_events=None, cap_data=None):
        """The strict reader (sw_unpack_message): None for bytes that are not the canonical form under this context's event
        class, else a dict of host arrays: head (32 uint8), ids / sp_ids / op_ids (K x 32), arity, creator (member index by
        set_member_keys' table, -1 for a key of no member), t, sig (K x 64), data, data_off (K + 1), data_none.  Nothing of
        `msg` is ever unpickled.  Capacities default to what a message of this length can hold; a smaller one that does not
        suffice raises SwirldHipError -34."""
        buf = np.frombuffer(bytes(msg), np.uint8)
        nb = buf.shape[0]
        ke = nb // 150 if cap_events is None else int(cap_events)
        kd = nb if cap_data is None else int(cap_data)
        d = dict(head=np.zeros(32, np.uint8), ids=np.zeros((ke, 32), np.uint8), sp_ids=np.zeros((ke, 32), np.uint8), op_ids=np.zeros((ke, 32), np.uint8),
                 arity=np.zeros(ke, np.uint8), creator=np.zeros(ke, np.int32), t=np.zeros(ke, np.float64), sig=np.zeros((ke, 64), np.uint8),
                 data=np.zeros(kd, np.uint8), data_off=np.zeros(ke + 1, np.int64), data_none=np.zeros(ke, np.uint8))
        n, m = C.c_int64(), C.c_int64()
        self._chk(self._L.sw_unpack_message(self._h, _p(buf) if nb else None, nb, ke, kd,
                                            *[_p(d[k]) for k in ("head", "ids", "sp_ids", "op_ids", "arity", "creator", "t", "sig", "data", "data_off", "data_none")],
                                            C.byref(n), C.byref(m)))
        K = int(n.value)
        if K < 0:
            return None
        out = {k: (v if k == "head" else v[:K]) for k, v in d.items()}
        out["data_off"] = d["data_off"][:K + 1]
        out["data"] = d["data"][:int(m.value)]
        return out

    def unpack_message_device(self, msg, msg_bytes, cap_events, cap_data, head_id, ids, sp_ids, op_ids, arity, creator, t, sig, data, data_off,
                              data_none, stream=0):
        """unpack_message between DEVICE arrays (sw_unpack_message_device): data 16-byte aligned, data_off cap_events + 1
        entries.  Returns (n_events, n_data_bytes); n_events -1: not canonical, nothing promised about the arrays."""
        a = [C.c_void_p(q) if q else None for q in (_dev_ptr(x)[0] for x in (msg, head_id, ids, sp_ids, op_ids, arity, creator, t, sig, data, data_off,
                                                                               data_none))]
        n, m = C.c_int64(), C.c_int64()
        self._chk(self._L.sw_unpack_message_device(self._h, a[0], int(msg_bytes), int(cap_events), int(cap_data), *a[1:], C.c_void_p(int(stream)),
                                                   C.byref(n), C.byref(m)))
        return int(n.value), int(m.value)

    def export_message(self, head, known=None, cap=None, *, data=True, want_count=False):
        """Node.ask_sync's reply body for the events of sync_walk(head, known, cap), built on the device in one call
        (sw_export_message): walk, export, data gather (data=False: every d is None) and the wire bytes.  Returns bytes."""
        kn, cp = self._heights_arg(known, "known"), self._heights_arg(cap, "cap")
        nb, ne = C.c_int64(), C.c_int64()
        msg = getattr(self, "_wire_buf", None)      # kept between calls: a message that does not fit costs one more call, once
        if msg is None:
            msg = self._wire_buf = np.empty(1 << 20, np.uint8)
        rc = self._L.sw_export_message(self._h, int(head), _p(kn), _p(cp), 1 if data else 0, _p(msg), msg.shape[0], C.byref(nb), C.byref(ne))
        if rc == -34 and nb.value > msg.shape[0]:
            msg = self._wire_buf = np.empty(int(nb.value) + int(nb.value) // 4, np.uint8)
            rc = self._L.sw_export_message(self._h, int(head), _p(kn), _p(cp), 1 if data else 0, _p(msg), msg.shape[0], C.byref(nb), C.byref(ne))
        self._chk(rc)
        out = msg[:nb.value].tobytes()
        return (out, int(ne.value)) if want_count else out

    def export_message_device(self, head, known, cap, msg, msg_cap, *, data=True, stream=0):
        """export_message into DEVICE memory (`known`, `cap`: n int32 in device memory, or None).  Returns (msg_bytes,
        n_events); a message longer than msg_cap raises SwirldHipError -34 and writes nothing."""
        a = [C.c_void_p(q) if q else None for q in (_dev_ptr(x)[0] for x in (known, cap, msg))]
        nb, ne = C.c_int64(), C.c_int64()
        self._chk(self._L.sw_export_message_device(self._h, int(head), a[0], a[1], 1 if data else 0, a[2], int(msg_cap), C.c_void_p(int(stream)),
                                                   C.byref(nb), C.byref(ne)))
        return int(nb.value), int(ne.value)

    def ingest_message(self, msg, validate=True, *, data=True):
        """Node.sync's intake of a reply body in the canonical wire form (sw_ingest_message): strict unpack, with `validate`
        the signed bytes built and judged by my keys and event class, then ingest_payload (data=True keeps the data).
        Returns None for bytes that are not canonical (nothing stored, nothing unpickled), else a dict: head (32 bytes),
        index (ingest_payload's codes per event of the message), n_events, n_valid (validate only), n_stored."""
        buf = np.frombuffer(bytes(msg), np.uint8)
        nb = buf.shape[0]
        head, index = np.zeros(32, np.uint8), np.zeros(nb // 150 + 1, np.int32)
        ne, nv, ns = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self._L.sw_ingest_message(self._h, _p(buf) if nb else None, nb, 1 if validate else 0, 1 if data else 0, _p(head), _p(index),
                                            C.byref(ne), C.byref(nv), C.byref(ns)))
        K = int(ne.value)
        if K < 0:
            return None
        return dict(head=head.tobytes(), index=index[:K].copy(), n_events=K, n_valid=int(nv.value) if validate else None, n_stored=int(ns.value))

    def ingest_message_device(self, msg, msg_bytes, validate=True, *, data=True, head_id=None, index=None, stream=0):
        """ingest_message for a message in DEVICE memory; head_id (32 uint8) and index (msg_bytes // 150 int32 at least) are
        optional device arrays.  Returns (n_events, n_valid, n_stored); n_events -1: not canonical, nothing stored."""
        a = [C.c_void_p(q) if q else None for q in (_dev_ptr(x)[0] for x in (msg, head_id, index))]
        ne, nv, ns = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self._L.sw_ingest_message_device(self._h, a[0], int(msg_bytes), 1 if validate else 0, 1 if data else 0, a[1], a[2],
                                                   C.c_void_p(int(stream)), C.byref(ne), C.byref(nv), C.byref(ns)))
        return int(ne.value), int(nv.value), int(ns.value)

    def wire_stats(self):
        """Message writer calls, events and bytes (forms that know the length), reader calls, events, refused messages."""
        v = [C.c_int64() for _ in range(6)]
        self._chk(self._L.sw_get_wire_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("pack_calls", "pack_events", "pack_bytes", "unpack_calls", "unpack_events", "refused"), (int(x.value) for x in v)))

    # ---- creating signed events (Node.new_event, swirld.py:82-95, for a batch; csrc/sign.hip.h) ----
    def set_signing_seeds(self, members, seeds):
        """The Ed25519 seeds (32 bytes each: K x 32 uint8, or K byte strings) of the members this context may sign for
        (sw_set_signing_keys); any subset of the members, after set_member_keys.  A seed that does not derive its member's
        key raises SwirldHipError -22 and changes nothing.  The secrets stay on the device."""
        members = np.ascontiguousarray(members, np.int32).reshape(-1)
        if isinstance(seeds, (list, tuple)):
            seeds = np.frombuffer(b"".join(bytes(s) for s in seeds), np.uint8)
        seeds = np.ascontiguousarray(seeds, np.uint8).reshape(-1)
        if seeds.shape[0] != 32 * members.shape[0]:
            raise ValueError("expected %d seeds of 32 bytes" % members.shape[0])
        self._chk(self._L.sw_set_signing_keys(self._h, members.shape[0], _p(members), _p(seeds)))

    def clear_signing_seeds(self):
        """Overwrites the device copy of the signing keys with zeros (sw_clear_signing_keys)."""
        self._chk(self._L.sw_clear_signing_keys(self._h))

    def signing_members(self):
        """One bool per member: does the context hold its signing key?"""
        has = np.zeros(self.n, np.uint8)
        self._chk(self._L.sw_get_signing_members(self._h, _p(has)))
        return has.astype(bool)

    def _event_arrays(self, creator, self_parent, other_parent, t):
        creator = np.ascontiguousarray(creator, np.int32)
        K = creator.shape[0]
        sp, op = np.ascontiguousarray(self_parent, np.int32), np.ascontiguousarray(other_parent, np.int32)
        t = np.ascontiguousarray(t, np.float64)
        if sp.shape != (K,) or op.shape != (K,) or t.shape != (K,):
            raise ValueError("creator, parents and t must have equal length")
        return K, creator, sp, op, t

    def sign_events(self, creator, self_parent, other_parent, t, data=None, data_off=None, data_none=None):
        """Signatures and ids of K events in topological order, host arrays (sw_sign_events): creator / parents as
        append_events takes them — a parent index below num_events names a stored event, one at or above it the batch
        position index - num_events — t float64, data a list of bytes | None or (data, data_off, data_none) as pack_events
        takes them.  Nothing is stored.  Returns a dict of ids, sp_ids, op_ids (K x 32 uint8), arity (uint8) and sig
        (K x 64 uint8): the arrays ingest_payload and pack_events take."""
        K, creator, sp, op, t = self._event_arrays(creator, self_parent, other_parent, t)
        d, off, none, nbytes = (None, None, None, 0) if data is None and data_off is None and data_none is None else self._data_arrays(K, data, data_off, data_none)
        out = dict(ids=np.zeros((K, 32), np.uint8), sp_ids=np.zeros((K, 32), np.uint8), op_ids=np.zeros((K, 32), np.uint8),
                   arity=np.zeros(K, np.uint8), sig=np.zeros((K, 64), np.uint8))
        self._chk(self._L.sw_sign_events(self._h, K, _p(creator), _p(sp), _p(op), _p(t), _p(d), _p(off), nbytes, _p(none), _p(out["ids"]),
                                         _p(out["sp_ids"]), _p(out["op_ids"]), _p(out["arity"]), _p(out["sig"])))
        return out

    def sign_events_device(self, creator, self_parent, other_parent, t, ids, sp_ids, op_ids, arity, sig, data=None, data_off=None, data_bytes=0,
                           data_none=None, stream=0, count=None):
        """sign_events between arrays in DEVICE memory (sw_sign_events_device): ids / sp_ids / op_ids (K x 32 uint8) and sig
        (K x 64 uint8) 16-byte aligned.  Complete for whatever is enqueued on `stream` afterwards; the call synchronises
        once, for the number of levels.  K comes from `creator`'s length where it has one, else from `count`."""
        ptrs = [_dev_ptr(a) for a in (creator, self_parent, other_parent, t, data, data_off, data_none, ids, sp_ids, op_ids, arity, sig)]
        K = count if count is not None else ptrs[0][1]
        if K is None:
            raise ValueError("the number of events is not known: pass count=")
        a = [C.c_void_p(q) if q else None for q, _ in ptrs]
        self._chk(self._L.sw_sign_events_device(self._h, int(K), a[0], a[1], a[2], a[3], a[4], a[5], int(data_bytes), a[6], a[7], a[8], a[9], a[10], a[11],
                                                C.c_void_p(int(stream))))

    def create_events(self, creator, self_parent, other_parent, t, data=None, data_off=None, data_none=None, *, want_ids=False):
        """sign_events, then the append, the id commit and (with a complete data store) the data append (sw_create_events):
        afterwards the context is in the state ingest_payload(..., data=...) would leave for the same, host-signed events.
        Atomic on rejection.  Returns the dense index of the first created event; with want_ids (first, ids, sig)."""
        K, creator, sp, op, t = self._event_arrays(creator, self_parent, other_parent, t)
        d, off, none, nbytes = (None, None, None, 0) if data is None and data_off is None and data_none is None else self._data_arrays(K, data, data_off, data_none)
        first = C.c_int64()
        ids, sig = (np.zeros((K, 32), np.uint8), np.zeros((K, 64), np.uint8)) if want_ids else (None, None)
        self._chk(self._L.sw_create_events(self._h, K, _p(creator), _p(sp), _p(op), _p(t), _p(d), _p(off), nbytes, _p(none), C.byref(first), _p(ids), _p(sig)))
        return (int(first.value), ids, sig) if want_ids else int(first.value)

    def create_events_device(self, creator, self_parent, other_parent, t, data=None, data_off=None, data_bytes=0, data_none=None, ids=None, sig=None,
                             stream=0, count=None):
        """create_events from arrays in DEVICE memory (sw_create_events_device); ids / sig (optional, 16-byte aligned)
        receive the batch's ids and signatures.  Returns the dense index of the first created event."""
        ptrs = [_dev_ptr(a) for a in (creator, self_parent, other_parent, t, data, data_off, data_none, ids, sig)]
        K = count if count is not None else ptrs[0][1]
        if K is None:
            raise ValueError("the number of events is not known: pass count=")
        a = [C.c_void_p(q) if q else None for q, _ in ptrs]
        first = C.c_int64()
        self._chk(self._L.sw_create_events_device(self._h, int(K), a[0], a[1], a[2], a[3], a[4], a[5], int(data_bytes), a[6], C.c_void_p(int(stream)),
                                                  C.byref(first), a[7], a[8]))
        return int(first.value)

    def sign_stats(self):
        """Sign calls and events signed so far, the levels of the last call, key sets, and (under set_profiling) the host
        milliseconds of the last call's levels + sort, signing and commit."""
        v = [C.c_int64() for _ in range(4)]
        ms = (C.c_double * 3)()
        self._chk(self._L.sw_get_sign_stats(self._h, *[C.byref(x) for x in v], ms))
        d = dict(zip(("calls", "events", "levels", "key_sets"), (int(x.value) for x in v)))
        d.update(zip(("levels_ms", "sign_ms", "commit_ms"), (float(x) for x in ms)))
        return d

    # ---- one event signed by one wavefront, and the gossip turn around it (swirld.py:82-95, 122-146, 322-328; csrc/turn.hip.h) ----
    def create_event(self, member, self_parent, other_parent, t, data=None, *, want_ids=False):
        """create_events for ONE event, whose signature the 64 lanes of a wave share (sw_create_event): member's event at time
        t on the stored events self_parent / other_parent (both -1: a root), data bytes | None.  The same verdicts, the same
        state afterwards.  Returns the event's dense index; with want_ids (index, id, sig) as 32 / 64 bytes."""
        idx = C.c_int64()
        eid, sig = (C.create_string_buffer(32), C.create_string_buffer(64)) if want_ids else (None, None)
        raw = None if data is None else bytes(data)
        self._chk(self._L.sw_create_event(self._h, int(member), int(self_parent), int(other_parent), float(t), raw, -1 if raw is None else len(raw),
                                          C.byref(idx), eid, sig))
        return (int(idx.value), eid.raw, sig.raw) if want_ids else int(idx.value)

    def gossip_turn(self, peer, member, my_head, peer_head, t, data=None, *, validate=True, data_store=False, trunks=False, consensus=True):
        """One step of a node (sw_gossip_turn; swirld.py:125-146, 324-328): pull what `peer` (a Hashgraph on the same device)
        knows at peer_head beyond my_head by the pruned walk, create member's event (data, (my_head, peer_head's event), t)
        — the other parent found in my id index on the device — then divide_rounds, decide_fame and find_order.  Leaves
        this context as pull_from(walk=True, ...), create_event, divide_rounds, decide_fame, find_order would.  Returns a
        TurnResult: n_sent, n_valid, n_stored, new_head (-1 when the peer's head did not arrive: no event), n_new_rounds,
        n_ordered, stage, and new_rounds (the rounds decide_fame added to the consensus)."""
        flags = ((_lib.SW_TURN_VALIDATE if validate else 0) | (_lib.SW_TURN_DATA if data_store else 0) | (_lib.SW_TURN_TRUNKS if trunks else 0) |
                 (0 if consensus else _lib.SW_TURN_NO_CONSENSUS))
        raw = None if data is None else bytes(data)
        res = _lib.TurnResult()
        # (a round is a function of an event's ancestry: what arrives has the peer's rounds, the new event at most one more)
        cap = max(self.max_round, peer.max_round) + 3 if consensus else 0
        rounds = np.empty(max(cap, 1), np.int32)
        rc = self._L.sw_gossip_turn(self._h, int(member), int(my_head), peer._h, int(peer_head), float(t), raw, -1 if raw is None else len(raw), flags,
                                    _p(rounds), cap, C.byref(res), C.sizeof(res))
        self._chk(rc)
        return TurnResult(*(int(getattr(res, k)) for k, _ in _lib.TurnResult._fields_), rounds[: res.n_new_rounds].copy())

    def turn_stats(self):
        """create_event calls, events the one-wave signer signed, gossip turns, stamped launches; under set_profiling the phase
        lengths of the last stamped launch in microseconds (phase_us: load, hash1, base_mult, encode, hash2, muladd, id) and
        the raw stamps."""
        v = [C.c_int64() for _ in range(4)]
        st = (C.c_uint64 * 8)()
        tick = C.c_double()
        self._chk(self._L.sw_get_turn_stats(self._h, *[C.byref(x) for x in v], st, C.byref(tick)))
        d = dict(zip(("create_calls", "events", "turns", "stamped"), (int(x.value) for x in v)))
        d["stamps"] = [int(x) for x in st]
        d["tick_ns"] = float(tick.value)
        names = ("load", "hash1", "base_mult", "encode", "hash2", "muladd", "id")
        d["phase_us"] = {k: (d["stamps"][i + 1] - d["stamps"][i]) * d["tick_ns"] / 1e3 for i, k in enumerate(names)}
        return d

    def export_stats(self):
        """Export calls and events exported since the context was created, and (under set_profiling) the host
        milliseconds of the most recent call's phases: ranges + count, gather."""
        v = [C.c_int64() for _ in range(2)]
        ms = (C.c_double * 2)()
        self._chk(self._L.sw_get_export_stats(self._h, *[C.byref(x) for x in v], ms))
        return dict(calls=int(v[0].value), events=int(v[1].value), ranges_ms=float(ms[0]), gather_ms=float(ms[1]))

    def transactions(self):
        n = C.c_int64()
        self._chk(self._L.sw_num_ordered(self._h, C.byref(n)))
        out = np.empty(n.value, np.int32)
        self._chk(self._L.sw_get_transactions(self._h, 0, n.value, _p(out)))
        return out

    # ---- what find_order decided per event (swirld.py:283-309; csrc/consensus.hip.h) ----
    @property
    def num_ordered(self):
        n = C.c_int64()
        self._chk(self._L.sw_num_ordered(self._h, C.byref(n)))
        return int(n.value)

    def round_received(self, first=0, K=None):
        """Round received of the events [first, first + K) (swirld.py:283), -1 = not ordered yet."""
        K = self.num_events - first if K is None else K
        out = np.empty(max(K, 0), np.int32)
        self._chk(self._L.sw_get_round_received(self._h, int(first), int(K), _p(out)))
        return out

    def consensus_time(self, first=0, K=None):
        """Consensus timestamp of the events [first, first + K) (swirld.py:305, bit for bit), NaN = not ordered yet."""
        K = self.num_events - first if K is None else K
        out = np.empty(max(K, 0), np.float64)
        self._chk(self._L.sw_get_consensus_time(self._h, int(first), int(K), _p(out)))
        return out

    def export_ordered(self, first=0, K=None, ids=None, *, data=False):
        """Positions [first, first + K) of the order as numpy arrays: a dict with event (int32, the dense indices: a slice of
        transactions()), creator (int32), round_received (int32), time (float64) and — `ids` True, or None [default] and the id index
        complete — ids (K x 32 uint8).  data=True adds data, data_off, data_none: the events' data, through gather_event_data."""
        K = self.num_ordered - first if K is None else K
        k = max(int(K), 0)
        d = dict(event=np.empty(k, np.int32), creator=np.empty(k, np.int32), round_received=np.empty(k, np.int32), time=np.empty(k, np.float64))
        for with_ids in ((True, False) if ids is None else (bool(ids),)):
            i32 = np.empty((k, 32), np.uint8) if with_ids else None
            rc = self._L.sw_export_ordered(self._h, int(first), int(K), _p(d["event"]), _p(i32), _p(d["creator"]), _p(d["round_received"]), _p(d["time"]))
            if not (rc == -95 and with_ids and ids is None):    # (no complete id index: the same without ids)
                break
        self._chk(rc)
        if with_ids:
            d["ids"] = i32
        if data:
            d["data"], d["data_off"], d["data_none"] = self.gather_event_data(d["event"])
        return d

    def export_ordered_device(self, first, K, event=None, ids=None, creator=None, round_received=None, time=None, stream=0):
        """Positions [first, first + K) of the order written to DEVICE arrays (addresses, or objects with data_ptr() /
        __cuda_array_interface__, e.g. torch tensors): event, creator, round_received int32, time float64, ids K x 32 uint8
        and 16-byte aligned; None = not wanted.  `stream` (a raw hipStream_t) is made to wait for the arrays; there is no
        host synchronisation.  Returns K."""
        a = []
        for what, arr in (("event", event), ("ids", ids), ("creator", creator), ("round_received", round_received), ("time", time)):
            ptr, ln = _dev_ptr(arr)
            if ln is not None and ln < K:
                raise ValueError("%s holds %d entries, expected %d" % (what, ln, K))
            a.append(C.c_void_p(ptr) if ptr else None)
        self._chk(self._L.sw_export_ordered_device(self._h, int(first), int(K), *a, C.c_void_p(int(stream))))
        return int(K)

    def consensus_stats(self):
        """find_order calls that recorded events and the events they recorded, export_ordered[_device] calls and the
        positions they exported, since the context was created."""
        v = [C.c_int64() for _ in range(4)]
        self._chk(self._L.sw_get_consensus_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("record_calls", "recorded_events", "export_calls", "exported_events"), (int(x.value) for x in v)))

    # ---- measurement ----
    def counters(self):
        c = Counters()
        # (size-aware call: a library whose struct has grown cannot overrun this mirror)
        self._chk(self._L.sw_get_counters_sized(self._h, C.byref(c), C.sizeof(c)))
        return {k: int(getattr(c, k)) for k, _ in Counters._fields_}

    TALLY_KERNELS = ("k_tally", "k_tally_bits", "k_tally_tree")

    @property
    def tally_kernel(self):
        """Name of the step-3 kernel of the round loop the most recent divide_rounds used (sw_get_tally_impl)."""
        i = int(self._L.sw_get_tally_impl(self._h))
        if not 0 <= i < len(self.TALLY_KERNELS):
            raise SwirldHipError(i, "sw_get_tally_impl")
        return self.TALLY_KERNELS[i]

    def set_profiling(self, enable=True):
        self._chk(self._L.sw_set_profiling(self._h, 1 if enable else 0))

    def timings(self):
        t = Timings()
        self._chk(self._L.sw_get_timings(self._h, C.byref(t)))
        return {k: (int(getattr(t, k)) if k.endswith("_launches") else float(getattr(t, k)))
                for k, _ in Timings._fields_}

    def debug_clocks(self):
        """[4096][32] uint64 phase stamps of the round-loop kernels (needs SW_DEBUG_CLOCKS=1 at creation)."""
        out = np.zeros((4096, 32), np.uint64)
        self._chk(self._L.sw_debug_clocks(self._h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def debug_block_clocks(self, iters=1024):
        """[iters][2][2048] uint64: when every workgroup of k_resolve_band / the tally kernel was done (SW_DEBUG_CLOCKS=3)."""
        out = np.zeros((int(iters), 2, 2048), np.uint64)
        self._chk(self._L.sw_debug_block_clocks(self._h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def set_forks(self, accept=True):
        """Forked events: accepted (the context moves to the exact path, csrc/exact.hip.h — the reference's
        statements on the device, identical results, far slower) or refused with SW_ENOTSUP."""
        self._chk(self._L.sw_set_forks(self._h, 1 if accept else 0))

    @property
    def exact(self):
        """True once a forked event moved the context to the exact path."""
        v = C.c_int(0)
        self._chk(self._L.sw_get_exact(self._h, C.byref(v)))
        return bool(v.value)

    # ---- the history of the exact path (csrc/exact_history.hip.h; include/swirld_hip.h) ----
    def set_exact_history(self, enable=True):
        """Before the first append: keep round received, consensus time, the ordered stream and Node.votes (keyed by
        event) once a forked event has moved the context to the exact path.  Off by default: the vote history is the
        reference's unbounded dict."""
        self._chk(self._L.sw_set_exact_history(self._h, 1 if enable else 0))

    @property
    def exact_history(self):
        v = C.c_int(0)
        self._chk(self._L.sw_get_exact_history(self._h, C.byref(v), None))
        return bool(v.value)

    @property
    def votes_available(self):
        """exact_history is on and the vote store is complete (not over its ceiling, no KeyError, handed over by the fast path)."""
        v = C.c_int(0)
        self._chk(self._L.sw_get_exact_history(self._h, None, C.byref(v)))
        return bool(v.value)

    def votes_by_event(self, y, x):
        """Node.votes[y][x] for dense event indices (scalars or equally long arrays): 0 / 1, -1 = no entry."""
        ya, xa = np.ascontiguousarray(np.atleast_1d(y), np.int32), np.ascontiguousarray(np.atleast_1d(x), np.int32)
        if ya.shape != xa.shape:
            raise ValueError("voter and candidate arrays differ in length")
        out = np.empty(len(ya), np.int8)
        self._chk(self._L.sw_get_votes_by_event(self._h, len(ya), _p(ya), _p(xa), _p(out)))
        return int(out[0]) if np.ndim(y) == 0 and np.ndim(x) == 0 else out

    def vote_entries(self, first=0):
        """Every entry of Node.votes from position `first` of the store on as (voter, candidate, value) arrays of dense
        event indices and 0 / 1, in the store's order (entries of the fast path first, then first insertion)."""
        n = C.c_int64()
        rc = self._L.sw_export_vote_entries(self._h, int(first), 0, None, None, None, C.byref(n))
        if not (rc == -34 and n.value > first):
            self._chk(rc)
        K = max(int(n.value) - int(first), 0)
        out = (np.empty(K, np.int32), np.empty(K, np.int32), np.empty(K, np.int8))
        if K:
            self._chk(self._L.sw_export_vote_entries(self._h, int(first), K, *[_p(a) for a in out], C.byref(n)))
        return out

    def vote_entries_device(self, first, cap_entries, voter=None, cand=None, value=None, stream=0):
        """vote_entries written to DEVICE arrays (int32, int32, int8) of `cap_entries` entries; `stream` is made to wait for
        them.  Too small a capacity raises SwirldHipError with code -34 and writes nothing (cap_entries = 0 with no arrays:
        the size query, which does not raise).  Returns the number of entries in the store."""
        a = [C.c_void_p(q) if q else None for q in (_dev_ptr(t)[0] for t in (voter, cand, value))]
        n = C.c_int64()
        rc = self._L.sw_export_vote_entries_device(self._h, int(first), int(cap_entries), *a, C.byref(n), C.c_void_p(int(stream)))
        if not (rc == -34 and int(cap_entries) == 0 and n.value > first):
            self._chk(rc)
        return int(n.value)

    def vote_store_stats(self):
        v = [C.c_int64() for _ in range(7)]
        self._chk(self._L.sw_get_vote_store_stats(self._h, *[C.byref(t) for t in v]))
        return dict(zip(("entries", "capacity", "bytes", "grows", "imported", "lookups", "exported"), (int(t.value) for t in v)))

    def set_window(self, enable=True, chunk_mb=0, lapse_events=0):
        """Windowed can_see table (before the first append): rows no later call can read are evicted
        after every find_order (HIP virtual memory management, include/swirld_hip.h).  lapse_events > 0:
        a member silent for more than that many events stops holding the window back and its further
        events are refused (sw_set_window_lapse; the reference keeps every row)."""
        self._chk(self._L.sw_set_window(self._h, 1 if enable else 0, int(chunk_mb)))
        if enable and lapse_events:
            self._chk(self._L.sw_set_window_lapse(self._h, int(lapse_events)))

    def window(self):
        """(first resident event, bytes of the can_see table currently mapped, evictions so far)."""
        a, b, e = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self._L.sw_get_window(self._h, C.byref(a), C.byref(b), C.byref(e)))
        return int(a.value), int(b.value), int(e.value)

    # ---- multi-GPU split of the can_see table by event ranges (include/swirld_hip.h) ----
    @property
    def row_stride(self):
        """int32 elements per can_see row on the device (members padded to a multiple of 64)."""
        return int(self._L.sw_row_stride(self._h))

    def cansee_range(self, first, K):
        """Sweep the can_see rows of [first, first + K) from a halo (asynchronous); rows below the halo are leaves."""
        self._chk(self._L.sw_cansee_range(self._h, int(first), int(K)))

    def cansee_repair(self, first, K):
        """Repair the provisional entries of a swept range from the (imported) final rows below it; device-gated."""
        self._chk(self._L.sw_cansee_repair(self._h, int(first), int(K)))

    def export_rows(self, first, K, dst_ptr, stream=0):
        """Copy rows [first, first + K) to DEVICE memory at `dst_ptr` (K * row_stride int32); `stream` (a raw
        hipStream_t, e.g. torch.cuda.current_stream().cuda_stream) is made to wait for the copy."""
        self._chk(self._L.sw_export_rows(self._h, int(first), int(K), C.c_void_p(int(dst_ptr)), C.c_void_p(int(stream))))

    def import_rows(self, first, K, src_ptr, stream=0):
        """Copy rows [first, first + K) from DEVICE memory at `src_ptr` into the table, after what `stream` has
        enqueued so far; sw_divide_rounds will not sweep them."""
        self._chk(self._L.sw_import_rows(self._h, int(first), int(K), C.c_void_p(int(src_ptr)), C.c_void_p(int(stream))))

    def range_stats(self):
        """(provisional entries counted by the range sweeps, entries changed by the repairs, ranges swept twice)."""
        a, b, e = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self._L.sw_get_range_stats(self._h, C.byref(a), C.byref(b), C.byref(e)))
        return int(a.value), int(b.value), int(e.value)

    def rewind(self):
        """Forget all voting state; the ingested events stay resident (bench utility)."""
        self._chk(self._L.sw_rewind(self._h))

    def reset(self):
        """rewind() and forget the events too; device storage stays allocated (bench utility)."""
        self._chk(self._L.sw_reset(self._h))

    def synchronize(self):
        self._chk(self._L.sw_synchronize(self._h))


BatchSummary = collections.namedtuple("BatchSummary", "events divided rounds ordered n_new_rounds n_ordered stage code event")
BATCH_STAGES = {0: None, 1: "divide", 2: "fame", 3: "order"}
BatchStepArrays = collections.namedtuple("BatchStepArrays", "took rounds_off rounds tx_off event round_received time n_failed")
BatchExportStats = collections.namedtuple("BatchExportStats", "calls launches entries d2h_copies")
BatchSynthStats = collections.namedtuple("BatchSynthStats", "calls events launches mirror_refreshes")
BatchNetworkStatus = collections.namedtuple("BatchNetworkStatus", "begun turns created stage code view")
BatchNetworkStats = collections.namedtuple("BatchNetworkStats", "calls turns imported launches")


class HashgraphBatch:
    """B independent hashgraphs of one member count in one device allocation (sw_batch_*, csrc/batch.hip.h): a step runs the
    reference's main-loop step — divide_rounds(new events), decide_fame(), find_order(new_c) — for every hashgraph that
    takes part, one wavefront each, in one launch.  Exact with or without forks.  All capacity is fixed here: cap_events
    events per hashgraph, cap_rounds rounds (0: cap_events + 3, which always suffices; the vote layers take 2 n^2 bytes per
    round, so lower it where memory matters).  No id index, gossip, crypto or event-keyed vote log: those are Hashgraph's.
    Events come from the host (append) or are generated on the device: synth_begin(seed, mode, p0, p1) then synth(K), in
    instalments, leave in hashgraph b exactly what synth_hashgraph(n, N_b, seed_b, ...) returns, bit for bit, without the
    host generating, validating or uploading an event; events(b) reads stored events back."""

    def __init__(self, B, n_members, stake=None, coin_period=6, cap_events=1024, cap_rounds=0, device=0):
        self._L = _lib.load()
        self.B, self.n = int(B), int(n_members)
        st = None
        if stake is not None:
            raw = np.asarray(stake)
            if raw.shape == (self.n,):
                raw = np.broadcast_to(raw, (self.B, self.n))
            if raw.shape != (self.B, self.n):
                raise ValueError("stake must have one entry per member, or one row of them per hashgraph")
            if raw.dtype.kind not in "iu":
                as_f = raw.astype(np.float64)
                if not np.all(np.isfinite(as_f)) or np.any(as_f != np.floor(as_f)):
                    raise ValueError("stakes must be integers")
            if np.any(raw.astype(np.float64) < 0):
                raise ValueError("stakes must be non-negative")
            st = np.ascontiguousarray(raw, np.uint64)
        self._h = C.c_void_p()
        rc = self._L.sw_batch_create(self.B, self.n, _p(st), int(coin_period), int(cap_events), int(cap_rounds), int(device), C.byref(self._h))
        if rc != 0:
            raise SwirldHipError(rc, (self._L.sw_batch_last_error(None) or b"").decode())
        v = [C.c_int64(), C.c_int(), C.c_int(), C.c_int64(), C.c_int64(), C.c_int64()]
        self._chk(self._L.sw_batch_shape(self._h, *[C.byref(x) for x in v]))
        self.npad, self.cap_events, self.cap_rounds, self.device_bytes = int(v[2].value), int(v[3].value), int(v[4].value), int(v[5].value)

    @staticmethod
    def bytes_needed(B, n_members, cap_events, cap_rounds=0):
        """Device bytes a batch of this shape allocates (sw_batch_bytes)."""
        return int(_lib.load().sw_batch_bytes(int(B), int(n_members), int(cap_events), int(cap_rounds)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.sw_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise SwirldHipError(rc, (self._L.sw_batch_last_error(self._h) or b"").decode())

    def append(self, streams=None, *, off=None, creator=None, self_parent=None, other_parent=None, t=None, sig=None):
        """New events for every hashgraph: `streams` is a list of B entries, each None (nothing) or a tuple (creator,
        self_parent, other_parent[, t[, sig]]) with parents as indices local to the hashgraph; or the same as CSR arrays
        (off of B + 1 entries and the concatenated arrays).  Atomic over the batch: one bad event anywhere stores nothing."""
        if streams is not None:
            if len(streams) != self.B:
                raise ValueError("one entry per hashgraph (None for nothing)")
            empty = (np.zeros(0, np.int32),) * 3
            parts = [empty if s is None else tuple(s) for s in streams]
            off = np.zeros(self.B + 1, np.int64)
            np.cumsum([len(p[0]) for p in parts], out=off[1:])
            creator, self_parent, other_parent = (np.concatenate([np.asarray(p[i], np.int32) for p in parts]) for i in range(3))
            has_t = [len(p) > 3 and p[3] is not None for p in parts if len(p[0])]
            has_s = [len(p) > 4 and p[4] is not None for p in parts if len(p[0])]
            if any(has_t) != all(has_t) or any(has_s) != all(has_s):
                raise ValueError("timestamps / signatures for every hashgraph of the call, or for none")
            if has_t and has_t[0]:
                t = np.concatenate([np.asarray(p[3], np.float64) for p in parts if len(p[0])])
            if has_s and has_s[0]:
                sig = np.concatenate([np.asarray(p[4], np.uint8).reshape(-1, 64) for p in parts if len(p[0])])
        off = np.ascontiguousarray(off, np.int64)
        if off.shape != (self.B + 1,):
            raise ValueError("off must have B + 1 entries")
        total = int(off[-1])
        creator = np.ascontiguousarray(creator, np.int32)
        sp = np.ascontiguousarray(self_parent, np.int32)
        op = np.ascontiguousarray(other_parent, np.int32)
        if not (creator.shape == sp.shape == op.shape == (total,)):
            raise ValueError("creator / parents must have off[B] entries")
        t = None if t is None else np.ascontiguousarray(t, np.float64)
        sig = None if sig is None else np.ascontiguousarray(sig, np.uint8).reshape(total, 64)
        if t is not None and t.shape != (total,):
            raise ValueError("t must have off[B] entries")
        self._chk(self._L.sw_batch_append(self._h, _p(off), _p(creator), _p(sp), _p(op), _p(t), _p(sig)))

    def _per_hashgraph(self, v, dtype, what):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype), (self.B,)) if np.ndim(v) == 0 else v, dtype)
        if a.shape != (self.B,):
            raise ValueError("%s must be a scalar or have one entry per hashgraph" % what)
        return a

    def synth_begin(self, seed, mode=0, p0=0.0, p1=0.0, which=None):
        """Seed and parameters of synth_hashgraph per hashgraph (scalars broadcast over B; which: a mask, None = all).  The
        selected hashgraphs must be empty; calling again on a still-empty hashgraph replaces its parameters."""
        w = None if which is None else self._ctl(np.asarray(which) != 0, np.uint8, "which")
        self._chk(self._L.sw_synth_batch_begin(self._h, _p(w), _p(self._per_hashgraph(seed, np.uint64, "seed")),
                                               _p(self._per_hashgraph(mode, np.int32, "mode")), _p(self._per_hashgraph(p0, np.float64, "p0")),
                                               _p(self._per_hashgraph(p1, np.float64, "p1"))))

    def synth(self, K):
        """Every hashgraph generates and stores its next K[b] events on the device (an int broadcasts; 0: none).  Returns
        the number of events stored.  Atomic over the batch: beyond cap_events or cap_rounds anywhere nothing is stored."""
        total = C.c_int64(0)
        self._chk(self._L.sw_synth_batch(self._h, _p(self._per_hashgraph(K, np.int64, "K")), C.byref(total)))
        return int(total.value)

    def synth_stats(self):
        """(synth calls that stored events, events generated, kernel launches, refreshes of the append mirror)."""
        out = np.zeros(4, np.int64)
        self._chk(self._L.sw_synth_batch_stats(self._h, _p(out)))
        return BatchSynthStats(*[int(x) for x in out])

    def events(self, b, first=0, K=None):
        """The stored events [first, first + K) of hashgraph b as append() takes them: (creator, self_parent, other_parent,
        t, sig) with sig uint8 [K][64].  Generated or appended."""
        K = self._events(b) - first if K is None else K
        cr, sp, op = np.empty(K, np.int32), np.empty(K, np.int32), np.empty(K, np.int32)
        t, sig = np.empty(K, np.float64), np.empty((K, 64), np.uint8)
        self._chk(self._L.sw_get_batch_events(self._h, b, first, K, _p(cr), _p(sp), _p(op), _p(t), _p(sig)))
        return cr, sp, op, t, sig

    def step(self, K=None, collect=True):
        """One main-loop step.  K: events to divide per hashgraph (0: it sits the step out), None: all undivided ones.
        Returns the number of hashgraphs this step froze when collect is False; else a list of B entries: (new_c,
        transactions) of the step, or None for a hashgraph that sat out or is frozen (see summary())."""
        Ka = None
        if K is not None:
            Ka = np.ascontiguousarray(K, np.int64)
            if Ka.shape != (self.B,):
                raise ValueError("K must have one entry per hashgraph")
        before = self.summary_array() if collect else None
        failed = C.c_int64(0)
        self._chk(self._L.sw_batch_step(self._h, _p(Ka), C.byref(failed)))
        self.n_failed = int(failed.value)
        if not collect:
            return self.n_failed
        now = self.summary_array()
        out = [None] * self.B
        took = (now[:, 1] != before[:, 1]) & (now[:, 6] == 0)
        for b in np.nonzero(took)[0]:   # (counts from the read-back in hand: one or two copies per hashgraph that took part)
            b = int(b)
            n_new, n_out = int(now[b, 4]), int(now[b, 5])
            tx = self.transactions(b, int(now[b, 3]) - n_out, n_out) if n_out else np.zeros(0, np.int32)
            out[b] = (self.new_rounds(b, n_new) if n_new else np.zeros(0, np.int32), tx)
        return out

    def summary_array(self):
        """int64 [B][9]: events, divided, rounds, ordered, the last step's n_new_rounds and n_ordered, status (stage, code, event)."""
        out = np.zeros((self.B, 9), np.int64)
        self._chk(self._L.sw_batch_get_summary(self._h, _p(out)))
        return out

    def summary(self, b=None):
        s = self.summary_array()
        if b is not None:
            return BatchSummary(*[int(x) for x in s[b]])
        return [BatchSummary(*[int(x) for x in row]) for row in s]

    def _events(self, b):
        return self.summary(b).events

    def heights(self, b, first=0, K=None):
        K = self._events(b) - first if K is None else K
        out = np.empty(K, np.int32)
        self._chk(self._L.sw_batch_get_height(self._h, b, first, K, _p(out)))
        return out

    def rounds(self, b, first=0, K=None):
        K = self._events(b) - first if K is None else K
        out = np.empty(K, np.int32)
        self._chk(self._L.sw_batch_get_round(self._h, b, first, K, _p(out)))
        return out

    def can_see(self, b, first=0, K=None):
        K = self.summary(b).divided - first if K is None else K
        out = np.empty((K, self.n), np.int32)
        self._chk(self._L.sw_batch_get_can_see(self._h, b, first, K, _p(out)))
        return out

    def witnesses(self, b, r0=0, r1=None):
        r1 = self.summary(b).rounds if r1 is None else r1
        out = np.empty((r1 - r0, self.n), np.int32)
        self._chk(self._L.sw_batch_get_witnesses(self._h, b, r0, r1, _p(out)))
        return out

    def witness_order(self, b, r):
        out = np.empty(self.n, np.int32)
        cnt = C.c_int(0)
        self._chk(self._L.sw_batch_get_witness_order(self._h, b, r, _p(out), C.byref(cnt)))
        return out[:cnt.value].copy()

    def famous(self, b, r0=0, r1=None):
        r1 = self.summary(b).rounds if r1 is None else r1
        out = np.empty((r1 - r0, self.n), np.int8)
        self._chk(self._L.sw_batch_get_famous(self._h, b, r0, r1, _p(out)))
        return out

    def famous_events(self, b, first=0, K=None):
        K = self._events(b) - first if K is None else K
        out = np.empty(K, np.int8)
        self._chk(self._L.sw_batch_get_famous_events(self._h, b, first, K, _p(out)))
        return out

    def consensus(self, b, r0=0, r1=None):
        r1 = self.summary(b).rounds if r1 is None else r1
        out = np.empty(r1 - r0, np.uint8)
        self._chk(self._L.sw_batch_get_consensus(self._h, b, r0, r1, _p(out)))
        return out

    def new_rounds(self, b, count=None):
        """sorted(new_c) of hashgraph b's last step (count: its length where the caller has it from a summary)."""
        cap = max(1, self.summary(b).n_new_rounds if count is None else int(count))
        out = np.empty(cap, np.int32)
        cnt = C.c_int(0)
        self._chk(self._L.sw_batch_get_new_rounds(self._h, b, _p(out), cap, C.byref(cnt)))
        return out[:cnt.value].copy()

    def transactions(self, b, first=0, K=None):
        K = self.summary(b).ordered - first if K is None else K
        out = np.empty(K, np.int32)
        self._chk(self._L.sw_batch_get_transactions(self._h, b, first, K, _p(out), None, None))
        return out

    def ordered(self, b, first=0, K=None):
        """(events, round received, consensus timestamp) of hashgraph b's ordered events [first, first + K)."""
        K = self.summary(b).ordered - first if K is None else K
        ev, rr, ts = np.empty(K, np.int32), np.empty(K, np.int32), np.empty(K, np.float64)
        self._chk(self._L.sw_batch_get_transactions(self._h, b, first, K, _p(ev), _p(rr), _p(ts)))
        return ev, rr, ts

    # ---- the whole batch per call (sw_export_batch_*): ragged arrays, hashgraph b at [off[b], off[b + 1]) ----
    def _ctl(self, a, dtype, what):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype)
        if a.shape != (self.B,):
            raise ValueError("%s must have one entry per hashgraph" % what)
        return a

    def _export(self, fn, ctl, specs, cap=None):
        """Host form: a sizing call (none where the caller knows `cap`), then the export.  specs: (name, dtype, columns)."""
        off, total = np.zeros(self.B + 1, np.int64), C.c_int64(0)
        ctl = [_p(a) for a in ctl]
        if cap is None:
            self._chk(fn(self._h, *ctl, 0, _p(off), *([None] * len(specs)), C.byref(total)))
            cap = int(total.value)
        out = {name: np.empty(cap if cols == 1 else (cap, cols), dtype) for name, dtype, cols in specs}
        self._chk(fn(self._h, *ctl, int(cap), _p(off), *[_p(out[name]) for name, _, _ in specs], C.byref(total)))
        T = int(total.value)
        out = {name: a[:T] for name, a in out.items()}
        out["off"] = off
        return out

    def _export_device(self, fn, ctl, arrays, cap, stream):
        """Device form: arrays = (name, object or address or None, columns).  Returns (off, total)."""
        ptrs, room = [], []
        for name, a, cols in arrays:
            ptr, _ = _dev_ptr(a)
            ptrs.append(C.c_void_p(ptr) if ptr else None)
            shape = getattr(a, "shape", None)
            if ptr and shape is not None and not isinstance(a, (int, np.integer)):
                room.append(int(np.prod(shape, dtype=np.int64)) // cols)
        if cap is None:
            if not room:
                raise ValueError("the capacity of the arrays is not known: pass cap=")
            cap = min(room)
        elif room and min(room) < cap:
            raise ValueError("an array holds %d entries, cap is %d" % (min(room), cap))
        off, total = np.zeros(self.B + 1, np.int64), C.c_int64(0)
        self._chk(fn(self._h, *[_p(a) for a in ctl], int(cap), _p(off), *ptrs, C.byref(total), C.c_void_p(int(stream))))
        return off, int(total.value)

    def export_ordered(self, first=None, count=None):
        """Log positions [first[b], first[b] + count[b]) of every hashgraph (None: from 0 / to the end): a dict of off
        (int64 [B + 1]), event, round_received (int32) and time (float64).  One launch, one synchronisation."""
        ctl = [self._ctl(first, np.int64, "first"), self._ctl(count, np.int64, "count")]
        return self._export(self._L.sw_export_batch_ordered, ctl, [("event", np.int32, 1), ("round_received", np.int32, 1), ("time", np.float64, 1)])

    def export_new_rounds(self, which=None):
        """sorted(new_c) of every hashgraph's own last step (which[b] = 0: left out; a frozen hashgraph: empty): off, rounds."""
        w = None if which is None else self._ctl(np.asarray(which) != 0, np.uint8, "which")
        return self._export(self._L.sw_export_batch_new_rounds, [w], [("rounds", np.int32, 1)])

    def export_events(self, first=None, count=None):
        """Events [first[b], first[b] + count[b]) of every hashgraph: off, creator, height, round (-1: not divided), famous (int8)."""
        ctl = [self._ctl(first, np.int64, "first"), self._ctl(count, np.int64, "count")]
        return self._export(self._L.sw_export_batch_events, ctl,
                            [("creator", np.int32, 1), ("height", np.int32, 1), ("round", np.int32, 1), ("famous", np.int8, 1)])

    def export_rounds(self, r0=None, r1=None):
        """Rounds [r0[b], r1[b]) of every hashgraph: off (in rounds), witnesses (int32 [total][n]), famous (int8 [total][n]),
        consensus (uint8 [total])."""
        ctl = [self._ctl(r0, np.int32, "r0"), self._ctl(r1, np.int32, "r1")]
        return self._export(self._L.sw_export_batch_rounds, ctl, [("witnesses", np.int32, self.n), ("famous", np.int8, self.n), ("consensus", np.uint8, 1)])

    def export_ordered_device(self, first=None, count=None, event=None, round_received=None, time=None, cap=None, stream=0):
        """export_ordered into DEVICE arrays (addresses, or objects with data_ptr() / __cuda_array_interface__, 16-byte aligned;
        None = not wanted) of `cap` entries (default: the shortest array).  `stream` (a raw hipStream_t) is made to wait for
        them; no host synchronisation.  Returns (off, total); more than cap entries raise SwirldHipError -34, nothing written."""
        ctl = [self._ctl(first, np.int64, "first"), self._ctl(count, np.int64, "count")]
        return self._export_device(self._L.sw_export_batch_ordered_device, ctl,
                                   [("event", event, 1), ("round_received", round_received, 1), ("time", time, 1)], cap, stream)

    def export_new_rounds_device(self, which=None, rounds=None, cap=None, stream=0):
        """export_new_rounds into a DEVICE array (see export_ordered_device).  Returns (off, total)."""
        w = None if which is None else self._ctl(np.asarray(which) != 0, np.uint8, "which")
        return self._export_device(self._L.sw_export_batch_new_rounds_device, [w], [("rounds", rounds, 1)], cap, stream)

    def export_events_device(self, first=None, count=None, creator=None, height=None, round=None, famous=None, cap=None, stream=0):
        """export_events into DEVICE arrays (see export_ordered_device).  Returns (off, total)."""
        ctl = [self._ctl(first, np.int64, "first"), self._ctl(count, np.int64, "count")]
        return self._export_device(self._L.sw_export_batch_events_device, ctl,
                                   [("creator", creator, 1), ("height", height, 1), ("round", round, 1), ("famous", famous, 1)], cap, stream)

    def export_rounds_device(self, r0=None, r1=None, witnesses=None, famous=None, consensus=None, cap=None, stream=0):
        """export_rounds into DEVICE arrays (see export_ordered_device; witnesses and famous hold cap x n elements).  Returns
        (off, total), both in rounds."""
        ctl = [self._ctl(r0, np.int32, "r0"), self._ctl(r1, np.int32, "r1")]
        return self._export_device(self._L.sw_export_batch_rounds_device, ctl,
                                   [("witnesses", witnesses, self.n), ("famous", famous, self.n), ("consensus", consensus, 1)], cap, stream)

    def step_arrays(self, K=None):
        """step(K) with the results of the whole batch as ragged arrays: hashgraph b's new_c is rounds[rounds_off[b]:
        rounds_off[b + 1]], its newly ordered events event / round_received / time[tx_off[b]:tx_off[b + 1]].  `took` as
        step(collect=True) decides it; a hashgraph that sat out or froze has empty segments.  Two export calls, whatever B."""
        Ka = None
        if K is not None:
            Ka = np.ascontiguousarray(K, np.int64)
            if Ka.shape != (self.B,):
                raise ValueError("K must have one entry per hashgraph")
        before = self.summary_array()
        failed = C.c_int64(0)
        self._chk(self._L.sw_batch_step(self._h, _p(Ka), C.byref(failed)))
        self.n_failed = int(failed.value)
        now = self.summary_array()
        took = (now[:, 1] != before[:, 1]) & (now[:, 6] == 0)
        which = np.ascontiguousarray(took, np.uint8)
        r = self._export(self._L.sw_export_batch_new_rounds, [which], [("rounds", np.int32, 1)], cap=int(now[took, 4].sum()))
        n_out = np.where(took, now[:, 5], 0).astype(np.int64)
        first = np.where(took, now[:, 3] - now[:, 5], 0).astype(np.int64)
        o = self._export(self._L.sw_export_batch_ordered, [first, n_out],
                         [("event", np.int32, 1), ("round_received", np.int32, 1), ("time", np.float64, 1)], cap=int(n_out.sum()))
        return BatchStepArrays(took, r["off"], r["rounds"], o["off"], o["event"], o["round_received"], o["time"], self.n_failed)

    def export_stats(self):
        """(calls, kernel launches, entries written, device-to-host copies) of the export_* calls since the batch was made."""
        out = np.zeros(4, np.int64)
        self._chk(self._L.sw_export_batch_stats(self._h, _p(out)))
        return BatchExportStats(*[int(x) for x in out])

    # ---- gossip networks (sw_network_batch_*): hashgraph g * n + i is node i's view of network g; one wavefront runs a
    # network's turns, one launch.  No forks, no crypto, one turn at a time per network; cap_events bounds n + the turns.
    @property
    def n_networks(self):
        return self.B // self.n

    def _per_network(self, v, dtype, what):
        G = self.n_networks
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype), (G,)) if np.ndim(v) == 0 else v, dtype)
        if a.shape != (G,):
            raise ValueError("%s must be a scalar or have one entry per network" % what)
        return a

    def network_begin(self, seed, which=None, root_t=None, root_sig=None):
        """Begin the selected networks (which: a mask over the B // n networks, None = all): view i stores root i and divides
        it.  seed per network (a scalar broadcasts); root_t [G][n] and root_sig [G][n][64] replace the generated ones."""
        G = self.n_networks
        w = None if which is None else self._per_network(np.asarray(which) != 0, np.uint8, "which")
        rt = None if root_t is None else np.ascontiguousarray(root_t, np.float64)
        rs = None if root_sig is None else np.ascontiguousarray(root_sig, np.uint8)
        if rt is not None and rt.shape != (G, self.n):
            raise ValueError("root_t must be [networks][members]")
        if rs is not None and rs.shape != (G, self.n, 64):
            raise ValueError("root_sig must be [networks][members][64]")
        self._chk(self._L.sw_network_batch_begin(self._h, _p(w), _p(self._per_network(seed, np.uint64, "seed")), _p(rt), _p(rs)))

    def network_turns(self, schedules=None, *, off=None, puller=None, peer=None, t=None, sig=None):
        """Explicit turns: `schedules` is a list of one entry per network, each None or (puller, peer[, t[, sig]]); or the same
        as ragged arrays.  t and sig are the created events' (None: generated).  Returns the networks this call stopped."""
        G = self.n_networks
        if schedules is not None:
            if len(schedules) != G:
                raise ValueError("one entry per network (None for no turns)")
            parts = [(np.zeros(0, np.int32),) * 2 if s is None else tuple(s) for s in schedules]
            off = np.zeros(G + 1, np.int64)
            np.cumsum([len(p[0]) for p in parts], out=off[1:])
            puller = np.concatenate([np.asarray(p[0], np.int32) for p in parts])
            peer = np.concatenate([np.asarray(p[1], np.int32) for p in parts])
            has_t = [len(p) > 2 and p[2] is not None for p in parts if len(p[0])]
            has_s = [len(p) > 3 and p[3] is not None for p in parts if len(p[0])]
            if any(has_t) != all(has_t) or any(has_s) != all(has_s):
                raise ValueError("timestamps / signatures for every network of the call, or for none")
            if has_t and has_t[0]:
                t = np.concatenate([np.asarray(p[2], np.float64) for p in parts if len(p[0])])
            if has_s and has_s[0]:
                sig = np.concatenate([np.asarray(p[3], np.uint8).reshape(-1, 64) for p in parts if len(p[0])])
        off = np.ascontiguousarray(off, np.int64)
        if off.shape != (G + 1,):
            raise ValueError("off must have one entry per network and one more")
        total = int(off[-1])
        puller = np.ascontiguousarray(puller, np.int32)
        peer = np.ascontiguousarray(peer, np.int32)
        if not (puller.shape == peer.shape == (total,)):
            raise ValueError("puller / peer must have off[-1] entries")
        t = None if t is None else np.ascontiguousarray(t, np.float64)
        sig = None if sig is None else np.ascontiguousarray(sig, np.uint8).reshape(total, 64)
        if t is not None and t.shape != (total,):
            raise ValueError("t must have off[-1] entries")
        stopped = C.c_int64(0)
        self._chk(self._L.sw_network_batch_turns(self._h, _p(off), _p(puller), _p(peer), _p(t), _p(sig), C.byref(stopped)))
        return int(stopped.value)

    def network_run(self, T):
        """Every network runs its next T[g] turns of the schedule it draws itself (synth_schedule; an int broadcasts).
        Returns the networks this call stopped."""
        stopped = C.c_int64(0)
        self._chk(self._L.sw_network_batch_run(self._h, _p(self._per_network(T, np.int64, "T")), C.byref(stopped)))
        return int(stopped.value)

    def network_status(self, g=None):
        """Per network: BatchNetworkStatus(begun, turns, created, stage, code, view); stage 4 = broken."""
        out = np.zeros((self.n_networks, 6), np.int64)
        self._chk(self._L.sw_network_batch_get(self._h, _p(out)))
        if g is not None:
            return BatchNetworkStatus(*[int(x) for x in out[g]])
        return [BatchNetworkStatus(*[int(x) for x in row]) for row in out]

    def network_heads(self):
        """int32 [B]: the local index of each view's head (-1: not a view of a begun network)."""
        out = np.zeros(self.B, np.int32)
        self._chk(self._L.sw_network_batch_heads(self._h, _p(out)))
        return out

    def network_stats(self):
        """(calls that ran turns, turns run, events imported, kernel launches)."""
        out = np.zeros(4, np.int64)
        self._chk(self._L.sw_network_batch_stats(self._h, _p(out)))
        return BatchNetworkStats(*[int(x) for x in out])

    def event_numbers(self, b, first=0, K=None):
        """The network event numbers of view b's stored events [first, first + K)."""
        K = self._events(b) - first if K is None else K
        out = np.empty(K, np.int32)
        self._chk(self._L.sw_get_network_event_numbers(self._h, b, first, K, _p(out)))
        return out

    def export_event_numbers(self, first=None, count=None):
        """Network event numbers of the events [first[b], first[b] + count[b]) of every view: off, numbers."""
        ctl = [self._ctl(first, np.int64, "first"), self._ctl(count, np.int64, "count")]
        return self._export(self._L.sw_export_network_event_numbers, ctl, [("numbers", np.int32, 1)])

    def export_event_numbers_device(self, first=None, count=None, numbers=None, cap=None, stream=0):
        """export_event_numbers into a DEVICE array (see export_ordered_device).  Returns (off, total)."""
        ctl = [self._ctl(first, np.int64, "first"), self._ctl(count, np.int64, "count")]
        return self._export_device(self._L.sw_export_network_event_numbers_device, ctl, [("numbers", numbers, 1)], cap, stream)


LiveResources = collections.namedtuple("LiveResources", "device_bytes pinned_bytes events streams")


def live_resources():
    """What the library's contexts and calls hold in this process right now (sw_debug_live_resources): bytes of device
    memory, bytes of pinned host memory, events, streams.  Equal before a context is made and after it is closed."""
    v = [C.c_int64() for _ in range(4)]
    rc = _lib.load().sw_debug_live_resources(*[C.byref(x) for x in v])
    if rc != 0:
        raise SwirldHipError(rc, "sw_debug_live_resources")
    return LiveResources(*[int(x.value) for x in v])


def _pack_messages(msgs):
    off = np.zeros(len(msgs) + 1, np.int64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    return np.frombuffer(b"".join(msgs), np.uint8) if off[-1] else np.zeros(1, np.uint8), off


def verify_batch(msgs, sigs, pks, device=0):
    """Batch Ed25519 verification on the GPU (sw_crypto_verify_batch): one bool per (message,
    64-byte signature, 32-byte public key), equal to libsodium's crypto_sign_verify_detached
    accepting it (swirld.py:99-100)."""
    L = _lib.load()
    K = len(msgs)
    if not (len(sigs) == len(pks) == K):
        raise ValueError("msgs, sigs and pks must have equal length")
    if any(len(s) != 64 for s in sigs) or any(len(p) != 32 for p in pks):
        raise ValueError("signatures are 64 bytes, public keys 32 bytes")
    data, off = _pack_messages(msgs)
    sg = np.frombuffer(b"".join(sigs), np.uint8) if K else np.zeros(1, np.uint8)
    pk = np.frombuffer(b"".join(pks), np.uint8) if K else np.zeros(1, np.uint8)
    ok = np.zeros(max(K, 1), np.uint8)
    rc = L.sw_crypto_verify_batch(int(device), K, _p(data), _p(off), _p(sg), _p(pk), _p(ok))
    if rc != 0:
        raise SwirldHipError(rc, (L.sw_last_error(None) or b"").decode())
    return ok[:K].astype(bool)


def hash_batch(msgs, device=0):
    """Batch BLAKE2b-256 on the GPU (sw_crypto_hash_batch): the event ids of swirld.py:95, 103."""
    L = _lib.load()
    K = len(msgs)
    data, off = _pack_messages(msgs)
    out = np.zeros((max(K, 1), 32), np.uint8)
    rc = L.sw_crypto_hash_batch(int(device), K, _p(data), _p(off), _p(out))
    if rc != 0:
        raise SwirldHipError(rc, (L.sw_last_error(None) or b"").decode())
    return [bytes(out[i]) for i in range(K)]


def synth_schedule(n, seed, first_turn, T):
    """Turns [first_turn, first_turn + T) of the schedule a batch network of n nodes draws under `seed` (csrc/synth.cpp, no
    GPU): (puller, peer) as int32 arrays."""
    L = _lib.load()
    puller, peer = np.empty(max(int(T), 0), np.int32), np.empty(max(int(T), 0), np.int32)
    rc = L.sw_synth_schedule(int(n), int(seed), int(first_turn), int(T), _p(puller), _p(peer))
    if rc != 0:
        raise SwirldHipError(rc, "sw_synth_schedule: invalid arguments")
    return puller, peer


def synth_hashgraph(n, N, seed, mode=0, p0=0.0, p1=0.0, with_sig=True):
    """Host-side synthetic gossip hashgraph (csrc/synth.cpp): returns
    (creator, self_parent, other_parent, t, sig) as numpy arrays."""
    L = _lib.load()
    cr = np.empty(N, np.int32)
    sp = np.empty(N, np.int32)
    op = np.empty(N, np.int32)
    t = np.empty(N, np.float64)
    sig = np.empty((N, 64), np.uint8) if with_sig else None
    rc = L.sw_synth_hashgraph(int(n), int(N), int(seed), int(mode), float(p0), float(p1),
                              _p(cr), _p(sp), _p(op), _p(t), _p(sig))
    if rc != 0:
        raise SwirldHipError(rc, "sw_synth_hashgraph: invalid arguments")
    return cr, sp, op, t, sig
