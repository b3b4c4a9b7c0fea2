"""GPU (-m gpu): sw_append_events_device — the same events from DEVICE memory (validation, chain positions, per-member
tables, chain pool and heights on the device, csrc/ingest.hip.h).  Every view must equal a context fed through
sw_append_events, and the oracle; rejections are atomic and name the lowest offending event; everything outside the
bulk fork-free fast path falls back to the host path, correctly and counted (sw_get_ingest_stats) — a test that fell
back silently would prove nothing.

No torch here (a third file importing it late would bring a second HIP runtime into the process): device buffers come
from the runtime the library itself is linked against, through ctypes."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H2D = 1


class Hip:
    """hipMalloc / hipMemcpy / streams of the HIP runtime behind libswirld_hip.so."""

    def __init__(self, pkg):
        L = C.CDLL(pkg.LIB_PATH)
        self.L = L
        L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.hipFree.argtypes = [C.c_void_p]
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        L.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        L.hipStreamDestroy.argtypes = [C.c_void_p]
        L.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.bufs = []
        self.keep = []

    def up(self, a, dtype, stream=None):
        """Device copy of a host array (None stays None); with a stream: enqueued there, not waited for."""
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype)
        p = C.c_void_p()
        assert self.L.hipMalloc(C.byref(p), max(a.nbytes, 4)) == 0
        self.bufs.append(p)
        self.keep.append(a)
        if stream is None:
            assert self.L.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, H2D) == 0
        else:
            assert self.L.hipMemcpyAsync(p, a.ctypes.data_as(C.c_void_p), a.nbytes, H2D, stream) == 0
        return p.value

    def free(self):
        for p in self.bufs:
            self.L.hipFree(p)
        self.bufs, self.keep = [], []


@pytest.fixture
def hip(pkg):
    h = Hip(pkg)
    yield h
    h.free()


def dev_append(h, hip, cr, sp, op, t=None, sig=None, stream=None):
    K = len(cr)
    args = [hip.up(cr, np.int32, stream), hip.up(sp, np.int32, stream), hip.up(op, np.int32, stream),
            hip.up(t, np.float64, stream), hip.up(sig, np.uint8, stream)]
    try:
        h.append_events_device(*args, stream=stream or 0, count=K)
    finally:
        hip.free()


def finish(h, N):
    h.divide_rounds(0, N)
    nc = list(h.decide_fame())
    return nc, list(h.find_order(nc))


def same_views(a, b, N, n, what):
    """Every view of context `a` equals context `b`'s (both divided and decided already)."""
    assert np.array_equal(a.heights(), b.heights()), what + ": heights"
    for m in sorted({0, 1, n // 2, n - 1}):
        k = int(np.count_nonzero(a._cr == m))
        assert np.array_equal(a.chain_events(m, 0, k), b.chain_events(m, 0, k)), what + ": chain of member %d" % m
    assert np.array_equal(a.rounds(), b.rounds()), what + ": rounds"
    step = max(1, (32 << 20) // (4 * a.row_stride))
    for x in range(0, N, step):
        k = min(step, N - x)
        assert np.array_equal(a.can_see(x, k), b.can_see(x, k)), what + ": can_see rows %d.." % x
    assert np.array_equal(a.witnesses(), b.witnesses()), what + ": witnesses"
    assert np.array_equal(a.famous(), b.famous()), what + ": famous"
    assert np.array_equal(a.consensus(), b.consensus()), what + ": consensus"


def _oracle_run(n, stream):
    from oracle.oracle import Oracle
    o = Oracle(n)
    o.append_events(*stream)
    N = len(stream[0])
    o.divide_rounds(0, N)
    nco = list(o.decide_fame())
    return o, nco, list(o.find_order(nco))


CASES = [(32, 40_000, 0, 0.0, 0.0, True), (300, 200_000, 0, 0.0, 0.0, False), (1024, 150_000, 2, 0.40, 0.02, False),
         (256, 300_000, 0, 0.0, 0.0, True)]
_EX = ThreadPoolExecutor(max_workers=2)
_ORACLES = {}


def _stream(pkg, n, N, mode, p0, p1):
    return pkg.synth_hashgraph(n, N, 500 + n, mode, p0, p1)


@pytest.fixture(scope="module", autouse=True)
def oracles(pkg):
    """The oracle runs of the two parity cases that have one, started in threads when the first test of the file begins
    (the oracle's C calls release the GIL)."""
    from oracle import oracle as _o
    _o.lib()
    for n, N, mode, p0, p1, has in CASES:
        if has and n not in _ORACLES:
            _ORACLES[n] = _EX.submit(_oracle_run, n, _stream(pkg, n, N, mode, p0, p1))
    return _ORACLES


def _defects(cr, sp, op, N, n):
    k = 31_007
    other = int(np.nonzero(cr[:k] != cr[k])[0][-1])
    out = {}
    for name in ("creator_n", "creator_neg", "one_parent", "own_index", "beyond_batch", "self_by_other", "other_by_same"):
        c2, s2, o2 = cr.copy(), sp.copy(), op.copy()
        if name == "creator_n":
            c2[k] = n
        elif name == "creator_neg":
            c2[k] = -1
        elif name == "one_parent":
            o2[k] = -1
        elif name == "own_index":
            s2[k] = k
        elif name == "beyond_batch":
            o2[k] = N + 12345
        elif name == "self_by_other":
            s2[k] = other
        elif name == "other_by_same":
            o2[k] = sp[k]
        out[name] = (c2, s2, o2)
    return k, out


# what sw_last_error says for each defect (the host path's wording)
NAMED = {"creator_n": "creator out of range", "creator_neg": "creator out of range", "one_parent": "0 or 2 parents",
         "own_index": "parent index not earlier", "beyond_batch": "parent index not earlier",
         "self_by_other": "self-parent is by another member", "other_by_same": "other-parent is by the same member"}


def test_rejections_are_atomic_and_named(pkg, hip):
    n, N = 32, 40_000
    cr, sp, op, t, sig = stream = pkg.synth_hashgraph(n, N, 201)
    h = pkg.Hashgraph(n)
    k, defects = _defects(cr, sp, op, N, n)
    for name, (c2, s2, o2) in defects.items():
        with pytest.raises(pkg.SwirldHipError) as ei:
            dev_append(h, hip, c2, s2, o2, t, sig)
        assert ei.value.code == -22 and ("event %d:" % k) in str(ei.value), (name, str(ei.value))
        assert NAMED[name] in str(ei.value), (name, str(ei.value))      # ... and WHICH check found it
        assert h.num_events == 0, name
    # two defects: the lower event is reported, whichever check finds it
    for lo_name, hi_name in (("other_by_same", "creator_n"), ("own_index", "self_by_other"), ("self_by_other", "one_parent")):
        c2, s2, o2 = (x.copy() for x in defects[hi_name])
        # the low defect 4 000 events in front of it
        lo_k = k - 4_000
        if lo_name == "other_by_same":
            o2[lo_k] = sp[lo_k]
        elif lo_name == "own_index":
            s2[lo_k] = lo_k
        elif lo_name == "self_by_other":
            s2[lo_k] = op[lo_k]
        with pytest.raises(pkg.SwirldHipError) as ei:
            dev_append(h, hip, c2, s2, o2, t, sig)
        assert ei.value.code == -22 and ("event %d:" % lo_k) in str(ei.value), (lo_name, hi_name, str(ei.value))
        assert NAMED[lo_name] in str(ei.value), (lo_name, hi_name, str(ei.value))
        assert h.num_events == 0
    st = h.ingest_stats()
    assert st["device_batches"] == 0 and st["fallback_batches"] == 0
    # the context is untouched: it ingests the valid stream and equals the oracle
    dev_append(h, hip, *stream)
    o, nco, txo = _oracle_run(n, stream)
    assert finish(h, N) == (nco, txo)
    assert np.array_equal(h.heights(), o.height) and np.array_equal(h.rounds(), o.round)
    assert np.array_equal(h.can_see(), o.can_see) and np.array_equal(h.witnesses(), o.witnesses())
    assert h.ingest_stats()["device_batches"] == 1 and h.ingest_stats()["host_height_events"] == 0
    h.close()


@pytest.mark.parametrize("kind", ["older_self_parent", "second_root"])
def test_forks_fall_back_to_the_host_paths_decision(pkg, hip, kind):
    n, N = 32, 40_000
    cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, 201)
    f_sp, f_op = sp.copy(), op.copy()
    j = int(np.nonzero(cr[n:] == cr[n + 5])[0][3]) + n
    if kind == "older_self_parent":
        f_sp[j] = sp[sp[j]]
    else:
        f_sp[j] = f_op[j] = -1
    h = pkg.Hashgraph(n)
    h.set_forks(False)
    with pytest.raises(pkg.SwirldHipError) as ei:
        dev_append(h, hip, cr, f_sp, f_op, t, sig)
    assert ei.value.code == -95 and h.num_events == 0
    assert h.ingest_stats()["fallback_batches"] == 1 and h.ingest_stats()["device_batches"] == 0
    h.set_forks(True)
    dev_append(h, hip, cr, f_sp, f_op, t, sig)
    assert h.exact and h.num_events == N and h.ingest_stats()["fallback_batches"] == 2
    ref = pkg.Hashgraph(n)
    ref.append_events(cr, f_sp, f_op, t, sig)
    assert ref.exact
    assert finish(h, N) == finish(ref, N)
    assert np.array_equal(h.heights(), ref.heights()) and np.array_equal(h.rounds(), ref.rounds())
    assert np.array_equal(h.can_see(), ref.can_see()) and np.array_equal(h.witnesses(), ref.witnesses())
    assert np.array_equal(h.famous(), ref.famous()) and np.array_equal(h.consensus(), ref.consensus())
    h.close()
    ref.close()


def test_fallbacks_are_correct_and_counted(pkg, hip):
    n, N = 32, 40_000
    cr, sp, op, t, sig = stream = pkg.synth_hashgraph(n, N, 202)
    o, nco, txo = _oracle_run(n, stream)
    sl = lambda x, y: [z[x:y] for z in stream]
    # a sub-bulk batch behind a bulk one
    h = pkg.Hashgraph(n)
    dev_append(h, hip, *sl(0, 39_000))
    dev_append(h, hip, *sl(39_000, 39_100))
    assert h.ingest_stats() == {"device_batches": 1, "device_events": 39_000, "fallback_batches": 1, "host_height_events": 0}
    dev_append(h, hip, *sl(39_100, N))      # 900 events: small again
    assert h.ingest_stats()["fallback_batches"] == 2 and h.num_events == N
    assert finish(h, N) == (nco, txo)
    assert np.array_equal(h.heights(), o.height) and np.array_equal(h.can_see(), o.can_see)
    assert h.ingest_stats()["host_height_events"] == 0   # (small appends keep the mirror; device heights were downloaded)
    h.close()
    # a windowed context
    w = pkg.Hashgraph(n)
    w.set_window(True, chunk_mb=2)
    dev_append(w, hip, *stream)
    assert w.ingest_stats()["fallback_batches"] == 1 and w.ingest_stats()["device_batches"] == 0 and w.num_events == N
    assert finish(w, N) == (nco, txo)
    assert np.array_equal(w.rounds(), o.round)
    w.close()
    # a context already on the exact path
    x = pkg.Hashgraph(n)
    f_sp = sp.copy()
    j = int(np.nonzero(cr[n:] == cr[n + 5])[0][3]) + n
    f_sp[j] = sp[sp[j]]
    x.append_events(cr[:20_000], f_sp[:20_000], op[:20_000], t[:20_000], sig[:20_000])
    assert x.exact
    dev_append(x, hip, cr[20_000:], f_sp[20_000:], op[20_000:], t[20_000:], sig[20_000:])
    assert x.ingest_stats()["fallback_batches"] == 1 and x.num_events == N
    ref = pkg.Hashgraph(n)
    ref.append_events(cr, f_sp, op, t, sig)
    assert finish(x, N) == finish(ref, N) and np.array_equal(x.rounds(), ref.rounds())
    x.close()
    ref.close()


def test_pointer_checks_and_null_payload(pkg, hip):
    n, N = 32, 40_000
    cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, 203)
    h = pkg.Hashgraph(n)
    d_sp, d_op = hip.up(sp, np.int32), hip.up(op, np.int32)
    with pytest.raises(pkg.SwirldHipError) as ei:     # a numpy array's address
        h.append_events_device(cr.ctypes.data, d_sp, d_op, count=N)
    assert ei.value.code == -22 and h.num_events == 0
    d_cr = hip.up(cr, np.int32)
    with pytest.raises(pkg.SwirldHipError) as ei:     # ... for the payload too
        h.append_events_device(d_cr, d_sp, d_op, t=t.ctypes.data, count=N)
    assert ei.value.code == -22 and h.num_events == 0
    with pytest.raises(ValueError):                   # no length, no count
        h.append_events_device(d_cr, d_sp, d_op)

    class Tensor:                                     # the data_ptr() route of the front end
        def __init__(self, p, k):
            self.p, self.k = p, k

        def data_ptr(self):
            return self.p

        def __len__(self):
            return self.k

    h.append_events_device(Tensor(d_cr, N), Tensor(d_sp, N), Tensor(d_op, N))   # t / sig NULL: zeros, as the host path with None
    # ... a later call cannot trip over the pointer query's error state
    assert h.ingest_stats()["device_batches"] == 1
    ref = pkg.Hashgraph(n)
    ref.append_events(cr, sp, op)
    assert finish(h, N) == finish(ref, N)
    h._cr = cr
    same_views(h, ref, N, n, "NULL payload")
    h.close()
    ref.close()


def test_a_user_stream_orders_the_uploads(pkg, hip):
    n, N = 64, 120_000
    cr, sp, op, t, sig = stream = pkg.synth_hashgraph(n, N, 204)
    s = C.c_void_p()
    assert hip.L.hipStreamCreate(C.byref(s)) == 0
    h = pkg.Hashgraph(n)
    dev_append(h, hip, *stream, stream=s.value)       # hipMemcpyAsync on `s`, then the call, nothing waited for in between
    assert h.ingest_stats()["device_batches"] == 1
    ref = pkg.Hashgraph(n)
    ref.append_events(*stream)
    assert finish(h, N) == finish(ref, N)
    h._cr = cr
    same_views(h, ref, N, n, "user stream")
    assert hip.L.hipStreamSynchronize(s) == 0 and hip.L.hipStreamDestroy(s) == 0
    h.close()
    ref.close()


def test_reset_and_reingest_alternating(pkg, hip):
    n = 48
    h = pkg.Hashgraph(n)
    for i, (seed, N) in enumerate(((301, 30_000), (302, 12_000), (303, 30_000), (304, 20_000))):
        stream = pkg.synth_hashgraph(n, N, seed)
        o, nco, txo = _oracle_run(n, stream)
        h.reset()
        assert h.num_events == 0
        if i % 2 == 0:
            dev_append(h, hip, *stream)
        else:
            h.append_events(*stream)
        assert finish(h, N) == (nco, txo)
        assert np.array_equal(h.rounds(), o.round) and np.array_equal(h.heights(), o.height)
        assert np.array_equal(h.can_see(N - 2000, 2000), o.can_see[N - 2000:])
    st = h.ingest_stats()
    assert st["device_batches"] == 2 and st["fallback_batches"] == 0 and st["host_height_events"] == 12_000 + 20_000
    h.close()


# (last in the file: the oracle of the 256-member case takes tens of seconds of one core, and has been running since the first test)
@pytest.mark.parametrize("n,N,mode,p0,p1,has_oracle", CASES)
def test_parity_with_the_host_path_and_the_oracle(pkg, hip, oracles, n, N, mode, p0, p1, has_oracle):
    cr, sp, op, t, sig = stream = _stream(pkg, n, N, mode, p0, p1)
    host = pkg.Hashgraph(n)
    host.append_events(*stream)
    one = pkg.Hashgraph(n)
    dev_append(one, hip, *stream)
    assert one.num_events == N
    assert one.ingest_stats() == {"device_batches": 1, "device_events": N, "fallback_batches": 0, "host_height_events": 0}
    # three bulk device batches, a bulk host append and a run of small host appends between them
    a = N // 4
    b, c = a + 9000, a + 18_000     # (every device batch is bulk-sized: 8192 events or more)
    d = c + 45
    mix = pkg.Hashgraph(n)
    sl = lambda x, y: [z[x:y] for z in stream]
    dev_append(mix, hip, *sl(0, a))
    mix.append_events(*sl(a, b))
    dev_append(mix, hip, *sl(b, c))
    for x in range(c, d, 7):
        mix.append_events(*sl(x, min(d, x + 7)))
    dev_append(mix, hip, *sl(d, N))
    st = mix.ingest_stats()
    assert (st["device_batches"], st["device_events"], st["fallback_batches"]) == (3, a + (c - b) + (N - d), 0)
    res = {}
    for name, h in (("host", host), ("one", one), ("mix", mix)):
        h._cr = cr
        res[name] = finish(h, N)
    assert res["one"] == res["host"] and res["mix"] == res["host"]
    same_views(one, host, N, n, "single device batch")
    same_views(mix, host, N, n, "mixed batches")
    assert one.ingest_stats()["host_height_events"] == 0
    # the sequential host loop ran for the events of the bulk HOST append only, never for a device-appended one
    assert mix.ingest_stats()["host_height_events"] == b - a
    if has_oracle:
        o, nco, txo = oracles[n].result(timeout=600)
        assert res["one"] == (nco, txo)
        assert np.array_equal(one.heights(), o.height) and np.array_equal(one.rounds(), o.round)
        assert np.array_equal(one.witnesses(), o.witnesses())
        step = 50_000
        for x in range(0, N, step):
            assert np.array_equal(one.can_see(x, min(step, N - x)), o.can_see[x:x + step])
    for h in (host, one, mix):
        h.close()
