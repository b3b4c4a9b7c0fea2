"""CPU: what the exact (forked-hashgraph) path keeps when sw_set_exact_history is on — the vote store keyed by event
(py-swirld_amd/csrc/exact_history.hip.h, fed by swx::flush_votes of exact.hip.h) and the round received / consensus
timestamp of every produced item — compiled for the HOST (tests/exact_history_host.cpp: one "lane", and 16 cooperative
fibers that hand over at every sync) and compared with the unmodified reference's recorded `votes` dict, with the
fixtures of tests/golden/consensus_forked and with the oracle.  The GPU run is tests/test_gpu_exact_history.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN_DIR, load_golden
from oracle.oracle import Oracle, OracleError
from test_oracle_vs_reference_random import load_case

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "py-swirld_amd", "csrc")
SRC = os.path.join(HERE, "exact_history_host.cpp")
DEPS = [SRC, os.path.join(HERE, "exact_host.cpp"), os.path.join(CSRC, "exact.hip.h"), os.path.join(CSRC, "exact_history.hip.h")]
FORKED = ["n8_s11_forks", "n8_s12_forks_chunk9", "n5_s13_forks_chunk1", "n12_s14_forks_stake_chunk40"]


_OUT = HERE if os.access(HERE, os.W_OK) else tempfile.mkdtemp(prefix="swxh_host_")


def build_lib(lanes):
    so = os.path.join(_OUT, "libswxh_host_lanes.so" if lanes else "libswxh_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in DEPS):
        extra = ["-DSW_EXACT_HOST_LANES=16"] if lanes else []
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC"] + extra + [SRC, "-o", so])
    return so


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class HistoryHost:
    def __init__(self, n, stake=None, lanes=False, cap0=0, ceiling=0):
        L = C.CDLL(build_lib(lanes))
        L.xhh_create.restype = C.c_void_p
        L.xhh_create.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong]
        L.xhh_destroy.argtypes = [C.c_void_p]
        L.xhh_append.argtypes = [C.c_void_p, C.c_longlong] + [C.c_void_p] * 5
        L.xhh_divide.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong]
        L.xhh_fame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.xhh_order.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.xhh_store_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.xhh_store_get.argtypes = [C.c_void_p] * 4
        L.xhh_lookup.argtypes = [C.c_void_p, C.c_longlong] + [C.c_void_p] * 3
        L.xhh_consensus_get.argtypes = [C.c_void_p] * 3
        self.L, self.n, self.N = L, n, 0
        st = np.ones(n, np.uint32) if stake is None else np.ascontiguousarray(stake, np.uint32)
        self.h = L.xhh_create(n, _p(st), 6, cap0, ceiling)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.xhh_destroy(self.h)
            self.h = None

    def append_events(self, cr, sp, op, t, sig):
        a = [np.ascontiguousarray(cr, np.int32), np.ascontiguousarray(sp, np.int32), np.ascontiguousarray(op, np.int32),
             np.ascontiguousarray(t, np.float64), np.ascontiguousarray(sig, np.uint8)]
        assert self.L.xhh_append(self.h, len(a[0]), *[_p(x) for x in a]) == 0
        self.N += len(a[0])

    def divide_rounds(self, first, K):
        assert self.L.xhh_divide(self.h, first, K) == 0

    def decide_fame(self):
        out = np.zeros(self.N + 2, np.int32)
        k = C.c_int(0)
        assert self.L.xhh_fame(self.h, _p(out), C.byref(k)) == 0
        return out[:k.value].copy()

    def find_order(self, rounds):
        rounds = np.ascontiguousarray(list(rounds), np.int32)
        out = np.zeros(self.N + 1, np.int32)
        k = C.c_longlong(0)
        rc = self.L.xhh_order(self.h, _p(rounds), len(rounds), _p(out), C.byref(k))
        if rc != 0:
            raise IndexError(rc)
        return out[:k.value].copy()

    def stats(self):
        out = np.zeros(4, np.int64)
        self.L.xhh_store_stats(self.h, _p(out))
        return dict(count=int(out[0]), overflow=int(out[1]), cap=int(out[2]), grows=int(out[3]))

    def entries(self):
        k = self.stats()["count"]
        y, x, v = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.int8)
        self.L.xhh_store_get(self.h, _p(y), _p(x), _p(v))
        return y, x, v

    def votes_dict(self):
        y, x, v = self.entries()
        d = {(int(a), int(b)): int(c) for a, b, c in zip(y, x, v)}
        assert len(d) == len(y), "a key twice in the log"
        return d

    def lookup(self, y, x):
        y, x = np.ascontiguousarray(y, np.int32), np.ascontiguousarray(x, np.int32)
        out = np.zeros(len(y), np.int8)
        self.L.xhh_lookup(self.h, len(y), _p(y), _p(x), _p(out))
        return out

    def consensus(self):
        rr, cts = np.zeros(self.N, np.int32), np.zeros(self.N, np.uint64)
        self.L.xhh_consensus_get(self.h, _p(rr), _p(cts))
        return rr, cts


def crossing_stream():
    """(n, chunk, stream) of the case tests/golden/consensus_forked/crossing_n8_s12_chunk50.npz was recorded from: the first
    fork (event 563) arrives after fast-path calls have ordered 261 events and cast votes."""
    from synth_util import synth
    from test_exact_host import add_forks
    n = 8
    return n, 50, add_forks(synth(n, 900, 12), n, 12, 2, start=450)


def load_forked_consensus(name):
    with np.load(os.path.join(GOLDEN_DIR, "consensus_forked", name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def run_golden(g, t, lanes, **kw):
    x = HistoryHost(g["n"], g["stake"], lanes=lanes, **kw)
    tx = []
    for a, b in g["batches"]:
        x.append_events(g["creator"][a:b], g["self_parent"][a:b], g["other_parent"][a:b], t[a:b], g["sig"][a:b])
        x.divide_rounds(a, b - a)
        tx.extend(x.find_order(x.decide_fame()).tolist())
    return x, np.array(tx, np.int32)


def _golden_cases():  # (a fiber switch per lane and sync: the many-call schedules stay with the 1-lane build)
    return [pytest.param(name, lanes, id="%s-%s" % (name, "16lanes" if lanes else "1lane")) for name in FORKED for lanes in (False, True)
            if not (lanes and len(load_golden(name)["batches"]) > 60)]


@pytest.mark.parametrize("name,lanes", _golden_cases())
def test_store_equals_the_references_votes_dict(name, lanes):
    g, f = load_golden(name), load_forked_consensus(name)
    x, tx = run_golden(g, g["t"], lanes)
    assert np.array_equal(tx, g["transactions"])
    ref = {(int(y), int(xx)): int(v) for y, xx, v in g["votes"]}
    assert len(ref) == len(g["votes"])
    got = x.votes_dict()
    assert got.keys() == ref.keys()
    assert got == ref
    assert x.stats()["overflow"] == 0
    if name == "n5_s13_forks_chunk1":   # a voter a later fork sibling replaced in the witness table
        in_table = set(int(w) for w in g["witnesses"].ravel() if w >= 0)
        assert any(y not in in_table for y, _ in got), "the case must hold a replaced-sibling voter"
    # the look-up answers every entry, and -1 for pairs without one
    y, xx, v = x.entries()
    assert np.array_equal(x.lookup(y, xx), v)
    rng = np.random.default_rng(5)
    ay, ax = rng.integers(-2, x.N + 2, 400), rng.integers(-2, x.N + 2, 400)
    exp = np.array([ref.get((int(a), int(b)), -1) for a, b in zip(ay, ax)], np.int8)
    assert np.array_equal(x.lookup(ay, ax), exp)
    rr, cts = x.consensus()
    assert np.array_equal(rr, f["asis_round_received"])
    assert same_bits(f["asis_consensus_time"], cts)


@pytest.mark.parametrize("name,lanes", _golden_cases())
def test_wallclock_times_bit_for_bit(name, lanes):
    g, f = load_golden(name), load_forked_consensus(name)
    x, tx = run_golden(g, f["wallclock_t"], lanes)
    assert np.array_equal(tx, f["wallclock_transactions"])
    rr, cts = x.consensus()
    assert np.array_equal(rr, f["wallclock_round_received"])
    assert same_bits(f["wallclock_consensus_time"], cts)
    assert (rr >= 0).sum() == len(tx) > 0


@pytest.mark.parametrize("lanes", [False, True], ids=["1lane", "16lanes"])
def test_tiny_store_grows_and_a_low_ceiling_overflows_without_changing_consensus(lanes):
    g = load_golden("n8_s12_forks_chunk9")
    base, tx0 = run_golden(g, g["t"], lanes)
    tiny, tx1 = run_golden(g, g["t"], lanes, cap0=4)
    assert np.array_equal(tx0, tx1)
    assert tiny.stats()["grows"] >= 4 and tiny.stats()["overflow"] == 0
    for a, b in zip(base.entries(), tiny.entries()):   # same entries in the same order, whatever the capacity
        assert np.array_equal(a, b)
    low, tx2 = run_golden(g, g["t"], lanes, cap0=4, ceiling=50)
    assert np.array_equal(tx0, tx2)
    st = low.stats()
    assert st["overflow"] == 1 and st["count"] <= 50 == st["cap"]
    for a, b in zip(base.consensus(), low.consensus()):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("seed", range(16))
def test_random_forked_streams_against_the_oracle(seed):
    n, (cr, sp, op, t, sig), stake, chunk, calls, index_error_call, ex = load_case("forked", seed)
    N = len(cr)
    orc = Oracle(n, None if stake is None else stake.astype(np.uint64))
    x = HistoryHost(n, None if stake is None else stake.astype(np.uint32), lanes=bool(ex["lanes"]))
    for i, a in enumerate(range(0, N, chunk)):
        b = min(N, a + chunk)
        for d in (orc, x):
            d.append_events(cr[a:b], sp[a:b], op[a:b], t[a:b], sig[a:b])
            d.divide_rounds(a, b - a)
        nc = orc.decide_fame()
        assert list(nc) == list(x.decide_fame())
        if i == index_error_call:
            with pytest.raises(OracleError):
                orc.find_order(nc)
            rr0 = x.consensus()
            with pytest.raises(IndexError):
                x.find_order(nc)
            for p, q in zip(rr0, x.consensus()):   # a call that fails records nothing
                assert np.array_equal(p, q)
            break
        assert list(orc.find_order(nc)) == list(x.find_order(nc))
    y, xx, v = x.entries()
    assert len(y) == orc.num_votes
    if index_error_call < 0:
        assert len(y) == int(ex["n_votes"])
    assert len(set(zip(y.tolist(), xx.tolist()))) == len(y)
    assert [orc.vote(a, b) for a, b in zip(y, xx)] == v.tolist()
    rr, _ = x.consensus()
    ordered = np.zeros(N, bool)
    ordered[orc.transactions] = True
    assert np.array_equal(rr >= 0, ordered)
    name = "random_forked_%02d" % seed
    if os.path.exists(os.path.join(GOLDEN_DIR, "consensus_forked", name + ".npz")):
        f = load_forked_consensus(name)
        rr, cts = x.consensus()
        assert np.array_equal(rr, f["asis_round_received"])
        assert same_bits(f["asis_consensus_time"], cts)


@pytest.mark.parametrize("variant", ["asis", "wallclock"])
@pytest.mark.parametrize("lanes", [False, True], ids=["1lane", "16lanes"])
def test_crossing_stream_against_the_reference_fixture(lanes, variant):
    n, chunk, (cr, sp, op, t, sig) = crossing_stream()
    f = load_forked_consensus("crossing_n8_s12_chunk50")
    if variant == "wallclock":
        t = f["wallclock_t"]
    g = dict(n=n, stake=None, creator=cr, self_parent=sp, other_parent=op, sig=sig,
             batches=[(a, min(len(cr), a + chunk)) for a in range(0, len(cr), chunk)])
    x, tx = run_golden(g, t, lanes)
    assert np.array_equal(tx, f[variant + "_transactions"]) and len(tx) > 261
    rr, cts = x.consensus()
    assert np.array_equal(rr, f[variant + "_round_received"])
    assert same_bits(f[variant + "_consensus_time"], cts)
