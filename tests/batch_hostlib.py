"""Builder of the HOST build of csrc/batch.hip.h (tests/batch_host.cpp), and an oracle-like driver over it, for the CPU
suite (tests/test_batch_host.py).  The library is a build product next to the other host libraries of this directory."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "py-swirld_amd", "csrc")
SRC = os.path.join(HERE, "batch_host.cpp")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("batch.hip.h", "batch_layout.h", "exact.hip.h", "exact_history.hip.h")]
SO = os.path.join(HERE, "libswb_host.so")
SO_LANES = os.path.join(HERE, "libswb_host_lanes.so")


def build_batch_host(lanes=False):
    so, extra = (SO_LANES, ["-DSW_EXACT_HOST_LANES=16"]) if lanes else (SO, [])
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC"] + extra + [SRC, "-o", so])
    return so


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


STAGES = {0: None, 1: "divide", 2: "fame", 3: "order"}


class BatchHost:
    """B hashgraphs laid out by batch_layout.h in host memory; step(b, K) is swb::step as sw_batch_step launches it."""

    def __init__(self, B, n, stake=None, coin_period=6, cap_events=64, cap_rounds=0, lanes=False, npad=0):
        L = C.CDLL(build_batch_host(lanes))
        L.swb_host_create.restype = C.c_void_p
        L.swb_host_create.argtypes = [C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_int]
        L.swb_host_destroy.argtypes = [C.c_void_p]
        L.swb_host_npad.argtypes = [C.c_void_p]
        L.swb_host_cap_rounds.argtypes = [C.c_void_p]
        L.swb_host_cap_rounds.restype = C.c_longlong
        L.swb_host_append.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong] + [C.c_void_p] * 5
        L.swb_host_step.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong]
        L.swb_host_summary.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p]
        L.swb_host_get.argtypes = [C.c_void_p, C.c_longlong] + [C.c_void_p] * 10
        L.swb_host_new_rounds.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p]
        L.swb_host_log.argtypes = [C.c_void_p, C.c_longlong] + [C.c_void_p] * 3
        L.swb_host_visited_clear.argtypes = [C.c_void_p, C.c_longlong]
        self.L, self.B, self.n = L, B, n
        st = None
        if stake is not None:
            st = np.ascontiguousarray(stake, np.uint64)
            assert st.shape == (B, n)
        self.h = L.swb_host_create(B, n, _p(st), coin_period, cap_events, cap_rounds, npad)
        self.npad = L.swb_host_npad(self.h)
        self.N = [0] * B

    def __del__(self):
        if getattr(self, "h", None):
            self.L.swb_host_destroy(self.h)
            self.h = None

    def append(self, b, cr, sp, op, t=None, sig=None):
        cr = np.ascontiguousarray(cr, np.int32); sp = np.ascontiguousarray(sp, np.int32); op = np.ascontiguousarray(op, np.int32)
        t = None if t is None else np.ascontiguousarray(t, np.float64)
        sig = None if sig is None else np.ascontiguousarray(sig, np.uint8)
        rc = self.L.swb_host_append(self.h, b, len(cr), _p(cr), _p(sp), _p(op), _p(t), _p(sig))
        assert rc == 0, rc
        self.N[b] += len(cr)

    def summary(self, b):
        out = np.zeros(8, np.int64)
        self.L.swb_host_summary(self.h, b, _p(out))
        return dict(zip(("divided", "rounds", "ordered", "n_new", "n_out", "stage", "code", "event"), out.tolist()))

    def step(self, b, K, chunk=0):
        """(new_c, transactions of the step), or None where the hashgraph is frozen (by this step or before)."""
        before = self.summary(b)["ordered"]
        self.L.swb_host_step(self.h, b, K, chunk)
        s = self.summary(b)
        if s["stage"]:
            return None
        nc = np.zeros(max(s["n_new"], 1), np.int32)
        self.L.swb_host_new_rounds(self.h, b, _p(nc))
        assert s["ordered"] == before + s["n_out"]
        return nc[:s["n_new"]], self.log(b)[0][before:]

    def log(self, b):
        m = self.summary(b)["ordered"]
        ev, rr, ts = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.float64)
        self.L.swb_host_log(self.h, b, _p(ev), _p(rr), _p(ts))
        return ev[:m], rr[:m], ts[:m]

    def visited_clear(self, b):
        return bool(self.L.swb_host_visited_clear(self.h, b))

    def state(self, b):
        R, n, N = self.summary(b)["rounds"], self.n, self.N[b]
        ht = np.zeros(N, np.int32); rnd = np.zeros(N, np.int32); Lt = np.zeros((N, n), np.int32)
        wit = np.zeros((R, n), np.int32); wo = np.zeros((R, n), np.int32); wc = np.zeros(R, np.int32)
        cons = np.zeros(R, np.uint8); fam = np.zeros(N, np.int8); tbd = np.zeros(N, np.uint8); fs = np.zeros((R, n), np.int8)
        self.L.swb_host_get(self.h, b, _p(ht), _p(rnd), _p(Lt), _p(wit), _p(wo), _p(wc), _p(cons), _p(fam), _p(tbd), _p(fs))
        return dict(height=ht, round=rnd, can_see=Lt, wit=wit, worder=[wo[r, :wc[r]] for r in range(R)], cons=cons, fam=fam, tbd=tbd, fam_slot=fs)
