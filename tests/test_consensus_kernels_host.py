"""CPU: the kernels of csrc/consensus.hip.h run thread by thread on the host (tests/consensus_emul.cpp, a stand-alone
program built with AddressSanitizer and UBSan) against numpy: records of one slot and of a slot count that is no multiple
of the workgroup, two calls' records one behind the other, event ranges of 0 and 1 events, ranges that start inside the
stream and hold unordered events in their middle, member counts that are no multiple of 64, every output array absent in
turn, grids smaller than the range.  The host side of the library (checks, streams, growth of the tables) is NOT covered
here: tests/test_gpu_consensus.py does that on the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

THREADS, LANES = 256, 4
QNAN = np.uint64(0x7ff8000000000000)
EV, ID, CR, RR, TM = 1, 2, 4, 8, 16


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("consensus_emul") / "consensus_emul")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "consensus_emul.cpp"), "-o", exe])
    return exe


class Scene:
    """N events of n members in random creation order; two find_order calls' worth of ordered prefixes: the first call
    orders chain positions below pos1[m], the second those below pos2[m] >= pos1[m]."""

    def __init__(self, n, N, seed, frac1=0.4, frac2=0.8, only=None):
        rng = np.random.default_rng(seed)
        self.n, self.N = n, N
        self.cr = rng.integers(0, n, N).astype(np.int32)
        self.seq = np.zeros(N, np.int32)
        cnt = np.zeros(n, np.int64)
        for e in range(N):
            self.seq[e] = cnt[self.cr[e]]
            cnt[self.cr[e]] += 1
        pos1 = np.floor(cnt * frac1 * rng.uniform(0.5, 1.0, n)).astype(np.int32)
        pos2 = np.maximum(pos1, np.floor(cnt * frac2 * rng.uniform(0.5, 1.0, n))).astype(np.int32)
        if only is not None:          # exactly `only` events in the first call, nothing in the second
            pos1[:] = 0
            pos1[self.cr[0]] = only
            pos2 = pos1.copy()
        self.ordpos = pos2
        self.ids = rng.integers(0, 256, (N, 32), dtype=np.uint8)
        self.calls = []
        self.rr = np.full(N, -1, np.int32)
        self.cts = np.full(N, QNAN, np.uint64)
        tx = []
        base_round = 3
        for lo, hi in ((np.zeros(n, np.int32), pos1), (pos1, pos2)):
            ev = np.flatnonzero((self.seq >= lo[self.cr]) & (self.seq < hi[self.cr])).astype(np.int32)
            ev = ev[rng.permutation(len(ev))]                 # the round-major list is in no index order
            nr = 1 + int(rng.integers(0, 4))
            rounds = (base_round + np.sort(rng.choice(12, nr, replace=False))).astype(np.int32)
            base_round += 20
            ri = np.sort(rng.integers(0, nr, len(ev))).astype(np.int32)
            ts = (1.7e9 + rng.uniform(0, 1e4, len(ev))).view(np.uint64)
            self.calls.append((ev, ri, rounds, ts))
            self.rr[ev] = rounds[ri]
            self.cts[ev] = ts
            tx.append(ev[rng.permutation(len(ev))])
        self.tx = np.concatenate(tx).astype(np.int32)
        self.split = len(tx[0])           # positions below belong to the first call's records


def run(emul, tmp_path, s, ev_first, ev_K, g_first, g_K, ev_flags=3, g_flags=31, ev_grid=2, g_grid=3):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    (e1, ri1, r1, t1), (e2, ri2, r2, t2) = s.calls
    with open(src, "wb") as f:
        f.write(np.array([s.N, s.n, len(e1), len(r1), len(e2), len(r2), len(s.tx), ev_first, ev_K, ev_flags, ev_grid,
                          g_first, g_K, g_flags, g_grid], np.int32).tobytes())
        for ev, ri, rounds, ts in s.calls:
            f.write(ev.tobytes() + ri.tobytes() + rounds.tobytes() + ts.tobytes())
        for a in (s.seq, s.cr, s.ordpos, s.tx):
            f.write(np.ascontiguousarray(a, np.int32).tobytes())
        f.write(s.ids.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([emul, src, dst], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(dst, "rb").read()
    pos = 0
    out = {}

    def take(name, count, dtype):
        nonlocal pos
        a = np.frombuffer(raw, dtype, count, pos)
        pos += a.nbytes
        out[name] = a
    take("tab_rr", s.N, np.int32)
    take("tab_cts", s.N, np.uint64)
    if ev_flags & 1:
        take("ev_rr", ev_K, np.int32)
    if ev_flags & 2:
        take("ev_cts", ev_K, np.uint64)
    for bit, name, width, dtype in ((EV, "event", 1, np.int32), (ID, "ids", 32, np.uint8), (CR, "creator", 1, np.int32),
                                    (RR, "rr", 1, np.int32), (TM, "time", 1, np.uint64)):
        if g_flags & bit:
            take(name, g_K * width, dtype)
    assert pos == len(raw)
    return out


def check(emul, tmp_path, s, ev_first, ev_K, g_first, g_K, **kw):
    got = run(emul, tmp_path, s, ev_first, ev_K, g_first, g_K, **kw)
    ordered = s.seq < s.ordpos[s.cr]
    assert np.array_equal(ordered, s.rr >= 0)
    # the tables: recorded entries hold the call's values, every other entry was never written
    assert np.array_equal(got["tab_rr"][ordered], s.rr[ordered]) and np.array_equal(got["tab_cts"][ordered], s.cts[ordered])
    assert np.all(got["tab_rr"][~ordered] == np.int32(-1515870811)) and np.all(got["tab_cts"][~ordered] == np.uint64(0xA5A5A5A5A5A5A5A5))
    sl = slice(ev_first, ev_first + ev_K)
    if "ev_rr" in got:
        assert np.array_equal(got["ev_rr"], s.rr[sl])                  # -1 where not ordered
    if "ev_cts" in got:
        assert np.array_equal(got["ev_cts"], s.cts[sl])                # the quiet NaN's bits where not ordered
    ev = s.tx[g_first:g_first + g_K]
    exp = dict(event=ev, ids=s.ids[ev].reshape(-1), creator=s.cr[ev], rr=s.rr[ev], time=s.cts[ev])
    for k in exp:
        if k in got:
            assert np.array_equal(got[k], exp[k]), k
    return got, ordered


def test_two_calls_members_not_a_multiple_of_64_and_small_grids(emul, tmp_path):
    s = Scene(70, 3000, 1)
    (e1, *_), (e2, *_) = s.calls
    assert len(e1) % THREADS and len(e2) % THREADS and len(e1) > THREADS and len(e2) > THREADS      # slot counts no multiple of the workgroup
    # every event, every position; grids smaller than the ranges (one trip of the gather covers grid * 256 / 4 positions)
    got, ordered = check(emul, tmp_path, s, 0, s.N, 0, len(s.tx), ev_grid=2, g_grid=3)
    assert s.N > 2 * THREADS and len(s.tx) > 3 * THREADS // LANES
    # unordered events in the middle of the event range, ordered ones on both sides
    mid = np.flatnonzero(~ordered)
    assert ordered[:mid[0]].any() and ordered[mid[len(mid) // 2]:].any() and 0 < mid[0] < mid[-1]
    # first > 0 in both kernels, and a gather range that crosses the two calls' records
    a = s.split - 37
    assert a > 0
    check(emul, tmp_path, s, 129, 700, a, 101, ev_grid=1, g_grid=1)
    check(emul, tmp_path, s, s.N - 1, 1, len(s.tx) - 1, 1)


def test_one_slot_and_ranges_of_zero_and_one(emul, tmp_path):
    s = Scene(5, 200, 2, only=1)
    assert len(s.calls[0][0]) == 1 and len(s.calls[1][0]) == 0 and len(s.tx) == 1
    check(emul, tmp_path, s, 0, s.N, 0, 1)
    check(emul, tmp_path, s, 17, 0, 0, 0)              # K = 0 in both: nothing read, nothing written
    check(emul, tmp_path, s, 17, 1, 0, 1, ev_grid=1, g_grid=1)
    s = Scene(130, 5000, 3)
    check(emul, tmp_path, s, 4000, 1, 1, 0)
    check(emul, tmp_path, s, 0, 1, len(s.tx) // 2, 1)


def test_every_output_absent_in_turn(emul, tmp_path):
    s = Scene(33, 1500, 4)
    K = len(s.tx) - 11
    for bit in (EV, ID, CR, RR, TM):
        got, _ = check(emul, tmp_path, s, 3, 1200, 11, K, ev_flags=3, g_flags=31 ^ bit, g_grid=2)
        assert len(got) == 2 + 2 + 4
    for bit in (EV, ID, CR, RR, TM):                    # ... and each one alone
        check(emul, tmp_path, s, 3, 1200, 11, K, g_flags=bit, g_grid=5)
    check(emul, tmp_path, s, 3, 1200, 11, K, ev_flags=1, g_flags=0)
    check(emul, tmp_path, s, 3, 1200, 11, K, ev_flags=2, g_flags=0)
