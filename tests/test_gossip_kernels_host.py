"""CPU: the export kernels of csrc/gossip.hip.h run thread by thread on the host (tests/gossip_emul.cpp, a stand-alone
program built with AddressSanitizer and UBSan) against tests/model_gossip.py: member counts that are no multiple of 64,
empty ranges in the middle and at both ends, a payload of one event, absent timestamps / signatures, roots among the
exported events, every lane width, grids smaller than the payload.  The host side of the library (checks, streams, the
read-back of the count) is NOT covered here: tests/test_gpu_export.py does that on the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import model_gossip as mg
from conftest import ROOT


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gossip_emul") / "gossip_emul")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "gossip_emul.cpp"), "-o", exe])
    return exe


def graph(pkg, n, N, seed, mode=0, p0=0.0, p1=0.0):
    cr, sp, op, t, sig = pkg.synth_hashgraph(n, N, seed, mode, p0, p1)
    return mg.Graph(n, cr, sp, op, t, sig)


def run(emul, tmp_path, g, first, end, G=16, flags=7, grid=3):
    """The ranges through the emulated kernels; returns the arrays as the model names them."""
    n, N = g.n, g.N
    # a chain pool with slack between the members' segments, like the library's
    caps = [len(ch) + len(ch) // 4 + 16 for ch in g.chains]
    start = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int32)
    pool = np.full(int(sum(caps)), -1, np.int32)
    for m, ch in enumerate(g.chains):
        pool[start[m]:start[m] + len(ch)] = ch
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([n, N, len(pool), flags, grid], np.int32).tobytes())
        for a in (first, end, start, pool, g.sp, g.op):
            f.write(np.ascontiguousarray(a, np.int32).tobytes())
        f.write(g.ids.tobytes())
        f.write(g.t.tobytes())
        f.write(g.sig.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([emul, src, dst, str(G)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(dst, "rb").read()
    K = int(np.frombuffer(raw[:8], np.int64)[0])
    pos = 8
    out = {}

    def take(name, count, dtype, shape=None):
        nonlocal pos
        a = np.frombuffer(raw, dtype, count, pos)
        pos += a.nbytes
        out[name] = a if shape is None else a.reshape(shape)
    take("off", n + 1, np.int32)
    take("ids", K * 32, np.uint8, (K, 32))
    take("sp_ids", K * 32, np.uint8, (K, 32))
    take("op_ids", K * 32, np.uint8, (K, 32))
    take("arity", K, np.uint8)
    take("creator", K, np.int32)
    if flags & 1:
        take("t", K, np.float64)
    if flags & 2:
        take("sig", K * 64, np.uint8, (K, 64))
    if flags & 4:
        take("event", K, np.int32)
    assert pos == len(raw)
    return out


def check(emul, tmp_path, g, head, known, **kw):
    exp = g.export(head, known)
    got = run(emul, tmp_path, g, exp["first"], exp["end"], **kw)
    lens = exp["end"] - exp["first"]
    assert np.array_equal(got["off"], np.concatenate([[0], np.cumsum(lens)]))
    for k in got:
        if k != "off":
            assert got[k].tobytes() == np.ascontiguousarray(exp[k]).tobytes(), k
    return exp


def test_members_not_a_multiple_of_64_and_every_lane_width(pkg, emul, tmp_path):
    g = graph(pkg, 70, 3000, 41, 2, 0.3, 0.02)
    rng = np.random.default_rng(1)
    for G in (4, 8, 16):
        head, asker = int(rng.integers(70, g.N)), int(rng.integers(0, g.N))
        exp = check(emul, tmp_path, g, head, g.known_heights(asker), G=G, grid=2)
        assert len(exp["event"]) >= 1
    # an asker that knows nobody: every ancestor of the head, the roots (zero parent ids, arity 0) among them
    exp = check(emul, tmp_path, g, g.N - 1, None, grid=5)
    roots = exp["arity"] == 0
    assert roots.sum() >= 60 and not exp["sp_ids"][roots].any() and not exp["op_ids"][roots].any()
    assert len(exp["event"]) > 4 * 256          # more slots than the grid covers in one trip


def test_empty_ranges_in_the_middle_and_at_both_ends(pkg, emul, tmp_path):
    g = graph(pkg, 130, 5000, 42, 3, 0.6, 0)
    head = g.N - 1
    known = g.known_heights(head).copy()
    # the asker knows everything the head sees, except for a few members in the middle
    for m in (3, 64, 65, 100):
        known[m] = -1
    exp = check(emul, tmp_path, g, head, known)
    lens = exp["end"] - exp["first"]
    assert lens[0] == 0 and lens[129] == 0 and lens[4] == 0 and lens[64] > 0 and lens[65] > 0
    known[:] = g.known_heights(head)
    known[0] = known[129] = -1                      # ... and now only the two ends are not empty (and the head's creator)
    check(emul, tmp_path, g, head, known, G=8)


def test_payload_of_one_event_and_absent_arrays(pkg, emul, tmp_path):
    g = graph(pkg, 5, 300, 43)
    head = 250
    exp = check(emul, tmp_path, g, head, g.known_heights(head), flags=0)     # asker == head: the head alone; no t, sig, event
    assert exp["event"].tolist() == [head]
    check(emul, tmp_path, g, head, np.full(5, 2**31 - 1, np.int32), flags=1)
    check(emul, tmp_path, g, head, g.known_heights(40), flags=2, G=4)
    check(emul, tmp_path, g, head, g.known_heights(40), flags=4, G=8)
