"""CPU: the kernels of csrc/walk.hip.h run thread by thread on the host (tests/walk_emul.cpp, a stand-alone program built
with AddressSanitizer and UBSan) against tests/model_walk.py: forked and fork-free streams, member counts that are no
multiple of 64, event counts that are no multiple of 32, a head in the middle and a head that is a root, nobody known /
everything known / real and arbitrary heights / a cap, a workgroup narrower than the widest level, every lane width,
absent arrays, and the trunk heights with a second root.  The host side of the library (checks, streams, the read-back
of the count) is NOT covered here: tests/test_gpu_walk.py does that on the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import model_walk as mw
from conftest import ROOT
from test_exact_host import add_forks


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("walk_emul") / "walk_emul")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "walk_emul.cpp"), "-o", exe])
    return exe


def run(emul, tmp_path, g, head, known=None, cap=None, G=16, flags=7, grid=3, threads=1024):
    n, N = g.n, g.N
    fl = flags | (8 if known is not None else 0) | (16 if cap is not None else 0)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([n, N, head, fl, grid], np.int32).tobytes())
        for a in (np.zeros(n) if known is None else known, np.zeros(n) if cap is None else cap, g.sp, g.op, g.cr, g.height):
            f.write(np.ascontiguousarray(a, np.int32).tobytes())
        f.write(g.ids.tobytes())
        f.write(g.t.tobytes())
        f.write(g.sig.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([emul, src, dst, str(G), str(threads)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(dst, "rb").read()
    pos = 0
    out = {}

    def take(name, count, dtype, shape=None):
        nonlocal pos
        a = np.frombuffer(raw, dtype, count, pos)
        pos += a.nbytes
        out[name] = a if shape is None else a.reshape(shape)
    take("hdr", 8, np.int32)
    K = int(out["hdr"][0])
    take("nl", 1, np.int32)
    take("widths", int(out["nl"][0]), np.int32)
    take("event_list", K, np.int32)
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
    take("trunk", n, np.int32)
    assert pos == len(raw)
    return out


def check(emul, tmp_path, g, head, known=None, cap=None, **kw):
    got = run(emul, tmp_path, g, head, known, cap, **kw)
    lv = g.levels(head, known, cap)
    exp = g.export_walk(head, known, cap)
    assert got["hdr"][0] == len(exp["event"]) and got["hdr"][1] == len(lv) and got["hdr"][2] == 0
    assert got["hdr"][3] == exp["event"][0] and got["hdr"][4] == len(exp["event"])
    assert got["widths"].tolist() == [len(l) for l in lv]
    assert np.array_equal(got["event_list"], exp["event"])
    for k in ("ids", "sp_ids", "op_ids", "arity", "creator", "t", "sig", "event"):
        if k in got:
            assert got[k].tobytes() == np.ascontiguousarray(exp[k]).tobytes(), k
    assert np.array_equal(got["trunk"], g.trunks())
    return got, lv


def forked(pkg, n, N, seed, n_forks, second_root=None):
    stream = add_forks(pkg.synth_hashgraph(n, N, seed), n, seed + 1000, n_forks)
    if second_root is not None:
        stream = mw.with_second_root(stream, second_root, seed)
    return mw.WalkGraph(n, *stream)


@pytest.mark.parametrize("n,N,seed,n_forks", [(5, 301, 51, 4), (33, 1203, 52, 0), (70, 1501, 53, 9)])
def test_walk_list_gather_and_trunks_against_the_model(pkg, emul, tmp_path, n, N, seed, n_forks):
    g = forked(pkg, n, N, seed, n_forks, second_root=1 if n_forks else None)
    assert g.N % 32 != 0
    head, mid = g.N - 1, g.N // 2 + 1
    check(emul, tmp_path, g, head)                                            # nobody known: every ancestor
    got, _ = check(emul, tmp_path, g, head, np.full(n, mw.NO_CAP, np.int32))   # everything known: the head alone
    assert got["event_list"].tolist() == [head]
    got, _ = check(emul, tmp_path, g, mid, g.ancestors_heights(g.N // 5), G=8, grid=2)      # a head in the middle
    assert got["event_list"].max() == mid
    got, _ = check(emul, tmp_path, g, 2, None, G=4)                           # the head a root
    assert got["event_list"].tolist() == [2] and got["arity"].tolist() == [0]
    check(emul, tmp_path, g, head, mw.arbitrary_heights(g, head, seed), flags=0)
    check(emul, tmp_path, g, head, g.ancestors_heights(mid), g.trunks(), flags=5)
    if n_forks:
        assert (g.trunks() != mw.NO_CAP).any() and g.trunks()[1] == -1


def test_the_strict_subset_case(pkg, emul, tmp_path):
    n, N, seed, head, hseed = mw.STRICT_CASE
    g = mw.WalkGraph(n, *pkg.synth_hashgraph(n, N, seed))
    known = mw.arbitrary_heights(g, head, hseed)
    got, _ = check(emul, tmp_path, g, head, known)
    assert set(got["event_list"].tolist()) < mw.ranges_set(g, head, known)


def test_a_level_wider_than_the_workgroup(pkg, emul, tmp_path):
    g = forked(pkg, 130, 2001, 54, 5)
    head = g.N - 1
    lv = g.levels(head)
    assert max(len(l) for l in lv) > 64
    a, _ = check(emul, tmp_path, g, head, threads=64)
    b, _ = check(emul, tmp_path, g, head, threads=1024)
    assert np.array_equal(a["event_list"], b["event_list"])
    check(emul, tmp_path, g, head, threads=1)


def test_equal_height_siblings_and_the_cap(pkg, emul, tmp_path):
    """Two children of one self-parent with the same height: an asker that reports that height gets neither without the cap,
    both with it."""
    # members 0, 1, 2; roots 0 1 2; 3 = (0 on 1); siblings 4 = (1: sp 1, op 3), 5 = (1: sp 1, op 3); 6 = (2: sp 2, op 4); 7 = (0: sp 3, op 5); 8 = (2: sp 6, op 7)
    cr = np.array([0, 1, 2, 0, 1, 1, 2, 0, 2], np.int32)
    sp = np.array([-1, -1, -1, 0, 1, 1, 2, 3, 6], np.int32)
    op = np.array([-1, -1, -1, 1, 3, 3, 4, 5, 7], np.int32)
    g = mw.WalkGraph(3, cr, sp, op, np.arange(9.0), (np.arange(9 * 64) % 251).astype(np.uint8).reshape(9, 64))
    assert g.height[4] == g.height[5] == 2 and g.trunks().tolist() == [mw.NO_CAP, 0, mw.NO_CAP]
    known = np.array([1, 2, 0], np.int32)            # the asker holds sibling 4 (height 2) and not 5
    got, _ = check(emul, tmp_path, g, 8, known)
    assert 5 not in got["event_list"] and 4 not in got["event_list"]
    got, _ = check(emul, tmp_path, g, 8, known, g.trunks())
    assert 5 in got["event_list"] and 4 in got["event_list"] and 1 not in got["event_list"]
