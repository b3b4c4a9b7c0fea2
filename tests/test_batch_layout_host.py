"""CPU: csrc/batch_layout.h, where the hashgraphs of a batch lie in their one allocation, through tests/batch_layout_main.cpp
(a stand-alone program built with AddressSanitizer and UBSan).  The program checks, for the shape it is given, that segments
and slabs are disjoint, 64-byte aligned, monotone in b and end at the total; this file gives it the shapes — the batch's
own row strides, a stride wider than a wave, odd capacities, a lowered cap_rounds, and a batch above 4 GiB — and compares
the figures it prints with the memory formula the header documents."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("batch_layout") / "batch_layout_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "batch_layout_main.cpp"), "-o", exe])
    return exe


def run(prog, *args):
    r = subprocess.run([prog, *map(str, args)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-3000:]
    return {k: int(v) for k, v in (ln.split() for ln in r.stdout.splitlines())}


def up64(v):
    return (v + 63) // 64 * 64


def formula(n, np_, E, R):
    """Bytes of one hashgraph (include/swirld_hip.h, sw_batch_bytes), every array rounded up to 64 bytes."""
    R = R or E + 3
    per_event = 5 * [E * 4] + [E * 8, E * 64, E, E] + [(E + 1) * 4, E + 1, (E + 1) * 4, (E + 1) * 8, (E + 1) * 4] + [E * 4, E * 4, E * 8]
    per_round = [R * np_ * 4, R * np_ * 4, R * 4, R, R * np_, R, R * 4]
    rest = [np_ * 4, np_, np_ * 4, np_, np_ * 8, np_ * 8, 64, 128]
    return sum(up64(b) for b in [E * np_ * 4] + per_event + per_round + [2 * n * n * R] + rest)


@pytest.mark.parametrize("B,n,npad,E,R", [
    (1, 4, 16, 40, 0), (7, 4, 16, 41, 0), (10000, 4, 16, 40, 0), (48, 8, 16, 700, 0), (8, 70, 80, 1600, 0), (3, 16, 16, 1, 0),
    (5, 17, 32, 333, 29), (8192, 64, 64, 600, 40), (9, 130, 144, 77, 0), (2, 1024, 1024, 5, 0), (6, 4, 64, 100, 0),
])
def test_layout_shapes(prog, B, n, npad, E, R):
    got = run(prog, B, n, npad, E, R)
    assert got["slab"] == formula(n, npad, E, R)
    head = up64(B * 512) + up64(B * 64)
    assert got["total"] == head + B * got["slab"]
    assert got["last_slab"] == head + (B - 1) * got["slab"]
    assert got["npad_of"] == (n + 15) // 16 * 16 and got["npad_of"] >= n
    if npad == got["npad_of"]:
        assert got["batch_bytes"] == got["total"]


def test_layout_above_4_gib(prog):
    """B = 2048 hashgraphs of 8192 events at a row stride of 64: the can_see rows alone are 4 GiB, so the offsets of the
    later hashgraphs do not fit 32 bits."""
    B, n, npad, E, R = 2048, 64, 64, 8192, 64
    got = run(prog, B, n, npad, E, R)
    slab = formula(n, npad, E, R)
    assert got["slab"] == slab and slab >= E * npad * 4 == 2 << 20
    assert got["total"] > 4 << 30
    assert got["last_slab"] == up64(B * 512) + up64(B * 64) + (B - 1) * slab > 1 << 32
    assert got["last_hdr"] == got["last_slab"] + slab - 128
    assert got["batch_bytes"] == got["total"]


def test_shapes_whose_total_does_not_fit_are_recognised(prog):
    """Every argument within the entry points' limits, the product beyond 2^62 bytes (B = 8192, 1024 members, 2^30 events would
    wrap 64 bits): fits() says so before make() is asked."""
    assert run(prog, 8192, 1024, 1024, 1 << 30, 0) == dict(fits=0)
    assert run(prog, 1 << 24, 64, 64, 1 << 30, 64) == dict(fits=0)
    assert run(prog, 2048, 64, 64, 8192, 64)["fits"] == 1
