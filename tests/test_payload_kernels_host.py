"""CPU: the payload kernels of csrc/resolve.hip.h run thread by thread on the host (tests/payload_emul.cpp, a stand-alone
program built with AddressSanitizer and UBSan) against tests/model_payload.py: tables with colliding ids, every reject
code, a cycle, known ids, deep payloads.  The host side of the library (allocation, the wave batches' read-backs, the
sort through the rank kernels of ingest.hip.h) is NOT covered here: tests/test_gpu_payload.py does that on the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import model_payload as mp
from conftest import ROOT


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("payload_emul") / "payload_emul")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "payload_emul.cpp"), "-o", exe])
    return exe


def run(emul, tmp_path, index, events):
    ids, spi, opi, ar, cr, ok = mp.to_arrays(events)
    K, N0 = len(events), len(index.ids)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([index.n, N0, K], np.int32).tobytes())
        f.write(b"".join(index.ids))
        f.write(np.array(index.cr, np.int32).tobytes())
        for a in (ids, spi, opi, ar, ok, cr):
            f.write(a.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([emul, src, dst], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(dst, "rb").read()
    waves, A = np.frombuffer(raw[:8], np.int32)
    out = np.frombuffer(raw[8:8 + 4 * K], np.int32)
    rec = np.frombuffer(raw[8 + 4 * K:8 + 4 * K + 12 * A], np.int32).reshape(A, 3)
    gid = raw[8 + 4 * K + 12 * A:]
    return int(waves), out, rec, [gid[32 * r:32 * r + 32] for r in range(A)]


def check(emul, tmp_path, index, events):
    exp_out, order, waves, parents = mp.ingest(index, events, commit=False)
    got_w, out, rec, gid = run(emul, tmp_path, index, events)
    assert np.array_equal(out, exp_out), [(i, int(out[i]), int(exp_out[i])) for i in np.flatnonzero(out != exp_out)][:10]
    assert got_w == waves
    assert [tuple(r) for r in rec.tolist()] == [(events[i][2],) + tuple(parents[i]) for i in order]
    assert gid == [events[i][0] for i in order]
    return waves


def test_shuffled_chunks_with_known_ids(pkg, emul, tmp_path):
    n, N = 16, 6000
    cr, sp, op, _, _ = pkg.synth_hashgraph(n, N, 31, with_sig=False)
    rng = np.random.default_rng(3)
    index = mp.Index(n)
    for a, b in ((0, 700), (700, 5000), (5000, N)):
        extra = rng.choice(a, min(a, 25), replace=False).tolist() if a else []
        events = mp.from_stream(cr, sp, op, rng.permutation(np.array(list(range(a, b)) + extra)).tolist())
        check(emul, tmp_path, index, events)
        mp.ingest(index, events)


def test_every_reject_code_and_a_cycle(pkg, emul, tmp_path):
    n, N, known = 8, 300, 60
    cr, sp, op, _, _ = pkg.synth_hashgraph(n, N, 7, with_sig=False)
    index = mp.Index(n)
    for k in range(known):
        index.add(mp.event_id(k), cr[k])
    events, expect = mp.reject_payload(cr, sp, op, n, known, 7)
    check(emul, tmp_path, index, events)
    # nothing but rejects and a cycle: no wave accepts anything
    only = [events[p] for p in sorted(expect) if expect[p] != mp.DUP]
    assert check(emul, tmp_path, index, only) == 0


def test_deep_payload_and_colliding_ids(pkg, emul, tmp_path):
    n, N, known = 4, 3000, 1000
    cr, sp, op, _, _ = pkg.synth_hashgraph(n, N, 32, with_sig=False)
    # groups of 8 ids with the same first 8 bytes — the word the tables hash
    crafted = lambda k: mp.event_id(k // 8)[:8] + mp.event_id(1_000_000 + k)[8:]
    index = mp.Index(n)
    for k in range(known):
        index.add(crafted(k), cr[k])
    events = mp.from_stream(cr, sp, op, np.random.default_rng(4).permutation(np.arange(known, N)).tolist(), id_of=crafted)
    assert check(emul, tmp_path, index, events) > 600      # more waves than one batch of launches, by far
