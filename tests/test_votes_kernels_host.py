"""CPU: the kernels of csrc/votes.hip.h run thread by thread on the host (tests/votes_emul.cpp, a stand-alone program built
with AddressSanitizer and UBSan) against tests/model_votes.py, from the tables the library would hold after the golden's
call schedule: an incremental schedule with coin rounds, stakes, and 130 members (three mask words in rows of four).  The
host side of the library (checks, streams, the read-back of the counts) is NOT covered here: tests/test_gpu_votes.py does
that on the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import model_votes as mv
from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("votes_emul") / "votes_emul")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "votes_emul.cpp"), "-o", exe])
    return exe


def run(emul, tmp_path, g, t, rv0, rv1, coin_period=mv.COIN_PERIOD):
    wit = g["witnesses"]
    R, n = wit.shape
    nw = 1
    while nw * 64 < n:
        nw *= 2
    npad, nwo, N = 64 * nw, (n + 63) // 64, len(g["round"])
    pad = lambda a, fill: np.concatenate([a, np.full((R, npad - n), fill, a.dtype)], axis=1)   # noqa: E731
    Sbits = np.zeros((R, npad, nw * 64), bool)
    Sbits[:, :n, :n] = t["S"]
    stake = np.zeros(npad, np.uint32)
    stake[:n] = g["stake"]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([n, nw, R, N, coin_period, len(t["calls"]), rv0, rv1, int((g["stake"] == 1).all())], np.int32).tobytes())
        f.write(pad(wit.astype(np.int32), -1).tobytes())
        f.write(mv.pack_words(Sbits.reshape(R * npad, nw * 64)).tobytes())
        f.write((g["sig"][:, 0] >> 7).astype(np.uint8).tobytes())
        f.write(stake.tobytes())
        f.write(pad(t["dec_call"], -1).tobytes())
        f.write(pad(t["dec_by"], -1).tobytes())
        f.write(g["round"].astype(np.int32).tobytes())
        f.write(np.array([c[:2] for c in t["calls"]], np.int32).tobytes())
        f.write(np.array([c[2] for c in t["calls"]], np.int64).tobytes())
        f.write(t["cons_call"].astype(np.int32).tobytes())
    r = subprocess.run([emul, src, dst], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(dst, "rb").read()
    n_rows, n_entries, levels = np.frombuffer(raw, np.int64, 3).tolist()
    pos = 24
    out = {"n_rows": n_rows, "n_entries": n_entries, "levels": levels}
    for name, dtype, cols in (("row_voter", np.int32, 1), ("row_cand_round", np.int32, 1), ("exists", np.uint64, nwo), ("value", np.uint64, nwo)):
        a = np.frombuffer(raw, dtype, n_rows * cols, pos)
        pos += a.nbytes
        out[name] = a.reshape(n_rows, cols) if cols > 1 or name in ("exists", "value") else a
    assert pos == len(raw)
    return out


@pytest.mark.parametrize("name", ["n4_s6_chunk7", "n10_s1_stake", "n130_s4_batch"])
def test_the_kernels_reproduce_the_model(emul, tmp_path, name):
    g = load_golden(name)
    t = mv.model_votes(g)
    R = g["witnesses"].shape[0]
    seen = t["calls"][-1][1]
    got = run(emul, tmp_path, g, t, 0, seen)
    assert got["n_rows"] == len(t["row_voter"]) and got["n_entries"] == t["n_entries"] == len(g["votes"])
    for k in ("row_voter", "row_cand_round", "exists", "value"):
        assert np.array_equal(got[k], t[k]), k
    assert got["levels"] > 0 and seen <= R
    # a range in the middle: exactly the rows of its voter rounds
    a, b = seen // 3, 2 * seen // 3 + 1
    part = run(emul, tmp_path, g, t, a, b)
    rv = g["round"][t["row_voter"]]
    keep = (rv >= a) & (rv < b)
    assert keep.any()
    for k in ("row_voter", "row_cand_round", "exists", "value"):
        assert np.array_equal(part[k], t[k][keep]), k
    assert run(emul, tmp_path, g, t, 3, 3)["n_rows"] == 0
