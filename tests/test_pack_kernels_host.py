"""CPU: the kernels of csrc/pack.hip.h run thread by thread on the host (tests/pack_emul.cpp, a stand-alone program built
with AddressSanitizer and UBSan) against tests/model_pack.py: offsets, flags and both byte streams exact, a canary behind
off[K] untouched.  Event counts around the tile sizes, roots (61-byte messages: chunks that straddle two and three events),
every data length at which the encoding changes, events that cannot be encoded, data offsets that lead nowhere, grids
smaller than the stream.  The host side of the library is NOT covered here: tests/test_gpu_pack.py does that on the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import model_pack as mp
from conftest import ROOT

CANARY = 37


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("pack_emul") / "pack_emul")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "pack_emul.cpp"), "-o", exe])
    return exe


def events(K, n, seed, roots=0.3):
    """Random arrays of K events by n members; roots: the fraction of arity-0 events."""
    rng = np.random.default_rng(seed)
    a = dict(keys=rng.integers(0, 256, (n, 32), dtype=np.uint8), sp=rng.integers(0, 256, (K, 32), dtype=np.uint8),
             op=rng.integers(0, 256, (K, 32), dtype=np.uint8), sig=rng.integers(0, 256, (K, 64), dtype=np.uint8),
             arity=np.where(rng.random(K) < roots, 0, 2).astype(np.uint8), creator=rng.integers(0, n, K).astype(np.int32),
             t=rng.random(K) * 1e9)
    if K:
        a["t"][0] = -0.0
        a["t"][K // 2] = np.inf
    return a


def with_data(a, lens, seed, none=None, slack=0):
    rng = np.random.default_rng(seed)
    a["data_off"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    a["data"] = rng.integers(0, 256, int(a["data_off"][-1]) + slack, dtype=np.uint8)
    if none is not None:
        a["data_none"] = np.asarray(none, np.uint8)
    return a


def check(emul, tmp_path, a, grid=3, mod="swirld", qual="Event"):
    K, n = len(a["arity"]), len(a["keys"])
    has_data = "data_off" in a
    exp = mp.pack(a["keys"], a["sp"], a["op"], a["arity"], a["creator"], a["t"], a["sig"], a.get("data"), a.get("data_off"),
                  a.get("data_none"), mod, qual)
    e_msgs, e_moff, e_whole, e_woff, e_enc = exp
    caps = (int(e_moff[-1]) + CANARY, int(e_woff[-1]) + CANARY)
    hdr = mp.class_header(mod, qual)
    flags = (1 if has_data else 0) | (2 if "data_none" in a else 0)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([K, n, flags, len(a["data"]) if has_data else 0, grid, len(hdr), caps[0], caps[1]], np.int64).tobytes())
        for name, dt in (("sp", np.uint8), ("op", np.uint8), ("arity", np.uint8), ("creator", np.int32), ("t", np.float64), ("sig", np.uint8),
                         ("keys", np.uint8)):
            f.write(np.ascontiguousarray(a[name], dt).tobytes())
        f.write(hdr)
        if has_data:
            f.write(np.ascontiguousarray(a["data_off"], np.int64).tobytes())
            f.write(a["data"].tobytes())
        if "data_none" in a:
            f.write(a["data_none"].tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([emul, src, dst], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(dst, "rb").read()
    pos = 0

    def take(count, dtype):
        nonlocal pos
        x = np.frombuffer(raw, dtype, count, pos)
        pos += x.nbytes
        return x
    moff, woff, enc = take(K + 1, np.int64), take(K + 1, np.int64), take(K, np.uint8)
    msgs, whole = take(caps[0], np.uint8), take(caps[1], np.uint8)
    assert pos == len(raw)
    assert np.array_equal(moff, e_moff) and np.array_equal(woff, e_woff)
    assert np.array_equal(enc, e_enc)
    for got, want in ((msgs, e_msgs), (whole, e_whole)):
        bad = np.flatnonzero(got[:len(want)] != want)
        assert bad.size == 0, "first differing byte at %d of %d" % (bad[0], len(want))
        assert (got[len(want):] == 0xA5).all(), "bytes behind off[K] were written"
    return exp


@pytest.mark.parametrize("K", [0, 1, 2, 65, 1000])
def test_event_counts_and_root_mixes(emul, tmp_path, K):
    for roots in (1.0, 0.0, 0.4):       # all roots (61 B each: chunks straddle two and three events), none, mixed
        a = events(K, 5, 10 + K, roots)
        check(emul, tmp_path, a, grid=2)


def test_chunks_straddle_two_and_three_events(emul, tmp_path):
    # 61-byte messages in a row: nearly every event starts inside a chunk (two events per chunk); no message is shorter
    # than 61 bytes, so three events meet in one chunk only around an EMPTY one
    a = events(40, 5, 3, 1.0)
    a["arity"][[7, 8, 20]] = 3
    _, moff, _, _, enc = check(emul, tmp_path, a, grid=1)
    lens = np.diff(moff)
    assert (lens[enc == 1] == 61).all() and (lens[enc == 0] == 0).all()
    assert (moff[:-1][enc == 1] % 16 != 0).sum() >= 30
    assert moff[7] % 16 != 0 and moff[20] % 16 != 0     # the empty events sit inside a chunk


def test_member_count_no_multiple_of_64_and_class_names(emul, tmp_path):
    a = events(300, 70, 4)
    check(emul, tmp_path, a, mod="m", qual="Q")
    check(emul, tmp_path, a, mod="py-swirld_amd.node", qual="Event")
    check(emul, tmp_path, a, mod="x" * 255, qual="é" * 127 + "y")


def test_data_lengths_and_the_unencodable_length(emul, tmp_path):
    lens = [0, 1, 31, 32, 255, 256, 257, 4095, 60000, 60001, 5, 0]
    K = len(lens)
    none = np.zeros(K, np.uint8)
    none[[2, 10]] = 1
    for roots in (0.0, 1.0):
        a = with_data(events(K, 5, 6, roots), lens, 7, none)
        _, _, _, _, enc = check(emul, tmp_path, a, grid=4)
        assert enc.tolist() == [1] * 9 + [0, 1, 1]
    a = with_data(events(K, 5, 8), lens, 9)           # without the None flags
    check(emul, tmp_path, a, grid=7)


def test_bad_arity_and_creator(emul, tmp_path):
    a = events(200, 6, 11)
    a["arity"][[0, 17, 100, 199]] = [1, 3, 255, 1]
    a["creator"][[5, 64, 150]] = [-1, 6, 2 ** 31 - 1]
    _, _, _, _, enc = check(emul, tmp_path, a)
    assert enc.sum() == 200 - 7


def test_data_offsets_that_lead_nowhere(emul, tmp_path):
    K = 12
    a = with_data(events(K, 5, 12), [10] * K, 13)
    off = a["data_off"].copy()
    off[3] = 45                 # decreasing: event 3 is [45, 40) (event 2, [20, 45), is fine)
    off[6] = -5                 # negative: events 5 and 6
    off[9] = 10 ** 12           # beyond the buffer: events 8 and 9
    off[12] = 121               # one past the end: event 11
    a["data_off"] = off
    _, _, _, _, enc = check(emul, tmp_path, a)
    assert enc.tolist() == [1, 1, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0]


def test_grid_smaller_than_the_stream(emul, tmp_path):
    a = events(1000, 9, 14, 0.1)       # ~ 127 KB and ~ 215 KB: 31 and 53 trips of one workgroup
    check(emul, tmp_path, a, grid=1)
    a = with_data(events(3, 5, 15), [60000, 0, 60000], 16)   # one event longer than many trips; a tile of three offsets
    check(emul, tmp_path, a, grid=2)


def test_more_empty_events_than_an_offset_tile(emul, tmp_path):
    a = events(900, 5, 17)
    a["arity"][100:700] = 1            # 600 empty events in a row: the lane's event lies beyond the 256 staged offsets
    check(emul, tmp_path, a, grid=2)
