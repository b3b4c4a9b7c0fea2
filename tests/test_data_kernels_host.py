"""CPU: the kernels of csrc/data.hip.h run thread by thread on the host (tests/data_emul.cpp, a stand-alone program built
with AddressSanitizer and UBSan) against tests/model_data.py: offsets, flags and bytes exact, and the destination — which
starts as 0xA5 everywhere — unchanged below the stream's first byte and behind its last.  The three uses of the ragged gather
(store from a caller's buffer, append at an arena tail of every residue mod 16, gather by index from an arena), every length
at which a chunk changes its case, chunks that hold 16 segments, runs of empty slots longer than an LDS tile of offsets,
grids smaller than the stream, and offsets that lead nowhere.  The host side of the library is NOT covered here:
tests/test_gpu_event_data.py does that on the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import model_data as md
from conftest import ROOT

LENS = [None, 0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 4095, 60000]
CANARY = 37


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("data_emul") / "data_emul")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "data_emul.cpp"), "-o", exe])
    return exe


def run(emul, tmp_path, blob):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(blob)
    r = subprocess.run([emul, src, dst], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-3000:]
    return open(dst, "rb").read()


def datas(lens, seed):
    rng = np.random.default_rng(seed)
    return [None if n is None else rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]


def gather(emul, tmp_path, K, src, src_off, src_none, idx, n_src, arena, grid=3, dst_base=0, expect_bad=None):
    """One ragged gather through the emulation, checked against the model; returns the model's (data, off, none)."""
    src = np.zeros(0, np.uint8) if src is None else np.ascontiguousarray(src, np.uint8)
    e_data, e_off, e_none, e_bad = md.ragged_gather(K, src if src_off is not None else None, src_off, src_none, idx, n_src)
    cap = dst_base + (0 if e_bad else len(e_data)) + CANARY
    flags = (1 if src_off is not None else 0) | (2 if src_none is not None else 0) | (4 if idx is not None else 0) | (8 if arena else 0)
    blob = np.array([0, K, n_src, flags, len(src), grid, dst_base, cap, 0], np.int64).tobytes()
    if src_off is not None:
        blob += np.ascontiguousarray(src_off, np.int64).tobytes()
    blob += src.tobytes()
    if src_none is not None:
        blob += np.ascontiguousarray(src_none, np.uint8).tobytes()
    if idx is not None:
        blob += np.ascontiguousarray(idx, np.int32).tobytes()
    raw = run(emul, tmp_path, blob)
    bad = int(np.frombuffer(raw, np.int64, 1, 0)[0])
    off = np.frombuffer(raw, np.int64, K + 1, 8)
    none = np.frombuffer(raw, np.uint8, K, 8 + 8 * (K + 1))
    dst = np.frombuffer(raw, np.uint8, cap, 8 + 8 * (K + 1) + K)
    assert 8 + 8 * (K + 1) + K + cap == len(raw)
    assert bad == e_bad
    if expect_bad is not None:
        assert bad == expect_bad
    if bad:
        assert (dst == 0xA5).all(), "a refused gather wrote bytes"
        return None
    assert np.array_equal(off, e_off + dst_base) and np.array_equal(none, e_none)
    assert (dst[:dst_base] == 0xA5).all(), "bytes below the stream's first byte were written"
    got = dst[dst_base:dst_base + len(e_data)]
    diff = np.flatnonzero(got != e_data)
    assert diff.size == 0, "first differing byte at %d of %d" % (diff[0], len(e_data))
    assert (dst[dst_base + len(e_data):] == 0xA5).all(), "bytes behind the stream's last byte were written"
    return e_data, e_off, e_none


def test_every_length_from_a_callers_buffer_and_from_an_arena(emul, tmp_path):
    d = datas(LENS + LENS[::-1], 1)
    data, off, none = md.pack(d)
    K = len(d)
    got = gather(emul, tmp_path, K, data, off, none, None, K, arena=False, grid=2)       # the store from device memory
    assert md.unpack(*got) == d
    got = gather(emul, tmp_path, K, data, off, none, np.arange(K), K, arena=True, grid=2)  # the gather by index
    assert md.unpack(*got) == d


def test_sixteen_segments_in_one_chunk(emul, tmp_path):
    d = datas([1] * 40, 2)
    data, off, none = md.pack(d)
    for arena in (False, True):
        for base in (0, 5):
            got = gather(emul, tmp_path, 40, data, off, none, np.arange(40) if arena else None, 40, arena=arena, grid=1, dst_base=base)
            assert md.unpack(*got) == d


def test_more_empty_slots_than_an_offset_tile(emul, tmp_path):
    lens = [20] * 10 + [None, 0] * 300 + [33] * 10 + [0] * 300 + [5]
    d = datas(lens, 3)
    data, off, none = md.pack(d)
    K = len(d)
    for arena in (False, True):
        got = gather(emul, tmp_path, K, data, off, none, np.arange(K) if arena else None, K, arena=arena, grid=2)
        assert md.unpack(*got) == d


@pytest.mark.parametrize("residue", range(16))
def test_an_append_at_every_residue_of_the_arena_tail(emul, tmp_path, residue):
    # the arena holds `used` bytes already (0xA5 here: the canary is the earlier events' data) and the stream starts there
    for used in (residue, 4096 + residue):
        for lens in ([7], [16], [3, None, 40, 0, 1, 1, 1, 300], [1]):
            d = datas(lens, 4 + residue)
            data, off, none = md.pack(d)
            got = gather(emul, tmp_path, len(d), data, off, none, None, len(d), arena=False, grid=2, dst_base=used)
            assert md.unpack(*got) == d


@pytest.mark.parametrize("shift", range(4))
def test_source_offsets_at_every_residue_mod_4(emul, tmp_path, shift):
    d = datas([16, 48, 17, 100, 31], 5)
    data, off, none = md.pack(d)
    pad = np.concatenate([np.full(shift, 0xEE, np.uint8), data])       # every range starts `shift` bytes later
    for arena in (False, True):
        got = gather(emul, tmp_path, len(d), pad, off + shift, none, np.arange(len(d)) if arena else None, len(d), arena=arena)
        assert md.unpack(*got) == d
    for start in range(16):      # and an arena source at every residue mod 16: the two-piece funnel shift
        src = np.random.default_rng(start).integers(0, 256, start + 64, dtype=np.uint8)
        got = gather(emul, tmp_path, 1, src, np.array([start, start + 64], np.int64), None, [0], 1, arena=True)
        assert got[0].tobytes() == src[start:].tobytes()


def test_repeated_and_descending_indices(emul, tmp_path):
    d = datas(LENS[:12] * 2, 6)
    data, off, none = md.pack(d)
    n = len(d)
    rng = np.random.default_rng(7)
    for idx in (np.arange(n)[::-1], rng.integers(0, n, 3 * n), np.full(50, 9), np.array([0, 0, n - 1, n - 1])):
        got = gather(emul, tmp_path, len(idx), data, off, none, idx, n, arena=True, grid=2)
        assert md.unpack(*got) == [d[i] for i in idx]


def test_one_workgroup_for_a_stream_of_many_trips(emul, tmp_path):
    d = datas([60000, 0, 60000, 1, 4095] + [100] * 300, 8)       # ~ 154 KB: 38 trips of one workgroup
    data, off, none = md.pack(d)
    K = len(d)
    assert md.unpack(*gather(emul, tmp_path, K, data, off, none, None, K, arena=False, grid=1, dst_base=3)) == d
    assert md.unpack(*gather(emul, tmp_path, K, data, off, none, np.arange(K), K, arena=True, grid=1)) == d


def test_no_slot_and_one_slot(emul, tmp_path):
    data, off, none = md.pack([b"abc"])
    assert md.unpack(*gather(emul, tmp_path, 0, data, off, none, np.zeros(0, np.int32), 1, arena=True)) == []
    assert md.unpack(*gather(emul, tmp_path, 0, None, np.zeros(1, np.int64), None, None, 0, arena=False, dst_base=9)) == []
    assert md.unpack(*gather(emul, tmp_path, 1, data, off, none, [0], 1, arena=True)) == [b"abc"]
    assert md.unpack(*gather(emul, tmp_path, 1, data, off, np.array([1], np.uint8), None, 1, arena=False)) == [None]
    assert md.unpack(*gather(emul, tmp_path, 3, None, None, None, None, 3, arena=False, dst_base=2)) == [None] * 3


def test_offsets_and_indices_that_lead_nowhere(emul, tmp_path):
    K = 12
    d = datas([10] * K, 9)
    data, off, none = md.pack(d)
    bad = off.copy()
    bad[3] = 45                 # decreasing: slot 3 is [45, 40)
    bad[6] = -5                 # negative: slots 5 and 6
    bad[9] = 10 ** 12           # beyond the buffer: slots 8 and 9
    bad[12] = 121               # one past the end: slot 11
    gather(emul, tmp_path, K, data, bad, none, None, K, arena=False, expect_bad=6)
    long = np.zeros(md.MAX_DATA + 1, np.uint8)
    gather(emul, tmp_path, 1, long, np.array([0, md.MAX_DATA + 1], np.int64), None, None, 1, arena=False, expect_bad=1)
    for idx in ([0, K], [-1, 2], [2 ** 31 - 1], [-2 ** 31]):
        gather(emul, tmp_path, len(idx), data, off, none, idx, K, arena=True, expect_bad=1)


def test_fold_ok_follows_the_model(emul, tmp_path):
    K = 300
    rng = np.random.default_rng(10)
    off = np.concatenate([[0], np.cumsum(rng.integers(0, 50, K))]).astype(np.int64)
    off[[5, 70, 256, 299]] = [-1, 10 ** 15, 3, 0]
    nbytes = int(off[-1]) - 7
    ok = (rng.random(K) < 0.8).astype(np.uint8) * 3
    for use_ok, use_off in ((1, 1), (0, 1), (1, 0), (0, 0)):
        blob = np.array([1, K, use_ok | 2 * use_off, nbytes], np.int64).tobytes()
        blob += (ok.tobytes() if use_ok else b"") + (off.tobytes() if use_off else b"")
        raw = run(emul, tmp_path, blob)
        got, total = np.frombuffer(raw, np.uint8, K), int(np.frombuffer(raw, np.uint64, 1, K)[0])
        want = md.fold_ok(K, ok if use_ok else None, off if use_off else None, nbytes)
        assert np.array_equal(got, want) and len(raw) == K + 8
        assert total == md.fold_sum(K, want, off if use_off else None)
    assert 0 < md.fold_ok(K, ok, off, nbytes).sum() < ok.astype(bool).sum()


def test_slots_follow_the_model(emul, tmp_path):
    rng = np.random.default_rng(11)
    K, first_new, A = 700, 40, 300
    index_out = np.concatenate([first_new + rng.permutation(A), rng.integers(-8, first_new, K - A - 50),
                                first_new + rng.integers(0, A, 50)]).astype(np.int32)     # 50 repeats of stored events
    index_out[:A + 50] = rng.permutation(index_out[:A + 50])
    blob = np.array([2, K, first_new, A], np.int64).tobytes() + index_out.tobytes()
    got = np.frombuffer(run(emul, tmp_path, blob), np.int32)
    assert np.array_equal(got, md.slots(index_out, first_new, A))
    assert sorted(set(got.tolist())) == sorted(got.tolist()) and (got < K).all()
