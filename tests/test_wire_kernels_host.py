"""CPU: the kernels of csrc/wire.hip.h run thread by thread on the host (tests/wire_emul.cpp, a stand-alone program built
with AddressSanitizer and UBSan) against tests/model_wire.py.  The writer: the message exact, a canary behind its end
untouched, an unencodable event named and nothing written.  The reader: the model's message back to the arrays, and every
malformed message refused without an access outside the message (whose buffer has its exact size).  The host side of the
library is NOT covered here: tests/test_gpu_wire.py does that on the GPU, with the malformed messages that passed here."""
import os
import pickle
import shutil
import struct
import subprocess

import numpy as np
import pytest

import model_pack as mp
import model_wire as mw
from conftest import ROOT

CANARY = 37


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("wire_emul") / "wire_emul")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "wire_emul.cpp"), "-o", exe])
    return exe


def events(K, n, seed, roots=0.3):
    rng = np.random.default_rng(seed)
    a = dict(head=rng.integers(0, 256, 32, dtype=np.uint8), keys=rng.integers(0, 256, (n, 32), dtype=np.uint8),
             ids=rng.integers(0, 256, (K, 32), dtype=np.uint8), sp=rng.integers(0, 256, (K, 32), dtype=np.uint8),
             op=rng.integers(0, 256, (K, 32), dtype=np.uint8), sig=rng.integers(0, 256, (K, 64), dtype=np.uint8),
             arity=np.where(rng.random(K) < roots, 0, 2).astype(np.uint8), creator=rng.integers(0, n, K).astype(np.int32),
             t=1.7e9 + rng.random(K))
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


def model(a, mod="swirld", qual="Event"):
    return mw.pack_message(a["head"], a["keys"], a["ids"], a["sp"], a["op"], a["arity"], a["creator"], a["t"], a["sig"], a.get("data"),
                           a.get("data_off"), a.get("data_none"), mod, qual)


def run(emul, mode, src, dst):
    r = subprocess.run([emul, mode, src, dst], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-3000:]
    return open(dst, "rb").read()


def write(emul, tmp_path, a, grid=3, mod="swirld", qual="Event"):
    """The emulated writer against the model; returns the message, or the model's -(index + 1)."""
    K, n = len(a["arity"]), len(a["keys"])
    has_data = "data_off" in a
    exp = model(a, mod, qual)
    cap = (len(exp) if isinstance(exp, bytes) else mw.bound(K, len(a["data"]) if has_data else 0, mod, qual)) + CANARY
    pre = mw.prefix(mod, qual)
    flags = (1 if has_data else 0) | (2 if "data_none" in a else 0)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([K, n, flags, len(a["data"]) if has_data else 0, grid, len(pre), cap], np.int64).tobytes())
        for name, dt in (("head", np.uint8), ("ids", np.uint8), ("sp", np.uint8), ("op", np.uint8), ("arity", np.uint8), ("creator", np.int32),
                         ("t", np.float64), ("sig", np.uint8), ("keys", np.uint8)):
            f.write(np.ascontiguousarray(a[name], dt).tobytes())
        f.write(pre)
        if has_data:
            f.write(np.ascontiguousarray(a["data_off"], np.int64).tobytes())
            f.write(a["data"].tobytes())
        if "data_none" in a:
            f.write(a["data_none"].tobytes())
    raw = run(emul, "W", src, dst)
    msg_len, bad = struct.unpack_from("<qq", raw)
    body = np.frombuffer(raw, np.uint8, cap, 16)
    assert len(raw) == 16 + cap
    if not isinstance(exp, bytes):
        assert msg_len == -1 and bad == -exp - 1
        assert (body == 0xA5).all(), "an unbuildable message was written"
        return exp
    assert msg_len == len(exp) and bad == -1
    diff = np.flatnonzero(body[:msg_len] != np.frombuffer(exp, np.uint8))
    assert diff.size == 0, "first differing byte at %d of %d" % (diff[0], msg_len)
    assert (body[msg_len:] == 0xA5).all(), "bytes at or behind the message's end were written"
    return exp


def read(emul, tmp_path, msg, keys, mod="swirld", qual="Event", cap_events=None, cap_data=None):
    """The emulated reader: (rc, n_events, n_data, arrays or None)."""
    pre = mw.prefix(mod, qual)
    keys = np.asarray(keys, np.uint8).reshape(-1, 32)
    if cap_events is None:
        cap_events = len(msg) // 150 + 1
    if cap_data is None:
        cap_data = len(msg)
    src, dst = str(tmp_path / "rin.bin"), str(tmp_path / "rout.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(msg), len(keys), len(pre), cap_events, cap_data], np.int64).tobytes())
        f.write(keys.tobytes())
        f.write(pre)
        f.write(bytes(msg))
    raw = run(emul, "R", src, dst)
    rc, K, nd = struct.unpack_from("<qqq", raw)
    if rc != 0 or K < 0:
        assert len(raw) == 24
        return rc, K, nd, None
    pos = 24
    out = {}
    for name, count, dt in (("head", 32, np.uint8), ("ids", K * 32, np.uint8), ("sp", K * 32, np.uint8), ("op", K * 32, np.uint8),
                            ("arity", K, np.uint8), ("creator", K, np.int32), ("t", K, np.float64), ("sig", K * 64, np.uint8),
                            ("data_off", K + 1, np.int64), ("data_none", K, np.uint8), ("data", nd, np.uint8)):
        out[name] = np.frombuffer(raw, dt, count, pos)
        pos += out[name].nbytes
    assert pos == len(raw)
    for name in ("ids", "sp", "op"):
        out[name] = out[name].reshape(K, 32)
    out["sig"] = out["sig"].reshape(K, 64)
    return rc, K, nd, out


def same_as_model(got, msg, keys, mod="swirld", qual="Event"):
    want = mw.unpack_message(msg, keys, mod, qual)
    assert want is not None
    for name, w in want.items():
        g = got[name]
        if name == "t":
            g, w = g.view(np.uint64), w.view(np.uint64)
        assert np.array_equal(g, w), name


def refused(emul, tmp_path, msg, keys, **kw):
    assert mw.unpack_message(msg, keys, kw.get("mod", "swirld"), kw.get("qual", "Event")) is None
    rc, K, _, _ = read(emul, tmp_path, msg, keys, **kw)
    assert (rc, K) == (0, -1)


# ---------------------------------------------------------------------------------------------------------------- the writer

@pytest.mark.parametrize("K", [0, 1, 2, 65, 1000, 1025, 2049])
def test_writer_event_counts_and_root_mixes(emul, tmp_path, K):
    for roots in (1.0, 0.0, 0.4):
        write(emul, tmp_path, events(K, 5, 10 + K, roots), grid=2)


def test_writer_class_names_and_member_counts(emul, tmp_path):
    a = events(300, 70, 4)
    write(emul, tmp_path, a, mod="m", qual="Q")
    write(emul, tmp_path, a, mod="py-swirld_amd.node", qual="Event")
    write(emul, tmp_path, a, mod="x" * 255, qual="é" * 127 + "y")


def test_writer_data_lengths_and_the_unencodable_length(emul, tmp_path):
    lens = [0, 1, 31, 32, 255, 256, 257, 4095, 60000, 5, 0]
    K = len(lens)
    none = np.zeros(K, np.uint8)
    none[[2, 9]] = 1
    for roots in (0.0, 1.0):
        write(emul, tmp_path, with_data(events(K, 5, 6, roots), lens, 7, none), grid=4)
    write(emul, tmp_path, with_data(events(K, 5, 8), lens, 9), grid=7)           # without the None flags
    lens[3] = 60001
    assert write(emul, tmp_path, with_data(events(K, 5, 6), lens, 7, none)) == -4
    assert write(emul, tmp_path, with_data(events(K, 5, 6), lens, 7)) == -4


def test_writer_bad_arity_and_creator(emul, tmp_path):
    for field, idx, val in (("arity", 17, 1), ("arity", 100, 3), ("arity", 199, 255), ("creator", 5, -1), ("creator", 64, 6), ("creator", 0, 2 ** 31 - 1)):
        a = events(200, 6, 11)
        a[field][idx] = val
        assert write(emul, tmp_path, a) == -(idx + 1)
    a = events(200, 6, 11)
    a["arity"][[150, 30]] = 1
    a["creator"][90] = -1
    assert write(emul, tmp_path, a) == -31       # the lowest index is named


def test_writer_data_offsets_that_lead_nowhere(emul, tmp_path):
    K = 12
    for at, val, first in ((3, 45, 3), (6, -5, 5), (9, 10 ** 12, 8), (12, 121, 11)):
        a = with_data(events(K, 5, 12), [10] * K, 13)
        a["data_off"][at] = val
        assert write(emul, tmp_path, a) == -(first + 1)


def test_writer_grid_of_one_workgroup(emul, tmp_path):
    write(emul, tmp_path, events(1000, 9, 14, 0.1), grid=1)
    write(emul, tmp_path, with_data(events(3, 5, 15), [60000, 0, 60000], 16), grid=1)


# ---------------------------------------------------------------------------------------------------------------- the reader

def sample(K=6, seed=40):
    lens = [0, 0, 5, 256, 0, 300] + [7] * (K - 6)
    none = [1, 0, 0, 0, 1, 0] + [0] * (K - 6)
    a = with_data(events(K, 5, seed), lens[:K], seed + 1, none[:K])
    a["arity"][:6] = [0, 2, 0, 2, 2, 0]
    return a


@pytest.mark.parametrize("K", [0, 1, 2, 65, 1000, 1025])
def test_reader_round_trip(emul, tmp_path, K):
    a = sample(K) if K >= 6 else with_data(events(K, 5, 50 + K, 0.5), [3, 0][:K], 51, [0, 1][:K])
    a["keys"][3] = a["keys"][1]
    msg = model(a, "m", "Q")
    rc, k, nd, got = read(emul, tmp_path, msg, a["keys"], "m", "Q", cap_events=K, cap_data=len(a["data"]))
    assert (rc, k, nd) == (0, K, len(a["data"]))
    same_as_model(got, msg, a["keys"], "m", "Q")
    other = a["keys"].copy()
    other[0] ^= 1
    rc, k, nd, got = read(emul, tmp_path, msg, other, "m", "Q")
    same_as_model(got, msg, other, "m", "Q")
    assert (got["creator"][a["creator"] == 0] == -1).all()


def constant_positions(msg, K, mod="swirld", qual="Event"):
    """(header, per-record, trailer) positions of the bytes that are no field's content."""
    u = mw.unpack_message(msg, np.zeros((1, 32), np.uint8), mod, qual)
    t0 = len(mw.prefix(mod, qual)) + 8
    off = np.frombuffer(msg, "<u8", K + 1, t0).astype(np.int64)
    q = t0 + 8 * (K + 1)
    header = list(range(0, q + 3)) + [q + 35, q + 36]
    recs = []
    for i in range(K):
        s = int(off[i])
        dl = int(u["data_off"][i + 1] - u["data_off"][i])
        dsz = 1 if u["data_none"][i] else (2 + dl if dl < 256 else 5 + dl)
        c = [s, s + 1, s + 34, s + 35, s + 36] + list(range(s + 37, s + 37 + dsz - dl))
        p = s + 37 + dsz
        if u["arity"][i]:
            c += [p, p + 1, p + 34, p + 35, p + 68]
            p += 69
        else:
            c += [p]
            p += 1
        c += [p, p + 9, p + 10, p + 43, p + 44, p + 109, p + 110]
        recs.append(c)
    return header, recs, [len(msg) - 3, len(msg) - 2, len(msg) - 1]


def test_reader_refuses_a_flipped_constant(emul, tmp_path):
    a = sample()
    msg = model(a)
    header, recs, trailer = constant_positions(msg, 6)
    # every constant of the header, of a root and a non-root record of each data shape, and of the trailer
    for pos in header + recs[0] + recs[1] + recs[2] + recs[3] + trailer:
        bad = bytearray(msg)
        bad[pos] ^= 0x01
        refused(emul, tmp_path, bytes(bad), a["keys"])
    bad = bytearray(msg)
    bad[recs[5][-1] - 50] ^= 0x80            # a field's content is no constant
    assert read(emul, tmp_path, bytes(bad), a["keys"])[1] == 6


def test_reader_refuses_truncation(emul, tmp_path):
    a = sample(20)
    msg = model(a)
    for cut in range(0, len(msg), 97):
        refused(emul, tmp_path, msg[:cut], a["keys"])
    refused(emul, tmp_path, msg[:-1], a["keys"])
    refused(emul, tmp_path, msg + b".", a["keys"])


def test_reader_refuses_a_bad_table(emul, tmp_path):
    a = sample(20)
    msg = model(a)
    K = 20
    t0 = len(mw.prefix("swirld", "Event")) + 8
    off = np.frombuffer(msg, "<u8", K + 1, t0).copy()

    def with_table(o):
        return msg[:t0] + np.asarray(o, "<u8").tobytes() + msg[t0 + 8 * (K + 1):]
    assert with_table(off) == msg
    cases = []
    o = off.copy(); o[7], o[8] = off[8], off[7]; cases.append(o)            # decreases
    o = off.copy(); o[9] = o[8]; cases.append(o)                            # not strictly increasing
    o = off.copy(); o[10] = len(msg) + 1000; cases.append(o)                # points beyond the message
    o = off.copy(); o[10] = 2 ** 63 + 5; cases.append(o)
    o = off.copy(); o[K] = 2 ** 64 - 3; cases.append(o)
    o = off.copy(); o[5] += 40; cases.append(o)                             # into the middle of a record
    o = off.copy(); o[5] += 1; cases.append(o)                              # one byte off
    o = off.copy(); o[5] -= 1; cases.append(o)
    o = off.copy(); o[0] -= 1; cases.append(o)
    o = off.copy(); o[K] -= 1; cases.append(o)
    o = off.copy(); o[1:K] = off[0] + 1 + np.arange(K - 1); cases.append(o)     # records shorter than any record
    for o in cases:
        refused(emul, tmp_path, with_table(o), a["keys"])
    # a table length that promises more entries than the message holds, and one that is no multiple of 8
    for tb in (8 * (K + 2), 8 * (K + 1) + 1, 0, 2 ** 64 - 8, 8 * 10 ** 6):
        refused(emul, tmp_path, msg[:t0 - 8] + struct.pack("<Q", tb) + msg[t0:], a["keys"])


def test_reader_refuses_unencodable_lengths_and_other_pickles(emul, tmp_path):
    a = with_data(events(3, 5, 60, 0.5), [10, 60000, 10], 61)
    msg = bytearray(model(a))
    t0 = len(mw.prefix("swirld", "Event")) + 8
    off = np.frombuffer(bytes(msg), "<u8", 4, t0).astype(np.int64)
    # a data length of 60 001: one more data byte, the lengths and the table adjusted to it
    s = int(off[1])
    assert msg[s + 37] == ord("B")
    long = msg[:s + 38] + struct.pack("<I", 60001) + msg[s + 42:s + 42 + 60000] + b"x" + msg[s + 42 + 60000:]
    long[t0 + 16:t0 + 32] = np.asarray(off[2:] + 1, "<u8").tobytes()
    refused(emul, tmp_path, bytes(long), a["keys"])
    # 'B' for a length below 256 is not what the writer writes
    s = int(off[0])
    short = msg[:s + 37] + b"B" + struct.pack("<I", 10) + msg[s + 39:]
    short[t0 + 8:t0 + 32] = np.asarray(off[1:] + 3, "<u8").tobytes()
    with mp.event_class("swirld", "Event"):
        assert pickle.loads(bytes(short)) == pickle.loads(bytes(msg))     # a pickle of the same value, yet not canonical
    refused(emul, tmp_path, bytes(short), a["keys"])
    # pickle.dumps of the same value; the right bytes under another class name
    with mp.event_class("swirld", "Event"):
        framed = pickle.dumps(pickle.loads(bytes(msg)), protocol=4)
    refused(emul, tmp_path, framed, a["keys"])
    refused(emul, tmp_path, bytes(msg), a["keys"], mod="swirle", qual="Event")
    refused(emul, tmp_path, bytes(msg), a["keys"], mod="swirld", qual="Even")
    refused(emul, tmp_path, model(a, "swirld2", "Event"), a["keys"])
    refused(emul, tmp_path, b"", a["keys"])


def test_reader_capacities(emul, tmp_path):
    a = sample(20)
    msg = model(a)
    nd = len(a["data"])
    rc, K, need, _ = read(emul, tmp_path, msg, a["keys"], cap_events=19, cap_data=nd)
    assert (rc, K) == (-34, 20) and need >= nd
    rc, K, need, _ = read(emul, tmp_path, msg, a["keys"], cap_events=20, cap_data=nd - 1)
    assert (rc, K, need) == (-34, 20, nd)
    rc, K, need, _ = read(emul, tmp_path, msg, a["keys"], cap_events=20, cap_data=0)
    assert (rc, K, need) == (-34, 20, nd)
    rc, K, need, got = read(emul, tmp_path, msg, a["keys"], cap_events=20, cap_data=nd)
    assert (rc, K, need) == (0, 20, nd)


def refusal_cases():
    """[(name, message)] over sample(20)'s keys under swirld.Event: the malformed messages tests/test_gpu_wire.py hands to
    the library on the GPU.  test_reader_refuses_the_cases_of_the_gpu_suite runs every one of them here first."""
    a = sample(20)
    msg = model(a)
    K = 20
    t0 = len(mw.prefix("swirld", "Event")) + 8
    off = np.frombuffer(msg, "<u8", K + 1, t0).copy()
    header, recs, trailer = constant_positions(msg, K)
    cases = []
    for pos in header[::5] + recs[0] + recs[1] + recs[3] + trailer:
        bad = bytearray(msg)
        bad[pos] ^= 0x01
        cases.append(("flip %d" % pos, bytes(bad)))
    cases += [("cut %d" % cut, msg[:cut]) for cut in range(0, len(msg), 97)]

    def with_table(name, idx, val):
        o = off.copy()
        o[idx] = val
        cases.append((name, msg[:t0] + o.astype("<u8").tobytes() + msg[t0 + 8 * (K + 1):]))
    with_table("decreasing", 8, off[6])
    with_table("beyond", 10, len(msg) + 1000)
    with_table("huge", 10, 2 ** 63 + 5)
    with_table("middle", 5, off[5] + 40)
    with_table("one off", 5, off[5] + 1)
    with_table("last", K, off[K] - 1)
    b = with_data(events(3, 5, 60, 0.5), [10, 60000, 10], 61)
    b["keys"] = a["keys"]
    m3 = bytearray(model(b))
    o3 = np.frombuffer(bytes(m3), "<u8", 4, t0).astype(np.int64)
    s = int(o3[1])
    long = m3[:s + 38] + struct.pack("<I", 60001) + m3[s + 42:s + 42 + 60000] + b"x" + m3[s + 42 + 60000:]
    long[t0 + 16:t0 + 32] = np.asarray(o3[2:] + 1, "<u8").tobytes()
    cases.append(("60001", bytes(long)))
    with mp.event_class("swirld", "Event"):
        cases.append(("pickle.dumps", pickle.dumps(pickle.loads(msg), protocol=4)))
    cases.append(("other class", model(a, "swirld", "Evenu")))
    cases.append(("empty", b""))
    return a, msg, cases


def test_reader_refuses_the_cases_of_the_gpu_suite(emul, tmp_path):
    a, msg, cases = refusal_cases()
    assert read(emul, tmp_path, msg, a["keys"])[1] == 20
    assert len(cases) > 60
    for name, bad in cases:
        assert mw.unpack_message(bad, a["keys"]) is None, name
        rc, K, _, _ = read(emul, tmp_path, bad, a["keys"])
        assert (rc, K) == (0, -1), name
