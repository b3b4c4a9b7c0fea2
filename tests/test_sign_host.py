"""CPU: the functions the signing kernels execute (py-swirld_amd/csrc/sign.hip.h), compiled for the HOST by g++
(tests/sign_host.cpp) and run against libsodium 1.0.18, Python integers, pickle and hashlib: key expansion is
crypto_sign_seed_keypair, sc_muladd handles a clamped scalar above L, signatures are crypto_sign_detached bit for bit at the
padding edges of both SHA-512 inputs, and the segment iterator over the pickle template gives the signature and the id of
the real pickle.dumps bytes — for roots and two-parent events, every data shape, odd timestamps and both class headers.  The
same results from a stand-alone program built with the address and undefined-behaviour sanitizers.  The GPU run is
tests/test_gpu_sign.py."""
import ctypes as C
import hashlib
import os
import pickle
import random
import struct
import subprocess

import hostlibs
import model_pack
from test_crypto_host import L_ORDER, load_sodium

HERE = os.path.dirname(os.path.abspath(__file__))
SIGN_SO = os.path.join(HERE, "libsws_host.so")
SIGN_SRC = os.path.join(HERE, "sign_host.cpp")
SIGN_MAIN = os.path.join(HERE, "sign_host_main")
SIGN_MAIN_SRC = os.path.join(HERE, "sign_host_main.cpp")
HDRS = [os.path.join(hostlibs.CSRC, h) for h in ("sign.hip.h", "validate.hip.h", "crypto.hip.h", "tmpl.hip.h")]

LONG_NAME = "E" + "v" * 254          # a 255-byte qualified name
CLASSES = [("swirld", "Event"), ("swirld", LONG_NAME)]
DATA_LENGTHS = [None, 0, 1, 255, 256, 257, 60000]
NAN_BITS = 0x7ff8000000000123
TIMES = [0.0, -0.0, 1e300, struct.unpack("<d", struct.pack("<Q", NAN_BITS))[0]]


def build_sign_host():
    if hostlibs._stale(SIGN_SO, SIGN_SRC, *HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", SIGN_SRC, "-o", SIGN_SO])
    return SIGN_SO


def build_sign_main():
    if hostlibs._stale(SIGN_MAIN, SIGN_MAIN_SRC, *HDRS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-fno-omit-frame-pointer", SIGN_MAIN_SRC, "-o", SIGN_MAIN])
    return SIGN_MAIN


def sodium():
    sod = load_sodium()
    assert sod is not None, "libsodium is part of the image"
    return sod


def keypair(sod, seed):
    pk, sk = C.create_string_buffer(32), C.create_string_buffer(64)
    assert sod.crypto_sign_seed_keypair(pk, sk, seed) == 0
    return pk.raw, sk


def sodium_sign(sod, sk, m):
    sig = C.create_string_buffer(64)
    assert sod.crypto_sign_detached(sig, None, m, C.c_ulonglong(len(m)), sk) == 0
    return sig.raw


def rand_bytes(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n)) if n < 4096 else rng.getrandbits(8 * n).to_bytes(n, "little")


def event_cases(rng):
    """(seed, mod, qual, data, parents, t_bits) for every combination the issue lists."""
    cases = []
    for mod, qual in CLASSES:
        for two in (False, True):
            for dl in DATA_LENGTHS:
                for t in TIMES:
                    data = None if dl is None else rand_bytes(rng, dl)
                    p = (rand_bytes(rng, 32), rand_bytes(rng, 32)) if two else ()
                    cases.append((rand_bytes(rng, 32), mod, qual, data, p, struct.unpack("<Q", struct.pack("<d", t))[0]))
    return cases


def expected_event(sod, case):
    """Signature and id by the host route: pickle.dumps of the real namedtuple, libsodium, hashlib."""
    seed, mod, qual, data, p, t_bits = case
    t = struct.unpack("<d", struct.pack("<Q", t_bits))[0]
    pk, sk = keypair(sod, seed)
    with model_pack.event_class(mod, qual) as Event:
        m = pickle.dumps((data, p, t, pk), protocol=4)
        sig = sodium_sign(sod, sk, m)
        whole = pickle.dumps(Event(data, p, t, pk, sig), protocol=4)
    assert struct.pack(">Q", t_bits) in m, "the timestamp's bit pattern survives the pickler"
    return sig, hashlib.blake2b(whole, digest_size=32).digest()


def test_key_expansion_is_libsodiums():
    sod = sodium()
    L = C.CDLL(build_sign_host())
    rng = random.Random(21)
    a, prefix, pk = (C.create_string_buffer(32) for _ in range(3))
    for _ in range(64):
        seed = rand_bytes(rng, 32)
        L.sws_host_expand(seed, a, prefix, pk)
        exp_pk, _ = keypair(sod, seed)
        h = bytearray(hashlib.sha512(seed).digest())
        h[0] &= 248
        h[31] = (h[31] & 127) | 64
        assert pk.raw == exp_pk
        assert a.raw == bytes(h[:32]) and prefix.raw == bytes(h[32:])


def test_sc_muladd_against_python_integers():
    L = C.CDLL(build_sign_host())
    rng = random.Random(22)
    out = C.create_string_buffer(32)

    def clamped():
        return (rng.getrandbits(256) & ~7 & (2 ** 255 - 1)) | 2 ** 254

    scalars = [0, 1, L_ORDER - 1] + [rng.randrange(L_ORDER) for _ in range(6)]
    secrets = [2 ** 254, 2 ** 255 - 8] + [clamped() for _ in range(6)]
    assert all(a >= L_ORDER for a in secrets), "a clamped scalar lies above L"
    for r in scalars:
        for k in scalars:
            for a in secrets:
                L.sws_host_sc_muladd(r.to_bytes(32, "little"), k.to_bytes(32, "little"), a.to_bytes(32, "little"), out)
                assert int.from_bytes(out.raw, "little") == (r + k * a) % L_ORDER, (r, k, a)


def test_signatures_of_raw_messages_are_libsodiums():
    sod = sodium()
    L = C.CDLL(build_sign_host())
    rng = random.Random(23)
    sig = C.create_string_buffer(64)
    for n in range(301):   # 32 + n and 64 + n cross 111/112/127/128/239/240/255/256
        seed, m = rand_bytes(rng, 32), rand_bytes(rng, n)
        _, sk = keypair(sod, seed)
        L.sws_host_sign_raw(seed, m, C.c_ulonglong(n), sig)
        assert sig.raw == sodium_sign(sod, sk, m), n


def test_template_hasher_against_pickle_libsodium_and_hashlib():
    sod = sodium()
    L = C.CDLL(build_sign_host())
    cases = event_cases(random.Random(24))
    assert len(cases) == 2 * 2 * 7 * 4
    sig, eid = C.create_string_buffer(64), C.create_string_buffer(32)
    for case in cases:
        seed, mod, qual, data, p, t_bits = case
        hdr = model_pack.class_header(mod, qual)
        L.sws_host_sign_event(seed, hdr, len(hdr), data if data else b"\0", -1 if data is None else len(data), 2 if p else 0,
                              p[0] if p else bytes(32), p[1] if p else bytes(32), C.c_ulonglong(t_bits), sig, eid)
        exp_sig, exp_id = expected_event(sod, case)
        what = (qual[:8], len(p), None if data is None else len(data), hex(t_bits))
        assert sig.raw == exp_sig, what
        assert eid.raw == exp_id, what


def test_sanitized_standalone_program_gives_the_same_signatures(tmp_path):
    """sign_host_main.cpp with -fsanitize=address,undefined, as a child process, on a subset: the raw messages at the
    padding edges and one event of every data shape — a read outside a segment or an undefined shift in the host build of
    the kernels' functions ends the program instead."""
    sod = sodium()
    exe = build_sign_main()
    rng = random.Random(25)
    blob, exp = [], []
    raw = [0, 1, 47, 48, 63, 64, 79, 80, 95, 96, 175, 176, 191, 192, 300]
    for n in raw:
        seed, m = rand_bytes(rng, 32), rand_bytes(rng, n)
        _, sk = keypair(sod, seed)
        blob.append(struct.pack("<i", 0) + seed + struct.pack("<q", n) + m)
        exp.append(sodium_sign(sod, sk, m).hex())
    events = [c for i, c in enumerate(event_cases(rng)) if i % 4 == (i // 4) % 4]   # one timestamp per (class, arity, data)
    assert len(events) == 28
    for case in events:
        seed, mod, qual, data, p, t_bits = case
        hdr = model_pack.class_header(mod, qual)
        blob.append(struct.pack("<i", 1) + seed + struct.pack("<i", len(hdr)) + hdr + struct.pack("<i", -1 if data is None else len(data)) + (data or b"") +
                    struct.pack("<i", 2 if p else 0) + (p[0] if p else bytes(32)) + (p[1] if p else bytes(32)) + struct.pack("<Q", t_bits))
        s, i = expected_event(sod, case)
        exp.append(s.hex() + i.hex())
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(blob)) + b"".join(blob))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == exp
