"""CPU: the functions the one-wave signer executes (py-swirld_amd/csrc/turn.hip.h), compiled for the HOST by g++
(tests/turn_sign_host.cpp) with a "wave" of 64 array entries.  The cooperative base multiplication — one radix-16 digit per
lane, a six-level butterfly of complete additions — equals sign.hip.h's one-lane base_mult and a scalar multiplication in
Python integers, in every lane, at the edges of the recoder's carry chain; the file's own scalar reduction (32 bits per step)
equals Python integers and the bitwise one; whole signatures and ids equal libsodium, pickle.dumps and hashlib for every data
shape, roots and two-parent events and both class headers.  The same results from a stand-alone program built with the
address and undefined-behaviour sanitizers.  The GPU run is tests/test_gpu_turn.py."""
import ctypes as C
import os
import random
import struct
import subprocess

import hostlibs
import model_pack
from test_crypto_host import L_ORDER
from test_sign_host import CLASSES, DATA_LENGTHS, event_cases, expected_event, keypair, rand_bytes, sodium

HERE = os.path.dirname(os.path.abspath(__file__))
TURN_SO = os.path.join(HERE, "libswt_host.so")
TURN_SRC = os.path.join(HERE, "turn_sign_host.cpp")
TURN_MAIN = os.path.join(HERE, "turn_sign_host_main")
TURN_MAIN_SRC = os.path.join(HERE, "turn_sign_host_main.cpp")
HDRS = [os.path.join(hostlibs.CSRC, h) for h in ("turn.hip.h", "sign.hip.h", "validate.hip.h", "crypto.hip.h", "tmpl.hip.h")]

P = 2 ** 255 - 19
D = -121665 * pow(121666, P - 2, P) % P
BY = 4 * pow(5, P - 2, P) % P
BX = 15112221349535400772501151409588531511454012693041857206046113283949847762202


def build_turn_host():
    if hostlibs._stale(TURN_SO, TURN_SRC, *HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", TURN_SRC, "-o", TURN_SO])
    return TURN_SO


def build_turn_main():
    if hostlibs._stale(TURN_MAIN, TURN_MAIN_SRC, *HDRS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-fno-omit-frame-pointer", TURN_MAIN_SRC, "-o", TURN_MAIN])
    return TURN_MAIN


def pt_add(a, b):
    """Addition on -x^2 + y^2 = 1 + d x^2 y^2 in extended coordinates (X : Y : Z : T), T = XY / Z: the unified law, complete
    on this curve, so it doubles too."""
    (x1, y1, z1, t1), (x2, y2, z2, t2) = a, b
    A, B = (y1 - x1) * (y2 - x2) % P, (y1 + x1) * (y2 + x2) % P
    C, Z = 2 * D * t1 * t2 % P, 2 * z1 * z2 % P
    E, F, G, H = B - A, Z - C, Z + C, B + A
    return E * F % P, G * H % P, F * G % P, E * H % P


def base_mult_py(s):
    """encode([s]B) in Python integers: double and add from the lowest bit, one inversion at the end."""
    r, q = (0, 1, 1, 0), (BX, BY, 1, BX * BY % P)
    while s:
        if s & 1:
            r = pt_add(r, q)
        q = pt_add(q, q)
        s >>= 1
    zi = pow(r[2], P - 2, P)
    x, y = r[0] * zi % P, r[1] * zi % P
    return (y | (x & 1) << 255).to_bytes(32, "little")


def edge_scalars():
    """The scalars the recoder's carry chain can go wrong at, then 300 random ones below 2^255 with top nibble <= 7.  A top
    nibble of 8 without a carry into it is the digit +8 (every nibble 8; 8 * 16^63 = 2^255): the largest the last digit takes."""
    all8 = sum(8 << 4 * i for i in range(64))
    longest = sum(0xF << 4 * i for i in range(63)) | 7 << 252   # the carry runs through every digit, the last one absorbs it
    s = [0, 1, 8, 9, L_ORDER - 1, 2 ** 252, all8, longest]
    s += [8 * 16 ** k for k in (0, 31, 62, 63)]
    rng = random.Random(31)
    rnd = [rng.getrandbits(255) for _ in range(300)]
    assert all(0 <= x < 2 ** 255 and x >> 252 <= 7 for x in rnd)
    return s + rnd


def test_python_reference_is_ed25519():
    sod = sodium()
    rng = random.Random(30)
    for _ in range(4):
        seed = rand_bytes(rng, 32)
        pk, _ = keypair(sod, seed)
        import hashlib
        h = bytearray(hashlib.sha512(seed).digest())
        h[0] &= 248
        h[31] = (h[31] & 127) | 64
        assert base_mult_py(int.from_bytes(h[:32], "little")) == pk


def test_cooperative_base_mult_against_one_lane_and_python_integers():
    L = C.CDLL(build_turn_host())
    coop, serial = C.create_string_buffer(32), C.create_string_buffer(32)
    for k, s in enumerate(edge_scalars()):
        # every lane's sum for the edge cases and the first random scalars, lanes 0, 21, 42 and 63 for the rest
        differ = L.swt_host_base_mult(s.to_bytes(32, "little"), coop, serial, 1 if k < 24 else 21)
        assert differ == 0, "every lane of the butterfly ends with the whole sum (%x)" % s
        assert coop.raw == serial.raw, hex(s)
        assert coop.raw == base_mult_py(s), hex(s)


def test_every_lane_holds_its_digit_of_the_serial_recoding():
    """The recoder in Python integers: digits in [-7, 8], no carry out of the last one, and lane i holds digit i."""
    L = C.CDLL(build_turn_host())
    for s in edge_scalars()[:40]:
        carry, want = 0, []
        for i in range(64):
            v = (s >> 4 * i & 15) + carry
            carry = int(v > 8)
            want.append(v - 16 * carry)
        assert carry == 0 and all(-7 <= d <= 8 for d in want)
        assert sum(d * 16 ** i for i, d in enumerate(want)) == s
        b = s.to_bytes(32, "little")
        assert [L.swt_host_lane_digit(b, i) for i in range(64)] == want, hex(s)


def test_word_reduction_against_python_integers_and_the_bitwise_one():
    L = C.CDLL(build_turn_host())
    rng = random.Random(32)
    a, b = C.create_string_buffer(32), C.create_string_buffer(32)
    vals = [0, 1, L_ORDER - 1, L_ORDER, L_ORDER + 1, 2 ** 252 - 1, 2 ** 252, 2 ** 512 - 1, L_ORDER << 259, (L_ORDER << 259) - 1]
    vals += [k * L_ORDER + d for k in (1, 2 ** 32, 2 ** 64 - 1, 2 ** 200, 2 ** 259 - 1) for d in (-1, 0, 1)]
    vals += [(2 ** 252 + j) << 32 * w for w in range(8) for j in (0, 1, 27742317777372353535851937790883648493 - 1)]
    vals += [rng.getrandbits(512) for _ in range(2000)]
    vals += [rng.getrandbits(rng.randrange(1, 513)) for _ in range(500)]
    for x in vals:
        assert 0 <= x < 2 ** 512
        L.swt_host_reduce(x.to_bytes(64, "little"), a, b)
        assert int.from_bytes(a.raw, "little") == x % L_ORDER, hex(x)
        assert a.raw == b.raw, hex(x)


def test_sc_muladd_against_python_integers():
    L = C.CDLL(build_turn_host())
    rng = random.Random(33)
    out = C.create_string_buffer(32)

    def clamped():
        return (rng.getrandbits(256) & ~7 & (2 ** 255 - 1)) | 2 ** 254

    scalars = [0, 1, L_ORDER - 1] + [rng.randrange(L_ORDER) for _ in range(6)]
    secrets = [2 ** 254, 2 ** 255 - 8] + [clamped() for _ in range(6)]
    for r in scalars:
        for k in scalars:
            for s in secrets:
                L.swt_host_sc_muladd(r.to_bytes(32, "little"), k.to_bytes(32, "little"), s.to_bytes(32, "little"), out)
                assert int.from_bytes(out.raw, "little") == (r + k * s) % L_ORDER, (r, k, s)


def test_wave_signer_against_pickle_libsodium_and_hashlib():
    sod = sodium()
    L = C.CDLL(build_turn_host())
    cases = event_cases(random.Random(34))
    assert len(cases) == len(CLASSES) * 2 * len(DATA_LENGTHS) * 4
    sig, eid = C.create_string_buffer(64), C.create_string_buffer(32)
    for case in cases:
        seed, mod, qual, data, p, t_bits = case
        hdr = model_pack.class_header(mod, qual)
        L.swt_host_sign_event(seed, hdr, len(hdr), data if data else b"\0", -1 if data is None else len(data), 2 if p else 0,
                              p[0] if p else bytes(32), p[1] if p else bytes(32), C.c_ulonglong(t_bits), sig, eid)
        exp_sig, exp_id = expected_event(sod, case)
        what = (qual[:8], len(p), None if data is None else len(data), hex(t_bits))
        assert sig.raw == exp_sig, what
        assert eid.raw == exp_id, what


def test_sanitized_standalone_program_gives_the_same_results(tmp_path):
    """turn_sign_host_main.cpp with -fsanitize=address,undefined, as a child process: the edge scalars, reductions, and one
    event of every (class, arity, data shape) — a read outside a segment, an index outside the 64 lanes or an undefined shift
    in the host build of the kernel's functions ends the program instead."""
    sod = sodium()
    exe = build_turn_main()
    rng = random.Random(35)
    blob, exp = [], []
    for s in edge_scalars()[:20]:
        blob.append(struct.pack("<i", 0) + s.to_bytes(32, "little"))
        exp.append(base_mult_py(s).hex())
    for x in [0, L_ORDER, 2 ** 512 - 1] + [rng.getrandbits(512) for _ in range(13)]:
        blob.append(struct.pack("<i", 2) + x.to_bytes(64, "little"))
        exp.append((x % L_ORDER).to_bytes(32, "little").hex())
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
    # (the program's own loads and stores are instrumented at compile time; a library that an environment preloads in front of
    # the sanitizer's runtime is left where it is)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == exp
