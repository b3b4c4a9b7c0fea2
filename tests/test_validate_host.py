"""CPU: the functions the member-table and payload-validation kernels execute (py-swirld_amd/csrc/validate.hip.h),
compiled for the HOST by g++ (tests/validate_host.cpp) and run against libsodium 1.0.18 and hashlib: the table entries are
the true multiples, the digit recoding re-sums, and table build + comb verification gives libsodium's verdict — on valid,
corrupted, non-canonical and small-order inputs, on keys of MIXED order (where the verdict depends on (h mod L) mod 8), and
at the padding edges of both hashes.  The same verdicts from a stand-alone program built with the address and
undefined-behaviour sanitizers.  The GPU run of the same cases is tests/test_gpu_validate.py."""
import ctypes as C
import hashlib
import os
import random
import struct
import subprocess

import numpy as np

import hostlibs
from test_crypto_host import L_ORDER, load_sodium, signed_cases, sodium_verify

HERE = os.path.dirname(os.path.abspath(__file__))
VALIDATE_SO = os.path.join(HERE, "libswv_host.so")
VALIDATE_SRC = os.path.join(HERE, "validate_host.cpp")
VALIDATE_MAIN = os.path.join(HERE, "validate_host_main")
VALIDATE_MAIN_SRC = os.path.join(HERE, "validate_host_main.cpp")
HDRS = [os.path.join(hostlibs.CSRC, "validate.hip.h"), os.path.join(hostlibs.CSRC, "crypto.hip.h")]

# ---- edwards25519 in Python integers: the independent arithmetic behind the mixed-order keys and the table entries
P = 2 ** 255 - 19
D = -121665 * pow(121666, P - 2, P) % P
BY = 4 * pow(5, P - 2, P) % P


def _recover_x(y, sign):
    x2 = (y * y - 1) * pow(D * y * y + 1, P - 2, P) % P
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P:
        x = x * pow(2, (P - 1) // 4, P) % P
    assert (x * x - x2) % P == 0
    return P - x if (x & 1) != sign else x


def pt(x, y):   # points are (X, Y, Z, T) with x = X/Z, y = Y/Z, xy = T/Z: one inversion per point, at the end
    return (x % P, y % P, 1, x * y % P)


BASE = pt(_recover_x(BY, 0), BY)
NEUTRAL = pt(0, 1)


def pt_add(p, q):   # the unified addition law of RFC 8032, 5.1.4: complete on this curve
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a, b = (y1 - x1) * (y2 - x2) % P, (y1 + x1) * (y2 + x2) % P
    c, d = 2 * D * t1 * t2 % P, 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def pt_mul(s, p):
    r = NEUTRAL
    while s:
        if s & 1:
            r = pt_add(r, p)
        p = pt_add(p, p)
        s >>= 1
    return r


def pt_affine(p):
    zi = pow(p[2], P - 2, P)
    return p[0] * zi % P, p[1] * zi % P


def pt_enc(p):
    x, y = pt_affine(p)
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def pt_dec(b):
    v = int.from_bytes(b, "little")
    y = v & (2 ** 255 - 1)
    return pt(_recover_x(y, v >> 255), y)


# the order-8 point whose encoding is the third row of ge_has_small_order's list (crypto.hip.h)
TORSION8 = bytes.fromhex("26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc05")


def mixed_order_cases(rng, n_keys=4, n_msgs=40):
    """(sig, msg, pk) with pk = a B + T, T of order 8, and R = r B, S = r + (h mod L) a in Python integers: libsodium accepts
    exactly when (h mod L) = 0 mod 8 — a verifier that skips the reduction of h, or whose table is not made of true multiples
    of the key, answers differently."""
    T = pt_dec(TORSION8)
    assert pt_affine(pt_mul(8, T)) == (0, 1) and pt_affine(pt_mul(4, T)) != (0, 1)
    cases = []
    for _ in range(n_keys):
        a = rng.randrange(1, L_ORDER)
        pk = pt_enc(pt_add(pt_mul(a, BASE), T))
        for _ in range(n_msgs):
            m = bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 120)))
            r = rng.randrange(1, L_ORDER)
            R = pt_enc(pt_mul(r, BASE))
            h = int.from_bytes(hashlib.sha512(R + pk + m).digest(), "little") % L_ORDER
            cases.append((R + ((r + h * a) % L_ORDER).to_bytes(32, "little"), m, pk))
    return cases


# ---- builders and the host library
def build_validate_host():
    if hostlibs._stale(VALIDATE_SO, VALIDATE_SRC, *HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", VALIDATE_SRC, "-o", VALIDATE_SO])
    return VALIDATE_SO


def build_validate_main():
    if hostlibs._stale(VALIDATE_MAIN, VALIDATE_MAIN_SRC, *HDRS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-fno-omit-frame-pointer", VALIDATE_MAIN_SRC, "-o", VALIDATE_MAIN])
    return VALIDATE_MAIN


def sodium():
    sod = load_sodium()
    assert sod is not None, "libsodium is part of the image"
    return sod


def members_of(cases):
    """The distinct public keys of the cases as the member list (unusable ones included), and each case's creator."""
    keys = []
    for _, _, pk in cases:
        if pk not in keys:
            keys.append(pk)
    return keys, [keys.index(pk) for _, _, pk in cases]


def pack(items):
    off = np.zeros(len(items) + 1, np.int64)
    if items:
        np.cumsum([len(m) for m in items], out=off[1:])
    return np.frombuffer(b"".join(items) + b"\0", np.uint8), off   # (one spare byte: never a NULL pointer)


class HostValidator:
    """Table build + validation through the host library, with the calling convention of Hashgraph.validate_payload."""

    def __init__(self, keys):
        self.L = C.CDLL(build_validate_host())
        self.n = len(keys)
        self.pk = np.frombuffer(b"".join(keys), np.uint8).copy()
        self.tab = np.zeros((self.n + 1) * self.L.swv_host_row_entries() * self.L.swv_host_entry_bytes() + 32, np.uint8)
        self.tab_p = (self.tab.ctypes.data + 31) & ~31   # entries are 32-byte aligned
        self.usable = np.zeros(self.n, np.uint8)
        self.n_unusable = self.L.swv_host_build(self.n, self.pk.ctypes.data_as(C.c_void_p), C.c_void_p(self.tab_p), self.usable.ctypes.data_as(C.c_void_p))

    def validate(self, msgs, sig, creator, whole=None, ids=None, msg_bytes=None, msg_off=None):
        data, off = pack(msgs)
        if msg_off is not None:
            off = np.ascontiguousarray(msg_off, np.int64)
        K = len(off) - 1
        sg = np.frombuffer(b"".join(sig) + b"\0", np.uint8)
        cr = np.ascontiguousarray(creator, np.int32)
        ok = np.zeros(K, np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        if whole is not None:
            wdata, woff = pack(whole)
            idb = np.frombuffer(b"".join(ids) + b"\0", np.uint8)
            wargs = (p(wdata), p(woff), C.c_longlong(len(wdata) - 1))
        else:
            idb = np.zeros(1, np.uint8)
            wargs = (None, None, C.c_longlong(0))
        self.L.swv_host_validate(C.c_longlong(K), p(data), p(off), C.c_longlong(len(data) - 1 if msg_bytes is None else msg_bytes), *wargs,
                                 p(sg), p(cr), p(idb), self.n, p(self.pk), p(self.usable), C.c_void_p(self.tab_p), p(ok))
        return ok.astype(bool)

    def entry(self, m, pos, j):
        out = C.create_string_buffer(96)
        self.L.swv_host_entry(C.c_void_p(self.tab_p), m, pos, j, out)
        return out.raw


def expected_entry(point, pos, j):
    x, y = pt_affine(pt_mul(j * 16 ** pos, point))
    return b"".join(v.to_bytes(32, "little") for v in ((y + x) % P, (y - x) % P, 2 * D * x * y % P))


# ---- tests
def test_verdicts_match_libsodium_and_the_plain_verifier():
    sod = sodium()
    cases = signed_cases(sod, random.Random(3), 40)
    keys, creator = members_of(cases)
    hv = HostValidator(keys)
    assert 0 < hv.n_unusable < len(keys), "the case set has usable and unusable member keys"
    exp = np.array([sodium_verify(sod, s, m, p) for s, m, p in cases])
    got = hv.validate([m for _, m, _ in cases], [s for s, _, _ in cases], creator)
    assert np.array_equal(got, exp)
    assert exp.sum() >= 40 and (~exp).sum() > 300
    ref = np.array([hv.L.swv_host_verify_ref(s, m, C.c_uint64(len(m)), p) == 1 for s, m, p in cases])
    assert np.array_equal(got, ref)
    # a key is unusable exactly when libsodium refuses it whatever the signature: every event of such a member is invalid
    for k, u in zip(keys, hv.usable):
        if not u:
            assert not any(e for e, (_, _, p) in zip(exp, cases) if p == k)


def test_mixed_order_keys_need_the_reduced_h_and_true_multiples():
    sod = sodium()
    cases = mixed_order_cases(random.Random(5))
    keys, creator = members_of(cases)
    hv = HostValidator(keys)
    assert hv.n_unusable == 0
    exp = np.array([sodium_verify(sod, s, m, p) for s, m, p in cases])
    print("mixed-order keys: libsodium accepts %d, rejects %d" % (exp.sum(), (~exp).sum()))
    assert exp.sum() >= 8 and (~exp).sum() >= 8
    for e, (s, m, p) in zip(exp, cases):   # the rule the issue states, from the case's own numbers
        h = int.from_bytes(hashlib.sha512(s[:32] + p + m).digest(), "little") % L_ORDER
        assert e == (h % 8 == 0)
    assert np.array_equal(hv.validate([m for _, m, _ in cases], [s for s, _, _ in cases], creator), exp)


def _signed(sod, rng, n_keys, lengths):
    keys, sks = [], []
    for _ in range(n_keys):
        pk, sk = C.create_string_buffer(32), C.create_string_buffer(64)
        sod.crypto_sign_seed_keypair(pk, sk, bytes(rng.getrandbits(8) for _ in range(32)))
        keys.append(pk.raw)
        sks.append(sk)
    msgs, sigs, creator = [], [], []
    for i, n in enumerate(lengths):
        m = bytes(rng.getrandbits(8) for _ in range(n))
        sig = C.create_string_buffer(64)
        sod.crypto_sign_detached(sig, None, m, C.c_ulonglong(n), sks[i % n_keys])
        msgs.append(m)
        sigs.append(sig.raw)
        creator.append(i % n_keys)
    return keys, msgs, sigs, creator


MSG_EDGES = [0, 47, 48, 63, 64, 65, 175, 176, 191, 192]     # SHA-512 padding edges behind the 64 prefix bytes
WHOLE_EDGES = [0, 1, 127, 128, 129, 255, 256, 257]          # BLAKE2b block edges


def test_length_boundaries_of_both_hashes():
    sod = sodium()
    rng = random.Random(7)
    lengths = [a for a in MSG_EDGES for _ in WHOLE_EDGES]
    keys, msgs, sigs, creator = _signed(sod, rng, 3, lengths)
    whole = [bytes(rng.getrandbits(8) for _ in range(w)) for _ in MSG_EDGES for w in WHOLE_EDGES]
    ids = [hashlib.blake2b(w, digest_size=32).digest() for w in whole]
    hv = HostValidator(keys)
    assert all(sodium_verify(sod, s, m, keys[c]) for s, m, c in zip(sigs, msgs, creator))
    assert hv.validate(msgs, sigs, creator, whole, ids).all()
    # every message one byte longer or shorter, every id one bit off: nothing passes
    longer = [m + b"\0" for m in msgs]
    assert not hv.validate(longer, sigs, creator, whole, ids).any()
    assert not any(sodium_verify(sod, s, m, keys[c]) for s, m, c in zip(sigs, longer, creator))
    bad_ids = [bytes([i[0] ^ 1]) + i[1:] for i in ids]
    assert not hv.validate(msgs, sigs, creator, whole, bad_ids).any()
    assert hv.validate(msgs, sigs, creator).all()   # no id check


def test_out_of_range_events_are_invalid_and_read_nothing():
    sod = sodium()
    keys, msgs, sigs, creator = _signed(sod, random.Random(8), 2, [30, 40, 50, 60])
    hv = HostValidator(keys)
    _, off = pack(msgs)
    total = int(off[-1])
    assert hv.validate(msgs, sigs, creator).all()
    assert hv.validate(msgs, sigs, [0, -1, 2, 1]).tolist() == [True, False, False, True]
    assert hv.validate(msgs, sigs, creator, msg_bytes=total - 1).tolist() == [True, True, True, False]
    dec = off.copy()
    dec[2] = dec[1] - 1     # event 1 ends before it starts; event 2 then starts elsewhere: its bytes are not what was signed
    assert hv.validate(msgs, sigs, creator, msg_off=dec).tolist() == [True, False, False, True]
    neg = off.copy()
    neg[0] = -5
    assert hv.validate(msgs, sigs, creator, msg_off=neg).tolist() == [False, True, True, True]


def test_digit_recoding():
    L = C.CDLL(build_validate_host())
    rng = random.Random(9)
    d = (C.c_int8 * 64)()
    for s in [0, 1, L_ORDER - 1, 2 ** 252] + [rng.randrange(L_ORDER) for _ in range(300)]:
        L.swv_host_recode(s.to_bytes(32, "little"), d)
        digits = list(d)
        assert all(-8 <= v <= 8 for v in digits)
        assert sum(v * 16 ** i for i, v in enumerate(digits)) == s


def test_table_entries_are_the_true_multiples():
    sod = sodium()
    keys, _, _, _ = _signed(sod, random.Random(10), 2, [])
    keys.append(pt_enc(pt_add(pt_mul(12345, BASE), pt_dec(TORSION8))))   # and a key of mixed order
    hv = HostValidator(keys)
    out = C.create_string_buffer(96)
    for m in (1, 2, len(keys)):   # one honest member, the mixed-order one, and the base point's row
        if m < len(keys):
            x, y = pt_affine(pt_dec(keys[m]))
            point = pt(P - x, y)   # the table holds multiples of -A
        else:
            point = BASE
        for pos in (0, 1, 63):
            for j in range(1, 9):
                got = hv.entry(m, pos, j)
                assert hv.L.swv_host_entry_by_additions(keys[m] if m < len(keys) else None, 1, pos, j, out) == 1
                assert got == out.raw, "entry (%d, %d, %d) against repeated ge_add" % (m, pos, j)
                assert got == expected_entry(point, pos, j), "entry (%d, %d, %d) against Python integers" % (m, pos, j)


def write_case_file(path, keys, msgs, sigs, creator, whole=None, ids=None):
    data, off = pack(msgs)
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(keys)) + b"".join(keys))
        wb = -1 if whole is None else sum(len(w) for w in whole)
        f.write(struct.pack("<qqq", len(msgs), int(off[-1]), wb))
        f.write(off.tobytes() + data[:-1].tobytes())
        if whole is not None:
            wdata, woff = pack(whole)
            f.write(woff.tobytes() + wdata[:-1].tobytes())
        f.write(b"".join(sigs) + np.ascontiguousarray(creator, np.int32).tobytes())
        f.write(b"".join(ids) if ids is not None else bytes(32 * len(msgs)))


def test_sanitized_standalone_program_gives_the_same_verdicts(tmp_path):
    """validate_host_main.cpp with -fsanitize=address,undefined, as a child process: libsodium's verdicts on the adversarial
    set and on the length edges (with the id check), and a clean exit — a read outside a buffer or an undefined shift in the
    host build of the kernels' functions ends the program instead."""
    sod = sodium()
    exe = build_validate_main()
    cases = signed_cases(sod, random.Random(11), 6) + mixed_order_cases(random.Random(12), 1, 24)
    keys, creator = members_of(cases)
    exp = "".join("1" if sodium_verify(sod, s, m, p) else "0" for s, m, p in cases)
    path = str(tmp_path / "cases.bin")
    write_case_file(path, keys, [m for _, m, _ in cases], [s for s, _, _ in cases], creator)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == exp and "1" in exp and "0" in exp

    rng = random.Random(13)
    keys, msgs, sigs, creator = _signed(sod, rng, 2, MSG_EDGES)
    whole = [bytes(rng.getrandbits(8) for _ in range(w)) for w in (WHOLE_EDGES + [300, 5])]
    ids = [hashlib.blake2b(w, digest_size=32).digest() for w in whole]
    ids[3] = bytes(32)
    write_case_file(path, keys, msgs, sigs, creator, whole, ids)
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == "1110111111"
