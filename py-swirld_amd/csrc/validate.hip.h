// Validation of a sync payload against the hashgraph's FIXED member set (sw_set_member_keys, sw_validate_payload[_device];
// DESIGN.md §4.5): the crypto half of Node.is_valid_event (swirld.py:97-103) for K events at once, from device memory to a
// device array of verdicts — the d_ok sw_ingest_payload_device takes.
//
// A hashgraph has at most 1 024 members and every signature is checked against one of THEIR keys, so every base point of
// every verification is known when the keys are set.  Per member m the table holds the TRUE group multiples
//     j * 16^i * (-A_m),   i = 0..63, j = 1..8      (row n: j * 16^i * B, not negated)
// as affine (y + x, y - x, 2dxy): 512 entries of 96 B = 48 KB per member.  With S and h = SHA-512(R || A || M) mod L recoded
// to 64 signed radix-16 digits each, R' = [S]B + [h](-A) is 128 mixed additions (7 multiplications each), no doubling and no
// decompression; then one inversion, the encoding, and the byte comparison with R.
//
// Two things keep the verdict libsodium 1.0.18's (crypto.hip.h, ed25519_verify) where shortcuts would not:
//   * h is the REDUCED value.  For a key with a torsion component [h]A and [h + L]A differ, and libsodium reduces.
//   * the table holds true multiples, built with the complete addition law (ge_add is unified and complete on this curve:
//     a = -1 is a square, d is not), so that a key of mixed order contributes exactly [h mod L](-A).
//
// The arithmetic compiles for the host as crypto.hip.h does (g++ -DSW_CRYPTO_HOST; tests/validate_host.cpp): the CPU suite
// runs these very functions against libsodium.  The kernels at the end are device-only.
#pragma once
#include <stddef.h>

#include "crypto.hip.h"

namespace swv {

using swc::fe;
using swc::ge;
using swc::u64;

constexpr int POSITIONS = 64;                   // radix-16 digits of a scalar < 2^253
constexpr int PER_POS = 8;                      // |digit| = 1..8
constexpr int ROW = POSITIONS * PER_POS;        // entries per member

// an affine point in the form that makes the mixed addition 7 multiplications
struct alignas(32) niels { fe yplusx, yminusx, xy2d; };
static_assert(sizeof(niels) == 96, "a table entry is 96 bytes");

// libsodium 1.0.18's checks of a public key; on success *negA = -A in extended coordinates
SW_HD inline bool member_point(const uint8_t pk[32], ge* negA) {
    if (!swc::ge_is_canonical(pk) || swc::ge_has_small_order(pk)) return false;
    ge A;
    if (!swc::ge_frombytes(&A, pk)) return false;
    *negA = swc::ge_neg(A);
    return true;
}

// 16^pos * P
SW_HD inline ge position_base(const ge& P, int pos) {
    ge Q = P;
    for (int k = 0; k < 4 * pos; ++k) Q = swc::ge_double(Q);
    return Q;
}
// pts[j - 1] = j * Q, extended coordinates
SW_HD inline void position_points(const ge& Q, ge pts[PER_POS]) {
    pts[0] = Q;
    for (int j = 1; j < PER_POS; ++j) pts[j] = swc::ge_add(pts[j - 1], Q);
}
// c[k] = Z_0 * ... * Z_k; the return value is the whole product (never zero: the addition law is complete)
SW_HD inline fe position_zprod(const ge pts[PER_POS], fe c[PER_POS]) {
    c[0] = pts[0].Z;
    for (int k = 1; k < PER_POS; ++k) c[k] = swc::fe_mul(c[k - 1], pts[k].Z);
    return c[PER_POS - 1];
}
SW_HD inline niels niels_of(const ge& p, const fe& zinv) {
    const fe x = swc::fe_mul(p.X, zinv), y = swc::fe_mul(p.Y, zinv);
    niels e;
    e.yplusx = swc::fe_add(y, x);
    e.yminusx = swc::fe_sub(y, x);
    e.xy2d = swc::fe_mul(swc::fe_mul(x, y), swc::ge_2d());
    return e;
}
// the 8 entries of a position, given the inverse of its Z product (Montgomery's trick, walked backwards)
SW_HD inline void position_finish(const ge pts[PER_POS], const fe c[PER_POS], fe inv, niels* out) {
    for (int k = PER_POS - 1; k > 0; --k) {
        out[k] = niels_of(pts[k], swc::fe_mul(inv, c[k - 1]));
        inv = swc::fe_mul(inv, pts[k].Z);
    }
    out[0] = niels_of(pts[0], inv);
}
// a[i] <- 1 / a[i] for n non-zero elements with ONE inversion; pre: n elements of scratch
SW_HD inline void fe_batch_invert(fe* a, fe* pre, int n) {
    pre[0] = a[0];
    for (int i = 1; i < n; ++i) pre[i] = swc::fe_mul(pre[i - 1], a[i]);
    fe inv = swc::fe_invert(pre[n - 1]);
    for (int i = n - 1; i > 0; --i) {
        const fe t = swc::fe_mul(inv, pre[i - 1]);
        inv = swc::fe_mul(inv, a[i]);
        a[i] = t;
    }
    a[0] = inv;
}

// 64 signed radix-16 digits of a scalar < 2^253, least significant first, in [-7, 8]; fed one nibble at a time so that no
// digit array is ever indexed by a variable
struct Recoder {
    int carry = 0;
    SW_HD int next(u64 limb, int k) {
        const int v = (int)((limb >> (4 * k)) & 15u) + carry;
        carry = v > 8;
        return v - (carry << 4);
    }
};
SW_HD inline void recode(const u64 s[4], int8_t d[POSITIONS]) {
    Recoder r;
    for (int i = 0; i < POSITIONS; ++i) d[i] = (int8_t)r.next(s[i >> 4], i & 15);
}

// the entry |d| * 16^pos * P of P's table row; for d = 0 the neutral element (1, 1, 0), which the addition below maps
// r to itself with — no branch, and a wave of 64 lanes would take the addition for its other lanes anyway
SW_HD inline niels load_entry(const niels* __restrict__ row, int pos, int d) {
    const int a = d < 0 ? -d : d;
    niels e = row[pos * PER_POS + (a ? a - 1 : 0)];
    if (a == 0) { e.yplusx = swc::fe_one(); e.yminusx = swc::fe_one(); e.xy2d = swc::fe_zero(); }
    return e;
}
// r += e (neg: r -= e): ref10's ge_madd / ge_msub
SW_HD inline void madd_entry(ge& r, const niels& e, bool neg) {
    const fe A = swc::fe_mul(swc::fe_sub(r.Y, r.X), neg ? e.yplusx : e.yminusx);
    const fe B = swc::fe_mul(swc::fe_add(r.Y, r.X), neg ? e.yminusx : e.yplusx);
    const fe C = swc::fe_mul(r.T, e.xy2d);
    const fe D = swc::fe_add(r.Z, r.Z);
    const fe E = swc::fe_sub(B, A), H = swc::fe_add(B, A);
    const fe DmC = swc::fe_sub(D, C), DpC = swc::fe_add(D, C);
    const fe F = neg ? DpC : DmC, G = neg ? DmC : DpC;
    r.X = swc::fe_mul(E, F); r.Y = swc::fe_mul(G, H); r.T = swc::fe_mul(E, H); r.Z = swc::fe_mul(F, G);
}

SW_HD inline u64 pick_limb(const u64 s[4], int w) { return w == 0 ? s[0] : w == 1 ? s[1] : w == 2 ? s[2] : s[3]; }

// true iff libsodium's crypto_sign_verify_detached(sig, m, mlen, pk) returns 0, for a pk that passed member_point and
// whose table row is rowA; rowB is the base point's row
SW_HD inline bool comb_verify(const niels* __restrict__ rowA, const niels* __restrict__ rowB, const uint8_t sig[64],
                              const uint8_t* m, u64 mlen, const uint8_t pk[32]) {
    if (!swc::sc_is_canonical(sig + 32)) return false;
    if (swc::ge_has_small_order(sig)) return false;
    uint8_t hbytes[64];
    {
        swc::Sha512 sh;
        swc::sha512_init(&sh);
        swc::sha512_update(&sh, sig, 32);
        swc::sha512_update(&sh, pk, 32);
        swc::sha512_update(&sh, m, mlen);
        swc::sha512_final(&sh, hbytes);
    }
    u64 h[4], S[4];
    swc::sc_reduce512(hbytes, h);
    for (int i = 0; i < 4; ++i) S[i] = swc::load64_le(sig + 32 + 8 * i);
    ge R = swc::ge_identity();
    // 128 steps, even steps a digit of S (row of B), odd steps a digit of h (row of -A): ONE inlined copy of the addition, and
    // the entry of step t + 1 is requested before the addition of step t so that its latency hides behind 7 multiplications
    Recoder rs, rh;
    int d = rs.next(S[0], 0);
    niels e = load_entry(rowB, 0, d);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int t = 1; t <= 2 * POSITIONS; ++t) {
        const bool neg = d < 0;
        niels e_next = e;
        if (t < 2 * POSITIONS) {
            const int pos = t >> 1;
            const bool is_h = t & 1;
            Recoder rc = is_h ? rh : rs;
            d = rc.next(is_h ? pick_limb(h, pos >> 4) : pick_limb(S, pos >> 4), pos & 15);
            if (is_h) rh = rc; else rs = rc;
            e_next = load_entry(is_h ? rowA : rowB, pos, d);
        }
        madd_entry(R, e, neg);
        e = e_next;
    }
    uint8_t rcheck[32];
    swc::ge_tobytes(rcheck, R);
    uint8_t acc = 0;
    for (int i = 0; i < 32; ++i) acc |= rcheck[i] ^ sig[i];
    return acc == 0;
}

// [a, b) a valid range of a buffer of `bytes` bytes?  (The offsets are a peer's: nothing is read before this says yes.)
SW_HD inline bool range_ok(long long a, long long b, long long bytes) { return a >= 0 && b >= a && b <= bytes; }

// The whole verdict of event i (include/swirld_hip.h, sw_validate_payload_device).  tab: (n + 1) rows, row n the base point's.
struct Payload {
    const uint8_t* msgs; const long long* msg_off; long long msg_bytes;
    const uint8_t* whole; const long long* whole_off; long long whole_bytes;   // whole == NULL: no id check
    const uint8_t* sig; const int32_t* creator; const uint8_t* id;
};
SW_HD inline bool validate_event(const Payload& p, long long i, int n, const uint8_t* __restrict__ pk, const uint8_t* __restrict__ usable,
                                 const niels* __restrict__ tab) {
    const int cr = p.creator[i];
    if (cr < 0 || cr >= n || !usable[cr]) return false;
    const long long a = p.msg_off[i], b = p.msg_off[i + 1];
    if (!range_ok(a, b, p.msg_bytes)) return false;
    long long wa = 0, wb = 0;
    if (p.whole) {
        wa = p.whole_off[i]; wb = p.whole_off[i + 1];
        if (!range_ok(wa, wb, p.whole_bytes)) return false;
    }
    uint8_t key[32], sg[64];
    for (int k = 0; k < 32; ++k) key[k] = pk[(size_t)cr * 32 + k];
    for (int k = 0; k < 64; ++k) sg[k] = p.sig[(size_t)i * 64 + k];
    if (!comb_verify(tab + (size_t)cr * ROW, tab + (size_t)n * ROW, sg, p.msgs + a, (u64)(b - a), key)) return false;
    if (p.whole) {
        uint8_t dg[32];
        swc::blake2b_256(p.whole + wa, (u64)(wb - wa), dg);
        uint8_t acc = 0;
        for (int k = 0; k < 32; ++k) acc |= dg[k] ^ p.id[(size_t)i * 32 + k];
        if (acc) return false;
    }
    return true;
}

// Host form of the table build (the kernel below does the same with one lane per position): row of P, one inversion.
// Serial, so 16^i * P is carried from position to position instead of being doubled up from P every time.
inline void build_row_host(const ge& P, niels* row) {
    static ge pts[POSITIONS][PER_POS];
    static fe c[POSITIONS][PER_POS];
    fe t[POSITIONS], pre[POSITIONS];
    ge Q = P;
    for (int i = 0; i < POSITIONS; ++i) {
        position_points(Q, pts[i]);
        t[i] = position_zprod(pts[i], c[i]);
        Q = position_base(Q, 1);
    }
    fe_batch_invert(t, pre, POSITIONS);
    for (int i = 0; i < POSITIONS; ++i) position_finish(pts[i], c[i], t[i], row + i * PER_POS);
}

#if defined(__HIPCC__) && !defined(SW_CRYPTO_HOST)
// One block per table row, one lane per position: block m < n builds the row of -A_m (or marks the member unusable and
// leaves its row alone), block n the base point's.  The 512 Z's of a row are inverted with ONE field inversion: every lane
// multiplies its 8 together, lane 0 inverts the 64 products by Montgomery's trick in LDS, every lane unfolds its own 8.
__global__ void __launch_bounds__(POSITIONS)
k_validate_table(const uint8_t* __restrict__ pk, int n, niels* __restrict__ tab, uint8_t* __restrict__ usable) {
    __shared__ fe s_t[POSITIONS], s_pre[POSITIONS];
    const int m = blockIdx.x, pos = threadIdx.x;
    ge P;
    if (m < n) {
        uint8_t key[32];
        for (int k = 0; k < 32; ++k) key[k] = pk[(size_t)m * 32 + k];
        const bool good = member_point(key, &P);   // (the same answer in every lane of the block)
        if (pos == 0) usable[m] = good ? 1 : 0;
        if (!good) return;
    } else {
        P = swc::ge_base();
    }
    ge pts[PER_POS];
    fe c[PER_POS];
    position_points(position_base(P, pos), pts);
    s_t[pos] = position_zprod(pts, c);
    __syncthreads();
    if (pos == 0) fe_batch_invert(s_t, s_pre, POSITIONS);
    __syncthreads();
    position_finish(pts, c, s_t[pos], tab + (size_t)m * ROW + (size_t)pos * PER_POS);
}

// One lane per event: the verdict, as one byte.  The register budget is capped for SWV_WAVES_PER_SIMD resident waves: the
// hashes would take every register they can get (280 without a cap, one wave per SIMD), and the 128 additions behind them
// need other waves to fill their dependent-issue gaps.  Measured at 256 members, 1 M events on resident arrays
// (DESIGN.md 4.5): 24.4 ms uncapped, 14.1 ms at 2 waves, 12.2 ms at 3 (168 registers, 224 spilled by the compiler's report);
// no difference at 65 536 events, where every SIMD has one wave anyway.
#ifndef SWV_WAVES_PER_SIMD
#define SWV_WAVES_PER_SIMD 3
#endif
__global__ void __launch_bounds__(64, SWV_WAVES_PER_SIMD)
k_validate_payload(Payload p, long long K, int n, const uint8_t* __restrict__ pk, const uint8_t* __restrict__ usable,
                   const niels* __restrict__ tab, uint8_t* __restrict__ ok) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    ok[i] = validate_event(p, i, n, pk, usable, tab) ? 1 : 0;
}
#endif

}  // namespace swv
