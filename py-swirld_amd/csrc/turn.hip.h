// One event, signed by one wavefront (sw_create_event, sw_gossip_turn): what sign.hip.h's k_sign_level does
// with one lane per event, for the one event a gossip turn creates (swirld.py:82-95, 138-141).
//
// The signature is sws::sign_event's bit for bit.  What differs is [r]B: instead of 64 dependent mixed additions in one lane,
//   * lane i takes radix-16 position i of the recoded scalar (every lane runs the recoder's integer carry chain itself),
//   * loads its ONE entry |d_i| * 16^i * B of the base point's row and turns it into an extended point by one mixed addition
//     onto the neutral element (digit 0: the neutral entry, so the neutral element),
//   * and the 64 points are summed by a six-level butterfly of swc::ge_add: at level `off` = 32, 16, .., 1 lane l adds the
//     point of lane l ^ off to its own, so that every lane ends with the whole sum.  ge_add is unified and complete on this
//     curve (validate.hip.h says why), so the shape of the tree changes the projective representation and never the encoded
//     point.
// Coordinates cross lanes by __shfl_xor (ds_bpermute: the LDS crossbar, no LDS memory).  EVERY lane of the wave takes part in
// every level: a kernel built on this leaves no lane behind before the butterfly (no early return by lane).
//
// The hashes, the scalar arithmetic, the inversion and the encoding are sequential; here every lane runs them on the same
// values (the same instructions a single lane would cost the wave, and nothing to broadcast afterwards).
//
// Two sequential pieces have versions of their own here, used by this file only (sign.hip.h's stay as k_sign_level uses them):
// sc_reduce512w reduces 32 bits per step where swc::sc_reduce512 reduces one, and sc_muladd_w ends in it.
//
// The source compiles for the host as sign.hip.h does (g++ -DSW_CRYPTO_HOST; tests/turn_sign_host.cpp) with a "wave" of 64
// array entries: SWT_EACH_LANE runs its body once per lane on the host and once, for the calling lane, on the device, and
// lane_xor is the only thing that differs between the builds.
#pragma once
#include "sign.hip.h"

namespace swt {

using swc::fe;
using swc::ge;
using swc::u128;
using swc::u64;
using swv::niels;

constexpr int LANES = 64;
static_assert(LANES == swv::POSITIONS, "one lane per radix-16 position");

#if defined(__HIP_DEVICE_COMPILE__)
#define SWT_NL 1
#define SWT_IX(lane) 0
#define SWT_EACH_LANE(lane) for (int lane = (int)threadIdx.x, swt_once_ = 1; swt_once_; swt_once_ = 0)
#else
#define SWT_NL 64
#define SWT_IX(lane) (lane)
#define SWT_EACH_LANE(lane) for (int lane = 0; lane < swt::LANES; ++lane)
#endif

// digit `lane` of the recoding of s (s < 2^255 with top nibble at most 7, as sws::base_mult asks)
SW_HD inline int lane_digit(const u64 s[4], int lane) {
    swv::Recoder rc;
    int d = 0;
    for (int i = 0; i < swv::POSITIONS; ++i) {
        const int v = rc.next(swv::pick_limb(s, i >> 4), i & 15);
        if (i == lane) d = v;
    }
    return d;
}

// d_lane * 16^lane * B in extended coordinates
SW_HD inline ge lane_point(const niels* __restrict__ rowB, const u64 s[4], int lane) {
    const int d = lane_digit(s, lane);
    const niels e = swv::load_entry(rowB, lane, d);
    ge P = swc::ge_identity();
    swv::madd_entry(P, e, d < 0);
    return P;
}

// the point lane `lane ^ off` holds
SW_HD inline ge lane_xor(const ge* P, int lane, int off) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lane;
    ge q;
    for (int k = 0; k < 4; ++k) {
        q.X.v[k] = (u64)__shfl_xor((unsigned long long)P[0].X.v[k], off, LANES);
        q.Y.v[k] = (u64)__shfl_xor((unsigned long long)P[0].Y.v[k], off, LANES);
        q.Z.v[k] = (u64)__shfl_xor((unsigned long long)P[0].Z.v[k], off, LANES);
        q.T.v[k] = (u64)__shfl_xor((unsigned long long)P[0].T.v[k], off, LANES);
    }
    return q;
#else
    return P[lane ^ off];
#endif
}

// [s]B by the whole wave; every lane returns the sum (the host build: what lane `want` holds)
SW_HD inline ge coop_base_mult(const niels* __restrict__ rowB, const u64 s[4], int want = 0) {
    ge P[SWT_NL], Q[SWT_NL];
    SWT_EACH_LANE(lane) P[SWT_IX(lane)] = lane_point(rowB, s, lane);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int off = LANES / 2; off; off >>= 1) {
        SWT_EACH_LANE(lane) Q[SWT_IX(lane)] = lane_xor(P, lane, off);
        SWT_EACH_LANE(lane) P[SWT_IX(lane)] = swc::ge_add(P[SWT_IX(lane)], Q[SWT_IX(lane)]);
    }
    return P[SWT_IX(want)];
}

// 512-bit little-endian h -> h mod L, 32 bits per step.  acc < L on entry of a step; t = acc * 2^32 + word < 2^285;
// q = t >> 252 < 2^33; with L = 2^252 + c:  t - q L = (t mod 2^252) - q c > -2^158, so one addition of L brings a negative
// difference back into [0, L), and a difference that is not negative is below 2^252 < L.
SW_HD inline void sc_reduce512w(const uint8_t h[64], u64 r[4]) {
    const u64 c0 = swc::sc_L(0), c1 = swc::sc_L(1);   // (sc_L(2) = 0, sc_L(3) = 2^60)
    u64 a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int w = 15; w >= 0; --w) {
        const u64 word = (u64)h[4 * w] | (u64)h[4 * w + 1] << 8 | (u64)h[4 * w + 2] << 16 | (u64)h[4 * w + 3] << 24;
        const u64 t4 = a3 >> 32;
        u64 t3 = (a3 << 32) | (a2 >> 32);
        const u64 t2 = (a2 << 32) | (a1 >> 32), t1 = (a1 << 32) | (a0 >> 32), t0 = (a0 << 32) | word;
        const u64 q = (t3 >> 60) | (t4 << 4);
        t3 &= 0x0fffffffffffffffull;
        const u128 m0 = (u128)q * c0;
        const u128 m1 = (u128)q * c1 + (u64)(m0 >> 64);
        const u64 p0 = (u64)m0, p1 = (u64)m1, p2 = (u64)(m1 >> 64);
        u128 d = (u128)t0 - p0;
        a0 = (u64)d;
        u64 bw = (u64)(d >> 64) & 1u;
        d = (u128)t1 - p1 - bw; a1 = (u64)d; bw = (u64)(d >> 64) & 1u;
        d = (u128)t2 - p2 - bw; a2 = (u64)d; bw = (u64)(d >> 64) & 1u;
        d = (u128)t3 - bw; a3 = (u64)d; bw = (u64)(d >> 64) & 1u;
        if (bw) {   // negative: + L, the carry out of 2^256 cancels the borrow
            u128 s = (u128)a0 + c0;
            a0 = (u64)s;
            s = (u128)a1 + c1 + (u64)(s >> 64); a1 = (u64)s;
            s = (u128)a2 + (u64)(s >> 64); a2 = (u64)s;
            a3 = a3 + swc::sc_L(3) + (u64)(s >> 64);
        }
    }
    r[0] = a0; r[1] = a1; r[2] = a2; r[3] = a3;
}

// S = (r + k a) mod L as sws::sc_muladd, ending in the reduction above
SW_HD inline void sc_muladd_w(const u64 r[4], const u64 k[4], const u64 a[4], u64 S[4]) {
    u64 t[8] = {r[0], r[1], r[2], r[3], 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) {
        u64 carry = 0;
        for (int j = 0; j < 4; ++j) {
            const u128 p = (u128)k[i] * a[j] + t[i + j] + carry;
            t[i + j] = (u64)p;
            carry = (u64)(p >> 64);
        }
        t[i + 4] = carry;
    }
    uint8_t b[64];
    for (int i = 0; i < 8; ++i) swc::store64_le(b + 8 * i, t[i]);
    sc_reduce512w(b, S);
}

// the phase boundaries a profiling launch stamps (sw_get_turn_stats): stamp k is taken when phase k - 1 has ended
enum : int { ST_BEGIN = 0, ST_LOAD, ST_HASH1, ST_BASE, ST_ENCODE, ST_HASH2, ST_MULADD, ST_ID, ST_COUNT };

struct NoStamp {
    SW_HD void operator()(int, u64) const {}
};

// signature and id of one event as sws::sign_event gives them, by the whole wave; `stamp(k, v)` is called at the phase
// boundaries with a value the phase before it produced
template <class Stamp>
SW_HD inline void sign_event_wave(const sws::Secret& sk, const niels* __restrict__ rowB, const sws::Tmpl& v, uint8_t sig[64], uint8_t id[32],
                                  const Stamp& stamp) {
    uint8_t hb[64];
    u64 r[4], k[4], S[4];
    const sws::TmplMsg msg{&v};
    {
        sws::ShaSink s;
        swc::sha512_init(&s.st);
        s.bytes(sk.prefix, 32);
        msg(s);
        swc::sha512_final(&s.st, hb);
    }
    sc_reduce512w(hb, r);
    stamp(ST_HASH1, r[0]);
    const ge R = coop_base_mult(rowB, r);
    stamp(ST_BASE, R.Z.v[0]);
    swc::ge_tobytes(sig, R);
    stamp(ST_ENCODE, (u64)sig[0]);
    {
        sws::ShaSink s;
        swc::sha512_init(&s.st);
        s.bytes(sig, 32);
        s.bytes(v.pk, 32);
        msg(s);
        swc::sha512_final(&s.st, hb);
    }
    sc_reduce512w(hb, k);
    stamp(ST_HASH2, k[0]);
    sc_muladd_w(r, k, sk.a, S);
    for (int i = 0; i < 4; ++i) swc::store64_le(sig + 32 + 8 * i, S[i]);
    stamp(ST_MULADD, S[0]);
    sws::B2Sink b;
    b.init();
    sws::feed<true>(v, sig, b);
    b.final(id);
    stamp(ST_ID, (u64)id[0]);
}

#if defined(__HIPCC__) && !defined(SW_CRYPTO_HOST)

template <bool PROF>
struct DevStamp {
    unsigned long long* p;
    __device__ __forceinline__ void operator()(int k, u64 dep) const {
        if (PROF) {
            asm volatile("" ::"v"((unsigned)dep));   // the phase's result exists before its stamp is taken
            if (threadIdx.x == 0) p[k] = wall_clock64();
        }
    }
};

// One workgroup of ONE wave: event 0 of `in` (its parents stored events or none), signature, id and the parents' ids into
// slot 0 of `out`.  It runs behind sws::k_sign_check on the same stream and does nothing when that left a verdict (the same
// word in every lane: the wave leaves whole or not at all).  PROF: lane 0 stores wall_clock64() at the phase boundaries.
// Registers: one wave on its SIMD, as k_sign_level.
template <bool PROF>
__global__ void __launch_bounds__(LANES, 1)
k_sign_one(sws::SignIn in, sws::SignOut out, const unsigned long long* __restrict__ verdict, unsigned long long* stamps) {
    if (*verdict != ing::V_NONE) return;
    const DevStamp<PROF> stamp{stamps};
    stamp(ST_BEGIN, 0);
    const int m = in.creator[0], s = in.sp[0], o = in.op[0];
    uint8_t spid[32], opid[32], pk[32], sig[64], id[32];
    const int ar = s < 0 ? 0 : 2;
    if (ar) {
        const uint8_t* ps = in.stored_id + (size_t)s * 32;
        const uint8_t* po = in.stored_id + (size_t)o * 32;
        for (int k = 0; k < 32; ++k) { spid[k] = ps[k]; opid[k] = po[k]; }
    } else {
        for (int k = 0; k < 32; ++k) { spid[k] = 0; opid[k] = 0; }
    }
    for (int k = 0; k < 32; ++k) pk[k] = in.keys[(size_t)m * 32 + k];
    const sws::Secret sk = in.secret[m];
    const int dl = sws::data_len(in, 0);
    stamp(ST_LOAD, sk.a[0] ^ (u64)pk[0] ^ (u64)spid[0]);
    const sws::Tmpl v{in.hdr, in.hdr_len, dl > 0 ? in.data + in.data_off[0] : nullptr, dl, ar, spid, opid, in.t[0], pk};
    sign_event_wave(sk, in.rowB, v, sig, id, stamp);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 32; ++k) {
            out.id[k] = id[k];
            out.sp_id[k] = spid[k];
            out.op_id[k] = opid[k];
        }
        for (int k = 0; k < 64; ++k) out.sig[k] = sig[k];
        out.arity[0] = (uint8_t)ar;
    }
}
#endif

}  // namespace swt
