// Creating signed events on the device (sw_set_signing_keys, sw_sign_events[_device], sw_create_events[_device];
// DESIGN.md §4.8): the producing half of the reference's Node.new_event (swirld.py:82-95) for K events at once — the Ed25519
// signature over dumps((d, p, t, pk)) and the id crypto_generichash(dumps(ev)).
//
// Signing as libsodium 1.0.18 does it (RFC 8032, deterministic):
//     h = SHA-512(seed), a = clamp(h[0..32)), prefix = h[32..64), A = [a]B
//     r = SHA-512(prefix || M) mod L, R = [r]B, k = SHA-512(R || A || M) mod L, S = (r + k a) mod L, sig = R || S
// [r]B is 64 mixed additions on the base point's row of the member table (validate.hip.h: the row holds j * 16^i * B), with
// the recoder, the entry prefetch and the one inlined addition of comb_verify; then one inversion.
//
// Neither M = dumps(ev[:-1]) nor dumps(ev) exists in memory: feed() walks the template of tmpl.hip.h segment by segment
// (frame header, class header, data opcode and bytes, parents, timestamp, key, closing opcodes, signature) and hands every
// segment to a sink — a SHA-512 state or a streaming BLAKE2b state.
//
// An event's signed bytes hold its parents' ids and an id is the hash of bytes that hold the signature, so a batch is signed
// LEVEL by level: level 0 are the events whose parents are all stored already (or that have none), level l + 1 those whose
// deepest in-batch parent is of level l.  The kernels at the end (device only) assign the levels, sort the batch by level
// and sign one level per launch; no kernel waits for another workgroup.
//
// The arithmetic compiles for the host as validate.hip.h does (g++ -DSW_CRYPTO_HOST; tests/sign_host.cpp): the CPU suite
// runs these very functions against libsodium, pickle and hashlib.  Signing handles SECRET scalars with code that is not
// constant-time (the recoder's table index, sc_reduce512's branches): the keys of a context are those of the process that
// drives the device, not a defence against an observer of the device.
#pragma once
#include "tmpl.hip.h"
#include "validate.hip.h"
#if defined(__HIPCC__) && !defined(SW_CRYPTO_HOST)
#include "ingest.hip.h"
#endif

namespace sws {

using swc::fe;
using swc::ge;
using swc::u128;
using swc::u64;
using swv::niels;

// what a member signs with: the clamped scalar and the hash prefix (64 bytes per member, device memory only)
struct alignas(8) Secret {
    u64 a[4];
    uint8_t prefix[32];
};
static_assert(sizeof(Secret) == 64, "a member's secret is 64 bytes");

SW_HD inline void expand_seed(const uint8_t seed[32], Secret* s) {
    uint8_t h[64];
    swc::Sha512 sh;
    swc::sha512_init(&sh);
    swc::sha512_update(&sh, seed, 32);
    swc::sha512_final(&sh, h);
    h[0] &= 248;
    h[31] &= 127;
    h[31] |= 64;
    for (int i = 0; i < 4; ++i) s->a[i] = swc::load64_le(h + 8 * i);
    for (int i = 0; i < 32; ++i) s->prefix[i] = h[32 + i];
}

// [s]B from the base point's row, for s < 2^255 whose top nibble is at most 7 (a clamped scalar, or anything below L): the
// last digit then takes the recoder's carry without passing one on
SW_HD inline ge base_mult(const niels* __restrict__ rowB, const u64 s[4]) {
    ge R = swc::ge_identity();
    swv::Recoder rc;
    int d = rc.next(s[0], 0);
    niels e = swv::load_entry(rowB, 0, d);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int t = 1; t <= swv::POSITIONS; ++t) {
        const bool neg = d < 0;
        niels e_next = e;
        if (t < swv::POSITIONS) {
            d = rc.next(swv::pick_limb(s, t >> 4), t & 15);
            e_next = swv::load_entry(rowB, t, d);
        }
        swv::madd_entry(R, e, neg);
        e = e_next;
    }
    return R;
}

// the public key of a secret: encode([a]B)
SW_HD inline void public_key(const niels* __restrict__ rowB, const Secret& s, uint8_t pk[32]) {
    swc::ge_tobytes(pk, base_mult(rowB, s.a));
}

// S = (r + k a) mod L for r, k < L and ANY a < 2^255 (a clamped scalar is usually above L): the 512-bit value
// r + k a < 2^253 + 2^508, reduced as the hashes are
SW_HD inline void sc_muladd(const u64 r[4], const u64 k[4], const u64 a[4], u64 S[4]) {
    u64 t[8] = {r[0], r[1], r[2], r[3], 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) {
        u64 carry = 0;
        for (int j = 0; j < 4; ++j) {
            const u128 p = (u128)k[i] * a[j] + t[i + j] + carry;
            t[i + j] = (u64)p;
            carry = (u64)(p >> 64);
        }
        t[i + 4] = carry;   // (row i is the first to reach limb i + 4)
    }
    uint8_t b[64];
    for (int i = 0; i < 8; ++i) swc::store64_le(b + 8 * i, t[i]);
    swc::sc_reduce512(b, S);
}

// ---- sinks: what feed() writes into
struct ShaSink {
    swc::Sha512 st;
    SW_HD void bytes(const uint8_t* p, u64 n) { swc::sha512_update(&st, p, n); }
    SW_HD void konst(u64 packed, int n) {   // n <= 8 bytes, the lowest first
        uint8_t b[8];
        swc::store64_le(b, packed);
        swc::sha512_update(&st, b, (u64)n);
    }
};

// BLAKE2b-256, unkeyed, fed in pieces: a full buffer is compressed only when another byte arrives (the last block is
// compressed with the final flag, and a message that ends on a block edge has no empty block behind it)
struct B2Sink {
    u64 h[8];
    uint8_t buf[128];
    u64 len;   // bytes absorbed
    SW_HD void init() {
        const u64 iv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                           0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
        for (int i = 0; i < 8; ++i) h[i] = iv[i];
        h[0] ^= 0x01010000ull ^ 32ull;
        len = 0;
    }
    SW_HD void put(uint8_t v) {
        if (len && (len & 127) == 0) swc::blake2b_compress(h, buf, len, false);
        buf[len & 127] = v;
        len++;
    }
    SW_HD void bytes(const uint8_t* p, u64 n) { for (u64 i = 0; i < n; ++i) put(p[i]); }
    SW_HD void konst(u64 packed, int n) { for (int i = 0; i < n; ++i) put((uint8_t)(packed >> (8 * i))); }
    SW_HD void final(uint8_t out[32]) {
        const u64 fill = len == 0 ? 0 : ((len - 1) & 127) + 1;
        for (u64 i = fill; i < 128; ++i) buf[i] = 0;
        swc::blake2b_compress(h, buf, len, true);
        for (int i = 0; i < 4; ++i) swc::store64_le(out + 8 * i, h[i]);
    }
};

// ---- the template, segment by segment
struct Tmpl {               // one event as the hashes see it
    const uint8_t* hdr;     // the class header of dumps(ev) (sw_set_event_class), hdr_len bytes
    int hdr_len;
    const uint8_t* data;    // dl bytes; dl < 0: None
    int dl;
    int ar;                 // 0 or 2
    const uint8_t* sp;      // the parents' ids, 32 bytes each (read only where ar == 2)
    const uint8_t* op;
    u64 t_bits;             // the timestamp's bit pattern
    const uint8_t* pk;      // the creator's key
};

// dumps(ev[:-1]) (WHOLE = false) or dumps(ev) (WHOLE = true, sig: the 64 signature bytes) into the sink
template <bool WHOLE, class Sink>
SW_HD inline void feed(const Tmpl& v, const uint8_t* sig, Sink& s) {
    const u64 inner = (u64)((WHOLE ? tpl::WHOLE_FIXED + v.hdr_len : tpl::MSG_FIXED) - tpl::FRAME + tpl::var_size(v.dl, v.ar));
    s.konst(tpl::K_FRAME, 3);
    s.konst(inner, 8);
    if (WHOLE) s.bytes(v.hdr, (u64)v.hdr_len);
    if (v.dl < 0) s.konst(tpl::K_NONE, 2);
    else if (v.dl < 256) s.konst(tpl::K_BYTES8 | (u64)v.dl << 16, 3);
    else s.konst(tpl::K_BYTES32 | (u64)v.dl << 16, 6);
    if (v.dl >= 0) {
        s.bytes(v.data, (u64)v.dl);
        s.konst(tpl::K_MEMO, 1);
    }
    if (v.ar == 0) {
        s.konst(tpl::K_ROOT, 2);
    } else {
        s.konst(tpl::K_ID, 2);
        s.bytes(v.sp, 32);
        s.konst(tpl::K_ID_NEXT, 3);
        s.bytes(v.op, 32);
        s.konst(tpl::K_PARENTS_END, 4);
    }
    s.konst(__builtin_bswap64(v.t_bits), 8);   // most significant byte first
    s.konst(tpl::K_ID, 2);
    s.bytes(v.pk, 32);
    if (!WHOLE) {
        s.konst(tpl::K_MSG_END, 4);
    } else {
        s.konst(tpl::K_SIG, 3);
        s.bytes(sig, 64);
        s.konst(tpl::K_WHOLE_END, 6);
    }
}

// messages: something that can write itself into a sink, as often as asked
struct RawMsg {
    const uint8_t* m;
    u64 n;
    template <class Sink>
    SW_HD void operator()(Sink& s) const { s.bytes(m, n); }
};
struct TmplMsg {
    const Tmpl* v;
    template <class Sink>
    SW_HD void operator()(Sink& s) const { feed<false>(*v, nullptr, s); }
};

// sig = crypto_sign_detached(M, sk) for the secret `sk` whose public key is pk
template <class Msg>
SW_HD inline void sign_message(const Secret& sk, const uint8_t pk[32], const niels* __restrict__ rowB, const Msg& msg, uint8_t sig[64]) {
    uint8_t hb[64];
    u64 r[4], k[4], S[4];
    {
        ShaSink s;
        swc::sha512_init(&s.st);
        s.bytes(sk.prefix, 32);
        msg(s);
        swc::sha512_final(&s.st, hb);
    }
    swc::sc_reduce512(hb, r);
    swc::ge_tobytes(sig, base_mult(rowB, r));
    {
        ShaSink s;
        swc::sha512_init(&s.st);
        s.bytes(sig, 32);
        s.bytes(pk, 32);
        msg(s);
        swc::sha512_final(&s.st, hb);
    }
    swc::sc_reduce512(hb, k);
    sc_muladd(r, k, sk.a, S);
    for (int i = 0; i < 4; ++i) swc::store64_le(sig + 32 + 8 * i, S[i]);
}

// signature and id of one event
SW_HD inline void sign_event(const Secret& sk, const niels* __restrict__ rowB, const Tmpl& v, uint8_t sig[64], uint8_t id[32]) {
    sign_message(sk, v.pk, rowB, TmplMsg{&v}, sig);
    B2Sink b;
    b.init();
    feed<true>(v, sig, b);
    b.final(id);
}

#if defined(__HIPCC__) && !defined(SW_CRYPTO_HOST)
typedef long long i64;

// verdicts of k_sign_check beyond ingest.hip.h's (same word, same lowest-offender rule)
enum : int {
    V_NOKEY = 7,   // the creator has no signing key
    V_DATA = 8,    // the data range cannot be used, or is longer than MAX_DATA
};

struct SignIn {             // a batch in device memory, as sw_append_events_device and sw_pack_events_device take it
    const int* creator;
    const int* sp;          // dense indices: < N0 a stored event, >= N0 batch position (index - N0), < 0 none
    const int* op;
    const u64* t;
    const uint8_t* data;    // data, data_off both null: every event's data is None
    const i64* data_off;
    i64 data_bytes;
    const uint8_t* data_none;
    const int* stored_cr;   // creators of the stored events
    const uint8_t* stored_id;   // ids of the stored events, 32 B each
    int N0, n;
    const uint8_t* keys;    // n x 32 B
    const uint8_t* has_key; // n flags
    const Secret* secret;   // n
    const niels* rowB;      // the base point's row of the member table
    const uint8_t* hdr;
    int hdr_len;
};
struct SignOut { uint8_t* id; uint8_t* sp_id; uint8_t* op_id; uint8_t* arity; uint8_t* sig; };

// the length of event i's data: >= 0, -1 for None, -2 when the range cannot be used (pack.hip.h's rule)
__device__ __forceinline__ int data_len(const SignIn& in, i64 i) {
    if (!in.data_off) return -1;
    const i64 a = in.data_off[i], b = in.data_off[i + 1];
    if (a < 0 || b < a || b > in.data_bytes || b - a > tpl::MAX_DATA) return -2;
    if (in.data_none && in.data_none[i]) return -1;
    return (int)(b - a);
}

// Key expansion of `cnt` members: ok[j] = the seed's public key is member[j]'s.  With store != 0 (the caller has seen every
// ok) the secret goes to the member's slot and nowhere else.
__global__ void __launch_bounds__(64)
k_sign_keys(int cnt, const int* __restrict__ member, const uint8_t* __restrict__ seed, const uint8_t* __restrict__ keys,
            const niels* __restrict__ rowB, int store, Secret* secret, uint8_t* has_key, uint8_t* ok) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt) return;
    uint8_t sd[32], pk[32];
    for (int k = 0; k < 32; ++k) sd[k] = seed[(size_t)j * 32 + k];
    Secret s;
    expand_seed(sd, &s);
    public_key(rowB, s, pk);
    const int m = member[j];
    uint8_t acc = 0;
    for (int k = 0; k < 32; ++k) acc |= pk[k] ^ keys[(size_t)m * 32 + k];
    if (!store) { ok[j] = acc == 0; return; }
    if (acc == 0) { secret[m] = s; has_key[m] = 1; }
}

// One thread per event: the structural checks of sw_append_events_device (ingest.hip.h's codes, lowest offender first; a
// fork is no defect here), then the signer's own.  sum: the data bytes of the usable ranges (ranges may overlap).
__global__ void __launch_bounds__(256)
k_sign_check(SignIn in, int K, unsigned long long* v, unsigned long long* sum) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    const int e = in.N0 + i;
    const int m = in.creator[i], s = in.sp[i], o = in.op[i];
    int code = 0;
    if (m < 0 || m >= in.n) code = ing::V_CREATOR;
    else if ((s < 0) != (o < 0)) code = ing::V_ARITY;
    else if (s >= e || o >= e) code = ing::V_ORDER;
    else if (s >= 0) {
        const int cs = s < in.N0 ? in.stored_cr[s] : in.creator[s - in.N0];
        const int co = o < in.N0 ? in.stored_cr[o] : in.creator[o - in.N0];
        if (cs != m) code = ing::V_SELF;
        else if (co == m) code = ing::V_OTHER;
    }
    int dl = -1;
    if (!code) {
        dl = data_len(in, i);
        if (!in.has_key[m]) code = V_NOKEY;
        else if (dl == -2) code = V_DATA;
    }
    if (code) ing::verdict(v, e, code);
    else if (in.data_off) atomicAdd(sum, (unsigned long long)(in.data_off[i + 1] - in.data_off[i]));
}

// Levels, one workgroup streaming the batch in index order like ing::k_ingest_heights: lvl = 0 for a root or when both
// parents are stored, else 1 + the deepest in-batch parent's level.  Parents in front of the tile are gathered from lvl,
// parents inside it settle by a fixed point in LDS (a tile needs at most as many trips as it has events; more ends the kernel
// with stat[2] = 1).  cnt[l] counts the events of level l (zeroed by the caller); stat: [0] levels, [1] widest level.
constexpr int LV_TILE = 1024;
__global__ void __launch_bounds__(LV_TILE)
k_sign_levels(const int* __restrict__ sp, const int* __restrict__ op, int N0, int K, int* lvl, unsigned long long* cnt, int* stat) {
    __shared__ int h[LV_TILE];
    __shared__ int tops;
    const int tid = threadIdx.x;
    int top = -1;
    for (int t0 = 0; t0 < K; t0 += LV_TILE) {
        const int i = t0 + tid;
        const bool in = i < K;
        // a parent's level: -1 stored or none (settled), -2 inside the tile and not known yet
        int s = -1, o = -1, a = -1, b = -1, hv = 0;
        if (in) {
            s = sp[i] - N0; o = op[i] - N0;
            // (this kernel runs beside k_sign_check, before its verdict is read: a parent that is not earlier is none here)
            if (s >= i) s = -1;
            if (o >= i) o = -1;
            a = s < 0 ? -1 : s < t0 ? lvl[s] : -2;
            b = o < 0 ? -1 : o < t0 ? lvl[o] : -2;
            hv = (a > -2 && b > -2) ? 1 + max(a, b) : -1;
        }
        h[tid] = hv;
        int trips = 0;
        while (__syncthreads_count(hv < 0)) {
            if (++trips > LV_TILE) {   // (uniform)
                if (tid == 0) stat[2] = 1;
                return;
            }
            if (hv < 0) {
                if (a == -2 && h[s - t0] >= 0) a = h[s - t0];
                if (b == -2 && h[o - t0] >= 0) b = h[o - t0];
            }
            __syncthreads();   // every read of this trip before its writes
            if (hv < 0 && a > -2 && b > -2) { hv = 1 + max(a, b); h[tid] = hv; }
        }
        if (in) {
            lvl[i] = hv;
            atomicAdd(&cnt[hv], 1ull);
        }
        top = max(top, ing::wave_max(in ? hv : -1));
        __syncthreads();   // this tile's levels visible to the gathers of the next one
    }
    if (tid == 0) tops = -1;
    __syncthreads();
    if ((tid & 63) == 0) atomicMax(&tops, top);
    __threadfence();
    __syncthreads();
    const int nlev = tops + 1;
    int widest = 0;
    for (int l = tid; l < nlev; l += LV_TILE) widest = max(widest, (int)atomicAdd(&cnt[l], 0ull));   // (this workgroup's own atomics)
    widest = ing::wave_max(widest);
    __syncthreads();
    if (tid == 0) tops = 0;
    __syncthreads();
    if ((tid & 63) == 0) atomicMax(&tops, widest);
    __syncthreads();
    if (tid == 0) { stat[0] = nlev; stat[1] = tops; }
}

// level_events[level_off[l] ...): the events of level l (level_off: the exclusive scan of cnt; cursor zeroed by the caller).
// The order inside a level is that of arrival: nothing depends on it.
__global__ void __launch_bounds__(256)
k_sign_scatter(int K, const int* __restrict__ lvl, const i64* __restrict__ level_off, int* cursor, int* level_events) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    const int l = lvl[i];
    level_events[level_off[l] + atomicAdd(&cursor[l], 1)] = i;
}

// One launch per level, one lane per event of the level.  The parents' ids come from the id index (stored parents) or from
// out.id (in-batch parents: written by the launches of the levels below, which precede this one on the stream).
// Registers: k_validate_payload is capped for three resident waves because a million events fill every SIMD many times
// over.  A level is at most a few waves wide (one event per member without forks), so here nothing shares a SIMD and the
// cap would only buy spills: one wave per SIMD, every register the hashes want (140 by the compiler's report, none spilled;
// 1 808 bytes of scratch per lane are the hash states and message schedules, which are indexed by variables).
#ifndef SWS_WAVES_PER_SIMD
#define SWS_WAVES_PER_SIMD 1
#endif
__global__ void __launch_bounds__(64, SWS_WAVES_PER_SIMD)
k_sign_level(SignIn in, SignOut out, const i64* __restrict__ level_off, const int* __restrict__ level_events, int level) {
    const i64 a = level_off[level], b = level_off[level + 1];
    const i64 j = a + (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= b) return;
    const int i = level_events[j];
    const int m = in.creator[i], s = in.sp[i], o = in.op[i];
    uint8_t spid[32], opid[32], pk[32], sig[64], id[32];
    const int ar = s < 0 ? 0 : 2;
    if (ar) {
        const uint8_t* ps = s < in.N0 ? in.stored_id + (size_t)s * 32 : out.id + (size_t)(s - in.N0) * 32;
        const uint8_t* po = o < in.N0 ? in.stored_id + (size_t)o * 32 : out.id + (size_t)(o - in.N0) * 32;
        for (int k = 0; k < 32; ++k) { spid[k] = ps[k]; opid[k] = po[k]; }
    } else {
        for (int k = 0; k < 32; ++k) { spid[k] = 0; opid[k] = 0; }
    }
    for (int k = 0; k < 32; ++k) pk[k] = in.keys[(size_t)m * 32 + k];
    const Secret sk = in.secret[m];
    const int dl = data_len(in, i);
    const Tmpl v{in.hdr, in.hdr_len, dl > 0 ? in.data + in.data_off[i] : nullptr, dl, ar, spid, opid, in.t[i], pk};
    sign_event(sk, in.rowB, v, sig, id);
    for (int k = 0; k < 32; ++k) {
        out.id[(size_t)i * 32 + k] = id[k];
        out.sp_id[(size_t)i * 32 + k] = spid[k];
        out.op_id[(size_t)i * 32 + k] = opid[k];
    }
    for (int k = 0; k < 64; ++k) out.sig[(size_t)i * 64 + k] = sig[k];
    out.arity[i] = (uint8_t)ar;
}
#endif

}  // namespace sws
