// The gossip histories of a batch, generated on the device (include/swirld_hip.h: sw_synth_batch*):
// sw_synth_hashgraph (synth.cpp) per hashgraph, bit for bit, in instalments — one wavefront per participating hashgraph,
// one launch.  The specification is synth.cpp; every statement here that draws from a generator or compares doubles is
// that file's, in its order:
//   - the DAG stream is a dependency chain (head[], the rejection loop of mode 1, the walk of mode 3): lane 0 alone runs
//     it, a chunk of events at a time into a small table, and the whole wave stores the chunk;
//   - the signature stream is independent of the DAG and is 64 of the 88 bytes of an event: every lane steps the same
//     generator (wave-uniform, no lane waits for another), keeps its own two words, and the wave stores 16 bytes per lane
//     into the 64-byte-aligned signature rows.
// Exact arithmetic: below() is the high half of a 64x64-bit product; unit() is (next() >> 11) * 2^-53; every double
// expression is ONE product or ONE sum (unit() < p0, cum[mid] > u with u = unit() * cum[n - 1], cum[] accumulated by
// additions in member order, (int)(p0 * n)), so there is nothing a compiler could contract into a fused multiply-add.
//
// State per hashgraph (a device allocation of its own, sw_batch owns it): the parameters and cum[] (written by begin,
// constant afterwards) and TWO copies of what a call advances — both generators and head[].  A call reads the current
// copy and writes the other one; the events go straight into the slab slots behind the stored events, which nothing reads
// before the host has advanced its count.  The host flips `current` only once the whole batch has passed the capacity
// checks: a refused call leaves no trace.
// The functions are SWX_HD: tests/batch_synth_main.cpp runs them on the host (one lane) under the sanitizers.
#pragma once

#include <cstdint>
#include <cstring>

#ifndef SWX_HD   // (exact.hip.h's, where that file has not been included: the stand-alone host program)
#if defined(__HIPCC__) && !defined(SW_EXACT_HOST)
#define SWX_HD __device__
#define SWX_DEVICE 1
#else
#define SWX_HD
#define SWX_DEVICE 0
#endif
#endif

namespace swbs {

typedef uint64_t u64;

constexpr int CHUNK = 64;   // events lane 0 generates before the wave stores them

#if SWX_DEVICE
struct Lanes {
    static constexpr int nl = 64;
    static __device__ int lane() { return (int)threadIdx.x; }
    static __device__ void sync() { __syncthreads(); }   // one wave per workgroup
};
#else
struct Lanes {
    static constexpr int nl = 1;
    static int lane() { return 0; }
    static void sync() {}
};
#endif

SWX_HD inline u64 mulhi(u64 a, u64 b) {
#if SWX_DEVICE
    return __umul64hi(a, b);
#else
    return (u64)(((unsigned __int128)a * b) >> 64);
#endif
}

// synth.cpp's Xoshiro over a state that lives elsewhere
struct Rng {
    u64 s[4];
    SWX_HD static u64 rotl(u64 x, int k) { return (x << k) | (x >> (64 - k)); }
    SWX_HD u64 next() {
        const u64 r = rotl(s[1] * 5, 7) * 9, t = s[1] << 17;
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t; s[3] = rotl(s[3], 45);
        return r;
    }
    SWX_HD uint32_t below(uint32_t n) { return (uint32_t)mulhi(next(), (u64)n); }
    SWX_HD double unit() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    SWX_HD void seed(u64 x) {
        for (int i = 0; i < 4; ++i) {   // splitmix
            u64 z = (x += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            s[i] = z ^ (z >> 31);
        }
    }
};

struct Par { int mode, pad; double p0, p1; };   // followed by cum[n]
struct Mut { Rng dag, sig; };                   // followed by head[n]
static_assert(sizeof(Par) == 24 && sizeof(Mut) == 64, "state layout");

// where the state of hashgraph b lies in the allocation: [Par, cum[n]] [Mut, head[n]] x 2, each rounded up to 64 bytes
struct StateLayout {
    u64 par_bytes, mut_bytes, stride;
    SWX_HD const Par* par(const unsigned char* base, u64 b) const { return (const Par*)(base + b * stride); }
    SWX_HD const double* cum(const unsigned char* base, u64 b) const { return (const double*)(base + b * stride + 32); }
    SWX_HD const Mut* mut(const unsigned char* base, u64 b, int k) const { return (const Mut*)(base + b * stride + par_bytes + (u64)k * mut_bytes); }
    SWX_HD const int* head(const unsigned char* base, u64 b, int k) const { return (const int*)((const unsigned char*)mut(base, b, k) + sizeof(Mut)); }
};
inline StateLayout state_layout(int n) {
    StateLayout l;
    l.par_bytes = (32 + (u64)n * 8 + 63) / 64 * 64;
    l.mut_bytes = (sizeof(Mut) + (u64)n * 4 + 63) / 64 * 64;
    l.stride = l.par_bytes + 2 * l.mut_bytes;
    return l;
}

// the per-event arrays of one hashgraph (a slab's, or the host program's exactly-sized allocations)
struct Slab {
    int *cr, *sp, *op, *ht, *round;
    double* t;
    unsigned char* sig;   // 64 B per event, 16-byte aligned
    unsigned char* tbd;
    signed char* fam_ev;
    long long cap_events;
};

// one hashgraph's share of a call
struct Task {
    int n;
    long long first, K;   // it holds `first` events and generates [first, first + K)
    const Par* par;
    const double* cum;    // [n], read in mode 2 only
    const Mut* in;        // the current copy ...
    const int* head_in;
    Mut* out;             // ... and the one this call writes
    int* head_out;
};

enum { R_HEIGHT = 0, R_ERROR = 1 };   // result words: greatest height generated (-1: none), nonzero = refused arguments

// what the chunk table holds of the events [base, base + CHUNK)
struct Chunk { int cr[CHUNK], sp[CHUNK], op[CHUNK], ht[CHUNK]; };

// sw_synth_batch_begin for one hashgraph, by one thread: both generators seeded, cum[] accumulated as synth.cpp does
SWX_HD inline void begin(int n, u64 seed, int mode, double p0, double p1, Par* par, double* cum, Mut* m) {
    par->mode = mode; par->pad = 0; par->p0 = p0; par->p1 = p1;
    m->dag.seed(seed * 0x2545F4914F6CDD1Dull + 0x1234567ull + (u64)mode);
    m->sig.seed(seed ^ 0xA5A5A5A5DEADBEEFull);
    if (mode == 2) {
        int n_slow = (int)(p0 * n);
        if (n_slow >= n) n_slow = n - 1;
        double acc = 0;
        for (int c = 0; c < n; ++c) { acc += (c >= n - n_slow) ? p1 : 1.0; cum[c] = acc; }
    }
}

// The events [first, first + K) of one hashgraph.  head: n ints and ch: one Chunk, shared by the wave (LDS).
SWX_HD inline void generate(const Slab& s, const Task& g, int* head, Chunk* ch, int* result) {
    const int lane = Lanes::lane(), n = g.n;
    const long long first = g.first, K = g.K;
    if (n < 2 || first < 0 || K < 0 || first + K > s.cap_events || (first == 0 && K > 0 && K < n) || (first > 0 && first < n)) {
        if (lane == 0) { result[R_HEIGHT] = -1; result[R_ERROR] = 1; }   // (the host has checked all of it: never taken)
        return;
    }
    for (int i = lane; i < n; i += Lanes::nl) head[i] = g.head_in[i];
    Rng dag = g.in->dag;
    const int mode = g.par->mode;
    const double p0 = g.par->p0;
    const int half = n / 2;
    const bool cliques = mode == 1 && half >= 2 && n - half >= 2;
    const double cum_last = mode == 2 ? g.cum[n - 1] : 0.0;
    int hmax = -1;
    Lanes::sync();
    for (long long done = 0; done < K; done += CHUNK) {
        const long long base = first + done;
        const int m = K - done < CHUNK ? (int)(K - done) : CHUNK;
        if (lane == 0) {
            for (int j = 0; j < m; ++j) {
                const long long i = base + j;
                int a, sp, o, h;
                if (i < n) {   // one root per member
                    a = (int)i; sp = -1; o = -1; h = 0;
                } else {
                    int b;
                    if (mode == 2) {
                        const double u = dag.unit() * cum_last;
                        int lo = 0, hi = n - 1;
                        while (lo < hi) { const int mid = (lo + hi) / 2; if (g.cum[mid] > u) hi = mid; else lo = mid + 1; }
                        a = lo;
                    } else {
                        a = (int)dag.below((uint32_t)n);
                    }
                    if (cliques) {
                        const bool cross = dag.unit() < p0;
                        const bool a_low = a < half;
                        const bool pick_low = cross ? !a_low : a_low;
                        const int lowest = pick_low ? 0 : half, cnt = pick_low ? half : n - half;
                        do { b = lowest + (int)dag.below((uint32_t)cnt); } while (b == a);
                    } else {
                        b = (int)dag.below((uint32_t)(n - 1));
                        if (b >= a) ++b;
                    }
                    o = head[b];
                    if (mode == 3) {
                        for (;;) {   // stale other-parent: back along the peer's self-parent chain
                            const int back = o >= base ? ch->sp[o - base] : s.sp[o];
                            if (back < 0 || !(dag.unit() < p0)) break;
                            o = back;
                        }
                    }
                    sp = head[a];
                    const int hs = sp >= base ? ch->ht[sp - base] : s.ht[sp], ho = o >= base ? ch->ht[o - base] : s.ht[o];
                    h = (hs > ho ? hs : ho) + 1;   // swirld.py:117-120
                }
                head[a] = (int)i;
                ch->cr[j] = a; ch->sp[j] = sp; ch->op[j] = o; ch->ht[j] = h;
                if (h > hmax) hmax = h;
            }
        }
        Lanes::sync();
        for (int j = lane; j < m; j += Lanes::nl) {   // the chunk into the slab, with the per-event defaults of k_batch_scatter
            const long long e = base + j;
            s.cr[e] = ch->cr[j]; s.sp[e] = ch->sp[j]; s.op[e] = ch->op[j]; s.ht[e] = ch->ht[j];
            s.t[e] = (double)e;
            s.round[e] = -1; s.tbd[e] = 1; s.fam_ev[e] = -1;
        }
        Lanes::sync();   // the chunk is in memory before lane 0 reads it from there, and read before it is rewritten
    }
    // the signatures: piece q of the call is 16 bytes, the words 2q and 2q + 1 of the stream from where the last call stopped
    Rng sg = g.in->sig;
    const long long pieces = 4 * K;
    for (long long at = 0; at < pieces; at += Lanes::nl) {
        const int cnt = pieces - at < Lanes::nl ? (int)(pieces - at) : Lanes::nl;
        u64 w0 = 0, w1 = 0;
        for (int j = 0; j < cnt; ++j) {
            const u64 r0 = sg.next(), r1 = sg.next();
            if (j == lane) { w0 = r0; w1 = r1; }
        }
        if (lane < cnt) {
            unsigned char* out = s.sig + (size_t)(4 * first + at + lane) * 16;
#if SWX_DEVICE
            *(uint4*)out = make_uint4((unsigned)w0, (unsigned)(w0 >> 32), (unsigned)w1, (unsigned)(w1 >> 32));
#else
            memcpy(out, &w0, 8); memcpy(out + 8, &w1, 8);   // (little endian, as the device)
#endif
        }
    }
    // the copy the next call reads, should the host accept this one
    for (int i = lane; i < n; i += Lanes::nl) g.head_out[i] = head[i];
    if (lane == 0) {
        g.out->dag = dag; g.out->sig = sg;
        result[R_HEIGHT] = hmax; result[R_ERROR] = 0;
    }
}

}  // namespace swbs

#if SWX_DEVICE
// ---- kernels ---------------------------------------------------------------------------------------
// One workgroup of one wavefront per PARTICIPATING hashgraph (a compact list, as k_batch_step's).  cur[i]: which copy of
// the state is current.  res: two ints per list entry.
__global__ void __launch_bounds__(64) k_batch_synth(const swb::Rec* recs, unsigned char* state, swbs::StateLayout sl, const int* who,
                                                    const int* cur, const long long* first, const long long* K, int* res) {
    __shared__ int head[SW_MAX_MEMBERS];
    __shared__ swbs::Chunk ch;
    const unsigned i = blockIdx.x;
    const int b = who[i], k = cur[i] & 1;
    const swb::Rec& r = recs[b];
    swbs::Slab s;
    s.cr = (int*)r.s.cr; s.sp = (int*)r.s.sp; s.op = (int*)r.s.op; s.ht = (int*)r.s.ht; s.round = r.s.round;
    s.t = (double*)r.s.t; s.sig = (unsigned char*)r.s.sig; s.tbd = r.s.tbd; s.fam_ev = r.s.fam_ev; s.cap_events = r.cap_events;
    swbs::Task g;
    g.n = r.s.n; g.first = first[i]; g.K = K[i];
    g.par = sl.par(state, (unsigned)b); g.cum = sl.cum(state, (unsigned)b);
    g.in = sl.mut(state, (unsigned)b, k); g.head_in = sl.head(state, (unsigned)b, k);
    g.out = (swbs::Mut*)sl.mut(state, (unsigned)b, k ^ 1); g.head_out = (int*)sl.head(state, (unsigned)b, k ^ 1);
    swbs::generate(s, g, head, &ch, res + 2 * (size_t)i);
}

// sw_synth_batch_begin: one thread per selected hashgraph; copy 0 becomes the current one
__global__ void __launch_bounds__(64) k_batch_synth_begin(unsigned char* state, swbs::StateLayout sl, int n, long long m, const int* who,
                                                          const int* mode, const unsigned long long* seed, const double* p0, const double* p1) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const unsigned b = (unsigned)who[i];
    swbs::begin(n, seed[i], mode[i], p0[i], p1[i], (swbs::Par*)sl.par(state, b), (double*)sl.cum(state, b), (swbs::Mut*)sl.mut(state, b, 0));
}
#endif
