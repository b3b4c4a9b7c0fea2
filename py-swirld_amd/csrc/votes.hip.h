// Node.votes read out in bulk (sw_export_votes[_device]): every entry of the voter rounds [rv0, rv1) as a table of rows
// (voter witness y, candidate round rc) with two member bitmasks per row — which candidates of rc y has an entry for, and
// the entry's value.  Path (reference file:line): Node.decide_fame swirld.py:229-276 — the votes it stores at :258, :265
// and :272.  Value and existence of every bit are what sw_get_vote answers for the same slots; the comment above that
// function is the specification, tests/model_votes.py states the table in numpy.
//
// Nothing here holds an array with one entry per (voter, candidate round): a batch decide_fame leaves every earlier round a
// possible candidate round of every voter, and such an array would grow with rounds^2 x members.  What is kept per pair of
// rounds is one bit per voter (`rowmask`).
//
//   k_votes_prep     one workgroup per round: per witness slot the first decide_fame call that saw the witness (`born`) and
//                    the round of the voter that decided it (`rz`); the witnesses of the round ranked by dense index (the
//                    order the rows of a voter round come in); per round the latest deciding round and call (hr, hc), by
//                    which whole pairs of rounds are skipped: no voter of round rv has an entry for round rc when every
//                    witness of rc was decided by a voter of a round below rv in a call no later than the first that saw rv.
//   k_votes_lo       per voter round the lowest candidate round that is not skipped.
//   k_votes_count    one thread per voter (round, rank): rows and entries of that voter, its bit in the rowmask of every
//                    pair of rounds it has a row for.
//   k_votes_scan     ONE workgroup: exclusive scan of the rows per voter in (round, rank) order -> first row of every voter,
//                    the two totals the host reads.
//   k_votes_rows     one thread per voter again: row_voter, row_cand_round and the exists words of its rows.
//   k_votes_values   one workgroup per (candidate round, word of 64 candidates), one thread per voter slot: the election of
//                    the round replayed level by level, every witness voting (swirld.py:256-272).  The previous level is
//                    kept in LDS transposed — per candidate the member mask of the yes votes — so that with unit stake a
//                    tally is popcount(T[cand] & S[voter]) over the mask words; with stakes the set bits are weighted.
//                    A thread holds the 64 votes of its voter as ONE word, which is the word of `value` in the row phase
//                    one laid out (bits outside `exists` cleared).
// No kernel waits for another workgroup; every barrier is reached by every thread of its workgroup (no thread returns
// before the last one).  Every index comes from the context's own tables; dec_by is range-checked before it is followed.
//
// Each kernel body is a sequence of per-thread phases (plain functions of the thread index, LDS passed as pointers) with a
// barrier between them: tests/votes_emul.cpp runs the same phases thread by thread on the host, under sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace vts {

typedef unsigned long long u64;

constexpr int COUNT_THREADS = 256;
constexpr int SCAN_THREADS = 1024;
constexpr int NEVER = 0x7fffffff;      // born[] of an empty slot; hr[] of a round with an undecided witness
constexpr int C_ROWS = 0, C_ENTRIES = 1, C_LEVELS = 2, C_WORDS = 4;   // the counters (u64): this call's rows and entries, levels replayed so far

struct Tables {               // the context's tables
    const int* wit;           // [R][np] witness per (round, member), -1 none
    const u64* Sw;            // [R][np][nw] strongly seen witnesses of the round before, per witness slot
    const unsigned char* coin;   // per event: the coin bit (swirld.py:272)
    const uint32_t* stake;    // np
    const int* dec_call;      // [R][np] the decide_fame call that decided the witness, -1 undecided
    const int* dec_by;        // [R][np] the voter that decided it
    const int* round;         // per event
    long long N;              // events stored (bound of dec_by)
    int n, np, nw, nwo, coin_period;
    unsigned tot2;            // twice the total stake
};

struct Sched {                // the decide_fame calls so far (ascending, all three) and, per round, the call that put it into `consensus`
    const int* call_maxc;
    const long long* call_div;
    const int* cons_call;
    int ncalls;
};

struct Range {                // this call: voter rounds [rv0, rv1), candidate rounds from rc0 on; per voter round i = rv - rv0:
    int rv0, rv1, rc0;
    const int* lo;            // lowest candidate round the call schedule allows (rv: none)
    const int* c1v;           // last call in which the round's witnesses were voters
    const int* cf;            // first call that saw the round
    const long long* qbase;   // pair (rv, rc) has index qbase[i] + rc - lo[i]
};

struct Work {                 // scratch; per-round arrays are indexed by r - rc0
    int* born;                // [rounds][np]
    int* rz;                  // [rounds][np] round of the deciding voter, -1 undecided
    int* order;               // [rounds][np] member slot of the k-th witness by dense index
    int* rank;                // [rounds][np] the inverse, -1 no witness
    int* nwit;                // [rounds]
    int* hr;                  // [rounds] latest deciding round, NEVER while a witness is undecided, -1 no witness
    int* hc;                  // [rounds] latest deciding call
    int* lo_dev;              // [voter rounds] lowest candidate round that is not skipped
    u64* rowmask;             // [pairs][nw] bit k: the k-th voter of rv has a row for rc (zeroed before k_votes_count)
    int* vrows;               // [voter rounds][np] rows per voter
    long long* vent;          // [voter rounds][np] entries per voter
    long long* voff;          // [voter rounds][np] first row of the voter
    u64* counts;              // C_WORDS
};

struct Out {
    int* row_voter;
    int* row_cand_round;
    u64* exists;
    u64* value;
};

// ---- host: what the call records say about the voter rounds [rv0, rv1), rv0 >= 1 (no HIP in it: tests/votes_emul.cpp uses it too).
// A round rc put into `consensus` by call cc is skipped from then on (swirld.py:233), and the witnesses of round rv are first
// evaluated by the first call that saw rv (cf): rc is open for rv iff rc is not in `consensus` or cc >= cf.  Every array takes
// rv1 - rv0 entries, q one more; returns the lowest candidate round any voter round leaves open (rv0: none).
struct CallRec { int max_c, R; long long divided; };
inline int plan_rounds(const CallRec* calls, int ncalls, const int* cons_call, int rv0, int rv1, int* lo, int* c1v, int* cf, long long* q) {
    int a = 0, b = -1, open = 0, rc0 = rv0;
    q[0] = 0;
    for (int i = 0; i < rv1 - rv0; ++i) {
        const int rv = rv0 + i;
        while (a < ncalls && calls[a].R <= rv) ++a;                    // first call that saw round rv
        while (b + 1 < ncalls && calls[b + 1].max_c + 1 <= rv) ++b;    // last call in which round rv voted
        while (open < rv && cons_call[open] >= 0 && cons_call[open] < a) ++open;
        cf[i] = a;
        c1v[i] = b;
        lo[i] = b < a ? rv : (open < rv ? open : rv);
        if (lo[i] < rc0) rc0 = lo[i];
        q[i + 1] = q[i] + (rv - lo[i]);
    }
    return rc0;
}

#ifdef VTS_HOST_EMULATION
inline void atom_or64(u64* p, u64 v) { *p |= v; }
inline void atom_add64(u64* p, u64 v) { *p += v; }
inline int popc64(u64 v) { return __builtin_popcountll(v); }
inline int ctz64(u64 v) { return __builtin_ctzll(v); }
#define VTS_FN inline
#else
__device__ __forceinline__ void atom_or64(u64* p, u64 v) { atomicOr(p, v); }
__device__ __forceinline__ void atom_add64(u64* p, u64 v) { atomicAdd(p, v); }
__device__ __forceinline__ int popc64(u64 v) { return __popcll(v); }
__device__ __forceinline__ int ctz64(u64 v) { return __ffsll((long long)v) - 1; }
#define VTS_FN __device__ __forceinline__
#endif

VTS_FN int imin(int a, int b) { return a < b ? a : b; }
VTS_FN int imax(int a, int b) { return a > b ? a : b; }

// first call with `divided` >= need (ncalls: none)
VTS_FN int first_call_div(const Sched& s, long long need) {
    int a = 0, b = s.ncalls;
    while (a < b) {
        const int m = (a + b) >> 1;
        if (s.call_div[m] < need) a = m + 1; else b = m;
    }
    return a;
}

// no voter of round rv has an entry for a witness of round rc (see k_votes_prep above)
VTS_FN bool pair_skipped(const Range& g, const Work& w, int rv, int rc) {
    return rv > w.hr[rc - g.rc0] && w.hc[rc - g.rc0] <= g.cf[rv - g.rv0];
}

// ---- k_votes_prep, phase by phase (round r, one thread per member slot m)
VTS_FN void prep_slot(const Tables& t, const Sched& s, const Range& g, const Work& w, int r, int m) {
    const size_t i = (size_t)r * t.np + m, o = (size_t)(r - g.rc0) * t.np + m;
    const int e = t.wit[i];
    int b = NEVER, z = -1;
    if (e >= 0) {
        const int c0 = first_call_div(s, (long long)e + 1);
        b = c0 < s.ncalls ? c0 : NEVER;
        const int db = t.dec_by[i];
        if (t.dec_call[i] >= 0 && db >= 0 && db < t.N) z = t.round[db];
    }
    w.born[o] = b;
    w.rz[o] = z;
}

VTS_FN void prep_rank(const Tables& t, const Range& g, const Work& w, int r, int m) {
    const int* row = t.wit + (size_t)r * t.np;
    const size_t o = (size_t)(r - g.rc0) * t.np;
    const int e = row[m];
    int k = -1;
    if (e >= 0) {
        k = 0;
        for (int i = 0; i < t.np; ++i) k += row[i] >= 0 && row[i] < e;
        w.order[o + k] = m;
    }
    w.rank[o + m] = k;
    if (m == 0) {
        int cnt = 0, hr = -1, hc = -1;
        for (int i = 0; i < t.np; ++i) {
            if (row[i] < 0) continue;
            ++cnt;
            const int dc = t.dec_call[(size_t)r * t.np + i];
            if (dc < 0) hr = NEVER;
            else { hr = imax(hr, w.rz[o + i]); hc = imax(hc, dc); }
        }
        w.nwit[r - g.rc0] = cnt;
        w.hr[r - g.rc0] = hr;
        w.hc[r - g.rc0] = hc;
    }
}

// ---- k_votes_lo (one thread per voter round)
VTS_FN void lowest_round(const Range& g, const Work& w, int i) {
    const int rv = g.rv0 + i;
    int rc = g.lo[i];
    while (rc < rv && pair_skipped(g, w, rv, rc)) ++rc;
    w.lo_dev[i] = rc;
}

// The entries of voter y = witness (rv, .) for candidates 64 j .. 64 j + 63 of round rc, as sw_get_vote decides them: calls
// c0 .. c1 in which y evaluated x, c0 = the first call that saw both, c1 = the last call in which y was a voter (c1v), capped
// by the call that put rc into `consensus` and by the call that decided x — that call itself only for a voter before the
// deciding one in voter order (rounds ascending, dense index inside a round), which stores nothing itself.
VTS_FN u64 exist_word(const Tables& t, const Sched& s, const Range& g, const Work& w, int rv, int y, int by, int c1v, int rc, int j) {
    const int cc = s.cons_call[rc];
    const int c1r = cc >= 0 ? imin(c1v, cc) : c1v;
    if (c1r < by) return 0;
    u64 word = 0;
    const int m1 = imin(64, t.n - 64 * j);
    for (int b = 0; b < m1; ++b) {
        const size_t i = (size_t)rc * t.np + 64 * j + b, o = (size_t)(rc - g.rc0) * t.np + 64 * j + b;
        const int bx = w.born[o];
        if (bx == NEVER) continue;
        const int c0 = imax(by, bx);
        int c1 = c1r;
        const int dc = t.dec_call[i];
        if (dc >= 0) {
            const int db = t.dec_by[i], z = w.rz[o];
            const bool before = y != db && (rv < z || (rv == z && y < db));
            c1 = imin(c1, before ? dc : dc - 1);
        }
        if (c1 >= c0) word |= 1ull << b;
    }
    return word;
}

// ---- k_votes_count / k_votes_rows (one thread per voter: round rv0 + i, rank k); out == nullptr counts
VTS_FN void voter_rows(const Tables& t, const Sched& s, const Range& g, const Work& w, const Out* out, int i, int k) {
    const int rv = g.rv0 + i;
    const size_t vi = (size_t)i * t.np + k;
    int rows = 0;
    long long ent = 0;
    if (k < w.nwit[rv - g.rc0]) {
        const int mv = w.order[(size_t)(rv - g.rc0) * t.np + k];
        const int y = t.wit[(size_t)rv * t.np + mv];
        const int by = w.born[(size_t)(rv - g.rc0) * t.np + mv];
        const int c1v = g.c1v[i];
        long long row = out ? w.voff[vi] : 0;
        for (int rc = w.lo_dev[i]; rc < rv && by != NEVER; ++rc) {
            if (pair_skipped(g, w, rv, rc)) continue;
            u64* mask = w.rowmask + (size_t)(g.qbase[i] + rc - g.lo[i]) * t.nw + (k >> 6);
            if (out) {
                if (!((*mask >> (k & 63)) & 1ull)) continue;
                for (int j = 0; j < t.nwo; ++j) out->exists[(size_t)row * t.nwo + j] = exist_word(t, s, g, w, rv, y, by, c1v, rc, j);
                out->row_voter[row] = y;
                out->row_cand_round[row] = rc;
                ++row;
            } else {
                int cnt = 0;
                for (int j = 0; j < t.nwo; ++j) cnt += popc64(exist_word(t, s, g, w, rv, y, by, c1v, rc, j));
                if (!cnt) continue;
                atom_or64(mask, 1ull << (k & 63));
                ++rows;
                ent += cnt;
            }
        }
    }
    if (!out) { w.vrows[vi] = rows; w.vent[vi] = ent; }
}

// ---- k_votes_scan, phase by phase (V voters; s_rows, s_ent: SCAN_THREADS words of LDS each)
VTS_FN void scan_sum(const Work& w, long long V, int tid, long long* s_rows, long long* s_ent) {
    const long long chunk = (V + SCAN_THREADS - 1) / SCAN_THREADS;
    long long a = 0, b = 0;
    for (long long i = tid * chunk; i < (tid + 1) * chunk && i < V; ++i) { a += w.vrows[i]; b += w.vent[i]; }
    s_rows[tid] = a;
    s_ent[tid] = b;
}
VTS_FN void scan_top(const Work& w, int tid, long long* s_rows, long long* s_ent) {
    if (tid) return;
    long long a = 0, b = 0;
    for (int i = 0; i < SCAN_THREADS; ++i) { const long long x = s_rows[i]; s_rows[i] = a; a += x; b += s_ent[i]; }
    w.counts[C_ROWS] = (u64)a;
    w.counts[C_ENTRIES] = (u64)b;
}
VTS_FN void scan_write(const Work& w, long long V, int tid, const long long* s_rows) {
    const long long chunk = (V + SCAN_THREADS - 1) / SCAN_THREADS;
    long long a = s_rows[tid];
    for (long long i = tid * chunk; i < (tid + 1) * chunk && i < V; ++i) { w.voff[i] = a; a += w.vrows[i]; }
}

// ---- k_votes_values, phase by phase (candidate round rc, candidate word j; LDS: s_T[64][nw] the previous level transposed,
// s_W[np] this level's vote words, s_stake[np], s_ctl[1] the levels to replay)
VTS_FN void val_begin(const Tables& t, const Range& g, const Work& w, int rc, int j, int tid, unsigned* s_stake, int* s_ctl) {
    s_stake[tid] = t.stake[tid];
    if (tid) return;
    int last = rc;   // the last voter round with a row for rc
    for (int rv = imax(rc + 1, g.rv0); rv < g.rv1; ++rv)
        if (rc >= w.lo_dev[rv - g.rv0] && !pair_skipped(g, w, rv, rc)) last = rv;
    s_ctl[0] = last - rc;
    if (j == 0) atom_add64(w.counts + C_LEVELS, (u64)(last - rc));
}

VTS_FN unsigned wsum(u64 m, const unsigned* stake) {
    unsigned s = 0;
    while (m) { s += stake[ctz64(m)]; m &= m - 1; }
    return s;
}

// the votes of voter slot v at level d (round rc + d) on the candidates of word j
template <bool UNIT>
VTS_FN u64 val_vote(const Tables& t, int rc, int j, int d, int v, const u64* s_T, const unsigned* s_stake) {
    const int rv = rc + d;
    const int y = t.wit[(size_t)rv * t.np + v];
    if (y < 0) return 0;
    const u64* S = t.Sw + ((size_t)rv * t.np + v) * t.nw;
    if (d == 1) return S[j];                     // x in s (swirld.py:258)
    unsigned yes[64], all = 0;
#pragma unroll
    for (int b = 0; b < 64; ++b) yes[b] = 0;
    for (int wd = 0; wd < t.nw; ++wd) {
        const u64 s = S[wd];
        if (UNIT) {
            all += (unsigned)popc64(s);
#pragma unroll
            for (int b = 0; b < 64; ++b) yes[b] += (unsigned)popc64(s_T[b * t.nw + wd] & s);
        } else {
            all += wsum(s, s_stake + 64 * wd);
#pragma unroll
            for (int b = 0; b < 64; ++b) yes[b] += wsum(s_T[b * t.nw + wd] & s, s_stake + 64 * wd);
        }
    }
    const bool coin_round = d % t.coin_period == 0;
    const u64 coin = coin_round ? (u64)(t.coin[y] & 1) : 0;
    u64 word = 0;
#pragma unroll
    for (int b = 0; b < 64; ++b) {
        const unsigned no = all - yes[b];
        u64 vote = !(no > yes[b]);               // majority(): a tie is True (swirld.py:24-27)
        const u64 tt = vote ? yes[b] : no;
        if (coin_round && !(3 * tt > t.tot2)) vote = coin;   // swirld.py:272
        word |= vote << b;
    }
    return word;
}

// ... kept for the next level, and written to the voter's row for rc where it has one
VTS_FN void val_store(const Tables& t, const Range& g, const Work& w, const Out& out, int rc, int j, int d, int v, u64 word, u64* s_W) {
    s_W[v] = word;
    const int rv = rc + d, i = rv - g.rv0;
    if (rv < g.rv0 || rc < w.lo_dev[i]) return;
    const int k = w.rank[(size_t)(rv - g.rc0) * t.np + v];
    if (k < 0) return;
    const long long q0 = g.qbase[i] - g.lo[i];   // pair (rv, r) has index q0 + r
    const u64* mask = w.rowmask + (k >> 6);
    if (!((mask[(size_t)(q0 + rc) * t.nw] >> (k & 63)) & 1ull)) return;
    long long row = w.voff[(size_t)i * t.np + k];
    for (int r = w.lo_dev[i]; r < rc; ++r) row += (long long)((mask[(size_t)(q0 + r) * t.nw] >> (k & 63)) & 1ull);
    out.value[(size_t)row * t.nwo + j] = word & out.exists[(size_t)row * t.nwo + j];
}

// s_T[b][wd] = bit b of the vote words of voters 64 wd .. 64 wd + 63 (np = 64 nw items, one per thread)
VTS_FN void val_transpose(const Tables& t, int item, const u64* s_W, u64* s_T) {
    const int b = item / t.nw, wd = item - b * t.nw;
    u64 m = 0;
    for (int i = 0; i < 64; ++i) m |= ((s_W[64 * wd + i] >> b) & 1ull) << i;
    s_T[b * t.nw + wd] = m;
}

#ifndef VTS_HOST_EMULATION
__global__ void __launch_bounds__(1024) k_votes_prep(Tables t, Sched s, Range g, Work w) {
    const int r = g.rc0 + (int)blockIdx.x, m = (int)threadIdx.x;
    prep_slot(t, s, g, w, r, m);
    __syncthreads();
    prep_rank(t, g, w, r, m);
}

__global__ void __launch_bounds__(COUNT_THREADS) k_votes_lo(Range g, Work w) {
    const int i = (int)(blockIdx.x * COUNT_THREADS + threadIdx.x);
    if (i < g.rv1 - g.rv0) lowest_round(g, w, i);
}

template <bool WRITE>
__global__ void __launch_bounds__(COUNT_THREADS) k_votes_rows(Tables t, Sched s, Range g, Work w, Out out) {
    const long long tid = (long long)blockIdx.x * COUNT_THREADS + threadIdx.x;
    const int i = (int)(tid / t.np), k = (int)(tid - (long long)i * t.np);
    if (i < g.rv1 - g.rv0) voter_rows(t, s, g, w, WRITE ? &out : nullptr, i, k);
}

__global__ void __launch_bounds__(SCAN_THREADS) k_votes_scan(Work w, long long V) {
    __shared__ long long s_rows[SCAN_THREADS], s_ent[SCAN_THREADS];
    const int tid = (int)threadIdx.x;
    scan_sum(w, V, tid, s_rows, s_ent);
    __syncthreads();
    scan_top(w, tid, s_rows, s_ent);
    __syncthreads();
    scan_write(w, V, tid, s_rows);
}

// workgroup = np threads; dynamic LDS: (64 nw + np) u64, np unsigned, 4 int
template <bool UNIT>
__global__ void __launch_bounds__(1024) k_votes_values(Tables t, Range g, Work w, Out out) {
    extern __shared__ u64 s_votes[];
    u64* s_T = s_votes;
    u64* s_W = s_T + 64 * t.nw;
    unsigned* s_stake = (unsigned*)(s_W + t.np);
    int* s_ctl = (int*)(s_stake + t.np);
    const int rc = g.rc0 + (int)blockIdx.x / t.nwo, j = (int)blockIdx.x % t.nwo, tid = (int)threadIdx.x;
    val_begin(t, g, w, rc, j, tid, s_stake, s_ctl);
    __syncthreads();
    const int levels = s_ctl[0];
    for (int d = 1; d <= levels; ++d) {
        val_store(t, g, w, out, rc, j, d, tid, val_vote<UNIT>(t, rc, j, d, tid, s_T, s_stake), s_W);
        __syncthreads();
        val_transpose(t, tid, s_W, s_T);
        __syncthreads();
    }
}
#endif

}  // namespace vts
