// Answering a sync from a forked hashgraph on the device (sw_sync_walk, sw_export_walk[_device], sw_sync_pull_walk,
// sw_get_fork_trunks): the reference's height-pruned walk itself instead of the per-member chain ranges of k_sync_diff,
// which describe the answer only while every member's events form ONE chain.
// Path (reference file:line): Node.ask_sync swirld.py:148-161 — a BFS from the head over the parents (swirld.py:154-161)
// that does not descend into an event whose height the asker reported knowing; what the reference then pickles per event,
// swirld.py:76-95, is gathered through gsp::export_piece.  tests/model_walk.py states the set, the list, the slot contents
// and the trunk heights in numpy.
//
// Four kernels:
//   k_walk_bfs      ONE workgroup, level-synchronous: the frontiers lie one behind the other in ONE queue of at most head + 1
//                   entries, the threads stride over the current level [begin, end), a parent that passes the height test is
//                   claimed by an atomicOr on its bit of the visited bitmap and appended by the claimer alone.  The pruning
//                   heights are staged in LDS as min(known, cap) per member.  One barrier per level: the tail of level k is
//                   counted in s_cnt[k % 3], which was zeroed during level k - 1, so no thread can still be reading it.
//                   Writes {count, levels, error, lowest claimed event} to the header.
//   k_walk_list     ONE workgroup: the bitmap words between the lowest claimed event and the head, compacted into the
//                   ascending list of dense indices (count per thread | scan | write).
//   k_walk_gather   over the output slots: slot s takes event list[s] of member cr[list[s]]; G lanes share a slot and deal
//                   the 13 pieces of gsp::export_piece among them, as k_export_gather does.
//   k_fork_trunks   over the events: the SECOND child that counts itself at a self-parent p lowers trunk[cr[p]] to ht[p], the
//                   second root of a member lowers it to -1: the minimum over the fork points, whatever the order.
// Every index a kernel follows comes from the context's own tables, and is bounds-checked where a wrong table entry would
// take a write outside its array; the asker's heights are compared and nowhere used as an index.  No kernel waits for
// another workgroup, and k_walk_bfs ends whatever the tables hold: at most head + 2 levels, and a queue slot beyond the
// capacity sets the error word and stops the walk.
//
// Each kernel body is a sequence of per-thread phases (plain functions of the thread index, LDS passed as a pointer) with a
// barrier between them: tests/walk_emul.cpp runs the same phases thread by thread on the host, under sanitizers.
#pragma once
#include "gossip.hip.h"

namespace wlk {

constexpr int MAX_THREADS = 1024;      // k_walk_bfs: the workgroup size is a knob of the context (SW_WALK_THREADS)
constexpr int LIST_THREADS = 256;
constexpr int GATHER_THREADS = 256;
constexpr int TRUNK_THREADS = 256;
constexpr int NO_CAP = 0x7fffffff;     // trunk[c] of a member that has not forked; cap[c] that caps nothing

// the header both walk kernels share
constexpr int H_COUNT = 0, H_LEVELS = 1, H_ERR = 2, H_MIN = 3, H_LISTED = 4, H_WORDS = 8;
constexpr int E_QUEUE = 1, E_TABLE = 2, E_LEVELS = 3, E_LIST = 4;   // values of the error word
// the control words of k_walk_bfs in LDS, behind the n pruning heights
constexpr int C_CNT = 0 /* 3 words */, C_ERR = 3, C_MIN = 4, C_WORDS = 8;
constexpr int STOP = 0x40000000;       // ORed into a level's counter with an error: every thread reads it behind the barrier

struct WalkIn {     // the answering context's tables
    const int* sp;
    const int* op;
    const int* cr;
    const int* ht;
    int n, head;
};

#ifdef GSP_HOST_EMULATION
inline unsigned atom_or(unsigned* p, unsigned v) { const unsigned o = *p; *p = o | v; return o; }
inline int atom_add(int* p, int v) { const int o = *p; *p = o + v; return o; }
inline int atom_min(int* p, int v) { const int o = *p; if (v < o) *p = v; return o; }
inline int popc(unsigned v) { return __builtin_popcount(v); }
inline int ctz(unsigned v) { return __builtin_ctz(v); }
#else
__device__ __forceinline__ unsigned atom_or(unsigned* p, unsigned v) { return atomicOr(p, v); }
__device__ __forceinline__ int atom_add(int* p, int v) { return atomicAdd(p, v); }
__device__ __forceinline__ int atom_min(int* p, int v) { return atomicMin(p, v); }
__device__ __forceinline__ int popc(unsigned v) { return __popc(v); }
__device__ __forceinline__ int ctz(unsigned v) { return __ffs((int)v) - 1; }
#endif

// an error inside level `lvl`: the code for the header, and the level's counter marked so that the whole workgroup leaves
// the loop at the same barrier (C_ERR itself may be written while slower threads still test the previous level)
__device__ __forceinline__ void walk_error(int* s_ctl, int* cnt, int code) {
    s_ctl[C_ERR] = code;
    atom_or((unsigned*)cnt, (unsigned)STOP);
}

// ---- k_walk_bfs, phase by phase (s_known: n ints of LDS, s_ctl: C_WORDS)
// the pruning heights, and the head as level 0 (the bitmap arrives zeroed)
__device__ __forceinline__ void walk_stage(int tid, int threads, const WalkIn& in, const int* known, const int* cap, int* s_known, int* s_ctl,
                                           unsigned* bits, int* queue) {
    for (int c = tid; c < in.n; c += threads) {
        int k = known ? known[c] : -1;
        if (cap) { const int t = cap[c]; if (t < k) k = t; }
        s_known[c] = k;
    }
    if (tid == 0) {
        s_ctl[C_CNT] = 0; s_ctl[C_CNT + 1] = 0; s_ctl[C_CNT + 2] = 0;
        s_ctl[C_ERR] = 0;
        s_ctl[C_MIN] = in.head;
        bits[in.head >> 5] = 1u << (in.head & 31);
        queue[0] = in.head;
    }
}

// level `lvl` = queue[begin .. end): its parents that the asker lacks are claimed and appended from `end` on
__device__ __forceinline__ void walk_expand(int tid, int threads, const WalkIn& in, int lvl, int begin, int end, const int* s_known, int* s_ctl,
                                            unsigned* bits, int* queue) {
    if (tid == 0) s_ctl[C_CNT + (lvl + 1) % 3] = 0;   // (read last behind the barrier of level lvl - 2)
    int* cnt = s_ctl + C_CNT + lvl % 3;
    for (int i = begin + tid; i < end; i += threads) {
        const int e = queue[i];
        for (int k = 0; k < 2; ++k) {
            const int p = k ? in.op[e] : in.sp[e];
            if (p < 0) continue;                      // a root
            if (p >= e) { walk_error(s_ctl, cnt, E_TABLE); continue; }   // (parents have lower indices: e <= head bounds the bitmap)
            const int c = in.cr[p];
            if (c < 0 || c >= in.n) { walk_error(s_ctl, cnt, E_TABLE); continue; }
            const int kn = s_known[c];
            if (kn >= 0 && in.ht[p] <= kn) continue;  // the asker has it (swirld.py:157-159)
            const unsigned bit = 1u << (p & 31);
            if (atom_or(bits + (p >> 5), bit) & bit) continue;   // claimed before: by another child, maybe of this level
            const long long slot = (long long)end + atom_add(cnt, 1);
            if (slot > in.head) { walk_error(s_ctl, cnt, E_QUEUE); continue; }
            queue[slot] = p;
            atom_min(s_ctl + C_MIN, p);
        }
    }
}

__device__ __forceinline__ void walk_finish(int tid, int count, int levels, bool overrun, const int* s_ctl, int* hdr) {
    if (tid != 0) return;
    hdr[H_COUNT] = count;
    hdr[H_LEVELS] = levels;
    hdr[H_ERR] = s_ctl[C_ERR] ? s_ctl[C_ERR] : (overrun ? E_LEVELS : 0);
    hdr[H_MIN] = s_ctl[C_MIN];
}

// ---- k_walk_list, phase by phase (part: LIST_THREADS ints of LDS).  The words [w0, w1] are dealt in consecutive runs.
__device__ __forceinline__ void list_bounds(const int* hdr, int head, int* w0, int* per) {
    int lo = hdr[H_MIN];
    if (lo < 0 || lo > head) lo = 0;
    *w0 = lo >> 5;
    const int words = (head >> 5) - *w0 + 1;
    *per = (words + LIST_THREADS - 1) / LIST_THREADS;
}
__device__ __forceinline__ void list_count(int tid, const unsigned* bits, int head, const int* hdr, int* part) {
    int w0, per;
    list_bounds(hdr, head, &w0, &per);
    const int w1 = head >> 5;
    int sum = 0;
    for (int j = 0; j < per; ++j) {
        const long long w = (long long)w0 + (long long)tid * per + j;
        if (w <= w1) sum += popc(bits[w]);
    }
    part[tid] = sum;
}
__device__ __forceinline__ void list_scan(int tid, int* part, int* hdr) {
    if (tid != 0) return;
    int run = 0;
    for (int k = 0; k < LIST_THREADS; ++k) { const int v = part[k]; part[k] = run; run += v; }
    hdr[H_LISTED] = run;
    if (run != hdr[H_COUNT] && !hdr[H_ERR]) hdr[H_ERR] = E_LIST;
}
__device__ __forceinline__ void list_write(int tid, const unsigned* bits, int head, const int* hdr, const int* part, int* list) {
    int w0, per;
    list_bounds(hdr, head, &w0, &per);
    const int w1 = head >> 5, count = hdr[H_COUNT];
    int at = part[tid];
    for (int j = 0; j < per; ++j) {
        const long long w = (long long)w0 + (long long)tid * per + j;
        if (w > w1) return;
        unsigned v = bits[w];
        while (v) {
            const int b = ctz(v);
            v &= v - 1;
            if (at < count) list[at] = (int)(w * 32 + b);   // (count bounds the list whatever the bitmap holds)
            ++at;
        }
    }
}

// ---- k_walk_gather: slot s <- event list[s]
template <int G>
__device__ __forceinline__ void walk_slots(int tid, int threads, unsigned block, unsigned blocks, const gsp::ExportIn& in, const gsp::ExportOut& out,
                                           const int* list, const int* cr, int total) {
    const int per = threads / G;
    const int lane = tid % G;
    for (long long s0 = (long long)block * per; s0 < total; s0 += (long long)blocks * per) {
        const long long sl = s0 + tid / G;
        if (sl >= total) continue;
        const int s = (int)sl;
        const int e = list[s];
        const int m = cr[e];
        for (int q = lane; q < gsp::PIECES; q += G) gsp::export_piece(in, out, q, s, m, e);
    }
}

// ---- k_fork_trunks: children[N] and roots[n] arrive zeroed, trunk[n] filled with NO_CAP
__device__ __forceinline__ void fork_event(long long e, const int* sp, const int* cr, const int* ht, int n, long long N, int* children, int* roots,
                                           int* trunk) {
    const int c = cr[e];
    if (c < 0 || c >= n) return;
    const int p = sp[e];
    if (p < 0) {
        if (atom_add(roots + c, 1) >= 1) atom_min(trunk + c, -1);           // a second root: nothing of c is common to all
    } else if (p < N) {
        if (atom_add(children + p, 1) == 1) atom_min(trunk + c, ht[p]);     // the second child of p: p is a fork point
    }
}

#ifndef GSP_HOST_EMULATION
__global__ void __launch_bounds__(MAX_THREADS)
k_walk_bfs(WalkIn in, const int* __restrict__ known, const int* __restrict__ cap, unsigned* bits, int* queue, int* hdr) {
    extern __shared__ int s_walk[];   // n pruning heights, then the control words
    int* s_known = s_walk;
    int* s_ctl = s_walk + in.n;
    const int tid = threadIdx.x, threads = blockDim.x;
    walk_stage(tid, threads, in, known, cap, s_known, s_ctl, bits, queue);
    __syncthreads();
    int begin = 0, end = 1, lvl = 0;
    const int max_levels = in.head + 2;
    while (begin < end && lvl < max_levels) {
        walk_expand(tid, threads, in, lvl, begin, end, s_known, s_ctl, bits, queue);
        __syncthreads();   // workgroup-scope release / acquire: the queue entries and the counter of this level
        const int added = s_ctl[C_CNT + lvl % 3];
        if ((unsigned)added >= (unsigned)STOP) break;   // an error: the same word for every thread
        begin = end;
        end += added;
        ++lvl;
    }
    walk_finish(tid, end, lvl, begin < end, s_ctl, hdr);
}

__global__ void __launch_bounds__(LIST_THREADS)
k_walk_list(const unsigned* __restrict__ bits, int head, int* hdr, int* list) {
    __shared__ int part[LIST_THREADS];
    const int tid = threadIdx.x;
    list_count(tid, bits, head, hdr, part);
    __syncthreads();
    list_scan(tid, part, hdr);
    __syncthreads();
    list_write(tid, bits, head, hdr, part, list);
}

template <int G>
__global__ void __launch_bounds__(GATHER_THREADS)
k_walk_gather(gsp::ExportIn in, gsp::ExportOut out, const int* __restrict__ list, const int* __restrict__ cr, int total) {
    walk_slots<G>(threadIdx.x, blockDim.x, blockIdx.x, gridDim.x, in, out, list, cr, total);
}

__global__ void __launch_bounds__(TRUNK_THREADS)
k_fork_trunks(const int* __restrict__ sp, const int* __restrict__ cr, const int* __restrict__ ht, int n, long long N, int* children, int* roots,
              int* trunk) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < N; e += (long long)gridDim.x * blockDim.x)
        fork_event(e, sp, cr, ht, n, N, children, roots, trunk);
}
#endif

}  // namespace wlk
