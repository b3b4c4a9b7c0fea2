// Answering a sync on the device (sw_export_payload[_device], sw_sync_pull): the events sw_sync_diff names, written as the
// arrays sw_ingest_payload_device takes — id, parents' ids, arity, creator, timestamp, signature per event.
// Path (reference file:line): Node.ask_sync swirld.py:148-161 (the height-pruned walk is k_sync_diff of kernels.hip.h,
// called as it is; what the reference then pickles per event, swirld.py:76-95, is gathered here).  tests/model_gossip.py
// states the ranges, the slot order and the slot contents in numpy.
//
// Two kernels behind k_sync_diff:
//   k_export_offsets   one workgroup: exclusive scan of the (at most 1024) range lengths -> off[0 .. n], the total, and
//                      per member base[m] = chain_start[m] + pos_first[m] - off[m], so that slot s of member m is the event
//                      chain_ev[base[m] + s].
//   k_export_gather    over the output slots, member-major: G lanes of a wave share one slot.  The slot's 13 PIECES — ten
//                      16-byte pieces (id 2, self-parent id 2, other-parent id 2, signature 4) and three scalar pieces
//                      (arity + creator, timestamp, dense index) — are dealt to the G lanes, piece q to lane q mod G; every
//                      lane turns its piece into ONE source and ONE destination address and all lanes issue the same 16-byte
//                      load and store, so the stores of one instruction to one array cover consecutive events (64 / G of
//                      them) as consecutive memory.  The member of a slot comes from a bounded binary search over the
//                      offsets, which every workgroup holds in LDS.
// Every index a kernel follows comes from the context's own tables (can_see row, chain pool, parent arrays); the asker's
// heights are compared in k_sync_diff and nowhere used as an index.  No kernel waits for another workgroup.
//
// Each kernel body is a sequence of per-thread phases (plain functions of the thread index, LDS passed as a pointer) with a
// barrier between them: tests/gossip_emul.cpp runs the same phases thread by thread on the host, under sanitizers.
#pragma once
#ifndef GSP_HOST_EMULATION
#include <hip/hip_runtime.h>
#endif

namespace gsp {

constexpr int MAX_MEMBERS = 1024;
constexpr int SCAN_THREADS = 64;                          // k_export_offsets: one wave ...
constexpr int SCAN_PER = MAX_MEMBERS / SCAN_THREADS;      // ... 16 consecutive members per lane
constexpr int PIECES = 13;
constexpr int GATHER_THREADS = 256;

struct alignas(16) V16 { unsigned x, y, z, w; };

struct ExportIn {    // the exporting context's tables
    const int* off;            // [n + 1] exclusive prefix sums of the range lengths
    const int* base;           // [n]
    const int* chain_ev;
    const int* sp;
    const int* op;
    const unsigned char* id;   // 32 B per event
    const unsigned char* sig;  // 64 B per event
    const unsigned long long* t;   // (timestamps move as 64-bit words: bit-exact whatever the value)
};
struct ExportOut {   // sig, t, event may be null
    unsigned char* id;
    unsigned char* sp_id;
    unsigned char* op_id;
    unsigned char* arity;
    int* creator;
    unsigned long long* t;
    unsigned char* sig;
    int* event;
};

// ---- k_export_offsets, phase by phase (part: SCAN_THREADS ints of LDS)
__device__ __forceinline__ void offsets_sum(int l, const int* pos_first, const int* pos_end, int n, int* part) {
    int sum = 0;
    for (int j = 0; j < SCAN_PER; ++j) {
        const int m = l * SCAN_PER + j;
        if (m < n) sum += pos_end[m] - pos_first[m];
    }
    part[l] = sum;
}
__device__ __forceinline__ void offsets_scan(int l, int n, int* part, int* off, long long* total) {
    if (l != 0) return;
    int run = 0;
    for (int k = 0; k < SCAN_THREADS; ++k) { const int v = part[k]; part[k] = run; run += v; }
    off[n] = run;
    *total = run;
}
__device__ __forceinline__ void offsets_write(int l, const int* pos_first, const int* pos_end, const int* chain_start, int n,
                                              const int* part, int* off, int* base) {
    int run = part[l];
    for (int j = 0; j < SCAN_PER; ++j) {
        const int m = l * SCAN_PER + j;
        if (m >= n) return;
        off[m] = run;
        base[m] = chain_start[m] + pos_first[m] - run;
        run += pos_end[m] - pos_first[m];
    }
}

// ---- k_export_gather, phase by phase (s_off: n + 1 ints of LDS, s_base: n)
__device__ __forceinline__ void gather_stage(int tid, int threads, const ExportIn& in, int n, int* s_off, int* s_base) {
    for (int m = tid; m <= n; m += threads) s_off[m] = in.off[m];
    for (int m = tid; m < n; m += threads) s_base[m] = in.base[m];
}

// the member whose range holds slot s (0 <= s < off[n]): the largest m in [0, n) with off[m] <= s.  At most 10 halvings.
__device__ __forceinline__ int member_of_slot(const int* s_off, int n, int s) {
    int lo = 0, hi = n - 1;
    for (int it = 0; it < 11 && lo < hi; ++it) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_off[mid] <= s) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void export_piece(const ExportIn& in, const ExportOut& out, int q, int s, int m, int e) {
    const size_t S = (size_t)s;
    if (q < 10) {
        const unsigned char* src;
        unsigned char* dst;
        bool zero = false;
        if (q < 2) {
            src = in.id + (size_t)e * 32 + q * 16;
            dst = out.id + S * 32 + q * 16;
        } else if (q < 6) {
            const int p = q < 4 ? in.sp[e] : in.op[e];   // (-1 for a root: 32 zero bytes)
            const int h = q & 1;
            zero = p < 0;
            src = in.id + (size_t)(zero ? 0 : p) * 32 + h * 16;
            dst = (q < 4 ? out.sp_id : out.op_id) + S * 32 + h * 16;
        } else {
            if (!out.sig) return;
            src = in.sig + (size_t)e * 64 + (q - 6) * 16;
            dst = out.sig + S * 64 + (q - 6) * 16;
        }
        V16 v = {0u, 0u, 0u, 0u};
        if (!zero) v = *(const V16*)src;
        *(V16*)dst = v;
    } else if (q == 10) {
        out.arity[S] = in.sp[e] < 0 ? 0 : 2;
        out.creator[S] = m;
    } else if (q == 11) {
        if (out.t) out.t[S] = in.t[e];
    } else {
        if (out.event) out.event[S] = e;
    }
}

template <int G>
__device__ __forceinline__ void gather_slots(int tid, int threads, unsigned block, unsigned blocks, const ExportIn& in, const ExportOut& out,
                                             int n, int total, const int* s_off, const int* s_base) {
    const int per = threads / G;   // slots of one workgroup per trip
    const int lane = tid % G;
    for (long long s0 = (long long)block * per; s0 < total; s0 += (long long)blocks * per) {
        const long long sl = s0 + tid / G;
        if (sl >= total) continue;
        const int s = (int)sl;
        const int m = member_of_slot(s_off, n, s);
        const int e = in.chain_ev[s_base[m] + s];
        for (int q = lane; q < PIECES; q += G) export_piece(in, out, q, s, m, e);
    }
}

#ifndef GSP_HOST_EMULATION
__global__ void __launch_bounds__(SCAN_THREADS)
k_export_offsets(const int* __restrict__ pos_first, const int* __restrict__ pos_end, const int* __restrict__ chain_start, int n,
                 int* off, int* base, long long* total) {
    __shared__ int part[SCAN_THREADS];
    const int l = threadIdx.x;
    offsets_sum(l, pos_first, pos_end, n, part);
    __syncthreads();
    offsets_scan(l, n, part, off, total);
    __syncthreads();
    offsets_write(l, pos_first, pos_end, chain_start, n, part, off, base);
}

template <int G>
__global__ void __launch_bounds__(GATHER_THREADS)
k_export_gather(ExportIn in, ExportOut out, int n, int total) {
    extern __shared__ int s_tab[];   // (2 n + 1) ints from the launch: one block for every instantiation, sized by the member count
    int* s_off = s_tab;
    int* s_base = s_tab + n + 1;
    gather_stage(threadIdx.x, blockDim.x, in, n, s_off, s_base);
    __syncthreads();
    gather_slots<G>(threadIdx.x, blockDim.x, blockIdx.x, gridDim.x, in, out, n, total, s_off, s_base);
}
#endif

}  // namespace gsp
