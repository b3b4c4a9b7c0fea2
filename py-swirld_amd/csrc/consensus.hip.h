// What find_order decides per event, kept on the device and given out (sw_get_round_received, sw_get_consensus_time,
// sw_export_ordered[_device]): the round that received the event and its consensus timestamp.
// Path (reference file:line): Node.find_order swirld.py:283-309.  There `r` (:283, the round whose famous witnesses all see
// the event) and `ts[x]` (:305, the median of the times at which those witnesses' creators first saw it) are locals that
// only steer the sort of :306 and are dropped; here every find_order call leaves them in two per-event tables, and the
// order it produced in a device copy of `transactions`.  tests/model_consensus.py states both values in numpy.
//
// Three kernels, all behind the call that ordered the events (order.hip.h is not touched: what it leaves in device memory —
// acc_ev, acc_ri, ts per slot of the round-major list, the sorted order — is read here):
//   k_consensus_record   one thread per slot a of the call's round-major list: rr[acc_ev[a]] = rounds[acc_ri[a]],
//                        cts[acc_ev[a]] = ts[a].  Every event is in at most one slot, so no two threads write one entry.
//   k_consensus_events   one thread per event of [first, first + K): its two values, or -1 / a quiet NaN when it is not
//                        ordered.  Ordered events are a prefix of every member's chain (order.hip.h head comment), so the
//                        test is seq[e] < ordpos[cr[e]] and the tables are never read for an event nobody recorded.
//   k_ordered_gather     over positions [first, first + K) of the order: G lanes of a wave share one position.  The
//                        position's 6 PIECES — the id as two 16-byte pieces, and four scalars (dense index, creator, round
//                        received, consensus time) — are dealt to the G lanes, piece q to lane q mod G, as k_export_gather
//                        deals its 13: the id moves as one 16-byte load and one 16-byte store per lane, and the stores of
//                        one instruction to one array cover consecutive positions (64 / G of them) as consecutive memory.
//                        Every output array is optional.
// Timestamps move as 64-bit words: bit-exact whatever the value.  Every index a kernel follows comes from the context's own
// tables.  Plain vector loads and stores; no kernel waits for another workgroup.
//
// Each kernel body is a per-thread function of the thread index: tests/consensus_emul.cpp runs the same functions thread by
// thread on the host, under sanitizers.
#pragma once
#ifndef CNS_HOST_EMULATION
#include <hip/hip_runtime.h>
#endif

namespace cns {

constexpr int THREADS = 256;
constexpr int PIECES = 6;
// Lanes per position of k_ordered_gather.  ASSUMED from the structure, not measured: 6 pieces over 4 lanes are at most two
// dependent gathers per lane behind the shared tx[p] load, no lane idles on a full request, and one store instruction covers
// 16 consecutive positions (256 B of ids, 64 B of a scalar array).  8 lanes would leave two of them without a piece.
constexpr int GATHER_LANES = 4;
constexpr unsigned long long QNAN_BITS = 0x7ff8000000000000ull;   // "not ordered yet" of a consensus time

struct alignas(16) V16 { unsigned x, y, z, w; };

struct OrderedIn {     // the context's tables
    const int* tx;                  // the order: dense event index per position
    const unsigned char* id;        // 32 B per event (read only when out.id is wanted)
    const int* cr;
    const int* rr;                  // per event, valid for ordered events
    const unsigned long long* cts;  // per event, valid for ordered events
};
struct OrderedOut {    // each may be null: not wanted
    int* event;
    unsigned char* id;
    int* creator;
    int* rr;
    unsigned long long* t;
};

// ---- k_consensus_record: slot a of the call's round-major list
__device__ __forceinline__ void record_slot(long long a, const int* acc_ev, const int* acc_ri, const int* rounds,
                                            const unsigned long long* ts, int* rr, unsigned long long* cts) {
    const int e = acc_ev[a];
    rr[e] = rounds[acc_ri[a]];
    cts[e] = ts[a];
}

// ---- k_consensus_events: event first + i -> out[i]
__device__ __forceinline__ void events_one(long long i, long long first, const int* seq, const int* cr, const int* ordpos, const int* rr,
                                           const unsigned long long* cts, int* out_rr, unsigned long long* out_cts) {
    const long long e = first + i;
    const bool ordered = seq[e] < ordpos[cr[e]];
    if (out_rr) out_rr[i] = ordered ? rr[e] : -1;
    if (out_cts) out_cts[i] = ordered ? cts[e] : QNAN_BITS;
}

// ---- k_ordered_gather: piece q of output slot s, which holds event ev
__device__ __forceinline__ void ordered_piece(const OrderedIn& in, const OrderedOut& out, int q, long long s, int ev) {
    const size_t S = (size_t)s;
    if (q < 2) {
        if (!out.id) return;
        *(V16*)(out.id + S * 32 + q * 16) = *(const V16*)(in.id + (size_t)ev * 32 + q * 16);
    } else if (q == 2) {
        if (out.event) out.event[S] = ev;
    } else if (q == 3) {
        if (out.creator) out.creator[S] = in.cr[ev];
    } else if (q == 4) {
        if (out.rr) out.rr[S] = in.rr[ev];
    } else {
        if (out.t) out.t[S] = in.cts[ev];
    }
}

template <int G>
__device__ __forceinline__ void gather_positions(int tid, int threads, unsigned block, unsigned blocks, const OrderedIn& in, const OrderedOut& out,
                                                 long long first, long long K) {
    const int per = threads / G;   // positions of one workgroup per trip
    const int lane = tid % G;
    for (long long s0 = (long long)block * per; s0 < K; s0 += (long long)blocks * per) {
        const long long s = s0 + tid / G;
        if (s >= K) continue;
        const int ev = in.tx[first + s];
        for (int q = lane; q < PIECES; q += G) ordered_piece(in, out, q, s, ev);
    }
}

#ifndef CNS_HOST_EMULATION
__global__ void __launch_bounds__(THREADS)
k_consensus_record(const int* __restrict__ acc_ev, const int* __restrict__ acc_ri, const int* __restrict__ rounds,
                   const unsigned long long* __restrict__ ts, long long n_acc, int* rr, unsigned long long* cts) {
    const long long a = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (a < n_acc) record_slot(a, acc_ev, acc_ri, rounds, ts, rr, cts);
}

__global__ void __launch_bounds__(THREADS)
k_consensus_events(long long first, long long K, const int* __restrict__ seq, const int* __restrict__ cr, const int* __restrict__ ordpos,
                   const int* __restrict__ rr, const unsigned long long* __restrict__ cts, int* out_rr, unsigned long long* out_cts) {
    for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < K; i += (long long)gridDim.x * THREADS)
        events_one(i, first, seq, cr, ordpos, rr, cts, out_rr, out_cts);
}

template <int G>
__global__ void __launch_bounds__(THREADS)
k_ordered_gather(OrderedIn in, OrderedOut out, long long first, long long K) {
    gather_positions<G>(threadIdx.x, blockDim.x, blockIdx.x, gridDim.x, in, out, first, K);
}
#endif

}  // namespace cns
