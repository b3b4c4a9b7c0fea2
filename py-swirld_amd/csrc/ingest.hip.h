// Device-side ingest (sw_append_events_device): validation, chain positions, per-member tables and heights
// of a bulk, fork-free batch whose parent arrays already lie in the uncommitted tail of d_cr / d_sp / d_op.
// Path (reference file:line): Node.is_valid_event swirld.py:104-108 (structural half), Node.add_event
// swirld.py:114-120 (height).  tests/model_ingest.py states the same steps in numpy, tile by tile.
//
// One verdict word per batch, settled by atomicMin: (event index << 8) | code.  The lowest offending event
// wins, and an event fails at most one check per kernel, in the order of the codes.
#pragma once
#include <hip/hip_runtime.h>

namespace ing {

constexpr int TILE = 4096;        // events per workgroup of the histogram / rank kernels (4 waves x 1024)
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int SUB = TILE / WAVES; // consecutive events ranked by one wave
constexpr int HT_TILE = 1024;     // events per fixed point of the heights kernel (one per thread)
constexpr int MAX_KEYS = 1024;    // npad never exceeds this

enum : int {
    V_CREATOR = 1,   // creator out of range
    V_ARITY = 2,     // one parent only
    V_ORDER = 3,     // a parent index not earlier than the event
    V_SELF = 4,      // self-parent by another member
    V_OTHER = 5,     // other-parent by the same member
    V_FORK = 6,      // self-parent is not the creator's latest event / a second root (not a defect: the host path decides)
};
constexpr unsigned long long V_NONE = ~0ull;

__device__ __forceinline__ void verdict(unsigned long long* v, int e, int code) {
    atomicMin(v, ((unsigned long long)(unsigned)e << 8) | (unsigned)code);
}

// 1. Local checks, one thread per event.  An event that fails gets creator -1 in the (uncommitted) tail and
// takes part in nothing that follows: no later kernel reads through one of its indices.
__global__ void k_ingest_local(int* cr, const int* __restrict__ sp, const int* __restrict__ op, int first, int K, int n,
                               unsigned long long* v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    const int e = first + i;
    const int m = cr[e], s = sp[e], o = op[e];
    int code = 0;
    if (m < 0 || m >= n) code = V_CREATOR;
    else if ((s < 0) != (o < 0)) code = V_ARITY;
    else if (s >= e || o >= e) code = V_ORDER;
    if (code) {
        cr[e] = -1;
        verdict(v, e, code);
    }
}

// 2a. Per-tile histogram of the creators, and the last / first event of every member (tab: [nev | head | first],
// npad ints each; `first` holds INT_MAX for a member without events).
__global__ __launch_bounds__(THREADS) void k_ingest_hist(const int* __restrict__ cr, int first, int K, int npad, int* __restrict__ hist,
                                                         int* tab) {
    __shared__ int cnt[MAX_KEYS], last[MAX_KEYS], frst[MAX_KEYS];
    for (int k = threadIdx.x; k < npad; k += THREADS) { cnt[k] = 0; last[k] = -1; frst[k] = 0x7fffffff; }
    __syncthreads();
    const int t0 = blockIdx.x * TILE;
    for (int j = threadIdx.x; j < TILE; j += THREADS) {
        const int i = t0 + j;
        if (i >= K) break;
        const int m = cr[first + i];
        if (m < 0) continue;
        atomicAdd(&cnt[m], 1);
        atomicMax(&last[m], first + i);
        atomicMin(&frst[m], first + i);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < npad; k += THREADS) {
        hist[(size_t)blockIdx.x * npad + k] = cnt[k];
        if (cnt[k]) {
            atomicMax(&tab[npad + k], last[k]);
            atomicMin(&tab[2 * npad + k], frst[k]);
        }
    }
}

// 2b. Exclusive scan over the tiles, one thread per member, starting at the member's event count so far:
// hist[tile][m] becomes the chain position of the member's first event of that tile, tab[m] its new count.
__global__ void k_ingest_scan(int* hist, int tiles, int npad, int* tab) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= npad) return;
    int run = tab[m];
    for (int t = 0; t < tiles; ++t) {
        const int c = hist[(size_t)t * npad + m];
        hist[(size_t)t * npad + m] = run;
        run += c;
    }
    tab[m] = run;
}

// Lanes of the wave that hold the same key (all of them valid), by ballots over the key's bits.
__device__ __forceinline__ unsigned long long wave_peers(int key, bool valid, int nbits) {
    unsigned long long peers = __ballot(valid);
    for (int b = 0; b < nbits; ++b) {
        const unsigned long long bal = __ballot(valid && ((key >> b) & 1));
        peers &= ((key >> b) & 1) ? bal : ~bal;
    }
    return peers;
}

// 2c. Chain positions: seq[e] = (position of the member's first event of the tile) + (earlier events of the tile by
// the same member).  Each wave owns SUB consecutive events: it counts them per member, the counts of the waves in
// front of it give its base, and it walks its events 64 at a time with a running count per member.
__global__ __launch_bounds__(THREADS) void k_ingest_rank(const int* __restrict__ cr, int first, int K, int npad, int nbits,
                                                         const int* __restrict__ hist, int* __restrict__ seq) {
    __shared__ int wcnt[WAVES][MAX_KEYS];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = threadIdx.x; k < WAVES * npad; k += THREADS) wcnt[k / npad][k % npad] = 0;
    __syncthreads();
    const int w0 = blockIdx.x * TILE + w * SUB;
    for (int j = lane; j < SUB; j += 64) {
        const int i = w0 + j;
        if (i >= K) break;
        const int m = cr[first + i];
        if (m >= 0) atomicAdd(&wcnt[w][m], 1);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < npad; k += THREADS) {
        int run = hist[(size_t)blockIdx.x * npad + k];
        for (int q = 0; q < WAVES; ++q) {
            const int c = wcnt[q][k];
            wcnt[q][k] = run;
            run += c;
        }
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int j = 0; j < SUB; j += 64) {   // (the same trips in every lane: the ballots see the whole wave)
        const int i = w0 + j + lane;
        const int m = i < K ? cr[first + i] : -1;
        const bool valid = m >= 0;
        const unsigned long long peers = wave_peers(m, valid, nbits);
        if (valid) {
            seq[first + i] = wcnt[w][m] + __popcll(peers & below);
            // ASSUMES wave lockstep: every lane of the group has read wcnt[w][m] (the line above) before the group's highest
            // lane adds to it — the DS operations of one wave execute in order and the ballots above are convergent; a
            // register copy fenced by wave barriers would say so to the compiler (not done here: no GPU run behind it yet)
            if ((peers >> lane) == 1ull) wcnt[w][m] += __popcll(peers);   // (the highest lane of the group; after the reads above)
        } else if (i < K) {
            seq[first + i] = -1;
        }
    }
}

// 3. Link checks, one thread per event that passed step 1 (all its indices are earlier events).
__global__ void k_ingest_links(const int* __restrict__ cr, const int* __restrict__ sp, const int* __restrict__ op,
                               const int* __restrict__ seq, int first, int K, unsigned long long* v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    const int e = first + i;
    const int m = cr[e];
    if (m < 0) return;
    const int s = sp[e], o = op[e];
    int code = 0;
    if (s < 0) {
        if (seq[e] != 0) code = V_FORK;   // a second root
    } else if (cr[s] != m) code = V_SELF;
    else if (cr[o] == m) code = V_OTHER;
    else if (seq[s] + 1 != seq[e]) code = V_FORK;   // (stable rank: exactly "s is the creator's previous event")
    if (code) verdict(v, e, code);
}

// 5. Heights (swirld.py:117-120): ht[e] = 0 for a root, else 1 + max(ht[sp], ht[op]).  ONE workgroup streams the batch
// in index order, HT_TILE events at a time: parents in front of the tile are gathered from ht (older events, or earlier
// tiles of this launch), parents inside the tile are resolved by a fixed point in LDS — a tile of a valid batch needs at
// most as many trips as it has events; a tile that needs more ends the kernel with stat[0] = 1 instead of spinning.
// stat: [0] error, [1] largest height, then [min, max] per 4096-event block from block `blk0` on (new events only).
__device__ __forceinline__ int wave_min(int v) {
    for (int d = 32; d; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
    for (int d = 32; d; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

__global__ __launch_bounds__(HT_TILE) void k_ingest_heights(const int* __restrict__ sp, const int* __restrict__ op, int* ht, int first,
                                                            int K, int blk0, int* stat) {
    __shared__ int h[HT_TILE];
    __shared__ int bmin[2], bmax[2];
    __shared__ int tops;
    const int tid = threadIdx.x;
    int top = -1;
    // parents of the tile are loaded one tile ahead (they do not depend on the heights)
    // (lanes beyond the end of the batch keep the indices of the tile before: every use is guarded by `in`.  The sums
    // t0 + HT_TILE + tid stay inside int for batches that end 2048 events below 2^31; sw_append_events_device's limit
    // of 0x7ffffff0 events does not quite guarantee that)
    int ns = -1, no = -1;
    if (tid < K) { ns = sp[first + tid]; no = op[first + tid]; }
    for (int t0 = 0; t0 < K; t0 += HT_TILE) {
        const int tile_first = first + t0;
        const int e = tile_first + tid;
        const bool in = t0 + tid < K;
        const int s = ns, o = no;
        int hv = 0, a = 0, b = 0;
        if (tid < 2) { bmin[tid] = 0x7fffffff; bmax[tid] = -1; }
        if (in && s >= 0) {
            a = s < tile_first ? ht[s] : -1;
            b = o < tile_first ? ht[o] : -1;
            hv = (a >= 0 && b >= 0) ? 1 + max(a, b) : -1;
        }
        if (t0 + HT_TILE + tid < K) { ns = sp[e + HT_TILE]; no = op[e + HT_TILE]; }
        h[tid] = hv;
        int trips = 0;
        while (__syncthreads_count(hv < 0)) {
            if (++trips > HT_TILE) {   // (uniform: every thread counts the same trips)
                if (tid == 0) stat[0] = 1;
                return;
            }
            if (hv < 0) {
                if (a < 0) a = h[s - tile_first];
                if (b < 0) b = h[o - tile_first];
            }
            __syncthreads();   // every read of this trip before its writes
            if (hv < 0 && a >= 0 && b >= 0) { hv = 1 + max(a, b); h[tid] = hv; }
        }
        if (in) ht[e] = hv;
        // height span of the (at most two) 4096-event blocks the tile touches: per wave, then one LDS atomic per wave
        const int q = in ? (e >> 12) - (tile_first >> 12) : -1;
        const int lo0 = wave_min(q == 0 ? hv : 0x7fffffff), hi0 = wave_max(q == 0 ? hv : -1);
        const int lo1 = wave_min(q == 1 ? hv : 0x7fffffff), hi1 = wave_max(q == 1 ? hv : -1);
        if ((tid & 63) == 0) {
            if (hi0 >= 0) { atomicMin(&bmin[0], lo0); atomicMax(&bmax[0], hi0); }
            if (hi1 >= 0) { atomicMin(&bmin[1], lo1); atomicMax(&bmax[1], hi1); }
        }
        top = max(top, max(hi0, hi1));
        __syncthreads();   // heights of this tile visible to the gathers of the next one; the spans complete
        if (tid < 2 && bmax[tid] >= 0) {
            const int blk = (tile_first >> 12) + tid - blk0;
            stat[2 + 2 * blk] = min(stat[2 + 2 * blk], bmin[tid]);
            stat[3 + 2 * blk] = max(stat[3 + 2 * blk], bmax[tid]);
        }
    }
    if (tid == 0) tops = -1;
    __syncthreads();
    if ((tid & 63) == 0) atomicMax(&tops, top);
    __syncthreads();
    if (tid == 0) stat[1] = tops;
}

}  // namespace ing
