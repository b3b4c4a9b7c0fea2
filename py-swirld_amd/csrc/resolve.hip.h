// Payload ingest by event id (sw_set_event_ids, sw_lookup_event_ids, sw_ingest_payload[_device]): the id index of the
// context, and the stage that turns a sync payload — events addressed by id, in any order, known events and invalid
// ones included — into the dense, topologically ordered batch that sw_append_events_device takes.
// Path (reference file:line): Node.sync swirld.py:130-136 (drop the known ids, toposort, is_valid_event's parent
// checks swirld.py:104-108 per event, store what is valid).  tests/model_payload.py states the same steps in Python.
//
// Tables: open addressing, linear probing, int32 slots (-1 empty, else the index of an id in the array the table is
// built over), power-of-two capacity, load <= 1/2.  The slot comes from the first 64-bit word of the id; a hit is
// confirmed on all 32 bytes.  Ids are attacker-chosen: every probe loop ends after `cap` slots at the latest.  The
// tables only grow: a slot, once taken, keeps holding the SAME id, so equal ids walk the same slots and meet in the
// first slot that holds their id; an atomicMin there leaves the lowest index, whatever the order of arrival.
//
// Nothing here hands data from one workgroup to another inside a launch except through the return values of atomics
// on the slots and plain counters: every array a kernel reads was written by an earlier launch (or is the payload),
// with ONE exception, the wave numbers, which the wave kernel reads and writes — see k_pl_wave.
#pragma once
#ifndef RSV_HOST_EMULATION   // (tests/payload_emul.cpp runs these kernels thread by thread on the host, under sanitizers)
#include <hip/hip_runtime.h>
#endif

namespace rsv {

typedef unsigned long long u64;

// index_out codes (include/swirld_hip.h)
enum : int {
    R_PENDING = -1,    // internal: not decided yet (never returned)
    R_DUP = -2,
    R_NOT_OK = -3,
    R_CREATOR = -4,
    R_ARITY = -5,
    R_PARENT = -6,
    R_SELF = -7,
    R_OTHER = -8,
};
// parent references: >= 0 a stored event (dense index), -1 none, <= -2 the payload position -2 - ref
__device__ __forceinline__ int ref_of_pos(int p) { return -2 - p; }

struct Id32 { u64 w[4]; };

__device__ __forceinline__ Id32 load_id(const unsigned char* ids, long long i) {   // (8-byte aligned: checked by the host)
    const u64* p = (const u64*)(ids + i * 32);
    Id32 r;
    r.w[0] = p[0]; r.w[1] = p[1]; r.w[2] = p[2]; r.w[3] = p[3];
    return r;
}
__device__ __forceinline__ bool same_id(const Id32& a, const Id32& b) {
    return ((a.w[0] ^ b.w[0]) | (a.w[1] ^ b.w[1]) | (a.w[2] ^ b.w[2]) | (a.w[3] ^ b.w[3])) == 0ull;
}
__device__ __forceinline__ unsigned slot_of(u64 w0, int log2cap) {
    return (unsigned)((w0 * 0x9E3779B97F4A7C15ull) >> (64 - log2cap));   // (log2cap >= 1)
}

// Insert the ids [first, first + K) of `ids` (the table's own array) under their indices.  An id that is already in the
// table — from before, or twice in this launch — leaves the LOWEST index in the slot and raises *dup.
__global__ void k_tab_insert(int* slots, int log2cap, const unsigned char* __restrict__ ids, int first, int K, int* dup) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    const int e = first + i;
    const Id32 me = load_id(ids, e);
    const unsigned mask = (1u << log2cap) - 1u;
    unsigned pos = slot_of(me.w[0], log2cap);
    for (unsigned trip = 0; trip <= mask; ++trip, pos = (pos + 1) & mask) {
        int s = slots[pos];
        if (s == -1) {
            s = atomicCAS(&slots[pos], -1, e);
            if (s == -1) return;
        }
        // (s may have been replaced by a lower index of the same id meanwhile: any occupant the slot ever had has this id)
        if (same_id(load_id(ids, s), me)) {
            atomicMin(&slots[pos], e);
            if (dup) *dup = 1;
            return;
        }
    }
    if (dup) *dup = 2;   // table full: cannot happen at load <= 1/2 (the host reads it as an internal error)
}

__device__ __forceinline__ int tab_find(const int* __restrict__ slots, int log2cap, const unsigned char* __restrict__ ids, const Id32& key) {
    const unsigned mask = (1u << log2cap) - 1u;
    unsigned pos = slot_of(key.w[0], log2cap);
    for (unsigned trip = 0; trip <= mask; ++trip, pos = (pos + 1) & mask) {
        const int s = slots[pos];
        if (s == -1) return -1;
        if (same_id(load_id(ids, s), key)) return s;
    }
    return -1;
}

// out[i] = index of keys[i] in the table over `ids`, or -1 (log2cap 0: no table yet)
__global__ void k_tab_lookup(const int* __restrict__ slots, int log2cap, const unsigned char* __restrict__ ids,
                             const unsigned char* __restrict__ keys, int K, int* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    out[i] = log2cap ? tab_find(slots, log2cap, ids, load_id(keys, i)) : -1;
}

// Local checks and parent resolution, one thread per payload event (after the payload-local table has been built:
// its slots hold the LOWEST position of every id).  out[i] = the stored index of a known id, a reject code, or
// R_PENDING with the event appended to the candidate list; pr[2i], pr[2i + 1] = parent references.
__global__ void k_pl_local(const int* __restrict__ cslots, int clog, const unsigned char* __restrict__ cids,
                           const int* __restrict__ lslots, int llog, const unsigned char* __restrict__ id, const unsigned char* __restrict__ spid,
                           const unsigned char* __restrict__ opid, const unsigned char* __restrict__ arity, const int* __restrict__ creator,
                           const unsigned char* __restrict__ ok, int K, int n, int* __restrict__ out, int* __restrict__ wave, int* __restrict__ pr,
                           int* __restrict__ list, int* count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    const Id32 me = load_id(id, i);
    wave[i] = -1;
    pr[2 * i] = pr[2 * i + 1] = -1;
    const int known = clog ? tab_find(cslots, clog, cids, me) : -1;
    int res = R_PENDING;
    const int ar = arity[i];
    if (known >= 0) res = known;
    else if (tab_find(lslots, llog, id, me) != i) res = R_DUP;
    else if (ok && !ok[i]) res = R_NOT_OK;
    else if (creator[i] < 0 || creator[i] >= n) res = R_CREATOR;
    else if (ar != 0 && ar != 2) res = R_ARITY;
    else if (ar == 2) {
        const unsigned char* pid[2] = {spid, opid};
        for (int q = 0; q < 2; ++q) {
            const Id32 p = load_id(pid[q], i);
            int r = clog ? tab_find(cslots, clog, cids, p) : -1;
            if (r < 0) {
                const int pos = tab_find(lslots, llog, id, p);
                r = pos >= 0 ? ref_of_pos(pos) : -1;
            }
            pr[2 * i + q] = r;
            if (r == -1) res = R_PARENT;
        }
    }
    out[i] = res;
    if (res == R_PENDING) list[atomicAdd(count, 1)] = i;
}

// One acceptance wave over the still-pending events lin[0 .. *nin).  An event is READY in wave w when each parent is
// stored or was accepted in a wave < w.  A ready event passes the creator checks and is accepted (wave[i] = w), or is
// rejected for good; one that is not ready goes to lout.  wave[] is read and written in the same launch: a reader
// takes any value that is not in [0, w) for "not accepted yet" — whether it sees -1 or the w another thread has just
// stored makes no difference, and values < w are from earlier launches.  Nothing waits for anything: an event whose
// parent never gets accepted (rejected, absent, a cycle) stays pending until the host stops launching.
__global__ void k_pl_wave(int w, const int* __restrict__ lin, const int* nin, int* __restrict__ lout, int* nout, int* nacc,
                          const int* __restrict__ pr, const int* __restrict__ creator, const int* __restrict__ stored_cr,
                          int* wave, int* __restrict__ out) {
    const int cnt = *nin;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < cnt; j += gridDim.x * blockDim.x) {
        const int i = lin[j];
        const int rs = pr[2 * i], ro = pr[2 * i + 1];
        bool ready = true;
        int cs = -1, co = -1;
        if (rs != -1) {   // (two parents: the local checks left either none or both)
            if (rs >= 0) cs = stored_cr[rs];
            else { const int p = -2 - rs; const int pw = __hip_atomic_load(&wave[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); ready = pw >= 0 && pw < w; cs = creator[p]; }
            if (ro >= 0) co = stored_cr[ro];
            else { const int p = -2 - ro; const int pw = __hip_atomic_load(&wave[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); ready = ready && pw >= 0 && pw < w; co = creator[p]; }
        }
        if (!ready) { lout[atomicAdd(nout, 1)] = i; continue; }
        const int m = creator[i];
        if (rs != -1 && cs != m) out[i] = R_SELF;
        else if (rs != -1 && co == m) out[i] = R_OTHER;
        else {
            __hip_atomic_store(&wave[i], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicAdd(nacc, 1);
        }
    }
}

// Sort keys of one LSD pass (10 bits of the wave number) for the stable-rank kernels of ingest.hip.h: pass 0 runs over
// the payload positions themselves (ord == nullptr; an event that was not accepted gets key -1 and takes no part),
// later passes over the order the pass before left.
__global__ void k_pl_keys(const int* __restrict__ wave, const int* __restrict__ ord, int cnt, int shift, int* __restrict__ key) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt) return;
    const int wv = wave[ord ? ord[j] : j];
    key[j] = wv < 0 ? -1 : (wv >> shift) & 1023;
}

// Exclusive scan of the 1024 key totals (one workgroup of 1024 threads).
#ifndef RSV_HOST_EMULATION   // (barriers: not for a thread-by-thread run)
__global__ __launch_bounds__(1024) void k_pl_bases(const int* __restrict__ total, int* __restrict__ base) {
    __shared__ int s[1024];
    const int t = threadIdx.x;
    s[t] = total[t];
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    base[t] = s[t] - total[t];
}
#endif

// Scatter of one LSD pass: the item at j goes to base[key] + (its stable rank among the items of its key).
__global__ void k_pl_scatter(const int* __restrict__ key, const int* __restrict__ seq, const int* __restrict__ base, const int* __restrict__ ord,
                             int cnt, int* __restrict__ ord_out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt) return;
    const int k = key[j];
    if (k < 0) return;
    ord_out[base[k] + seq[j]] = ord ? ord[j] : j;
}

// rank_of[payload position] = rank in the dense order, and the answer of the accepted events
__global__ void k_pl_ranks(const int* __restrict__ ord, int A, int N0, int* __restrict__ rank_of, int* __restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A) return;
    const int i = ord[r];
    rank_of[i] = r;
    out[i] = N0 + r;
}

// Whoever is still pending when the waves have ended never had its parents: R_PARENT.
__global__ void k_pl_leftover(const int* __restrict__ wave, int K, int* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    if (out[i] == R_PENDING && wave[i] < 0) out[i] = R_PARENT;
}

// The accepted events in dense order, parents as dense indices, ids behind the ids of the stored events.
__global__ void k_pl_gather(const int* __restrict__ ord, int A, int N0, const int* __restrict__ rank_of, const int* __restrict__ pr,
                            const int* __restrict__ creator, const unsigned char* __restrict__ id, const double* __restrict__ t,
                            int* __restrict__ g_cr, int* __restrict__ g_sp, int* __restrict__ g_op, double* __restrict__ g_t, unsigned char* __restrict__ g_id) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A) return;
    const int i = ord[r];
    const int rs = pr[2 * i], ro = pr[2 * i + 1];
    g_cr[r] = creator[i];
    g_sp[r] = rs == -1 ? -1 : rs >= 0 ? rs : N0 + rank_of[-2 - rs];
    g_op[r] = ro == -1 ? -1 : ro >= 0 ? ro : N0 + rank_of[-2 - ro];
    if (t) g_t[r] = t[i];
    const Id32 me = load_id(id, i);
    u64* d = (u64*)(g_id + (long long)r * 32);
    d[0] = me.w[0]; d[1] = me.w[1]; d[2] = me.w[2]; d[3] = me.w[3];
}

// Signatures: 64 bytes per event, 16 lanes x 4 bytes each (the payload's array has no alignment beyond its type's).
__global__ void k_pl_gather_sig(const int* __restrict__ ord, int A, const unsigned char* __restrict__ sig, unsigned char* __restrict__ g_sig) {
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long r = x >> 4;
    if (r >= A) return;
    const int part = (int)(x & 15) * 4;
    const unsigned char* s = sig + (long long)ord[r] * 64 + part;
    unsigned char* d = g_sig + r * 64 + part;
    d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3];
}

}  // namespace rsv
