// The data of events on the device (sw_set_event_data[_device], sw_gather_event_data[_device], sw_ingest_payload_data[_device],
// sw_sync_pull_data): Event.d, the transaction an event carries (swirld.py:30, :82-95), 0 .. MAX_DATA bytes
// or None per event.  A context keeps them in one byte arena with absolute int64 offsets (one entry more than the events
// that have data, contiguous: off[i + 1] - off[i] is the length) and one none flag per event, so that a slice of the store
// is an input of pack.hip.h without a copy.
//
// Every use is one primitive, a RAGGED GATHER: given K source ranges in a chosen order, write their bytes back to back and
// their offsets.
//   set from device   source the caller's buffer, slot k = range k,                     destination the arena's tail
//   ingest append     source the payload's buffer, slot r = the event of dense rank r,   destination the arena's tail
//   gather by index   source the arena, slot k = the stored event d_event[k],            destination the caller's buffer
//
// Kernels, none of which waits for another workgroup:
//   k_data_fold_ok   one thread per payload event: ok_out = ok AND "the data range can be used" (pack's d_encodable rule);
//                    the lengths of the ranges that stay ok are summed (ranges of a peer may overlap: the sum bounds what an
//                    ingest can append, and the host refuses a payload whose sum exceeds its buffer before anything is stored)
//   k_data_slots     one thread per payload event: slot[index_out - first_new] = its position (the lowest, for duplicates)
//   k_data_lengths   one thread per slot: index and range checks, the length (0 for None), the none flag, a bad-slot count
//   (the exclusive int64 scan of the lengths is pack.hip.h's: k_pack_tile_sums, k_pack_scan_sums, k_pack_offsets)
//   k_data_store_off the scanned offsets, plus a base, to where they stay; the none flags beside them
//   k_data_copy      OUTPUT-STATIONARY, as k_pack_write: a lane owns one aligned 16-byte chunk of the DESTINATION BUFFER
//                    and issues ONE 16-byte store.  A workgroup stages the stream offsets under its WRITE_THREADS chunks in
//                    LDS (one search over the global offsets per trip), each lane finds its first segment by a binary
//                    search in that tile.  Two cases only, so that a wave does not diverge over a layout:
//                      common   the whole chunk lies inside one segment.  Source = the arena (256-byte aligned base, 16
//                               bytes of slack behind its end): the one or two aligned 16-byte pieces that cover the 16
//                               source bytes, funnel-shifted into place.  Source = a caller's buffer (no alignment, no
//                               padding): 16 single bytes, as pack reads data.
//                      general  the chunk holds the ends of any number of segments (16 one-byte items, any run of empty
//                               ones): walked run by run, bytes read one by one.
//                    The stream starts at destination byte dst_base, which is arbitrary (the arena's tail), so its FIRST and
//                    LAST chunk may be partial: a partial chunk is written byte by byte, and nothing below dst_base or at or
//                    beyond dst_base + off[K] is ever written.
// Trust: a caller's offsets are checked in k_data_lengths / k_data_fold_ok before any of them is followed; a slot that
// fails has length 0 and is never visited by the copy.  No byte outside [0, src_bytes) of a source is read, except the
// arena's own slack.
//
// Each kernel body is a sequence of per-thread phases (plain functions of the thread index, LDS passed as a pointer) with a
// barrier between them: tests/data_emul.cpp runs the same phases thread by thread on the host, under sanitizers.
#pragma once
#include "pack.hip.h"

namespace dat {

using pck::i64;
using pck::u64;
using pck::V16;

constexpr int MAX_DATA = pck::MAX_DATA;
constexpr int WRITE_THREADS = pck::WRITE_THREADS;
constexpr int SLACK = 16;             // readable bytes behind the end of an arena
constexpr int NO_SLOT = 0x7f7f7f7f;   // k_data_slots' initial value (a byte fill)

struct SegIn {       // the source side of a ragged gather
    const unsigned char* src;
    const i64* src_off;               // null: every slot is None (and nothing is read)
    const unsigned char* src_none;    // may be null
    const int* idx;                   // slot -> source entry; null: slot k = entry k
    i64 n_src;                        // entries of the source (idx is checked against it)
    i64 src_bytes;
    int aligned;                      // the source is an arena: src 16-byte aligned, SLACK readable bytes behind src_bytes
};

// can entry e's range be used?  (the rule of pck::data_len)
__device__ __forceinline__ bool range_ok(const i64* off, i64 e, i64 bytes) {
    const i64 a = off[e], b = off[e + 1];
    return a >= 0 && b >= a && b <= bytes && b - a <= MAX_DATA;
}

// ---- k_data_fold_ok
__device__ __forceinline__ void fold_ok(i64 i, i64 K, const unsigned char* ok, const i64* data_off, i64 data_bytes, unsigned char* ok_out, u64* lane_sum) {
    if (i >= K) return;
    const bool v = (!ok || ok[i]) && (!data_off || range_ok(data_off, i, data_bytes));
    ok_out[i] = v;
    if (v && data_off) *lane_sum += (u64)(data_off[i + 1] - data_off[i]);
}

// ---- k_data_slots: slot[] starts as NO_SLOT everywhere
__device__ __forceinline__ int slot_of(i64 i, i64 K, const int* index_out, int first_new, i64 A) {
    if (i >= K) return -1;
    const i64 r = (i64)index_out[i] - first_new;
    return r >= 0 && r < A ? (int)r : -1;
}

// ---- k_data_lengths: len_off[k] = the length (the scan turns it into the offset), none_out[k], *bad += 1 for a slot whose
// index or range cannot be used
__device__ __forceinline__ void lengths(i64 k, i64 K, const SegIn& in, i64* len_off, unsigned char* none_out, int* lane_bad) {
    if (k >= K) return;
    i64 e = k;
    bool ok = true;
    if (in.idx) { e = in.idx[k]; ok = e >= 0 && e < in.n_src; }
    i64 len = 0;
    bool none = true;
    if (ok && in.src_off) {
        ok = range_ok(in.src_off, e, in.src_bytes);
        none = in.src_none && in.src_none[e];
        if (ok && !none) len = in.src_off[e + 1] - in.src_off[e];
    }
    if (!ok) { len = 0; none = true; *lane_bad += 1; }
    len_off[k] = len;
    none_out[k] = none;
}

// ---- k_data_store_off
__device__ __forceinline__ void store_off(i64 k, i64 K, const i64* off, i64 base, i64* off_out, const unsigned char* none, unsigned char* none_out) {
    if (k > K) return;
    off_out[k] = base + off[k];
    if (k < K && none_out) none_out[k] = none[k];
}

// ---- k_data_copy
struct Tile {        // LDS
    i64 off[WRITE_THREADS];
    i64 e0;          // off[j] = the stream's off[e0 + j], j < cnt
    int cnt;
};

// the first destination chunk (16 bytes of the destination BUFFER) of trip `trip` of workgroup `block`, counted from the
// chunk that holds dst_base
__device__ __forceinline__ i64 first_chunk(unsigned block, unsigned blocks, i64 trip) { return (trip * blocks + block) * WRITE_THREADS; }
// stream position of the first byte of relative chunk q (negative inside the first, partial chunk)
__device__ __forceinline__ i64 chunk_pos(i64 q, i64 dst_base) { return q * 16 - (dst_base & 15); }

__device__ __forceinline__ void copy_stage(int tid, i64 chunk0, i64 K, const i64* off, i64 dst_base, Tile* s) {
    i64 base = chunk_pos(chunk0, dst_base);
    if (base < 0) base = 0;
    if (K <= 0 || base >= off[K]) { if (tid == 0) { s->cnt = 0; s->e0 = 0; } return; }
    const i64 e0 = pck::event_of(off, 0, K - 1, base);   // (uniform over the workgroup)
    const i64 left = K + 1 - e0;
    if (tid < left) s->off[tid] = off[e0 + tid];
    if (tid == 0) { s->e0 = e0; s->cnt = (int)(left < WRITE_THREADS ? left : WRITE_THREADS); }
}

__device__ __forceinline__ i64 off_at(const i64* off, const Tile* s, i64 e) {
    const i64 j = e - s->e0;
    return j >= 0 && j < s->cnt ? s->off[j] : off[e];
}

// where slot e's bytes start in the source
__device__ __forceinline__ const unsigned char* seg_src(const SegIn& in, i64 e) {
    return in.src + in.src_off[in.idx ? in.idx[e] : e];
}

// 16 bytes at p from the aligned 16-byte pieces that cover them (p's buffer is an arena: the second piece may reach into the slack)
__device__ __forceinline__ V16 load16_aligned(const unsigned char* p) {
    const unsigned o = (unsigned)((size_t)p & 15);
    const V16* w = (const V16*)(p - o);
    const V16 a = w[0];
    if (o == 0) return a;
    const V16 b = w[1];
    const unsigned sh = 8 * (o & 7);
    u64 x0 = a.lo, x1 = a.hi, x2 = b.lo, x3 = b.hi;
    if (o >= 8) { x0 = x1; x1 = x2; x2 = x3; }
    if (sh == 0) return V16{x0, x1};
    return V16{x0 >> sh | x1 << (64 - sh), x1 >> sh | x2 << (64 - sh)};
}

__device__ __forceinline__ void put(u64* lo, u64* hi, int at, u64 x, int m) {   // m <= 8 bytes of x to byte `at` of the chunk
    if (m < 8) x &= (1ull << (8 * m)) - 1;
    if (at < 8) { *lo |= x << (8 * at); if (at) *hi |= x >> (64 - 8 * at); }
    else *hi |= x << (8 * (at - 8));
}

__device__ __forceinline__ void copy_chunk(int tid, i64 chunk0, i64 K, const SegIn& in, const i64* off, const Tile* s, unsigned char* dst, i64 dst_base) {
    if (s->cnt == 0) return;
    const i64 total = off[K];
    const i64 q = chunk0 + tid;
    i64 pos = chunk_pos(q, dst_base);              // stream position of the chunk's first byte
    int b0 = 0;                                    // first byte of the chunk that belongs to the stream
    if (pos < 0) { b0 = (int)-pos; pos = 0; }
    if (pos >= total) return;
    const int nbytes = total - pos < 16 - b0 ? (int)(total - pos) : 16 - b0;
    unsigned char* out = dst + dst_base + pos;     // (b0 == 0: 16-byte aligned)
    const int cnt = s->cnt;
    const i64 e0 = s->e0;
    i64 e;
    if (pos >= s->off[cnt - 1] && e0 + cnt - 1 < K) e = pck::event_of(off, e0 + cnt - 1, K - 1, pos);   // beyond the tile (runs of empty slots)
    else e = e0 + pck::event_of(s->off, 0, cnt - 2, pos);
    i64 start = off_at(off, s, e), end = off_at(off, s, e + 1);
    if (nbytes == 16 && end - pos >= 16) {         // common: one segment, one store
        const unsigned char* p = seg_src(in, e) + (pos - start);
        V16 v;
        if (in.aligned) v = load16_aligned(p);
        else { v.lo = pck::bytes8(p, 8); v.hi = pck::bytes8(p + 8, 8); }
        *(V16*)out = v;
        return;
    }
    u64 lo = 0, hi = 0;                            // general: run by run
    for (int b = 0; b < nbytes;) {
        while (end <= pos + b) { ++e; start = end; end = off_at(off, s, e + 1); }   // (pos + b < total = off[K]: ends at a slot with bytes)
        const i64 in_seg = pos + b - start;
        const int take = end - (pos + b) < nbytes - b ? (int)(end - (pos + b)) : nbytes - b;
        const unsigned char* p = seg_src(in, e) + in_seg;
        for (int done = 0; done < take; done += 8) {
            const int m = take - done < 8 ? take - done : 8;
            put(&lo, &hi, b + done, pck::bytes8(p + done, m), m);
        }
        b += take;
    }
    if (nbytes == 16) *(V16*)out = V16{lo, hi};
    else for (int b = 0; b < nbytes; ++b) out[b] = (unsigned char)((b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8))) & 0xff);
}

#ifndef PCK_HOST_EMULATION
__global__ void __launch_bounds__(256)
k_data_fold_ok(i64 K, const unsigned char* ok, const i64* data_off, i64 data_bytes, unsigned char* ok_out, u64* sum) {
    u64 mine = 0;
    fold_ok((i64)blockIdx.x * 256 + threadIdx.x, K, ok, data_off, data_bytes, ok_out, &mine);
    if (mine) atomicAdd(sum, mine);
}

__global__ void __launch_bounds__(256)
k_data_slots(i64 K, const int* index_out, int first_new, i64 A, int* slot) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const int r = slot_of(i, K, index_out, first_new, A);
    if (r >= 0) atomicMin(slot + r, (int)i);
}

__global__ void __launch_bounds__(256)
k_data_lengths(SegIn in, i64 K, i64* len_off, unsigned char* none_out, int* bad) {
    int mine = 0;
    lengths((i64)blockIdx.x * 256 + threadIdx.x, K, in, len_off, none_out, &mine);
    if (mine) atomicAdd(bad, mine);
}

__global__ void __launch_bounds__(256)
k_data_store_off(i64 K, const i64* off, i64 base, i64* off_out, const unsigned char* none, unsigned char* none_out) {
    store_off((i64)blockIdx.x * 256 + threadIdx.x, K, off, base, off_out, none, none_out);
}

// `trips`: an upper bound of the trips a workgroup makes; a trip beyond the stream's end stages nothing and writes nothing
__global__ void __launch_bounds__(WRITE_THREADS)
k_data_copy(SegIn in, i64 K, const i64* off, unsigned char* dst, i64 dst_base, i64 trips) {
    __shared__ Tile s;
    for (i64 trip = 0; trip < trips; ++trip) {
        const i64 chunk0 = first_chunk(blockIdx.x, gridDim.x, trip);
        if (chunk_pos(chunk0, dst_base) >= off[K]) break;   // (uniform)
        __syncthreads();                                    // the last trip's readers are done with the tile
        copy_stage(threadIdx.x, chunk0, K, off, dst_base, &s);
        __syncthreads();
        copy_chunk(threadIdx.x, chunk0, K, in, off, &s, dst, dst_base);
    }
}
#endif

}  // namespace dat
