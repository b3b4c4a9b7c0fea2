// The signed bytes of events, built on the device (sw_pack_events[_device], sw_sync_pull_validated): from
// the arrays sw_export_payload_device writes — parents' ids, arity, creator, timestamp, signature per event — to the two
// byte streams sw_validate_payload_device reads, dumps(ev[:-1]) (what the signature covers, swirld.py:99) and dumps(ev)
// (what the id is the hash of, swirld.py:95, :103).  For the shapes these arrays can hold the pickle is a fixed template
// (protocol 4, one frame, no memo reads; tests/model_pack.py states it in Python against pickle.dumps):
//
//   msg   = FRAME( '(' D P 'G' t_be64 'C' 0x20 pk32 0x94 't' 0x94 '.' )
//   whole = FRAME( HDR '(' D P 'G' t_be64 'C' 0x20 pk32 0x94 'C' 0x40 sig64 0x94 't' 0x94 0x81 0x94 '.' )
//   FRAME(x) = 0x80 0x04 0x95 u64le(len(x)) x
//   HDR  = 0x8c len(mod) mod 0x94 0x8c len(qual) qual 0x94 0x93 0x94         the Event class, a setting of the context
//   D    = 'N' | 'C' u8(len) data 0x94 (len < 256) | 'B' u32le(len) data 0x94 (len <= MAX_DATA)
//   P    = ')' | 'C' 0x20 sp32 0x94 'C' 0x20 op32 0x94 0x86 0x94
//
// Five kernels, none of which waits for another workgroup:
//   k_pack_lengths   one thread per event: range checks, the two lengths (0 for an event that cannot be encoded), the flag
//   k_pack_tile_sums one workgroup per tile of TILE events and stream: the sum of its lengths
//   k_pack_scan_sums one workgroup per stream: exclusive scan of the tile sums, off[K] = the total
//   k_pack_offsets   per tile: the lengths turned into exclusive offsets, in place
//   k_pack_write     OUTPUT-STATIONARY: every lane owns one aligned 16-byte chunk of the stream.  A workgroup covers
//                    WRITE_THREADS consecutive chunks per trip; it stages the offsets of the events under them in LDS (one
//                    search over the global offsets per trip, then WRITE_THREADS consecutive entries), each lane finds its
//                    event by a binary search over that tile and covers its 16 bytes RUN by run: the layout (constants,
//                    length fields, five array fields) is asked once per run, not once per byte; up to 8 bytes of a run
//                    are shifted into place at a time, and ONE 16-byte store is issued.  Array fields are read as
//                    aligned dwords; the data bytes, whose buffer has no alignment and no padding, are read as bytes.
//                    A chunk may span two events with a length (a root is 61 bytes) and any number of empty ones.
//                    Only the last chunk of a stream can be partial (the stream starts 16-byte aligned): its lane stores
//                    the bytes below off[K] one by one and nothing at or beyond off[K].
// Every index that derives from the caller's arrays is checked before it is followed: creator against the member count,
// the data range against the buffer.  An event that fails a check has length 0 in both streams and is never visited by
// the writer.
//
// Each kernel body is a sequence of per-thread phases (plain functions of the thread index, LDS passed as a pointer) with a
// barrier between them: tests/pack_emul.cpp runs the same phases thread by thread on the host, under sanitizers.
#pragma once
#ifndef PCK_HOST_EMULATION
#include <hip/hip_runtime.h>
#endif

#include "tmpl.hip.h"

namespace pck {

// (the template's lengths and opcode groups: tmpl.hip.h, shared with the signer)
constexpr int MAX_DATA = tpl::MAX_DATA;
constexpr int MAX_NAME = 255;
constexpr int HDR_MAX = 2 * MAX_NAME + 8;
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_PER = 4;
constexpr int TILE = SCAN_THREADS * SCAN_PER;   // events per tile of the scan
constexpr int WRITE_THREADS = 256;              // chunks per workgroup and trip; also the entries of the offset tile
constexpr int MSG_FIXED = tpl::MSG_FIXED;
constexpr int WHOLE_FIXED = tpl::WHOLE_FIXED;
constexpr int PARENTS = tpl::PARENTS;
constexpr int MSG_MAX = MSG_FIXED + PARENTS + 6;       // per event, without its data bytes
constexpr int WHOLE_MAX = WHOLE_FIXED + PARENTS + 6;   // ... and without HDR

typedef long long i64;
typedef unsigned long long u64;

struct alignas(16) V16 { u64 lo, hi; };

struct PackIn {
    const unsigned char* sp_id;       // 32 B per event (read only where the arity is 2)
    const unsigned char* op_id;
    const unsigned char* arity;
    const int* creator;
    const u64* t;                     // the doubles as 64-bit words: bit pattern kept
    const unsigned char* sig;         // 64 B per event
    const unsigned char* data;        // data, data_off both null: every event's data is None
    const i64* data_off;              // [K + 1]
    i64 data_bytes;
    const unsigned char* data_none;   // may be null: nonzero = None whatever the range
    const unsigned char* keys;        // n x 32 B, the members' keys
    const unsigned char* hdr;         // HDR, hdr_len bytes
    int hdr_len;
    int n;
};

// the length of event i's data: >= 0, -1 for None, -2 when the range cannot be used
__device__ __forceinline__ int data_len(const PackIn& in, i64 i) {
    if (!in.data_off) return -1;
    const i64 a = in.data_off[i], b = in.data_off[i + 1];
    if (a < 0 || b < a || b > in.data_bytes || b - a > MAX_DATA) return -2;
    if (in.data_none && in.data_none[i]) return -1;
    return (int)(b - a);
}
__device__ __forceinline__ int d_size(int dl) { return tpl::d_size(dl); }

// ---- k_pack_lengths
__device__ __forceinline__ void lengths(i64 i, i64 K, const PackIn& in, i64* msg_off, i64* whole_off, unsigned char* enc) {
    if (i >= K) return;
    const int ar = in.arity[i], cr = in.creator[i];
    bool ok = (ar == 0 || ar == 2) && cr >= 0 && cr < in.n;
    int dl = -1;
    if (ok) { dl = data_len(in, i); ok = dl > -2; }
    const int var = ok ? d_size(dl) + (ar ? PARENTS : 1) : 0;
    msg_off[i] = ok ? MSG_FIXED + var : 0;
    whole_off[i] = ok ? WHOLE_FIXED + in.hdr_len + var : 0;
    if (enc) enc[i] = ok;
}

// ---- the scan.  part: SCAN_THREADS i64 of LDS (+ 1 for the carry of k_pack_scan_sums)
__device__ __forceinline__ void tile_sum(int l, i64 tile, i64 K, const i64* off, i64* part) {
    i64 s = 0;
    for (int j = 0; j < SCAN_PER; ++j) {
        const i64 i = tile * TILE + (i64)l * SCAN_PER + j;
        if (i < K) s += off[i];
    }
    part[l] = s;
}
// lane 0: part[] -> its exclusive scan starting at `base`; returns the end value
__device__ __forceinline__ i64 part_scan(i64* part, i64 base) {
    i64 run = base;
    for (int k = 0; k < SCAN_THREADS; ++k) { const i64 v = part[k]; part[k] = run; run += v; }
    return run;
}
__device__ __forceinline__ void tile_total(int l, i64 tile, i64* part, i64* tsum) {
    if (l == 0) tsum[tile] = part_scan(part, 0);
}
// k_pack_scan_sums, pass p over SCAN_THREADS tiles: load | barrier | scan | barrier | store
__device__ __forceinline__ void sums_load(int l, i64 p, i64 tiles, const i64* tsum, i64* part) {
    const i64 k = p * SCAN_THREADS + l;
    part[l] = k < tiles ? tsum[k] : 0;
}
__device__ __forceinline__ void sums_scan(int l, i64 p, i64* part) {
    if (l == 0) part[SCAN_THREADS] = part_scan(part, p == 0 ? 0 : part[SCAN_THREADS]);
}
__device__ __forceinline__ void sums_store(int l, i64 p, i64 tiles, i64 K, const i64* part, i64* tsum, i64* off) {
    const i64 k = p * SCAN_THREADS + l;
    if (k < tiles) tsum[k] = part[l];
    if (l == 0 && (p + 1) * SCAN_THREADS >= tiles) off[K] = part[SCAN_THREADS];
}
// k_pack_offsets: tile_sum | barrier | offsets_scan | barrier | offsets_write
__device__ __forceinline__ void offsets_scan(int l, i64 tile, i64* part, const i64* tsum) {
    if (l == 0) (void)part_scan(part, tsum[tile]);
}
__device__ __forceinline__ void offsets_write(int l, i64 tile, i64 K, const i64* part, i64* off) {
    i64 run = part[l];
    for (int j = 0; j < SCAN_PER; ++j) {
        const i64 i = tile * TILE + (i64)l * SCAN_PER + j;
        if (i >= K) return;
        const i64 v = off[i];
        off[i] = run;
        run += v;
    }
}

// ---- k_pack_write
// the event that holds stream position pos (0 <= pos < off[K]): the largest e in [lo, hi] with off[e] <= pos
__device__ __forceinline__ i64 event_of(const i64* off, i64 lo, i64 hi, i64 pos) {
    for (int it = 0; it < 64 && lo < hi; ++it) {
        const i64 mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= pos) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct Tile {        // LDS of k_pack_write
    i64 off[WRITE_THREADS];
    i64 e0;          // off[j] = the stream's off[e0 + j], j < cnt
    int cnt;
    unsigned char hdr[HDR_MAX + 2];
};

__device__ __forceinline__ void write_hdr(int tid, const PackIn& in, Tile* s) {
    for (int j = tid; j < in.hdr_len; j += WRITE_THREADS) s->hdr[j] = in.hdr[j];
}
// the chunks of trip `trip` of workgroup `block` start at chunk number first_chunk(...)
__device__ __forceinline__ i64 first_chunk(unsigned block, unsigned blocks, i64 trip) { return (trip * blocks + block) * WRITE_THREADS; }

__device__ __forceinline__ void write_stage(int tid, i64 chunk0, i64 K, const i64* off, Tile* s) {
    const i64 base = chunk0 * 16;
    if (base >= off[K]) { if (tid == 0) { s->cnt = 0; s->e0 = 0; } return; }
    const i64 e0 = event_of(off, 0, K - 1, base);   // (uniform over the workgroup)
    const i64 left = K + 1 - e0;
    if (tid < left) s->off[tid] = off[e0 + tid];
    if (tid == 0) { s->e0 = e0; s->cnt = (int)(left < WRITE_THREADS ? left : WRITE_THREADS); }
}

__device__ __forceinline__ i64 off_at(const i64* off, const Tile* s, i64 e) {
    const i64 j = e - s->e0;
    return j < s->cnt ? s->off[j] : off[e];
}

struct Ev {          // one event as the writer sees it
    const unsigned* sp;
    const unsigned* op;
    const unsigned* pk;
    const unsigned* sig;
    const unsigned char* data;
    u64 t;           // the timestamp's bytes, most significant in the lowest byte
    u64 inner;       // the frame's length field
    int dl, ar;
};
// A RUN of the stream: `len` consecutive bytes of one segment of an event's layout, from the position asked about to the
// segment's end.  kind 0: the bytes are `packed`, lowest byte first (constants, length fields, the timestamp: at most 8);
// kind 1: bytes at `ptr` inside an array field, read as aligned dwords; kind 2: bytes at `ptr` read one by one (the data,
// whose buffer has no alignment and no padding, and the class header in LDS).
struct Run { const unsigned char* ptr; u64 packed; int len; int kind; };

__device__ __forceinline__ Run krun(u64 packed, int p, int len) { return Run{nullptr, packed >> (8 * p), len - p, 0}; }
__device__ __forceinline__ Run frun(const unsigned* base, int p, int len) { return Run{(const unsigned char*)base + p, 0ull, len - p, 1}; }
__device__ __forceinline__ Run brun(const unsigned char* base, int p, int len) { return Run{base + p, 0ull, len - p, 2}; }

__device__ __forceinline__ void load_event(const PackIn& in, i64 e, i64 len, Ev* v) {
    v->ar = in.arity[e];
    v->dl = data_len(in, e);
    v->t = __builtin_bswap64(in.t[e]);   // most significant byte first
    v->inner = (u64)(len - tpl::FRAME);
    v->sp = (const unsigned*)(in.sp_id + (size_t)e * 32);
    v->op = (const unsigned*)(in.op_id + (size_t)e * 32);
    v->sig = (const unsigned*)(in.sig + (size_t)e * 64);
    v->pk = (const unsigned*)(in.keys + (size_t)in.creator[e] * 32);   // (the creator of an event with a length is a member)
    v->data = v->dl > 0 ? in.data + in.data_off[e] : nullptr;
}

// the run that starts at byte p of the event's message (0 <= p < its length).  Neighbouring constants are one segment
// ('(' with the head of D; the tail of D with the head of P; all of them where there are no data bytes in between), so
// that 16 bytes of a stream hold few runs.
template <bool WHOLE>
__device__ __forceinline__ Run event_run(const Ev& v, const Tile* s, int hdr_len, int p) {
    if (p < 3) return krun(tpl::K_FRAME, p, 3);
    if (p < tpl::FRAME) return krun(v.inner, p - 3, 8);
    p -= tpl::FRAME;
    if (WHOLE) {
        if (p < hdr_len) return brun(s->hdr, p, hdr_len);
        p -= hdr_len;
    }
    const bool root = v.ar == 0;
    u64 A, B = root ? tpl::K_ROOT : tpl::K_ID;      // A: '(' and the head of D;  B: [0x94] and ")G" or "C\x20"
    int la, lb = 2;
    if (v.dl < 0) { A = tpl::K_NONE; la = 2; }
    else if (v.dl < 256) { A = tpl::K_BYTES8 | (u64)v.dl << 16; la = 3; }
    else { A = tpl::K_BYTES32 | (u64)v.dl << 16; la = 6; }
    if (v.dl >= 0) { B = B << 8 | tpl::K_MEMO; lb = 3; }
    if (v.dl <= 0) {
        if (p < la + lb) return krun(A | B << (8 * la), p, la + lb);
        p -= la + lb;
    } else {
        if (p < la) return krun(A, p, la);
        p -= la;
        if (p < v.dl) return brun(v.data, p, v.dl);
        p -= v.dl;
        if (p < lb) return krun(B, p, lb);
        p -= lb;
    }
    if (!root) {
        if (p < 32) return frun(v.sp, p, 32);
        p -= 32;
        if (p < 3) return krun(tpl::K_ID_NEXT, p, 3);
        p -= 3;
        if (p < 32) return frun(v.op, p, 32);
        p -= 32;
        if (p < 4) return krun(tpl::K_PARENTS_END, p, 4);
        p -= 4;
    }
    if (p < 8) return krun(v.t, p, 8);
    p -= 8;
    if (p < 2) return krun(tpl::K_ID, p, 2);
    p -= 2;
    if (p < 32) return frun(v.pk, p, 32);
    p -= 32;
    if (!WHOLE) return krun(tpl::K_MSG_END, p, 4);
    if (p < 3) return krun(tpl::K_SIG, p, 3);
    p -= 3;
    if (p < 64) return frun(v.sig, p, 64);
    p -= 64;
    return krun(tpl::K_WHOLE_END, p, 6);
}

// m <= 8 bytes at ptr, lowest first, from the aligned dwords that hold them (no dword without a wanted byte is read)
__device__ __forceinline__ u64 fetch8(const unsigned char* ptr, int m) {
    const unsigned o = (unsigned)((size_t)ptr & 3);
    const unsigned* w = (const unsigned*)(ptr - o);
    const u64 w0 = w[0], w1 = (int)o + m > 4 ? w[1] : 0u, w2 = (int)o + m > 8 ? w[2] : 0u;
    u64 x = (w0 | w1 << 32) >> (8 * o);
    if (o) x |= w2 << (64 - 8 * o);
    return x;
}
__device__ __forceinline__ u64 bytes8(const unsigned char* ptr, int m) {
    u64 x = 0;
    for (int j = 0; j < m; ++j) x |= (u64)ptr[j] << (8 * j);
    return x;
}

// One chunk, run by run: a lane asks the layout once per RUN (lanes of a wave sit in different segments, so a wave pays
// for every arm of event_run each time any lane asks), takes up to 8 bytes of it per step and shifts them into its two
// 64-bit halves.  A message is at least 61 bytes, so a chunk holds bytes of at most TWO events with a length (any number
// of empty ones between them): both are found and loaded first.
template <bool WHOLE>
__device__ __forceinline__ void write_chunk(int tid, i64 chunk0, i64 K, const PackIn& in, const i64* off, const Tile* s, unsigned char* out) {
    if (s->cnt == 0) return;
    const i64 total = off[K];
    const i64 pos = (chunk0 + tid) * 16;
    if (pos >= total) return;
    const int cnt = s->cnt;
    const i64 e0 = s->e0;
    i64 e;
    if (pos >= s->off[cnt - 1] && e0 + cnt - 1 < K) e = event_of(off, e0 + cnt - 1, K - 1, pos);   // beyond the tile (runs of empty events)
    else e = e0 + event_of(s->off, 0, cnt - 2, pos);
    const i64 start = off_at(off, s, e), end = off_at(off, s, e + 1);
    const int nbytes = total - pos < 16 ? (int)(total - pos) : 16;
    const int n1 = end - pos < nbytes ? (int)(end - pos) : nbytes;    // bytes of the first event
    Ev v, v2;
    load_event(in, e, end - start, &v);
    v2 = v;
    if (n1 < nbytes) {   // the next event with a length
        i64 e2 = e + 1, end2 = off_at(off, s, e2 + 1);
        while (end2 == end) { ++e2; end2 = off_at(off, s, e2 + 1); }
        load_event(in, e2, end2 - end, &v2);
    }
    int p = (int)(pos - start), stop = n1;
    u64 lo = 0, hi = 0;
    for (int b = 0; b < nbytes;) {
        if (b == stop) { v = v2; p = 0; stop = nbytes; }
        const Run r = event_run<WHOLE>(v, s, in.hdr_len, p);
        const int take = r.len < stop - b ? r.len : stop - b;
        for (int done = 0; done < take; done += 8) {
            const int m = take - done < 8 ? take - done : 8;
            u64 x = r.kind == 0 ? r.packed : r.kind == 1 ? fetch8(r.ptr + done, m) : bytes8(r.ptr + done, m);
            if (m < 8) x &= (1ull << (8 * m)) - 1;
            const int at = b + done;
            if (at < 8) { lo |= x << (8 * at); if (at) hi |= x >> (64 - 8 * at); }
            else hi |= x << (8 * (at - 8));
        }
        b += take;
        p += take;
    }
    if (nbytes == 16) {
        *(V16*)(out + pos) = V16{lo, hi};
    } else {
        for (int b = 0; b < nbytes; ++b) out[pos + b] = (unsigned char)((b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8))) & 0xff);
    }
}

// d_ok[i] &= enc[i], and the number of events still valid (sw_sync_pull_validated)
__device__ __forceinline__ void and_flag(i64 i, i64 K, unsigned char* ok, const unsigned char* enc, int* lane_count) {
    if (i >= K) return;
    const unsigned char v = ok[i] && enc[i];
    ok[i] = v;
    *lane_count += v;
}

#ifndef PCK_HOST_EMULATION
__global__ void __launch_bounds__(256)
k_pack_lengths(PackIn in, i64 K, i64* msg_off, i64* whole_off, unsigned char* enc) {
    lengths((i64)blockIdx.x * 256 + threadIdx.x, K, in, msg_off, whole_off, enc);
}

// blockIdx.y: 0 the msg stream, 1 the whole stream; tsum holds `tiles` entries per stream
__global__ void __launch_bounds__(SCAN_THREADS)
k_pack_tile_sums(i64 K, i64 tiles, const i64* msg_off, const i64* whole_off, i64* tsum) {
    __shared__ i64 part[SCAN_THREADS];
    const i64* off = blockIdx.y ? whole_off : msg_off;
    tile_sum(threadIdx.x, blockIdx.x, K, off, part);
    __syncthreads();
    tile_total(threadIdx.x, blockIdx.x, part, tsum + blockIdx.y * tiles);
}

__global__ void __launch_bounds__(SCAN_THREADS)
k_pack_scan_sums(i64 K, i64 tiles, i64* msg_off, i64* whole_off, i64* tsum) {
    __shared__ i64 part[SCAN_THREADS + 1];
    i64* off = blockIdx.x ? whole_off : msg_off;
    i64* ts = tsum + blockIdx.x * tiles;
    const i64 passes = (tiles + SCAN_THREADS - 1) / SCAN_THREADS;
    if (passes == 0 && threadIdx.x == 0) off[K] = 0;
    for (i64 p = 0; p < passes; ++p) {
        sums_load(threadIdx.x, p, tiles, ts, part);
        __syncthreads();
        sums_scan(threadIdx.x, p, part);
        __syncthreads();
        sums_store(threadIdx.x, p, tiles, K, part, ts, off);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(SCAN_THREADS)
k_pack_offsets(i64 K, i64 tiles, i64* msg_off, i64* whole_off, const i64* tsum) {
    __shared__ i64 part[SCAN_THREADS];
    i64* off = blockIdx.y ? whole_off : msg_off;
    tile_sum(threadIdx.x, blockIdx.x, K, off, part);
    __syncthreads();
    offsets_scan(threadIdx.x, blockIdx.x, part, tsum + blockIdx.y * tiles);
    __syncthreads();
    offsets_write(threadIdx.x, blockIdx.x, K, part, off);
}

// `trips`: an upper bound of the trips a workgroup makes, from the stream's capacity (the host does not know off[K]); a
// trip beyond the stream's end stages nothing and writes nothing
template <bool WHOLE>
__global__ void __launch_bounds__(WRITE_THREADS)
k_pack_write(PackIn in, i64 K, const i64* off, unsigned char* out, i64 trips) {
    __shared__ Tile s;
    if (WHOLE) write_hdr(threadIdx.x, in, &s);
    for (i64 trip = 0; trip < trips; ++trip) {
        const i64 chunk0 = first_chunk(blockIdx.x, gridDim.x, trip);
        if (chunk0 * 16 >= off[K]) break;          // (uniform)
        __syncthreads();                           // the last trip's readers are done with the tile
        write_stage(threadIdx.x, chunk0, K, off, &s);
        __syncthreads();
        write_chunk<WHOLE>(threadIdx.x, chunk0, K, in, off, &s, out);
    }
}

// grid-stride: the verdicts ANDed with the flags, the survivors counted into *n_valid (zeroed by the caller)
__global__ void __launch_bounds__(256)
k_pack_and_count(i64 K, unsigned char* ok, const unsigned char* enc, int* n_valid) {
    int mine = 0;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < K; i += (i64)gridDim.x * 256) and_flag(i, K, ok, enc, &mine);
    if (mine) atomicAdd(n_valid, mine);
}
#endif

}  // namespace pck
