// The wire bytes of a sync answer, built and parsed on the device (sw_pack_message[_device], sw_unpack_message[_device],
// sw_export_message, sw_ingest_message).  The canonical form is a protocol-4 pickle WITHOUT frames that any
// pickle.loads turns into (head, {id: Event(d, p, t, c, s)}) (tests/model_wire.py states it in Python against pickle):
//
//   message = 0x80 0x04
//             0x8c u8(len mod) mod 0x8c u8(len qual) qual 0x93 0x94 '0'   the class: STACK_GLOBAL, MEMOIZE (memo 0), POP
//             0x8e u64le(8*(K+1)) off[0..K] as u64le '0'                  BINBYTES8: the record-offset table, POPped again
//             'C' 0x20 head32  '}' '('
//             record_0 ... record_{K-1}
//             'u' 0x86 '.'
//   record  = 'C' 0x20 id32  'h' 0x00  '(' D P 'G' t_be64 'C' 0x20 pk32 'C' 0x40 sig64 't' 0x81
//   D = 'N' | 'C' u8(len) data (len < 256) | 'B' u32le(len) data (256 <= len <= MAX_DATA)
//   P = ')' | 'C' 0x20 sp32 'C' 0x20 op32 0x86
//
// off[i] is the absolute position of record i, off[K] that of 'u'.  The table is invisible to an unpickler; it is what lets
// one lane own one record.
//
// Writing (the scan is pack.hip.h's, one stream):
//   k_wire_lengths   one thread per event: k_pack_lengths' range checks, the record's length; an event that cannot be
//                    encoded makes the whole message unbuildable: the lowest such index is kept in *bad
//   k_wire_write     OUTPUT-STATIONARY like k_pack_write: every lane owns one aligned 16-byte chunk of the message, header,
//                    table and trailer included, covers it run by run and issues ONE 16-byte store; the last chunk is
//                    stored byte by byte and nothing at or beyond the message's end is written.  With *bad set it writes
//                    nothing; the length (or -1) goes to *msg_len.
// Reading (strict: a message passes only if it is byte for byte what the writer produces for some arrays):
//   k_wire_header    the bytes in front of the table against the context's, the table's length: K, or -1
//   k_wire_table     one thread per table entry, BEFORE any offset is followed: off[0] is the header's end, the table
//                    increases strictly, off[K] + 3 is the message's length; the constants around the head, the trailer
//   k_wire_records   one thread per record, inside [off[i], off[i+1]) only: the length bytes are read first, the record's
//                    length must be exactly what they imply, then every constant is checked and the fields are copied out;
//                    the creator's key is looked up in the sorted key table (-1: no member's)
//   k_wire_data      output-stationary copy of the data bytes behind the scanned lengths; writes the verdict
// Every kernel body is a sequence of per-thread phases, run thread by thread on the host by tests/wire_emul.cpp.
#pragma once
#include <algorithm>
#include <cstring>

#include "pack.hip.h"

namespace wir {

using pck::i64;
using pck::u64;
using pck::V16;
using pck::Run;

constexpr int MAX_DATA = pck::MAX_DATA;
constexpr int REC_FIXED = 148;              // a record without D and P
constexpr int REC_MIN = REC_FIXED + 2;      // a root whose data is None
constexpr int REC_PARENTS = 69;
constexpr int REC_MAX = REC_FIXED + 5 + REC_PARENTS;   // without the data bytes
constexpr int PRE_MAX = 2 * pck::MAX_NAME + 10;        // the bytes in front of the table's length field
constexpr int HEAD_PART = 37;               // '0' 'C' 0x20 head32 '}' '('
constexpr int WRITE_THREADS = pck::WRITE_THREADS;
constexpr u64 NO_BAD = ~0ull;

constexpr u64 K_ID = 0x2043ull;             // 'C' 0x20
constexpr u64 K_HEAD = 0x204330ull;         // '0' 'C' 0x20
constexpr u64 K_DICT = 0x287dull;           // '}' '('
constexpr u64 K_TRAILER = 0x2e8675ull;      // 'u' TUPLE2 '.'
constexpr u64 K_NONE = 0x4e280068ull;       // 'h' 0 '(' 'N'
constexpr u64 K_BYTES8 = 0x43280068ull;     // 'h' 0 '(' 'C', the length in byte 4
constexpr u64 K_BYTES32 = 0x42280068ull;    // 'h' 0 '(' 'B', the length in bytes 4..7
constexpr u64 K_ROOT = 0x4729ull;           // ')' 'G'
constexpr u64 K_PARENTS_END = 0x4786ull;    // TUPLE2 'G'
constexpr u64 K_SIG = 0x4043ull;            // 'C' 0x40
constexpr u64 K_REC_END = 0x8174ull;        // 't' NEWOBJ

__device__ __forceinline__ int d_size(int dl) { return dl < 0 ? 1 : dl < 256 ? dl + 2 : dl + 5; }
// the position of the first record: prefix, length field, table, head part
__device__ __forceinline__ i64 base_of(i64 K, int pre_len) { return (i64)pre_len + 8 + 8 * (K + 1) + HEAD_PART; }

struct WireIn {
    pck::PackIn in;                   // hdr / hdr_len: the bytes in front of the table's length field
    const unsigned char* id;          // 32 B per event
    const unsigned char* head;        // 32 B
};

#ifdef PCK_HOST_EMULATION
inline void note_min(u64* p, u64 v) { if (v < *p) *p = v; }
#else
__device__ __forceinline__ void note_min(u64* p, u64 v) { atomicMin(p, v); }
#endif

// ---- k_wire_lengths
__device__ __forceinline__ void lengths(i64 i, i64 K, const WireIn& w, i64* off, u64* bad) {
    if (i >= K) return;
    const int ar = w.in.arity[i], cr = w.in.creator[i];
    bool ok = (ar == 0 || ar == 2) && cr >= 0 && cr < w.in.n;
    int dl = -1;
    if (ok) { dl = pck::data_len(w.in, i); ok = dl > -2; }
    off[i] = ok ? REC_FIXED + d_size(dl) + (ar ? REC_PARENTS : 1) : 0;
    if (!ok) note_min(bad, (u64)i);
}

// ---- k_wire_write
struct Rec {         // the record a lane is inside: [start, end) relative to the first record
    i64 start, end;
    const unsigned* id;
    const unsigned* sp;
    const unsigned* op;
    const unsigned* pk;
    const unsigned* sig;
    const unsigned char* data;
    u64 t;
    int dl, ar;
};

__device__ __forceinline__ void load_rec(const WireIn& w, const i64* off, i64 e, Rec* r) {
    r->start = off[e];
    r->end = off[e + 1];
    r->ar = w.in.arity[e];
    r->dl = pck::data_len(w.in, e);
    r->t = __builtin_bswap64(w.in.t[e]);
    r->id = (const unsigned*)(w.id + (size_t)e * 32);
    r->sp = (const unsigned*)(w.in.sp_id + (size_t)e * 32);
    r->op = (const unsigned*)(w.in.op_id + (size_t)e * 32);
    r->sig = (const unsigned*)(w.in.sig + (size_t)e * 64);
    r->pk = (const unsigned*)(w.in.keys + (size_t)w.in.creator[e] * 32);   // (checked by k_wire_lengths: the writer runs only without *bad)
    r->data = r->dl > 0 ? w.in.data + w.in.data_off[e] : nullptr;
}

// the run that starts at byte p of a record
__device__ __forceinline__ Run rec_run(const Rec& v, int p) {
    if (p < 2) return pck::krun(K_ID, p, 2);
    p -= 2;
    if (p < 32) return pck::frun(v.id, p, 32);
    p -= 32;
    const bool root = v.ar == 0;
    const u64 B = root ? K_ROOT : K_ID;
    u64 A;
    int la;
    if (v.dl < 0) { A = K_NONE; la = 4; }
    else if (v.dl < 256) { A = K_BYTES8 | (u64)v.dl << 32; la = 5; }
    else { A = K_BYTES32 | (u64)v.dl << 32; la = 8; }
    if (v.dl <= 0) {
        if (p < la + 2) return pck::krun(A | B << (8 * la), p, la + 2);
        p -= la + 2;
    } else {
        if (p < la) return pck::krun(A, p, la);
        p -= la;
        if (p < v.dl) return pck::brun(v.data, p, v.dl);
        p -= v.dl;
        if (p < 2) return pck::krun(B, p, 2);
        p -= 2;
    }
    if (!root) {
        if (p < 32) return pck::frun(v.sp, p, 32);
        p -= 32;
        if (p < 2) return pck::krun(K_ID, p, 2);
        p -= 2;
        if (p < 32) return pck::frun(v.op, p, 32);
        p -= 32;
        if (p < 2) return pck::krun(K_PARENTS_END, p, 2);
        p -= 2;
    }
    if (p < 8) return pck::krun(v.t, p, 8);
    p -= 8;
    if (p < 2) return pck::krun(K_ID, p, 2);
    p -= 2;
    if (p < 32) return pck::frun(v.pk, p, 32);
    p -= 32;
    if (p < 2) return pck::krun(K_SIG, p, 2);
    p -= 2;
    if (p < 64) return pck::frun(v.sig, p, 64);
    p -= 64;
    return pck::krun(K_REC_END, p, 2);
}

// the run that starts at position pos of the message (0 <= pos < total)
__device__ __forceinline__ Run msg_run(const WireIn& w, i64 K, const i64* off, i64 base, i64 pos, Rec* rc) {
    const i64 pre = w.in.hdr_len;
    if (pos < pre) return pck::brun(w.in.hdr, (int)pos, (int)pre);
    if (pos < pre + 8) return pck::krun((u64)(8 * (K + 1)), (int)(pos - pre), 8);
    const i64 t0 = pre + 8, q = t0 + 8 * (K + 1);
    if (pos < q) return pck::krun((u64)(base + off[(pos - t0) >> 3]), (int)((pos - t0) & 7), 8);
    if (pos < q + 3) return pck::krun(K_HEAD, (int)(pos - q), 3);
    if (pos < q + 35) return pck::brun(w.head, (int)(pos - q - 3), 32);
    if (pos < base) return pck::krun(K_DICT, (int)(pos - q - 35), 2);
    const i64 rel = pos - base;
    if (rel >= off[K]) return pck::krun(K_TRAILER, (int)(rel - off[K]), 3);
    if (rel < rc->start || rel >= rc->end) {
        const i64 hi = rel / REC_MIN < K - 1 ? rel / REC_MIN : K - 1;    // no record is shorter than REC_MIN
        load_rec(w, off, pck::event_of(off, 0, hi, rel), rc);
    }
    return rec_run(*rc, (int)(rel - rc->start));
}

__device__ __forceinline__ i64 first_chunk(unsigned block, unsigned blocks, i64 trip) { return (trip * blocks + block) * WRITE_THREADS; }

__device__ __forceinline__ void write_chunk(int tid, i64 chunk0, i64 K, const WireIn& w, const i64* off, i64 base, unsigned char* out) {
    const i64 total = base + off[K] + 3;
    const i64 pos = (chunk0 + tid) * 16;
    if (pos >= total) return;
    const int nbytes = total - pos < 16 ? (int)(total - pos) : 16;
    Rec rc;
    rc.start = rc.end = -1;
    u64 lo = 0, hi = 0;
    for (int b = 0; b < nbytes;) {
        const Run r = msg_run(w, K, off, base, pos + b, &rc);
        const int take = r.len < nbytes - b ? r.len : nbytes - b;
        for (int done = 0; done < take; done += 8) {
            const int m = take - done < 8 ? take - done : 8;
            u64 x = r.kind == 0 ? r.packed : r.kind == 1 ? pck::fetch8(r.ptr + done, m) : pck::bytes8(r.ptr + done, m);
            if (m < 8) x &= (1ull << (8 * m)) - 1;
            const int at = b + done;
            if (at < 8) { lo |= x << (8 * at); if (at) hi |= x >> (64 - 8 * at); }
            else hi |= x << (8 * (at - 8));
        }
        b += take;
    }
    if (nbytes == 16) {
        *(V16*)(out + pos) = V16{lo, hi};
    } else {
        for (int b = 0; b < nbytes; ++b) out[pos + b] = (unsigned char)((b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8))) & 0xff);
    }
}

__device__ __forceinline__ void write_len(i64 K, const i64* off, i64 base, const u64* bad, i64* msg_len) {
    *msg_len = *bad != NO_BAD ? -1 : base + off[K] + 3;
}

// ---- the reader
struct ReadIn {
    const unsigned char* msg;
    i64 msg_bytes;
    const unsigned char* pre;         // the bytes in front of the table's length field, under this context's class
    int pre_len;
    const unsigned char* skeys;       // the members' keys sorted (by key, then index), n x 32 B
    const int* sperm;                 // ... and the member each belongs to
    int n;
};
struct ReadOut {
    unsigned char* head;
    unsigned char* id;
    unsigned char* sp;
    unsigned char* op;
    unsigned char* arity;
    int* creator;
    u64* t;
    unsigned char* sig;
    i64* data_off;                    // [K + 1]: the lengths, scanned in place
    unsigned char* data_none;
    i64* src;                         // [K] scratch: where the data bytes of record i start in the message
};

// the key table of the reader, built on the host with the keys: sorted by key, then by member index
inline void sort_keys(const unsigned char* keys, int n, unsigned char* skeys, int* sperm) {
    for (int i = 0; i < n; ++i) sperm[i] = i;
    std::sort(sperm, sperm + n, [keys](int a, int b) {
        const int c = memcmp(keys + (size_t)a * 32, keys + (size_t)b * 32, 32);
        return c ? c < 0 : a < b;
    });
    for (int i = 0; i < n; ++i) memcpy(skeys + (size_t)i * 32, keys + (size_t)sperm[i] * 32, 32);
}

// m <= 8 bytes of the message, lowest first.  Byte reads: the message has no padding behind its end.
__device__ __forceinline__ u64 rd(const unsigned char* p, int m) { return pck::bytes8(p, m); }

// k_wire_header: res[0] = K or -1, res[1] = 0 (the refusal flag of the later kernels; the verdict goes elsewhere).  The caller has checked
// msg_bytes >= pre_len + 8.  header_cmp | barrier | header_fin
__device__ __forceinline__ void header_cmp(int tid, int threads, const ReadIn& in, int* differ) {
    for (int j = tid; j < in.pre_len; j += threads)
        if (in.msg[j] != in.pre[j]) *differ = 1;
}
__device__ __forceinline__ void header_fin(int tid, const ReadIn& in, const int* differ, i64* res) {
    if (tid) return;
    res[1] = 0;
    res[0] = -1;
    if (*differ) return;
    const u64 tb = rd(in.msg + in.pre_len, 8);
    if ((tb & 7) || tb < 8 || tb > (u64)in.msg_bytes) return;
    const i64 K = (i64)(tb >> 3) - 1;
    if (K > 0x7fffffff || base_of(K, in.pre_len) + 3 + K * REC_MIN > in.msg_bytes) return;
    res[0] = K;
}

// k_wire_table, thread j <= K.  base_of(K) + 3 <= msg_bytes holds (k_wire_header).
__device__ __forceinline__ void table(i64 j, i64 K, const ReadIn& in, unsigned char* head_out, i64* flag) {
    if (j > K) return;
    const i64 t0 = (i64)in.pre_len + 8, base = base_of(K, in.pre_len);
    const u64 a = rd(in.msg + t0 + 8 * j, 8);
    bool ok = j > 0 || a == (u64)base;
    if (j < K) {
        ok = ok && a < rd(in.msg + t0 + 8 * (j + 1), 8);
    } else {
        const i64 q = t0 + 8 * (K + 1);
        ok = ok && a == (u64)(in.msg_bytes - 3) && rd(in.msg + in.msg_bytes - 3, 3) == K_TRAILER && rd(in.msg + q, 3) == K_HEAD &&
             rd(in.msg + q + 35, 2) == K_DICT;
        for (int b = 0; b < 32; ++b) head_out[b] = in.msg[q + 3 + b];
    }
    if (!ok) *flag = 1;
}

__device__ __forceinline__ int key_cmp(const unsigned char* a, const unsigned char* b) {
    for (int j = 0; j < 32; ++j)
        if (a[j] != b[j]) return a[j] < b[j] ? -1 : 1;
    return 0;
}
// the member whose key is at `key` (the lowest index of equal keys), -1 for the key of no member
__device__ __forceinline__ int member_of(const ReadIn& in, const unsigned char* key) {
    int lo = 0, hi = in.n;                     // the first sorted key that is not below `key`
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = lo + (hi - lo) / 2;
        if (key_cmp(in.skeys + (size_t)mid * 32, key) < 0) lo = mid + 1; else hi = mid;
    }
    return lo < in.n && key_cmp(in.skeys + (size_t)lo * 32, key) == 0 ? in.sperm[lo] : -1;
}

__device__ __forceinline__ void copy_bytes(unsigned char* dst, const unsigned char* src, int m) {
    for (int j = 0; j < m; ++j) dst[j] = src[j];
}

// k_wire_records, thread i < K, only behind a table that passed: [s, e) lies inside the message and s < e
__device__ __forceinline__ void record(i64 i, i64 K, const ReadIn& in, const ReadOut& o, i64* flag) {
    if (i >= K || *flag) return;
    const i64 t0 = (i64)in.pre_len + 8;
    const i64 s = (i64)rd(in.msg + t0 + 8 * i, 8), e = (i64)rd(in.msg + t0 + 8 * (i + 1), 8);
    const i64 L = e - s;
    const unsigned char* r = in.msg + s;
    o.data_off[i] = 0;
    o.src[i] = s;
    if (L < REC_MIN) { *flag = 1; return; }
    // the length bytes first (all below REC_MIN), then the record's length judged before anything else is read
    const unsigned kind = r[37];
    int dl, dsz;
    if (kind == 'N') { dl = -1; dsz = 1; }
    else if (kind == 'C') { dl = r[38]; dsz = 2 + dl; }
    else if (kind == 'B') {
        const u64 ln = rd(r + 38, 4);
        if (ln < 256 || ln > (u64)MAX_DATA) { *flag = 1; return; }
        dl = (int)ln;
        dsz = 5 + dl;
    } else { *flag = 1; return; }
    i64 p = 37 + dsz;
    if (p >= L) { *flag = 1; return; }
    const bool root = r[p] == ')';
    if ((!root && r[p] != 'C') || L != REC_FIXED + dsz + (root ? 1 : REC_PARENTS)) { *flag = 1; return; }
    bool ok = rd(r, 2) == K_ID && rd(r + 34, 3) == (K_NONE & 0xffffff);
    unsigned char* sp = o.sp + (size_t)i * 32;
    unsigned char* op = o.op + (size_t)i * 32;
    if (root) {
        for (int j = 0; j < 32; ++j) sp[j] = op[j] = 0;
        p += 1;
    } else {
        ok = ok && r[p + 1] == 0x20 && rd(r + p + 34, 2) == K_ID && r[p + 68] == 0x86;
        copy_bytes(sp, r + p + 2, 32);
        copy_bytes(op, r + p + 36, 32);
        p += REC_PARENTS;
    }
    ok = ok && r[p] == 'G' && rd(r + p + 9, 2) == K_ID && rd(r + p + 43, 2) == K_SIG && rd(r + p + 109, 2) == K_REC_END;
    if (!ok) { *flag = 1; return; }
    copy_bytes(o.id + (size_t)i * 32, r + 2, 32);
    o.arity[i] = root ? 0 : 2;
    o.t[i] = __builtin_bswap64(rd(r + p + 1, 8));
    o.creator[i] = member_of(in, r + p + 11);
    copy_bytes(o.sig + (size_t)i * 64, r + p + 45, 64);
    o.data_none[i] = dl < 0;
    o.data_off[i] = dl < 0 ? 0 : dl;
    o.src[i] = s + 37 + dsz - (dl < 0 ? 0 : dl);
}

// k_wire_data: the verdict (thread 0 of workgroup 0), and chunk `chunk` of the data bytes: 16 bytes of the output, from the
// records that hold them.  Nothing is copied for a refused message or above the capacity.
__device__ __forceinline__ void verdict(i64 K, const i64* data_off, const i64* flag, i64* res) {
    res[0] = *flag ? -1 : K;
    res[1] = *flag ? 0 : data_off[K];
}
__device__ __forceinline__ void data_chunk(i64 chunk, i64 K, const unsigned char* msg, const ReadOut& o, i64 cap_data, const i64* flag,
                                           unsigned char* data) {
    if (*flag) return;
    const i64 total = o.data_off[K];
    const i64 pos = chunk * 16;
    if (total > cap_data || pos >= total) return;
    const int nbytes = total - pos < 16 ? (int)(total - pos) : 16;
    i64 e = pck::event_of(o.data_off, 0, K - 1, pos);
    i64 start = o.data_off[e], end = o.data_off[e + 1];
    u64 lo = 0, hi = 0;
    for (int b = 0; b < nbytes; ++b) {
        while (pos + b >= end) { ++e; start = end; end = o.data_off[e + 1]; }     // (pos + b < total = data_off[K]: e stays below K)
        const u64 x = msg[o.src[e] + (pos + b - start)];
        if (b < 8) lo |= x << (8 * b); else hi |= x << (8 * (b - 8));
    }
    if (nbytes == 16) {
        *(V16*)(data + pos) = V16{lo, hi};
    } else {
        for (int b = 0; b < nbytes; ++b) data[pos + b] = (unsigned char)((b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8))) & 0xff);
    }
}

#ifndef PCK_HOST_EMULATION
__global__ void __launch_bounds__(256)
k_wire_lengths(WireIn w, i64 K, i64* off, u64* bad) {
    lengths((i64)blockIdx.x * 256 + threadIdx.x, K, w, off, bad);
}

// `trips`: an upper bound from sw_pack_message_bound (the host does not know the length); a trip beyond the end writes nothing
__global__ void __launch_bounds__(WRITE_THREADS)
k_wire_write(WireIn w, i64 K, const i64* off, i64 base, const u64* bad, unsigned char* out, i64* msg_len, i64 trips) {
    if (blockIdx.x == 0 && threadIdx.x == 0) write_len(K, off, base, bad, msg_len);
    if (*bad != NO_BAD) return;                    // (uniform)
    const i64 total = base + off[K] + 3;
    for (i64 trip = 0; trip < trips; ++trip) {
        const i64 chunk0 = first_chunk(blockIdx.x, gridDim.x, trip);
        if (chunk0 * 16 >= total) break;
        write_chunk(threadIdx.x, chunk0, K, w, off, base, out);
    }
}

__global__ void __launch_bounds__(256)
k_wire_header(ReadIn in, i64* res) {
    __shared__ int differ;
    if (threadIdx.x == 0) differ = 0;
    __syncthreads();
    header_cmp(threadIdx.x, 256, in, &differ);
    __syncthreads();
    header_fin(threadIdx.x, in, &differ, res);
}

__global__ void __launch_bounds__(256)
k_wire_table(ReadIn in, i64 K, unsigned char* head_out, i64* flag) {
    table((i64)blockIdx.x * 256 + threadIdx.x, K, in, head_out, flag);
}

__global__ void __launch_bounds__(256)
k_wire_records(ReadIn in, i64 K, ReadOut o, i64* flag) {
    record((i64)blockIdx.x * 256 + threadIdx.x, K, in, o, flag);
}

// grid-stride over the chunks of cap_data
__global__ void __launch_bounds__(256)
k_wire_data(const unsigned char* msg, i64 K, ReadOut o, i64 cap_data, const i64* flag, unsigned char* data, i64* res) {
    if (blockIdx.x == 0 && threadIdx.x == 0) verdict(K, o.data_off, flag, res);
    const i64 chunks = (cap_data + 15) / 16;
    for (i64 q = (i64)blockIdx.x * 256 + threadIdx.x; q < chunks; q += (i64)gridDim.x * 256) data_chunk(q, K, msg, o, cap_data, flag, data);
}
#endif

}  // namespace wir
