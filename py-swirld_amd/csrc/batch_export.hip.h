// The results of a whole batch in one launch (include/swirld_hip.h: sw_export_batch_*): an
// output-stationary ragged gather, the idiom of pack.hip.h / data.hip.h — one aligned 16-byte store per lane.
// The output of an array is the concatenation of one segment per hashgraph, off[b] .. off[b + 1] ENTRIES (off is the host's
// prefix sum over the ranges it has checked); an entry is `cols` elements of `width` bytes, read `stride` elements apart
// per entry from the hashgraph's source address (rows of n columns out of rows of npad, or plain arrays: cols = stride = 1).
// The host computes the source addresses (slab segment + range start), so nothing here knows the layout of a slab, and
// a batch above 4 GiB is no special case: every index is 64-bit.
// The per-chunk function is SWX_HD: tests/batch_export_main.cpp runs it over host arrays under the sanitizers.
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

namespace swbx {

constexpr int MAX_ARRAYS = 4;   // arrays one call gathers (blockIdx.y)
constexpr int CHUNK = 16;       // output bytes a thread owns
constexpr int THREADS = 256;

struct Array {
    const unsigned long long* src;   // [B] address of the first element hashgraph b contributes
    unsigned char* dst;              // 16-byte aligned; total * cols * width bytes are written, no byte more
    int width;                       // bytes per element: 1, 4 or 8
    int cols;                        // elements per entry
    long long stride;                // source elements from one entry to the next (>= cols)
};

struct Plan {
    const long long* off;   // [B + 1] entries, off[0] = 0, off[B] = total
    long long B, total;
    int n_arrays;
    Array a[MAX_ARRAYS];
};

template <int W> struct Elem;
template <> struct Elem<1> { typedef uint8_t T; };
template <> struct Elem<4> { typedef uint32_t T; };
template <> struct Elem<8> { typedef uint64_t T; };

// chunks (threads) an array of `total` entries needs
constexpr long long chunks_of(long long total, int cols, int width) { return (total * cols * width + CHUNK - 1) / CHUNK; }

template <int W>
SWX_HD inline void export_chunk_w(const Plan& p, const Array& a, long long chunk) {
    typedef typename Elem<W>::T T;
    constexpr int PER = CHUNK / W;
    const long long elems = p.total * a.cols;
    const long long i0 = chunk * PER;
    if (chunk < 0 || i0 >= elems) return;
    long long e = i0 / a.cols;            // the entry and the column of the chunk's first element
    int col = (int)(i0 - e * a.cols);
    long long lo = 0, hi = p.B;           // its hashgraph: the last b with off[b] <= e (off[B] = total > e, so b's segment holds e)
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (p.off[mid] <= e) lo = mid; else hi = mid;
    }
    long long b = lo, end = p.off[b + 1];
    const T* row = (const T*)(uintptr_t)a.src[b] + (e - p.off[b]) * a.stride;
    const int m = elems - i0 < PER ? (int)(elems - i0) : PER;
    uint32_t w[4] = {0, 0, 0, 0};
    T* out = (T*)a.dst + i0;
#if SWX_DEVICE
#pragma unroll   // (w[] stays in registers)
#endif
    for (int j = 0; j < PER; ++j) {
        if (j < m) {
            const T v = row[col];
            if (m < PER) out[j] = v;      // the last, partial chunk: element by element, nothing beyond the end
            else if constexpr (W == 1) w[j >> 2] |= (uint32_t)v << (8 * (j & 3));
            else if constexpr (W == 4) w[j] = (uint32_t)v;
            else { w[2 * j] = (uint32_t)v; w[2 * j + 1] = (uint32_t)((uint64_t)v >> 32); }
            if (++col == a.cols && j + 1 < m) {   // on to the next entry: over the segment's end and the empty segments behind it
                col = 0;
                ++e;
                if (e < end) row += a.stride;
                else {
                    do { ++b; end = p.off[b + 1]; } while (e >= end);   // (e < total = off[B]: ends at a b < B)
                    row = (const T*)(uintptr_t)a.src[b];
                }
            }
        }
    }
    if (m == PER) {
#if SWX_DEVICE
        *(uint4*)out = make_uint4(w[0], w[1], w[2], w[3]);
#else
        memcpy(out, w, CHUNK);            // (little endian, as the device)
#endif
    }
}

// 16 output bytes of array k: 16, 4 or 2 elements
SWX_HD inline void export_chunk(const Plan& p, int k, long long chunk) {
    const Array& a = p.a[k];
    if (a.width == 1) export_chunk_w<1>(p, a, chunk);
    else if (a.width == 4) export_chunk_w<4>(p, a, chunk);
    else export_chunk_w<8>(p, a, chunk);
}

}  // namespace swbx

#if SWX_DEVICE
// blockIdx.y: the array; blockIdx.x * THREADS + threadIdx.x: the chunk.  The grid is sized by the array of most chunks.
__global__ void __launch_bounds__(swbx::THREADS) k_batch_export(const swbx::Plan p) {
    swbx::export_chunk(p, (int)blockIdx.y, (long long)blockIdx.x * swbx::THREADS + threadIdx.x);
}
#endif
