// Host emulation of the kernels of py-swirld_amd/csrc/data.hip.h: the per-thread phases of k_data_fold_ok, k_data_slots,
// k_data_lengths, the scan (pack.hip.h's three kernels, as the library launches them), k_data_store_off and k_data_copy are
// run thread by thread, a barrier being the end of a phase, by one host thread — workgroup by workgroup, the LDS of each
// as a plain object.  Built with -fsanitize=address,undefined by tests/test_data_kernels_host.py, which compares with
// tests/model_data.py: an index outside an array, a misaligned 16-byte access, or a search that leaves its range shows up
// here without a GPU.  Every input array has its exact size (an "arena" source: 16-byte aligned with the 16 bytes of slack
// the library guarantees, and nothing more), so the sanitizer sees every overrun; the destination starts as 0xA5 everywhere.
//
// usage: data_emul IN OUT
//   IN : int64 mode, then
//     mode 0 (ragged gather): K, n_src, flags (1 offsets, 2 none flags, 4 indices, 8 arena source), src_bytes, grid, dst_base,
//        dst_cap; [n_src + 1 int64 src_off] [src_bytes B] [n_src B none] [K int32 idx]
//        OUT: int64 bad, K + 1 int64 off (plus dst_base), K B none, dst_cap B destination   (bad != 0: no copy was made)
//     mode 1 (fold ok): K, flags (1 ok given, 2 offsets given), data_bytes; [K B ok] [K + 1 int64 data_off]    OUT: K B, uint64 sum of the ok lengths
//     mode 2 (slots): K, first_new, A; K int32 index_out                                                   OUT: A int32
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define PCK_HOST_EMULATION
#define __device__
#define __forceinline__ inline
#include "../py-swirld_amd/csrc/data.hip.h"

using dat::i64;

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
template <class T>
static void wr(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

static void scan(i64 K, i64* off) {   // the launches of data_plan: one stream, grid (tiles, 1) / 1 / (tiles, 1)
    const i64 tiles = (K + pck::TILE - 1) / pck::TILE;
    std::vector<i64> tsum((size_t)tiles + 1), part(pck::SCAN_THREADS + 1);
    const int T = pck::SCAN_THREADS;
    for (i64 b = 0; b < tiles; ++b) {
        for (int l = 0; l < T; ++l) pck::tile_sum(l, b, K, off, part.data());
        for (int l = 0; l < T; ++l) pck::tile_total(l, b, part.data(), tsum.data());
    }
    const i64 passes = (tiles + T - 1) / T;
    if (passes == 0) off[K] = 0;
    for (i64 p = 0; p < passes; ++p) {
        for (int l = 0; l < T; ++l) pck::sums_load(l, p, tiles, tsum.data(), part.data());
        for (int l = 0; l < T; ++l) pck::sums_scan(l, p, part.data());
        for (int l = 0; l < T; ++l) pck::sums_store(l, p, tiles, K, part.data(), tsum.data(), off);
    }
    for (i64 b = 0; b < tiles; ++b) {
        for (int l = 0; l < T; ++l) pck::tile_sum(l, b, K, off, part.data());
        for (int l = 0; l < T; ++l) pck::offsets_scan(l, b, part.data(), tsum.data());
        for (int l = 0; l < T; ++l) pck::offsets_write(l, b, K, part.data(), off);
    }
}

static int gather(FILE* f, FILE* g) {
    const std::vector<i64> h = rd<i64>(f, 8);
    const i64 K = h[0], n_src = h[1], flags = h[2], src_bytes = h[3], grid = h[4], dst_base = h[5], dst_cap = h[6];
    const size_t k = (size_t)K;
    std::vector<i64> src_off;
    std::vector<unsigned char> none;
    std::vector<int> idx;
    if (flags & 1) src_off = rd<i64>(f, (size_t)n_src + 1);
    const std::vector<unsigned char> raw = rd<unsigned char>(f, (size_t)src_bytes);
    if (flags & 2) none = rd<unsigned char>(f, (size_t)n_src);
    if (flags & 4) idx = rd<int>(f, k);
    // the source: exact size, or — an arena — 16-byte aligned with exactly the slack behind it
    const bool arena = flags & 8;
    const size_t src_alloc = arena ? ((size_t)src_bytes + dat::SLACK + 15) / 16 * 16 : (size_t)src_bytes;
    unsigned char* src = arena ? (unsigned char*)aligned_alloc(16, src_alloc) : (unsigned char*)malloc(src_alloc ? src_alloc : 1);
    if (arena) memset(src, 0x5A, src_alloc);
    if (src_bytes) memcpy(src, raw.data(), (size_t)src_bytes);
    const dat::SegIn in{src, flags & 1 ? src_off.data() : nullptr, flags & 2 ? none.data() : nullptr, flags & 4 ? idx.data() : nullptr, n_src, src_bytes,
                        arena ? 1 : 0};
    std::vector<i64> off(k + 2, -7), off_out(k + 1, -7);
    std::vector<unsigned char> none_s(k, 0xA5), none_out(k, 0xA5);
    int bad = 0;
    const i64 blocks = (K + 255) / 256;   // k_data_lengths
    for (i64 i = 0; i < blocks * 256; ++i) dat::lengths(i, K, in, off.data(), none_s.data(), &bad);
    scan(K, off.data());
    const size_t dst_alloc = ((size_t)dst_cap + 15) / 16 * 16;
    unsigned char* dst = (unsigned char*)aligned_alloc(16, dst_alloc ? dst_alloc : 16);
    memset(dst, 0xA5, dst_alloc);
    if (!bad) {
        const i64 total = off[k];
        if (dst_base + total > dst_cap) { fprintf(stderr, "total %lld beyond the capacity\n", (long long)total); return 3; }
        const int T = dat::WRITE_THREADS;
        const i64 chunks = ((dst_base & 15) + total + 15) / 16;
        const i64 trips = (chunks + grid * T - 1) / (grid * T) + 1;   // (one trip more than needed: it must do nothing)
        if (total > 0)
            for (unsigned b = 0; b < (unsigned)grid; ++b) {
                dat::Tile s;
                memset(&s, 0xEE, sizeof s);
                for (i64 trip = 0; trip < trips; ++trip) {
                    const i64 chunk0 = dat::first_chunk(b, (unsigned)grid, trip);
                    if (dat::chunk_pos(chunk0, dst_base) >= off[k]) break;
                    for (int t = 0; t < T; ++t) dat::copy_stage(t, chunk0, K, off.data(), dst_base, &s);
                    for (int t = 0; t < T; ++t) dat::copy_chunk(t, chunk0, K, in, off.data(), &s, dst, dst_base);
                }
            }
        for (i64 i = 0; i < (K + 256) / 256 * 256; ++i) dat::store_off(i, K, off.data(), dst_base, off_out.data(), none_s.data(), none_out.data());
    }
    const std::vector<i64> b1{bad};
    wr(g, b1);
    wr(g, off_out);
    wr(g, none_out);
    fwrite(dst, 1, (size_t)dst_cap, g);
    free(dst);
    free(src);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    const i64 mode = rd<i64>(f, 1)[0];
    int rc = 0;
    if (mode == 0) {
        rc = gather(f, g);
    } else if (mode == 1) {
        const std::vector<i64> h = rd<i64>(f, 3);
        const i64 K = h[0], flags = h[1], data_bytes = h[2];
        std::vector<unsigned char> ok, out((size_t)K, 0xA5);
        std::vector<i64> off;
        if (flags & 1) ok = rd<unsigned char>(f, (size_t)K);
        if (flags & 2) off = rd<i64>(f, (size_t)K + 1);
        dat::u64 sum = 0;
        for (i64 i = 0; i < (K + 255) / 256 * 256; ++i)
            dat::fold_ok(i, K, flags & 1 ? ok.data() : nullptr, flags & 2 ? off.data() : nullptr, data_bytes, out.data(), &sum);
        wr(g, out);
        wr(g, std::vector<dat::u64>{sum});
    } else if (mode == 2) {
        const std::vector<i64> h = rd<i64>(f, 3);
        const i64 K = h[0], first_new = h[1], A = h[2];
        const std::vector<int> index_out = rd<int>(f, (size_t)K);
        std::vector<int> slot((size_t)A, dat::NO_SLOT);
        for (i64 i = 0; i < (K + 255) / 256 * 256; ++i) {
            const int r = dat::slot_of(i, K, index_out.data(), (int)first_new, A);
            if (r >= 0 && (int)i < slot[(size_t)r]) slot[(size_t)r] = (int)i;   // atomicMin
        }
        wr(g, slot);
    } else {
        rc = 2;
    }
    fclose(f);
    fclose(g);
    return rc;
}
