// Host emulation of the kernels of py-swirld_amd/csrc/pack.hip.h: the per-thread phases of k_pack_lengths, the three scan
// kernels and k_pack_write are run thread by thread, a barrier being the end of a phase, by one host thread — workgroup by
// workgroup, the LDS of each as a plain object.  Built with -fsanitize=address,undefined by
// tests/test_pack_kernels_host.py, which compares offsets, flags and both streams with tests/model_pack.py: an index outside
// an array, a misaligned dword or 16-byte access, or a search that leaves its range shows up here without a GPU.  Every
// input array has its exact size, so the sanitizer sees every overrun; the two output streams carry a canary behind off[K].
//
// usage: pack_emul IN OUT
//   IN : int64 K, n, flags (1 data arrays, 2 data_none), data_bytes, grid, hdr_len, msg_cap, whole_cap;
//        K x 32 B sp, K x 32 B op, K B arity, K int32 creator, K x 8 B t, K x 64 B sig, n x 32 B keys, hdr_len B header,
//        [K + 1 int64 data_off, data_bytes B data, [K B data_none]]
//   OUT: K + 1 int64 msg_off, K + 1 int64 whole_off, K B flags, msg_cap B, whole_cap B (0xA5 where nothing was written)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define PCK_HOST_EMULATION
#define __device__
#define __forceinline__ inline
#include "../py-swirld_amd/csrc/pack.hip.h"

using pck::i64;

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
template <class T>
static void wr(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

// 16-byte aligned storage; the tail up to the next multiple of 16 belongs to the allocation, so the canary is what
// catches a store beyond off[K]
struct Bytes {
    unsigned char* p;
    size_t n;
    explicit Bytes(size_t bytes) : p((unsigned char*)aligned_alloc(16, (bytes + 16) / 16 * 16)), n(bytes) { memset(p, 0xA5, (bytes + 16) / 16 * 16); }
    ~Bytes() { free(p); }
};

static void scan(i64 K, i64* off) {
    const i64 tiles = (K + pck::TILE - 1) / pck::TILE;
    std::vector<i64> tsum((size_t)tiles), part(pck::SCAN_THREADS + 1);
    const int T = pck::SCAN_THREADS;
    for (i64 b = 0; b < tiles; ++b) {   // k_pack_tile_sums
        for (int l = 0; l < T; ++l) pck::tile_sum(l, b, K, off, part.data());
        for (int l = 0; l < T; ++l) pck::tile_total(l, b, part.data(), tsum.data());
    }
    const i64 passes = (tiles + T - 1) / T;   // k_pack_scan_sums
    if (passes == 0) off[K] = 0;
    for (i64 p = 0; p < passes; ++p) {
        for (int l = 0; l < T; ++l) pck::sums_load(l, p, tiles, tsum.data(), part.data());
        for (int l = 0; l < T; ++l) pck::sums_scan(l, p, part.data());
        for (int l = 0; l < T; ++l) pck::sums_store(l, p, tiles, K, part.data(), tsum.data(), off);
    }
    for (i64 b = 0; b < tiles; ++b) {   // k_pack_offsets
        for (int l = 0; l < T; ++l) pck::tile_sum(l, b, K, off, part.data());
        for (int l = 0; l < T; ++l) pck::offsets_scan(l, b, part.data(), tsum.data());
        for (int l = 0; l < T; ++l) pck::offsets_write(l, b, K, part.data(), off);
    }
}

template <bool WHOLE>
static void write(unsigned grid, i64 cap, const pck::PackIn& in, i64 K, const i64* off, unsigned char* out) {
    const int T = pck::WRITE_THREADS;
    const i64 chunks = (cap + 15) / 16;
    const i64 trips = (chunks + (i64)grid * T - 1) / ((i64)grid * T);
    for (unsigned b = 0; b < grid; ++b) {
        pck::Tile s;
        memset(&s, 0xEE, sizeof s);
        if (WHOLE) for (int t = 0; t < T; ++t) pck::write_hdr(t, in, &s);
        for (i64 trip = 0; trip < trips; ++trip) {
            const i64 chunk0 = pck::first_chunk(b, grid, trip);
            if (chunk0 * 16 >= off[K]) break;
            for (int t = 0; t < T; ++t) pck::write_stage(t, chunk0, K, off, &s);
            for (int t = 0; t < T; ++t) pck::write_chunk<WHOLE>(t, chunk0, K, in, off, &s, out);
        }
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<i64> h = rd<i64>(f, 8);
    const i64 K = h[0], n = h[1], flags = h[2], data_bytes = h[3], grid = h[4], hdr_len = h[5], msg_cap = h[6], whole_cap = h[7];
    const size_t k = (size_t)K;
    const std::vector<unsigned char> sp = rd<unsigned char>(f, k * 32), op = rd<unsigned char>(f, k * 32), arity = rd<unsigned char>(f, k);
    const std::vector<int> creator = rd<int>(f, k);
    const std::vector<pck::u64> t = rd<pck::u64>(f, k);
    const std::vector<unsigned char> sig = rd<unsigned char>(f, k * 64), keys = rd<unsigned char>(f, (size_t)n * 32), hdr = rd<unsigned char>(f, (size_t)hdr_len);
    std::vector<i64> data_off;
    std::vector<unsigned char> data, data_none;
    if (flags & 1) { data_off = rd<i64>(f, k + 1); data = rd<unsigned char>(f, (size_t)data_bytes); }
    if (flags & 2) data_none = rd<unsigned char>(f, k);
    fclose(f);
    const pck::PackIn in{sp.data(), op.data(), arity.data(), creator.data(), t.data(), sig.data(), flags & 1 ? data.data() : nullptr,
                         flags & 1 ? data_off.data() : nullptr, data_bytes, flags & 2 ? data_none.data() : nullptr, keys.data(), hdr.data(),
                         (int)hdr_len, (int)n};
    std::vector<i64> msg_off(k + 1, -7), whole_off(k + 1, -7);
    std::vector<unsigned char> enc(k, 0xA5);
    const i64 blocks = (K + 255) / 256;   // k_pack_lengths
    for (i64 i = 0; i < blocks * 256; ++i) pck::lengths(i, K, in, msg_off.data(), whole_off.data(), enc.data());
    scan(K, msg_off.data());
    scan(K, whole_off.data());
    if (msg_off[k] > msg_cap || whole_off[k] > whole_cap) { fprintf(stderr, "totals %lld / %lld beyond the capacities\n", msg_off[k], whole_off[k]); return 3; }
    Bytes msgs((size_t)msg_cap), whole((size_t)whole_cap);
    write<false>((unsigned)grid, msg_cap, in, K, msg_off.data(), msgs.p);
    write<true>((unsigned)grid, whole_cap, in, K, whole_off.data(), whole.p);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    wr(f, msg_off);
    wr(f, whole_off);
    wr(f, enc);
    fwrite(msgs.p, 1, msgs.n, f);
    fwrite(whole.p, 1, whole.n, f);
    fclose(f);
    return 0;
}
