// Host emulation of the kernels of py-swirld_amd/csrc/wire.hip.h: the per-thread phases of the message writer (k_wire_lengths,
// pack.hip.h's scan, k_wire_write) and of the strict reader (k_wire_header, k_wire_table, k_wire_records, the scan, k_wire_data)
// are run thread by thread by one host thread, a barrier being the end of a phase.  Built with -fsanitize=address,undefined by
// tests/test_wire_kernels_host.py, which compares with tests/model_wire.py.  Every array has its exact size, the message read
// included, so the sanitizer sees every access outside; the message written carries a canary behind its end.
//
// usage: wire_emul W IN OUT
//   IN : int64 K, n, flags (1 data arrays, 2 data_none), data_bytes, grid, pre_len, cap; 32 B head, K x 32 B id, sp, op, K B arity,
//        K int32 creator, K x 8 B t, K x 64 B sig, n x 32 B keys, pre_len B prefix, [K + 1 int64 data_off, data_bytes B data, [K B none]]
//   OUT: int64 msg_len (-1: not buildable), int64 bad (the first unencodable event, -1: none), cap B (0xA5 where nothing was written)
// usage: wire_emul R IN OUT
//   IN : int64 msg_bytes, n, pre_len, cap_events, cap_data; n x 32 B keys, pre_len B prefix, msg_bytes B message
//   OUT: int64 rc (0, -34 SW_ERANGE), n_events, n_data; for rc 0 and n_events >= 0: 32 B head, K x 32 B id, sp, op, K B arity,
//        K int32 creator, K x 8 B t, K x 64 B sig, K + 1 int64 data_off, K B none, n_data B data
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define PCK_HOST_EMULATION
#define __device__
#define __forceinline__ inline
#include "../py-swirld_amd/csrc/wire.hip.h"

using pck::i64;
using pck::u64;

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
template <class T>
static void wr(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

// 16-byte aligned storage for 16-byte stores; the tail up to the next multiple of 16 belongs to the allocation, so the
// canary is what catches a store beyond the end
struct Bytes {
    unsigned char* p;
    size_t n;
    explicit Bytes(size_t bytes) : p((unsigned char*)aligned_alloc(16, (bytes + 16) / 16 * 16)), n(bytes) { memset(p, 0xA5, (bytes + 16) / 16 * 16); }
    ~Bytes() { free(p); }
};

static void scan(i64 K, i64* off) {     // k_pack_tile_sums, k_pack_scan_sums, k_pack_offsets on one stream
    const i64 tiles = (K + pck::TILE - 1) / pck::TILE;
    std::vector<i64> tsum((size_t)tiles), part(pck::SCAN_THREADS + 1);
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

static int writer(FILE* f, const char* out_path) {
    const std::vector<i64> h = rd<i64>(f, 7);
    const i64 K = h[0], n = h[1], flags = h[2], data_bytes = h[3], grid = h[4], pre_len = h[5], cap = h[6];
    const size_t k = (size_t)K;
    const std::vector<unsigned char> head = rd<unsigned char>(f, 32), id = rd<unsigned char>(f, k * 32), sp = rd<unsigned char>(f, k * 32),
                                     op = rd<unsigned char>(f, k * 32), arity = rd<unsigned char>(f, k);
    const std::vector<int> creator = rd<int>(f, k);
    const std::vector<u64> t = rd<u64>(f, k);
    const std::vector<unsigned char> sig = rd<unsigned char>(f, k * 64), keys = rd<unsigned char>(f, (size_t)n * 32), pre = rd<unsigned char>(f, (size_t)pre_len);
    std::vector<i64> data_off;
    std::vector<unsigned char> data, data_none;
    if (flags & 1) { data_off = rd<i64>(f, k + 1); data = rd<unsigned char>(f, (size_t)data_bytes); }
    if (flags & 2) data_none = rd<unsigned char>(f, k);
    fclose(f);
    const wir::WireIn w{pck::PackIn{sp.data(), op.data(), arity.data(), creator.data(), t.data(), sig.data(), flags & 1 ? data.data() : nullptr,
                                    flags & 1 ? data_off.data() : nullptr, data_bytes, flags & 2 ? data_none.data() : nullptr, keys.data(),
                                    pre.data(), (int)pre_len, (int)n},
                        id.data(), head.data()};
    std::vector<i64> off(k + 1, -7);
    u64 bad = wir::NO_BAD;
    const i64 blocks = (K + 255) / 256;
    for (i64 i = 0; i < blocks * 256; ++i) wir::lengths(i, K, w, off.data(), &bad);
    scan(K, off.data());
    const i64 base = wir::base_of(K, (int)pre_len);
    Bytes msg((size_t)cap);
    i64 msg_len = -7;
    // k_wire_write
    wir::write_len(K, off.data(), base, &bad, &msg_len);
    if (bad == wir::NO_BAD) {
        if (msg_len > cap) { fprintf(stderr, "length %lld beyond the capacity\n", (long long)msg_len); return 3; }
        const int T = wir::WRITE_THREADS;
        const i64 chunks = (cap + 15) / 16;
        const i64 trips = (chunks + grid * T - 1) / (grid * T);
        for (unsigned b = 0; b < (unsigned)grid; ++b)
            for (i64 trip = 0; trip < trips; ++trip) {
                const i64 chunk0 = wir::first_chunk(b, (unsigned)grid, trip);
                if (chunk0 * 16 >= msg_len) break;
                for (int tid = 0; tid < T; ++tid) wir::write_chunk(tid, chunk0, K, w, off.data(), base, msg.p);
            }
    }
    f = fopen(out_path, "wb");
    if (!f) return 2;
    const i64 res[2] = {msg_len, bad == wir::NO_BAD ? -1 : (i64)bad};
    fwrite(res, 8, 2, f);
    fwrite(msg.p, 1, msg.n, f);
    fclose(f);
    return 0;
}

static int reader(FILE* f, const char* out_path) {
    const std::vector<i64> h = rd<i64>(f, 5);
    const i64 msg_bytes = h[0], n = h[1], pre_len = h[2], cap_events = h[3], cap_data = h[4];
    const std::vector<unsigned char> keys = rd<unsigned char>(f, (size_t)n * 32), pre = rd<unsigned char>(f, (size_t)pre_len),
                                     msg = rd<unsigned char>(f, (size_t)msg_bytes);
    fclose(f);
    std::vector<unsigned char> skeys((size_t)n * 32);
    std::vector<int> sperm((size_t)n);
    wir::sort_keys(keys.data(), (int)n, skeys.data(), sperm.data());
    const wir::ReadIn in{msg.data(), msg_bytes, pre.data(), (int)pre_len, skeys.data(), sperm.data(), (int)n};
    i64 rc = 0, n_events = -1, n_data = 0;
    std::vector<unsigned char> head(32), id, sp, op, arity, sig, none, data;
    std::vector<int> creator;
    std::vector<u64> t;
    std::vector<i64> data_off;
    i64 res[4] = {-7, -7, -7, -7};
    if (msg_bytes >= pre_len + 8) {           // (the library's check in front of k_wire_header)
        int differ = 0;
        for (int tid = 0; tid < 256; ++tid) wir::header_cmp(tid, 256, in, &differ);
        for (int tid = 0; tid < 256; ++tid) wir::header_fin(tid, in, &differ, res);
    } else {
        res[0] = -1;
    }
    const i64 K = res[0];
    if (K > cap_events) {
        rc = -34;
        n_events = K;
        n_data = msg_bytes - wir::base_of(K, (int)pre_len) - 3 - K * wir::REC_MIN;
    } else if (K >= 0) {
        const size_t k = (size_t)K;
        id.resize(k * 32); sp.resize(k * 32); op.resize(k * 32); arity.resize(k); sig.resize(k * 64); none.resize(k); creator.resize(k); t.resize(k);
        data_off.assign(k + 1, -7);
        std::vector<i64> src(k);
        Bytes out((size_t)cap_data);
        const wir::ReadOut o{head.data(), id.data(), sp.data(), op.data(), arity.data(), creator.data(), t.data(), sig.data(), data_off.data(),
                             none.data(), src.data()};
        i64* flag = res + 1;
        for (i64 j = 0; j < (K + 256) / 256 * 256; ++j) wir::table(j, K, in, head.data(), flag);
        for (i64 i = 0; i < (K + 255) / 256 * 256; ++i) wir::record(i, K, in, o, flag);
        scan(K, data_off.data());
        wir::verdict(K, data_off.data(), flag, res + 2);
        for (i64 q = 0; q < (cap_data + 15) / 16; ++q) wir::data_chunk(q, K, msg.data(), o, cap_data, flag, out.p);
        n_events = res[2];
        n_data = res[3];
        if (n_events >= 0 && n_data > cap_data) rc = -34;
        for (size_t b = (size_t)(rc == 0 && n_events >= 0 ? n_data : 0); b < out.n; ++b)
            if (out.p[b] != 0xA5) { fprintf(stderr, "data byte %zu behind the end was written\n", b); return 4; }
        if (rc == 0 && n_events >= 0) data.assign(out.p, out.p + n_data);
    }
    f = fopen(out_path, "wb");
    if (!f) return 2;
    const i64 r3[3] = {rc, n_events, n_data};
    fwrite(r3, 8, 3, f);
    if (rc == 0 && n_events >= 0) {
        wr(f, head); wr(f, id); wr(f, sp); wr(f, op); wr(f, arity); wr(f, creator); wr(f, t); wr(f, sig); wr(f, data_off); wr(f, none); wr(f, data);
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    return argv[1][0] == 'W' ? writer(f, argv[3]) : reader(f, argv[3]);
}
