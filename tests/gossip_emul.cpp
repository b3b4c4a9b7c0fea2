// Host emulation of the export kernels of py-swirld_amd/csrc/gossip.hip.h: the per-thread phases of k_export_offsets and
// k_export_gather are run thread by thread, a barrier being the end of a phase, by one host thread — the offsets in their
// sequential form (one lane after the other), the gather workgroup by workgroup with its LDS tables as plain arrays.
// Built with -fsanitize=address,undefined by tests/test_gossip_kernels_host.py, which compares the arrays with
// tests/model_gossip.py: an index outside a table, a misaligned 16-byte access or a search that leaves its range shows up
// here without a GPU.  Every array has its exact size, so the sanitizer sees every overrun.
//
// usage: gossip_emul IN OUT G     G = lanes per slot (4, 8 or 16)
//   IN : int32 n, N, pool, flags (1 t, 2 sig, 4 event), grid; n int32 pos_first, pos_end, chain_start; pool int32 chain_ev;
//        N int32 sp, op; N x 32 B ids; N x 8 B t; N x 64 B sig
//   OUT: int64 total; n + 1 int32 off; then total x 32 B id, sp_id, op_id; total B arity; total int32 creator;
//        [total x 8 B t] [total x 64 B sig] [total int32 event]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define GSP_HOST_EMULATION
#define __device__
#define __forceinline__ inline
#include "../py-swirld_amd/csrc/gossip.hip.h"

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
template <class T>
static void wr(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

// 16-byte aligned storage of exactly `bytes` bytes (every size here is a multiple of 32)
struct Bytes {
    unsigned char* p;
    size_t n;
    explicit Bytes(size_t bytes) : p(bytes ? (unsigned char*)aligned_alloc(16, (bytes + 15) / 16 * 16) : nullptr), n(bytes) {}
    ~Bytes() { free(p); }
};

template <int G>
static void gather(unsigned grid, const gsp::ExportIn& in, const gsp::ExportOut& out, int n, int total) {
    for (unsigned b = 0; b < grid; ++b) {
        std::vector<int> s_off((size_t)n + 1), s_base((size_t)n);
        for (int t = 0; t < gsp::GATHER_THREADS; ++t) gsp::gather_stage(t, gsp::GATHER_THREADS, in, n, s_off.data(), s_base.data());
        for (int t = 0; t < gsp::GATHER_THREADS; ++t)
            gsp::gather_slots<G>(t, gsp::GATHER_THREADS, b, grid, in, out, n, total, s_off.data(), s_base.data());
    }
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int G = atoi(argv[3]);
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int> hdr = rd<int>(f, 5);
    const int n = hdr[0], N = hdr[1], pool = hdr[2], flags = hdr[3], grid = hdr[4];
    const std::vector<int> pos_first = rd<int>(f, n), pos_end = rd<int>(f, n), chain_start = rd<int>(f, n), chain_ev = rd<int>(f, pool);
    const std::vector<int> sp = rd<int>(f, N), op = rd<int>(f, N);
    Bytes ids((size_t)N * 32), sig((size_t)N * 64);
    const std::vector<unsigned char> ids_raw = rd<unsigned char>(f, (size_t)N * 32);
    const std::vector<unsigned long long> t = rd<unsigned long long>(f, N);
    const std::vector<unsigned char> sig_raw = rd<unsigned char>(f, (size_t)N * 64);
    fclose(f);
    if (N) { memcpy(ids.p, ids_raw.data(), ids_raw.size()); memcpy(sig.p, sig_raw.data(), sig_raw.size()); }
    // k_export_offsets: sum | barrier | scan | barrier | write
    std::vector<int> part(gsp::SCAN_THREADS), off((size_t)n + 1, -1), base((size_t)n, -1);
    long long total = -1;
    for (int l = 0; l < gsp::SCAN_THREADS; ++l) gsp::offsets_sum(l, pos_first.data(), pos_end.data(), n, part.data());
    for (int l = 0; l < gsp::SCAN_THREADS; ++l) gsp::offsets_scan(l, n, part.data(), off.data(), &total);
    for (int l = 0; l < gsp::SCAN_THREADS; ++l) gsp::offsets_write(l, pos_first.data(), pos_end.data(), chain_start.data(), n, part.data(), off.data(), base.data());
    if (total < 0 || total > N) { fprintf(stderr, "total %lld\n", total); return 3; }
    // k_export_gather
    const size_t K = (size_t)total;
    Bytes o_id(K * 32), o_sp(K * 32), o_op(K * 32), o_sig(flags & 2 ? K * 64 : 0);
    std::vector<unsigned char> o_ar(K, 0xA5);
    std::vector<int> o_cr(K, -7), o_ev(flags & 4 ? K : 0, -7);
    std::vector<unsigned long long> o_t(flags & 1 ? K : 0, 0xA5A5A5A5A5A5A5A5ull);
    if (K) { memset(o_id.p, 0xA5, K * 32); memset(o_sp.p, 0xA5, K * 32); memset(o_op.p, 0xA5, K * 32); }
    if (o_sig.n) memset(o_sig.p, 0xA5, o_sig.n);
    const gsp::ExportIn in{off.data(), base.data(), chain_ev.data(), sp.data(), op.data(), ids.p, sig.p, t.data()};
    const gsp::ExportOut out{o_id.p, o_sp.p, o_op.p, o_ar.data(), o_cr.data(), flags & 1 ? o_t.data() : nullptr, flags & 2 ? o_sig.p : nullptr,
                             flags & 4 ? o_ev.data() : nullptr};
    if (G == 4) gather<4>((unsigned)grid, in, out, n, (int)total);
    else if (G == 8) gather<8>((unsigned)grid, in, out, n, (int)total);
    else if (G == 16) gather<16>((unsigned)grid, in, out, n, (int)total);
    else return 2;
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(&total, sizeof total, 1, f);
    wr(f, off);
    if (K) { fwrite(o_id.p, 1, K * 32, f); fwrite(o_sp.p, 1, K * 32, f); fwrite(o_op.p, 1, K * 32, f); }
    wr(f, o_ar);
    wr(f, o_cr);
    wr(f, o_t);
    if (o_sig.n) fwrite(o_sig.p, 1, o_sig.n, f);
    wr(f, o_ev);
    fclose(f);
    return 0;
}
