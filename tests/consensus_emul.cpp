// Host emulation of the kernels of py-swirld_amd/csrc/consensus.hip.h: k_consensus_record (two calls, one behind the other,
// as two find_order calls leave them), k_consensus_events and k_ordered_gather are run thread by thread by one host thread,
// workgroup by workgroup, with the guards and the grid-stride loops of the __global__ wrappers restated here.
// Built with -fsanitize=address,undefined by tests/test_consensus_kernels_host.py, which compares the arrays with numpy: an
// index outside a table, a read of the ordered-prefix row beyond the members, a misaligned 16-byte access shows up here
// without a GPU.  Every array has its exact size, so the sanitizer sees every overrun; the per-event tables start out
// filled with 0xA5, so a value read for an event nobody recorded shows up in the comparison.
//
// usage: consensus_emul IN OUT
//   IN : int32 header[15] = N, n, n_acc1, nr1, n_acc2, nr2, tx_total, ev_first, ev_K, ev_flags (1 rr, 2 time), ev_grid,
//        g_first, g_K, g_flags (1 event, 2 id, 4 creator, 8 rr, 16 time), g_grid;
//        per call: n_acc int32 acc_ev, n_acc int32 acc_ri, nr int32 rounds, n_acc x 8 B ts;
//        N int32 seq, N int32 cr, n int32 ordpos, tx_total int32 tx, N x 32 B ids
//   OUT: N int32 rr, N x 8 B cts (the tables); [ev_K int32] [ev_K x 8 B] of k_consensus_events;
//        [g_K int32 event] [g_K x 32 B id] [g_K int32 creator] [g_K int32 rr] [g_K x 8 B time] of k_ordered_gather
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CNS_HOST_EMULATION
#define __device__
#define __forceinline__ inline
#include "../py-swirld_amd/csrc/consensus.hip.h"

typedef unsigned long long u64;

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
    explicit Bytes(size_t bytes) : p(bytes ? (unsigned char*)aligned_alloc(16, bytes) : nullptr), n(bytes) {}
    ~Bytes() { free(p); }
};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int> h = rd<int>(f, 15);
    const int N = h[0], n = h[1], tx_total = h[6], ev_flags = h[9], ev_grid = h[10], g_flags = h[13], g_grid = h[14];
    const long long n_acc[2] = {h[2], h[4]}, ev_first = h[7], ev_K = h[8], g_first = h[11], g_K = h[12];
    const int nr[2] = {h[3], h[5]};
    std::vector<int> acc_ev[2], acc_ri[2], rounds[2];
    std::vector<u64> ts[2];
    for (int k = 0; k < 2; ++k) {
        acc_ev[k] = rd<int>(f, (size_t)n_acc[k]);
        acc_ri[k] = rd<int>(f, (size_t)n_acc[k]);
        rounds[k] = rd<int>(f, (size_t)nr[k]);
        ts[k] = rd<u64>(f, (size_t)n_acc[k]);
    }
    const std::vector<int> seq = rd<int>(f, N), cr = rd<int>(f, N), ordpos = rd<int>(f, n), tx = rd<int>(f, tx_total);
    const std::vector<unsigned char> ids_raw = rd<unsigned char>(f, (size_t)N * 32);
    fclose(f);
    Bytes ids((size_t)N * 32);
    if (N) memcpy(ids.p, ids_raw.data(), ids_raw.size());

    // k_consensus_record, call after call: one thread per slot, whole workgroups launched
    std::vector<int> rr((size_t)N, (int)0xA5A5A5A5);
    std::vector<u64> cts((size_t)N, 0xA5A5A5A5A5A5A5A5ull);
    for (int k = 0; k < 2; ++k) {
        const long long blocks = (n_acc[k] + cns::THREADS - 1) / cns::THREADS;
        for (long long b = 0; b < blocks; ++b)
            for (int t = 0; t < cns::THREADS; ++t) {
                const long long a = b * cns::THREADS + t;
                if (a < n_acc[k]) cns::record_slot(a, acc_ev[k].data(), acc_ri[k].data(), rounds[k].data(), ts[k].data(), rr.data(), cts.data());
            }
    }

    // k_consensus_events: grid-stride over [0, ev_K)
    std::vector<int> e_rr(ev_flags & 1 ? (size_t)ev_K : 0, -7);
    std::vector<u64> e_cts(ev_flags & 2 ? (size_t)ev_K : 0, 0x5A5A5A5A5A5A5A5Aull);
    for (int b = 0; b < ev_grid; ++b)
        for (int t = 0; t < cns::THREADS; ++t)
            for (long long i = (long long)b * cns::THREADS + t; i < ev_K; i += (long long)ev_grid * cns::THREADS)
                cns::events_one(i, ev_first, seq.data(), cr.data(), ordpos.data(), rr.data(), cts.data(),
                                ev_flags & 1 ? e_rr.data() : nullptr, ev_flags & 2 ? e_cts.data() : nullptr);

    // k_ordered_gather
    const size_t K = (size_t)g_K;
    std::vector<int> o_ev(g_flags & 1 ? K : 0, -7), o_cr(g_flags & 4 ? K : 0, -7), o_rr(g_flags & 8 ? K : 0, -7);
    std::vector<u64> o_t(g_flags & 16 ? K : 0, 0x5A5A5A5A5A5A5A5Aull);
    Bytes o_id(g_flags & 2 ? K * 32 : 0);
    if (o_id.n) memset(o_id.p, 0x5A, o_id.n);
    const cns::OrderedIn in{tx.data(), ids.p, cr.data(), rr.data(), cts.data()};
    const cns::OrderedOut out{g_flags & 1 ? o_ev.data() : nullptr, g_flags & 2 ? o_id.p : nullptr, g_flags & 4 ? o_cr.data() : nullptr,
                              g_flags & 8 ? o_rr.data() : nullptr, g_flags & 16 ? o_t.data() : nullptr};
    for (int b = 0; b < g_grid; ++b)
        for (int t = 0; t < cns::THREADS; ++t)
            cns::gather_positions<cns::GATHER_LANES>(t, cns::THREADS, (unsigned)b, (unsigned)g_grid, in, out, g_first, g_K);

    f = fopen(argv[2], "wb");
    if (!f) return 2;
    wr(f, rr); wr(f, cts); wr(f, e_rr); wr(f, e_cts);
    wr(f, o_ev);
    if (o_id.n) fwrite(o_id.p, 1, o_id.n, f);
    wr(f, o_cr); wr(f, o_rr); wr(f, o_t);
    fclose(f);
    return 0;
}
