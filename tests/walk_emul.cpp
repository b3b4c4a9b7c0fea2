// Host emulation of the kernels of py-swirld_amd/csrc/walk.hip.h: the per-thread phases of k_walk_bfs, k_walk_list,
// k_walk_gather and k_fork_trunks are run thread by thread, a barrier being the end of a phase, by one host thread — the
// walk with the workgroup size given on the command line (so that a level wider than the workgroup takes the stride loop),
// its LDS as plain arrays.  Built with -fsanitize=address,undefined by tests/test_walk_kernels_host.py, which compares the
// results with tests/model_walk.py: an index outside a table, a queue slot past the capacity, a misaligned 16-byte access
// shows up here without a GPU.  Every array has its exact size, so the sanitizer sees every overrun.
//
// usage: walk_emul IN OUT G THREADS     G = lanes per slot (4, 8 or 16), THREADS = workgroup size of the walk
//   IN : int32 n, N, head, flags (1 t, 2 sig, 4 event, 8 known given, 16 cap given), grid; n int32 known, cap;
//        N int32 sp, op, cr, ht; N x 32 B ids; N x 8 B t; N x 64 B sig
//   OUT: 8 int32 header; int32 levels run, then that many int32 level widths; count int32 list; then count x 32 B id, sp_id,
//        op_id; count B arity; count int32 creator; [count x 8 B t] [count x 64 B sig] [count int32 event]; n int32 trunk
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define GSP_HOST_EMULATION
#define __device__
#define __forceinline__ inline
#include "../py-swirld_amd/csrc/walk.hip.h"

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
static void gather(unsigned grid, const gsp::ExportIn& in, const gsp::ExportOut& out, const int* list, const int* cr, int total) {
    for (unsigned b = 0; b < grid; ++b)
        for (int t = 0; t < wlk::GATHER_THREADS; ++t) wlk::walk_slots<G>(t, wlk::GATHER_THREADS, b, grid, in, out, list, cr, total);
}

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const int G = atoi(argv[3]), threads = atoi(argv[4]);
    if (threads < 1 || threads > wlk::MAX_THREADS) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int> h = rd<int>(f, 5);
    const int n = h[0], N = h[1], head = h[2], flags = h[3], grid = h[4];
    if (head < 0 || head >= N) return 2;
    const std::vector<int> known = rd<int>(f, n), cap = rd<int>(f, n);
    const std::vector<int> sp = rd<int>(f, N), op = rd<int>(f, N), cr = rd<int>(f, N), ht = rd<int>(f, N);
    Bytes ids((size_t)N * 32), sig((size_t)N * 64);
    const std::vector<unsigned char> ids_raw = rd<unsigned char>(f, (size_t)N * 32);
    const std::vector<unsigned long long> t = rd<unsigned long long>(f, N);
    const std::vector<unsigned char> sig_raw = rd<unsigned char>(f, (size_t)N * 64);
    fclose(f);
    memcpy(ids.p, ids_raw.data(), ids_raw.size());
    memcpy(sig.p, sig_raw.data(), sig_raw.size());

    // k_walk_bfs: stage | barrier | { expand | barrier } per level | finish
    const wlk::WalkIn in{sp.data(), op.data(), cr.data(), ht.data(), n, head};
    std::vector<int> s_known((size_t)n, 0x5A5A5A5A), s_ctl(wlk::C_WORDS, 0x5A5A5A5A), hdr(wlk::H_WORDS, 0), queue((size_t)head + 1, -7), widths;
    std::vector<unsigned> bits(((size_t)head + 32) / 32, 0u);
    for (int tid = 0; tid < threads; ++tid)
        wlk::walk_stage(tid, threads, in, flags & 8 ? known.data() : nullptr, flags & 16 ? cap.data() : nullptr, s_known.data(), s_ctl.data(), bits.data(), queue.data());
    int begin = 0, end = 1, lvl = 0;
    const int max_levels = head + 2;
    while (begin < end && lvl < max_levels) {
        for (int tid = 0; tid < threads; ++tid) wlk::walk_expand(tid, threads, in, lvl, begin, end, s_known.data(), s_ctl.data(), bits.data(), queue.data());
        const int added = s_ctl[wlk::C_CNT + lvl % 3];
        if ((unsigned)added >= (unsigned)wlk::STOP) break;
        widths.push_back(end - begin);
        begin = end;
        end += added;
        ++lvl;
    }
    for (int tid = 0; tid < threads; ++tid) wlk::walk_finish(tid, end, lvl, begin < end, s_ctl.data(), hdr.data());
    const int count = hdr[wlk::H_COUNT];
    if (hdr[wlk::H_ERR] || count < 1 || count > head + 1) { fprintf(stderr, "walk: error %d, count %d\n", hdr[wlk::H_ERR], count); return 3; }

    // k_walk_list: count | barrier | scan | barrier | write
    std::vector<int> part(wlk::LIST_THREADS, 0x5A5A5A5A), list((size_t)count, -7);
    for (int tid = 0; tid < wlk::LIST_THREADS; ++tid) wlk::list_count(tid, bits.data(), head, hdr.data(), part.data());
    for (int tid = 0; tid < wlk::LIST_THREADS; ++tid) wlk::list_scan(tid, part.data(), hdr.data());
    for (int tid = 0; tid < wlk::LIST_THREADS; ++tid) wlk::list_write(tid, bits.data(), head, hdr.data(), part.data(), list.data());
    if (hdr[wlk::H_ERR]) { fprintf(stderr, "list: error %d, listed %d of %d\n", hdr[wlk::H_ERR], hdr[wlk::H_LISTED], count); return 3; }

    // k_walk_gather
    const size_t K = (size_t)count;
    Bytes o_id(K * 32), o_sp(K * 32), o_op(K * 32), o_sig(flags & 2 ? K * 64 : 0);
    std::vector<unsigned char> o_ar(K, 0xA5);
    std::vector<int> o_cr(K, -7), o_ev(flags & 4 ? K : 0, -7);
    std::vector<unsigned long long> o_t(flags & 1 ? K : 0, 0xA5A5A5A5A5A5A5A5ull);
    memset(o_id.p, 0xA5, K * 32); memset(o_sp.p, 0xA5, K * 32); memset(o_op.p, 0xA5, K * 32);
    if (o_sig.n) memset(o_sig.p, 0xA5, o_sig.n);
    const gsp::ExportIn gin{nullptr, nullptr, nullptr, sp.data(), op.data(), ids.p, sig.p, t.data()};
    const gsp::ExportOut gout{o_id.p, o_sp.p, o_op.p, o_ar.data(), o_cr.data(), flags & 1 ? o_t.data() : nullptr, flags & 2 ? o_sig.p : nullptr,
                              flags & 4 ? o_ev.data() : nullptr};
    if (G == 4) gather<4>((unsigned)grid, gin, gout, list.data(), cr.data(), count);
    else if (G == 8) gather<8>((unsigned)grid, gin, gout, list.data(), cr.data(), count);
    else if (G == 16) gather<16>((unsigned)grid, gin, gout, list.data(), cr.data(), count);
    else return 2;

    // k_fork_trunks: the events in the order a grid of `grid` workgroups takes them, workgroup by workgroup
    std::vector<int> children((size_t)N, 0), roots((size_t)n, 0), trunk((size_t)n, wlk::NO_CAP);
    for (int b = 0; b < grid; ++b)
        for (int tid = 0; tid < wlk::TRUNK_THREADS; ++tid)
            for (long long e = (long long)b * wlk::TRUNK_THREADS + tid; e < N; e += (long long)grid * wlk::TRUNK_THREADS)
                wlk::fork_event(e, sp.data(), cr.data(), ht.data(), n, N, children.data(), roots.data(), trunk.data());

    f = fopen(argv[2], "wb");
    if (!f) return 2;
    wr(f, hdr);
    const int nl = (int)widths.size();
    fwrite(&nl, sizeof nl, 1, f);
    wr(f, widths);
    wr(f, list);
    fwrite(o_id.p, 1, K * 32, f); fwrite(o_sp.p, 1, K * 32, f); fwrite(o_op.p, 1, K * 32, f);
    wr(f, o_ar);
    wr(f, o_cr);
    wr(f, o_t);
    if (o_sig.n) fwrite(o_sig.p, 1, o_sig.n, f);
    wr(f, o_ev);
    wr(f, trunk);
    fclose(f);
    return 0;
}
