// Host emulation of the payload kernels of py-swirld_amd/csrc/resolve.hip.h: every kernel without a barrier is run thread
// by thread, in launch order, by one host thread (atomics become plain operations), in the sequence payload_core of
// swirld_hip.hip launches them; the stable sort by wave, which the library does with the rank kernels of ingest.hip.h,
// is a std::stable_sort here.  Built with -fsanitize=address,undefined by tests/test_payload_kernels_host.py, which
// compares the answers with tests/model_payload.py: an index outside an array, or a probe loop that does not end, shows
// up here without a GPU.  A serial run sees one interleaving only; the waves are written so that the interleaving does
// not matter (k_pl_wave), and in-order execution is the one in which a thread sees the most of the running launch.
//
// usage: payload_emul IN OUT      IN: int32 n, N0, K; N0 x 32 B ids; N0 int32 creators; then the payload arrays
//                                 id, sp_id, op_id (K x 32 B each), arity (K B), ok (K B), creator (K int32)
//                                 OUT: int32 waves, accepted; K int32 index_out; accepted x (int32 cr, sp, op); accepted x 32 B ids
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define RSV_HOST_EMULATION
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
struct Dim { unsigned x = 1, y = 1, z = 1; };
static Dim threadIdx, blockIdx, blockDim, gridDim;
static inline int atomicCAS(int* p, int cmp, int v) { const int o = *p; if (o == cmp) *p = v; return o; }
static inline int atomicMin(int* p, int v) { const int o = *p; if (v < o) *p = v; return o; }
static inline int atomicAdd(int* p, int v) { const int o = *p; *p = o + v; return o; }
#define __hip_atomic_load(p, order, scope) (*(p))
#define __hip_atomic_store(p, v, order, scope) (*(p) = (v))
#include "../py-swirld_amd/csrc/resolve.hip.h"

template <class F>
static void launch(unsigned grid, unsigned block, F f) {
    gridDim.x = grid; blockDim.x = block;
    for (unsigned b = 0; b < grid; ++b)
        for (unsigned t = 0; t < block; ++t) { blockIdx.x = b; threadIdx.x = t; f(); }
}
static unsigned blocks(long long n) { return (unsigned)std::max<long long>(1, (n + 255) / 256); }

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int> hdr = rd<int>(f, 3);
    const int n = hdr[0], N0 = hdr[1], K = hdr[2];
    std::vector<unsigned char> cids = rd<unsigned char>(f, (size_t)N0 * 32);
    const std::vector<int> stored_cr = rd<int>(f, N0);
    const std::vector<unsigned char> id = rd<unsigned char>(f, (size_t)K * 32), spid = rd<unsigned char>(f, (size_t)K * 32),
                                     opid = rd<unsigned char>(f, (size_t)K * 32), arity = rd<unsigned char>(f, K), ok = rd<unsigned char>(f, K);
    const std::vector<int> creator = rd<int>(f, K);
    fclose(f);
    // the context's table over its N0 ids (exact sizes everywhere: the sanitizer sees every overrun)
    int clog = 10;
    while ((1ll << clog) < 2ll * (N0 + K)) ++clog;
    std::vector<int> cslots((size_t)1 << clog, -1);
    int dup = 0;
    launch(blocks(N0), 256, [&] { rsv::k_tab_insert(cslots.data(), clog, cids.data(), 0, N0, &dup); });
    if (dup) { fprintf(stderr, "stored ids: duplicate flag %d\n", dup); return 3; }
    // resolve
    int llog = 4;
    while ((1ll << llog) < 2ll * K) ++llog;
    std::vector<int> lslots((size_t)1 << llog, -1), out(K), wave(K), pr(2 * (size_t)K), la(K), lb(K), pend(K + 34, 0), acc(K + 34, 0);
    launch(blocks(K), 256, [&] { rsv::k_tab_insert(lslots.data(), llog, id.data(), 0, K, nullptr); });
    launch(blocks(K), 256, [&] {
        rsv::k_pl_local(cslots.data(), N0 ? clog : 0, cids.data(), lslots.data(), llog, id.data(), spid.data(), opid.data(), arity.data(),
                        creator.data(), ok.data(), K, n, out.data(), wave.data(), pr.data(), la.data(), &pend[0]);
    });
    // waves, 32 at a time like the library
    int* lst[2] = {la.data(), lb.data()};
    long long W = -1, A = 0;
    for (long long w0 = 0; W < 0; w0 += 32) {
        if (w0 > K + 1) { fprintf(stderr, "waves did not end\n"); return 3; }
        for (long long w = w0; w < w0 + 32; ++w)
            launch(std::min(blocks(K), 3u), 256, [&] {   // (a small grid: the grid-stride loop has to do the rest)
                rsv::k_pl_wave((int)w, lst[w & 1], &pend[w], lst[(w + 1) & 1], &pend[w + 1], &acc[w], pr.data(), creator.data(), stored_cr.data(),
                               wave.data(), out.data());
            });
        for (int j = 0; j < 32 && W < 0; ++j) {
            if (acc[w0 + j] == 0) W = w0 + j;
            else A += acc[w0 + j];
        }
    }
    launch(blocks(K), 256, [&] { rsv::k_pl_leftover(wave.data(), K, out.data()); });
    // dense order (the library: LSD passes of k_pl_keys + rank kernels + k_pl_scatter; here the definition)
    std::vector<int> ord;
    for (int i = 0; i < K; ++i) if (wave[i] >= 0) ord.push_back(i);
    if ((long long)ord.size() != A) { fprintf(stderr, "accepted %lld, waves hold %zu\n", A, ord.size()); return 3; }
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return wave[a] < wave[b]; });
    std::vector<int> rank_of(K, -1), g_cr(A), g_sp(A), g_op(A);
    std::vector<unsigned char> g_id((size_t)A * 32);
    launch(blocks(A), 256, [&] { rsv::k_pl_ranks(ord.data(), (int)A, N0, rank_of.data(), out.data()); });
    launch(blocks(A), 256, [&] {
        rsv::k_pl_gather(ord.data(), (int)A, N0, rank_of.data(), pr.data(), creator.data(), id.data(), nullptr, g_cr.data(), g_sp.data(), g_op.data(),
                         nullptr, g_id.data());
    });
    // commit: the new ids behind the stored ones, into the table
    cids.insert(cids.end(), g_id.begin(), g_id.end());
    launch(blocks(A), 256, [&] { rsv::k_tab_insert(cslots.data(), clog, cids.data(), N0, (int)A, &dup); });
    if (dup) { fprintf(stderr, "commit: duplicate flag %d\n", dup); return 3; }
    std::vector<int> back(N0 + A);
    launch(blocks(N0 + A), 256, [&] { rsv::k_tab_lookup(cslots.data(), clog, cids.data(), cids.data(), (int)(N0 + A), back.data()); });
    for (long long e = 0; e < N0 + A; ++e) if (back[e] != e) { fprintf(stderr, "lookup of event %lld gives %d\n", e, back[e]); return 3; }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    const int head[2] = {(int)W, (int)A};
    fwrite(head, sizeof(int), 2, f);
    fwrite(out.data(), sizeof(int), K, f);
    for (long long r = 0; r < A; ++r) { const int rec[3] = {g_cr[r], g_sp[r], g_op[r]}; fwrite(rec, sizeof(int), 3, f); }
    if (!g_id.empty()) fwrite(g_id.data(), 1, g_id.size(), f);
    fclose(f);
    return 0;
}
