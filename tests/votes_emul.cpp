// Host emulation of the kernels of py-swirld_amd/csrc/votes.hip.h: the per-thread phases of k_votes_prep, k_votes_lo,
// k_votes_rows (counting and writing), k_votes_scan and k_votes_values are run thread by thread, a barrier being the end of
// a phase, by one host thread — LDS as plain arrays, the grid workgroup by workgroup.  Built with
// -fsanitize=address,undefined by tests/test_votes_kernels_host.py, which compares the table with tests/model_votes.py: an
// index outside a table or a row behind the counted ones shows up here without a GPU.  Every array has its exact size, so
// the sanitizer sees every overrun.
//
// usage: votes_emul IN OUT
//   IN : int32 n, nw, R, N, coin_period, ncalls, rv0, rv1, unit;  then  int32 wit[R][np];  uint64 Sw[R][np][nw];
//        uint8 coin[N];  uint32 stake[np];  int32 dec_call[R][np], dec_by[R][np];  int32 round[N];
//        int32 (max_c, rounds)[ncalls];  int64 divided[ncalls];  int32 cons_call[R]            (np = 64 nw)
//   OUT: int64 n_rows, n_entries, levels;  int32 row_voter[n_rows], row_cand_round[n_rows];  uint64 exists[n_rows][nwo],
//        value[n_rows][nwo]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define VTS_HOST_EMULATION
#include "../py-swirld_amd/csrc/votes.hip.h"

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
template <class T>
static void wr(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

using vts::u64;

template <bool UNIT>
static void values(const vts::Tables& t, const vts::Range& g, const vts::Work& w, const vts::Out& out) {
    const int np = t.np;
    for (int blk = 0; blk < (g.rv1 - 1 - g.rc0) * t.nwo; ++blk) {
        const int rc = g.rc0 + blk / t.nwo, j = blk % t.nwo;
        std::vector<u64> s_T((size_t)64 * t.nw, 0xA5A5A5A5A5A5A5A5ull), s_W(np, 0xA5A5A5A5A5A5A5A5ull);
        std::vector<unsigned> s_stake(np, 0xA5A5A5A5u);
        int s_ctl[1] = {-1};
        for (int tid = 0; tid < np; ++tid) vts::val_begin(t, g, w, rc, j, tid, s_stake.data(), s_ctl);
        for (int d = 1; d <= s_ctl[0]; ++d) {
            for (int tid = 0; tid < np; ++tid)
                vts::val_store(t, g, w, out, rc, j, d, tid, vts::val_vote<UNIT>(t, rc, j, d, tid, s_T.data(), s_stake.data()), s_W.data());
            for (int tid = 0; tid < np; ++tid) vts::val_transpose(t, tid, s_W.data(), s_T.data());
        }
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int> h = rd<int>(f, 9);
    const int n = h[0], nw = h[1], R = h[2], N = h[3], coin_period = h[4], ncalls = h[5], unit = h[8];
    const int np = 64 * nw, nwo = (n + 63) / 64;
    if (n < 1 || n > np || R < 1 || h[6] < 0 || h[7] > R) return 2;
    const size_t slots = (size_t)R * np;
    const std::vector<int> wit = rd<int>(f, slots);
    const std::vector<u64> Sw = rd<u64>(f, slots * nw);
    const std::vector<unsigned char> coin = rd<unsigned char>(f, N);
    const std::vector<unsigned> stake = rd<unsigned>(f, np);
    const std::vector<int> dec_call = rd<int>(f, slots), dec_by = rd<int>(f, slots), round = rd<int>(f, N);
    const std::vector<int> call_pairs = rd<int>(f, (size_t)2 * ncalls);
    const std::vector<long long> call_div = rd<long long>(f, ncalls);
    const std::vector<int> cons_call = rd<int>(f, R);
    fclose(f);
    unsigned tot = 0;
    for (unsigned s : stake) tot += s;

    std::vector<int> o_voter, o_cand;
    std::vector<u64> o_ex, o_val;
    long long n_rows = 0, n_entries = 0, levels = 0;
    const int rv0 = std::max(h[6], 1), rv1 = h[7], nrv = rv1 - rv0;
    if (nrv > 0) {
        // the host's plan
        std::vector<vts::CallRec> recs(ncalls);
        std::vector<int> call_maxc(ncalls);
        for (int i = 0; i < ncalls; ++i) { recs[i] = vts::CallRec{call_pairs[2 * i], call_pairs[2 * i + 1], call_div[i]}; call_maxc[i] = recs[i].max_c; }
        std::vector<int> lo(nrv), c1v(nrv), cf(nrv);
        std::vector<long long> q(nrv + 1);
        const int rc0 = vts::plan_rounds(recs.data(), ncalls, cons_call.data(), rv0, rv1, lo.data(), c1v.data(), cf.data(), q.data());
        const vts::Tables t{wit.data(), Sw.data(), coin.data(), stake.data(), dec_call.data(), dec_by.data(), round.data(), N, n, np, nw, nwo, coin_period, 2u * tot};
        const vts::Sched s{call_maxc.data(), call_div.data(), cons_call.data(), ncalls};
        const vts::Range g{rv0, rv1, rc0, lo.data(), c1v.data(), cf.data(), q.data()};
        const size_t NR = (size_t)(rv1 - rc0), V = (size_t)nrv * np;
        std::vector<int> born(NR * np, 0x5A5A5A5A), rz(NR * np, 0x5A5A5A5A), order(NR * np, 0x5A5A5A5A), rank(NR * np, 0x5A5A5A5A), nwit(NR, 0x5A5A5A5A),
            hr(NR, 0x5A5A5A5A), hc(NR, 0x5A5A5A5A), lo_dev(nrv, 0x5A5A5A5A), vrows(V, 0x5A5A5A5A);
        std::vector<u64> rowmask((size_t)q[nrv] * nw, 0), counts(vts::C_WORDS, 0);
        std::vector<long long> vent(V, 0x5A5A5A5A), voff(V, 0x5A5A5A5A);
        const vts::Work w{born.data(), rz.data(), order.data(), rank.data(), nwit.data(), hr.data(), hc.data(), lo_dev.data(), rowmask.data(), vrows.data(),
                          vent.data(), voff.data(), counts.data()};
        // k_votes_prep: slot | barrier | rank
        for (int r = rc0; r < rv1; ++r) {
            for (int m = 0; m < np; ++m) vts::prep_slot(t, s, g, w, r, m);
            for (int m = 0; m < np; ++m) vts::prep_rank(t, g, w, r, m);
        }
        for (int i = 0; i < nrv; ++i) vts::lowest_round(g, w, i);
        // k_votes_rows<false>
        for (int i = 0; i < nrv; ++i)
            for (int k = 0; k < np; ++k) vts::voter_rows(t, s, g, w, nullptr, i, k);
        // k_votes_scan: sum | barrier | top | barrier | write
        std::vector<long long> s_rows(vts::SCAN_THREADS, 0x5A5A5A5A), s_ent(vts::SCAN_THREADS, 0x5A5A5A5A);
        for (int tid = 0; tid < vts::SCAN_THREADS; ++tid) vts::scan_sum(w, (long long)V, tid, s_rows.data(), s_ent.data());
        for (int tid = 0; tid < vts::SCAN_THREADS; ++tid) vts::scan_top(w, tid, s_rows.data(), s_ent.data());
        for (int tid = 0; tid < vts::SCAN_THREADS; ++tid) vts::scan_write(w, (long long)V, tid, s_rows.data());
        n_rows = (long long)counts[vts::C_ROWS];
        n_entries = (long long)counts[vts::C_ENTRIES];
        o_voter.assign(n_rows, -7);
        o_cand.assign(n_rows, -7);
        o_ex.assign((size_t)n_rows * nwo, 0xA5A5A5A5A5A5A5A5ull);
        o_val.assign((size_t)n_rows * nwo, 0xA5A5A5A5A5A5A5A5ull);
        const vts::Out out{o_voter.data(), o_cand.data(), o_ex.data(), o_val.data()};
        if (n_rows) {
            for (int i = 0; i < nrv; ++i)
                for (int k = 0; k < np; ++k) vts::voter_rows(t, s, g, w, &out, i, k);
            if (unit) values<true>(t, g, w, out);
            else values<false>(t, g, w, out);
        }
        levels = (long long)counts[vts::C_LEVELS];
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    const std::vector<long long> hdr{n_rows, n_entries, levels};
    wr(f, hdr);
    wr(f, o_voter);
    wr(f, o_cand);
    wr(f, o_ex);
    wr(f, o_val);
    fclose(f);
    return 0;
}
