// Stand-alone host program (its own main; built with -fsanitize=address,undefined by tests/test_batch_network_host.py) around
// csrc/batch_network.hip.h: it runs swbn::begin and swbn::turns — the very functions k_batch_network_begin and
// k_batch_network_turns run, one lane — for ONE network whose views' slab segments are separate allocations of exactly their
// size (no rounding up to 64 bytes: an access one element beyond a column is an error here), and whose network state is an
// allocation of exactly swbn::Layout::total bytes.  TEST INFRASTRUCTURE: the product never builds this file.
//
//   batch_network_main CASE OUT
// CASE: int64 {n, coin_period, cap_events, seed, T, drawn, given, chunk}, uint64 stake[n], then with drawn = 0: int32
// puller[T], peer[T]; with given = 1 also double t[T], uint8 sig[T][64], double root_t[n], uint8 root_sig[n][64].
// The T turns run in calls of `chunk` turns (0: one call), as sw_network_batch_turns / _run split a long call.
// OUT: int64 {begun, turns, created, imported, stage, code, view}, then per view int64 {events, head, hmax, summary[8]} and
// the columns creator, self_parent, other_parent, height, round, number (int32), t (double), sig, tbd, fam_ev (bytes),
// can_see (int32 [events][n]) and the log: event, round received (int32), consensus time (double).
#define SW_EXACT_HOST 1
#include "../py-swirld_amd/csrc/batch_network.hip.h"

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <vector>

// Built with -DSW_EXACT_HOST_LANES=16 (and without the sanitizers, which do not follow swapcontext) the same program runs
// the turns as 16 cooperative fibers that hand over at every sync(), the scheme of tests/batch_host.cpp: each lane runs
// alone to its next sync, the opposite extreme of a wavefront's lockstep, so equal results need nothing but the syncs.
#ifdef SW_EXACT_HOST_LANES
#include <ucontext.h>
namespace emul {
constexpr int NL = SW_EXACT_HOST_LANES;
ucontext_t main_ctx, ctx[NL];
std::vector<char> stacks;
bool done[NL];
int cur = 0, syncs[NL];
unsigned long long slot[NL];
const std::function<void()>* body = nullptr;
void entry() { (*body)(); done[cur] = true; swapcontext(&ctx[cur], &main_ctx); }
void run(const std::function<void()>& f) {
    body = &f;
    if (stacks.empty()) stacks.resize((size_t)NL * (256 << 10));
    for (int i = 0; i < NL; ++i) {
        getcontext(&ctx[i]);
        ctx[i].uc_stack.ss_sp = stacks.data() + (size_t)i * (256 << 10);
        ctx[i].uc_stack.ss_size = 256 << 10;
        ctx[i].uc_link = &main_ctx;
        makecontext(&ctx[i], entry, 0);
        done[i] = false; syncs[i] = 0;
    }
    for (;;) {
        int live = 0;
        for (int i = 0; i < NL; ++i) {
            if (done[i]) continue;
            cur = i;
            swapcontext(&main_ctx, &ctx[i]);
            live += !done[i];
        }
        if (!live) break;
        for (int i = 0; i < NL; ++i)
            if (done[i] != done[0] || syncs[i] != syncs[0]) { fprintf(stderr, "lanes disagree on the number of syncs (lane %d)\n", i); abort(); }
    }
}
}  // namespace emul
extern "C" int swx_emul_lane() { return emul::cur; }
extern "C" void swx_emul_sync() { emul::syncs[emul::cur]++; swapcontext(&emul::ctx[emul::cur], &emul::main_ctx); }
extern "C" unsigned long long swx_emul_sum(unsigned long long v) {
    emul::slot[emul::cur] = v;
    swx_emul_sync();
    unsigned long long t = 0;
    for (int i = 0; i < emul::NL; ++i) t += emul::slot[i];
    swx_emul_sync();
    return t;
}
static void run(const std::function<void()>& f) { emul::run(f); }
#else
static void run(const std::function<void()>& f) { f(); }
#endif

namespace {

std::vector<std::unique_ptr<unsigned char[]>> g_blocks;

template <class T>
T* exact(size_t count) {
    const size_t bytes = count * sizeof(T);
    g_blocks.emplace_back(new unsigned char[bytes > 0 ? bytes : 1]);
    memset(g_blocks.back().get(), 0x5a, bytes);   // (garbage: whatever is read was initialised by the code under test)
    return (T*)g_blocks.back().get();
}

// swb::bind over separate allocations: the element counts of batch_layout.h's make(), not rounded
swb::Rec make_rec(int n, int np, long long E, long long R, int coin_period, const uint64_t* stake) {
    swb::Rec r{};
    swx::State& s = r.s;
    uint64_t tot = 0;
    uint32_t* st = exact<uint32_t>((size_t)np);
    for (int i = 0; i < np; ++i) { st[i] = i < n ? (uint32_t)stake[i] : 0; tot += st[i]; }
    s.n = n; s.npad = np; s.coin_period = coin_period; s.tot = tot; s.stake = st;
    s.cr = exact<int>(E); s.sp = exact<int>(E); s.op = exact<int>(E); s.ht = exact<int>(E);
    s.t = exact<double>(E); s.sig = exact<unsigned char>(E * 64);
    s.round = exact<int>(E); s.L = exact<int>(E * np); s.tbd = exact<unsigned char>(E); s.fam_ev = exact<signed char>(E);
    s.Rcap = (int)R;
    s.wit = exact<int>(R * np); s.worder = exact<int>(R * np); s.wcnt = exact<int>(R); s.cons = exact<unsigned char>(R);
    s.fam_slot = exact<signed char>(R * np); s.hdr = exact<long long>(swx::H_WORDS);
    r.fx.votes = exact<signed char>((size_t)2 * n * n * R); r.fx.win = 1; r.fx.layer = (size_t)n * n;
    r.fx.s_m = exact<unsigned char>(np); r.fx.done = exact<unsigned char>(R); r.fx.new_rounds = exact<int>(R);
    swx::OrderScratch& o = r.ox;
    o.queue = exact<int>(E + 1); o.visited = exact<unsigned char>(E + 1); o.fw = exact<int>(np);
    o.sflag = exact<unsigned char>(np); o.times = exact<double>(np); o.tsort = exact<double>(np);
    o.white = exact<unsigned char>(64); o.items_ev = exact<int>(E + 1); o.items_ts = exact<double>(E + 1); o.items_rr = exact<int>(E + 1);
    r.log_ev = exact<int>(E); r.log_rr = exact<int>(E); r.log_ts = exact<double>(E);
    r.sum = exact<long long>(swb_layout::SUMMARY_WORDS);
    r.cap_events = E;
    run([&] { swb::init_slab(r, st); });
    return r;
}

template <class T>
bool get(FILE* f, T* p, size_t count) { return fread(p, sizeof(T), count, f) == count; }
template <class T>
void put(FILE* f, const T* p, size_t count) { if (fwrite(p, sizeof(T), count, f) != count) { perror("write"); exit(2); } }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s CASE OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    long long hd[8];
    if (!f || !get(f, hd, 8)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const int n = (int)hd[0], coin_period = (int)hd[1];
    const long long E = hd[2], T = hd[4], chunk = hd[7] > 0 ? hd[7] : (T > 0 ? T : 1);
    const uint64_t seed = (uint64_t)hd[3];
    const bool drawn = hd[5] != 0, given = hd[6] != 0;
    std::vector<uint64_t> stake((size_t)n);
    std::vector<int> puller((size_t)T), peer((size_t)T);
    std::vector<double> t((size_t)T), root_t((size_t)n);
    std::vector<unsigned char> sig((size_t)T * 64), root_sig((size_t)n * 64);
    bool ok = get(f, stake.data(), (size_t)n);
    if (!drawn) ok = ok && get(f, puller.data(), (size_t)T) && get(f, peer.data(), (size_t)T);
    if (given) ok = ok && get(f, t.data(), (size_t)T) && get(f, sig.data(), (size_t)T * 64) && get(f, root_t.data(), (size_t)n) && get(f, root_sig.data(), (size_t)n * 64);
    fclose(f);
    if (!ok || n < 2) { fprintf(stderr, "short case file\n"); return 2; }

    const int np = swb_layout::npad_of(n);
    const long long R = E + 3;
    std::vector<swb::Rec> recs;
    for (int i = 0; i < n; ++i) recs.push_back(make_rec(n, np, E, R, coin_period, stake.data()));
    const swbn::Layout nl = swbn::layout((uint64_t)n, (uint64_t)n, (uint64_t)E);
    unsigned char* st = exact<unsigned char>((size_t)nl.total);
    memset(st, 0, (size_t)nl.cols);

    run([&] { swbn::begin(recs.data(), st, nl, 0, seed, given ? root_t.data() : nullptr, given ? root_sig.data() : nullptr); });
    for (long long a = 0; a < T; a += chunk) {
        const long long k = T - a < chunk ? T - a : chunk;
        run([&] {
            swbn::turns(recs.data(), st, nl, 0, k, drawn ? nullptr : puller.data() + a, drawn ? nullptr : peer.data() + a, given ? t.data() + a : nullptr,
                        given ? sig.data() + (size_t)a * 64 : nullptr);
        });
    }

    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const swbn::Net* net = nl.net(st, 0);
    const long long nw[7] = {net->begun, net->turns, net->created, net->imported, net->stage, net->code, net->view};
    put(o, nw, 7);
    for (int i = 0; i < n; ++i) {
        const swb::Rec& r = recs[(size_t)i];
        const swbn::View* v = nl.view(st, (uint64_t)i);
        const size_t N = (size_t)v->events;
        for (long long e = 0; e <= E; ++e)
            if (r.ox.visited[e]) { fprintf(stderr, "view %d: the BFS map is not all zero behind the turns (entry %lld)\n", i, e); return 1; }
        long long w[3 + swb_layout::SUMMARY_WORDS] = {(long long)N, v->head, v->hmax};
        memcpy(w + 3, r.sum, sizeof(long long) * swb_layout::SUMMARY_WORDS);
        put(o, w, 3 + swb_layout::SUMMARY_WORDS);
        put(o, r.s.cr, N); put(o, r.s.sp, N); put(o, r.s.op, N); put(o, r.s.ht, N); put(o, r.s.round, N); put(o, nl.number(st, (uint64_t)i), N);
        put(o, r.s.t, N); put(o, r.s.sig, N * 64); put(o, r.s.tbd, N); put(o, r.s.fam_ev, N);
        for (size_t e = 0; e < (size_t)r.sum[swb::S_DIVIDED]; ++e) put(o, r.s.L + e * np, (size_t)n);
        const size_t m = (size_t)r.sum[swb::S_ORDERED];
        put(o, r.log_ev, m); put(o, r.log_rr, m); put(o, r.log_ts, m);
    }
    fclose(o);
    g_blocks.clear();
    printf("ok %lld %lld\n", nw[1], nw[2]);
    return 0;
}
