// Host build of batch.hip.h (g++ -DSW_EXACT_HOST) — TEST INFRASTRUCTURE: lets the CPU suite run swb::step, the very
// function a wavefront of k_batch_step executes, on a batch laid out by batch_layout.h in host memory, against the
// reference's fixtures and the oracle (tests/test_batch_host.py).  The product never loads this library.
// One "lane", or — built with -DSW_EXACT_HOST_LANES=16 — cooperative fibers that hand over at every sync(), as in
// tests/exact_host.cpp.
#define SW_EXACT_HOST 1
#include "../py-swirld_amd/csrc/batch.hip.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

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
    for (;;) {  // one sweep = every live lane runs to its next sync (or to its end)
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
struct Batch {
    swb_layout::Layout lay;
    std::vector<uint64_t> words;      // (the allocation; base = its first 64-byte boundary)
    unsigned char* base = nullptr;
    const swb::Rec* recs = nullptr;   // in the allocation, at Layout::recs, indexed as the kernels index them
    std::vector<long long> events;
};
}  // namespace

extern "C" {
// npad = 0: the batch's own stride (swb_layout::npad_of)
void* swb_host_create(long long B, int n, const uint64_t* stake, int coin_period, long long cap_events, long long cap_rounds, int npad) {
    Batch* c = new Batch;
    const int np = npad ? npad : swb_layout::npad_of(n);
    c->lay = swb_layout::make((uint64_t)B, (uint64_t)n, (uint64_t)np, (uint64_t)cap_events, (uint64_t)cap_rounds);
    c->words.assign(c->lay.total / 8 + 8, 0x5a5a5a5a5a5a5a5aull);   // (garbage: whatever is read was initialised by the code under test)
    c->base = (unsigned char*)(((uintptr_t)c->words.data() + 63) & ~(uintptr_t)63);
    c->events.assign((size_t)B, 0);
    c->recs = (const swb::Rec*)(c->base + c->lay.recs);
    for (long long b = 0; b < B; ++b) {
        std::vector<uint32_t> st((size_t)np, 0);
        uint64_t tot = 0;
        for (int i = 0; i < n; ++i) { st[i] = stake ? (uint32_t)stake[b * n + i] : 1; tot += st[i]; }
        const swb::Rec r = swb::bind(c->base, c->lay, (uint64_t)b, coin_period, tot);
        memcpy(c->base + c->lay.rec_at((uint64_t)b), &r, sizeof r);   // (as sw_batch_create uploads it)
        run([&] { swb::init_slab(r, st.data()); });
    }
    return c;
}
void swb_host_destroy(void* p) { delete (Batch*)p; }
int swb_host_npad(void* p) { return (int)((Batch*)p)->lay.npad; }
long long swb_host_cap_rounds(void* p) { return (long long)((Batch*)p)->lay.cap_rounds; }

// what k_batch_scatter stores for the events of one hashgraph (heights: swirld.py:117-120); -34 beyond a capacity
int swb_host_append(void* p, long long b, long long K, const int* cr, const int* sp, const int* op, const double* t, const unsigned char* sig) {
    Batch* c = (Batch*)p;
    const swb::Rec& r = c->recs[(size_t)b];
    const long long N0 = c->events[(size_t)b];
    if (N0 + K > r.cap_events) return -34;
    int *d_cr = (int*)r.s.cr, *d_sp = (int*)r.s.sp, *d_op = (int*)r.s.op, *d_ht = (int*)r.s.ht;
    for (long long i = 0; i < K; ++i) {
        const long long e = N0 + i;
        d_cr[e] = cr[i]; d_sp[e] = sp[i]; d_op[e] = op[i];
        d_ht[e] = sp[i] < 0 ? 0 : std::max(d_ht[sp[i]], d_ht[op[i]]) + 1;
        if (d_ht[e] + 3 > r.s.Rcap) return -34;
        ((double*)r.s.t)[e] = t ? t[i] : 0.0;
        for (int k = 0; k < 64; ++k) ((unsigned char*)r.s.sig)[64 * e + k] = sig ? sig[64 * i + k] : 0;
        r.s.round[e] = -1; r.s.tbd[e] = 1; r.s.fam_ev[e] = -1;
    }
    c->events[(size_t)b] = N0 + K;
    return 0;
}

// One step of hashgraph b over its next K undivided events, as sw_batch_step launches it: `chunk` events per launch at the
// most (the product: 8192), divide-only launches first, the last one goes on to fame and order.
void swb_host_step(void* p, long long b, long long K, long long chunk) {
    Batch* c = (Batch*)p;
    const swb::Rec r = c->recs[(size_t)b];
    long long first = r.sum[swb::S_DIVIDED];
    if (chunk <= 0) chunk = swb::MAX_DIVIDE_PER_LAUNCH;
    for (long long a = 0; a < K || a == 0; a += chunk) {
        const long long k = std::min(chunk, K - a);
        const int phases = swb::PH_HEAD | (a + k >= K ? swb::PH_TAIL : 0);
        run([&] { swb::step(r, first + a, k, phases); });
    }
}

void swb_host_summary(void* p, long long b, long long* out) {
    Batch* c = (Batch*)p;
    memcpy(out, c->recs[(size_t)b].sum, swb_layout::SUMMARY_WORDS * sizeof(long long));
}

void swb_host_get(void* p, long long b, int* height, int* round, int* L, int* wit, int* worder, int* wcnt, unsigned char* cons, signed char* fam_ev,
                  unsigned char* tbd, signed char* fam_slot) {
    Batch* c = (Batch*)p;
    const swb::Rec& r = c->recs[(size_t)b];
    const swx::State& s = r.s;
    const long long N = c->events[(size_t)b];
    const int R = (int)s.hdr[swx::H_R], n = s.n, np = s.npad;
    memcpy(height, s.ht, N * sizeof(int));
    memcpy(round, s.round, N * sizeof(int));
    for (long long e = 0; e < N; ++e) memcpy(L + e * n, s.L + e * np, n * sizeof(int));
    for (int q = 0; q < R; ++q) {
        memcpy(wit + (size_t)q * n, s.wit + (size_t)q * np, n * sizeof(int));
        memcpy(worder + (size_t)q * n, s.worder + (size_t)q * np, n * sizeof(int));
        memcpy(fam_slot + (size_t)q * n, s.fam_slot + (size_t)q * np, n);
        wcnt[q] = s.wcnt[q]; cons[q] = s.cons[q];
    }
    memcpy(fam_ev, s.fam_ev, N);
    memcpy(tbd, s.tbd, N);
}

// the step's sorted(new_c) (S_NNEW entries) and the log (S_ORDERED entries)
void swb_host_new_rounds(void* p, long long b, int* out) {
    const swb::Rec& r = ((Batch*)p)->recs[(size_t)b];
    memcpy(out, r.fx.new_rounds, (size_t)r.sum[swb::S_NNEW] * sizeof(int));
}
void swb_host_log(void* p, long long b, int* ev, int* rr, double* ts) {
    const swb::Rec& r = ((Batch*)p)->recs[(size_t)b];
    const size_t m = (size_t)r.sum[swb::S_ORDERED];
    memcpy(ev, r.log_ev, m * sizeof(int)); memcpy(rr, r.log_rr, m * sizeof(int)); memcpy(ts, r.log_ts, m * sizeof(double));
}
// 1 if the BFS map of hashgraph b is all zero (find_order must leave it so)
int swb_host_visited_clear(void* p, long long b) {
    const swb::Rec& r = ((Batch*)p)->recs[(size_t)b];
    for (long long i = 0; i <= r.cap_events; ++i) if (r.ox.visited[i]) return 0;
    return 1;
}
}
