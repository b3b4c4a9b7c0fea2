// Host build of the exact path WITH its history (exact.hip.h + exact_history.hip.h) — TEST INFRASTRUCTURE, like
// exact_host.cpp, whose context, lane emulation and plain calls it takes over by inclusion.  Added here: what the product's
// host code does around the kernels when sw_set_exact_history is on — the vote store grown before every decide_fame
// (log copied, index rebuilt entry by entry), its ceiling, the record step behind a successful find_order.
#include "exact_host.cpp"

namespace {
struct HCtx {
    Ctx* c = nullptr;
    std::vector<int> voter, cand, tab, rr, items_rr;
    std::vector<signed char> value;
    std::vector<unsigned long long> cts;
    std::vector<int> tx;
    long long cap = 0, cap0 = 4096, ceiling = 1ll << 40, grows = 0;
    xh::Store store() {
        xh::Store s{};
        s.voter = voter.data(); s.cand = cand.data(); s.value = value.data(); s.tab = tab.data();
        s.cap = cap; s.tmask = (unsigned)tab.size() - 1;
        return s;
    }
    // room for `need` entries in all (at most the ceiling): the log keeps its entries, the index is rebuilt
    void reserve(long long need) {
        need = std::min(need, ceiling);
        if (need <= cap && !tab.empty()) return;
        long long nc = std::max<long long>(cap0, 1);
        while (nc < need) nc *= 2;
        nc = std::min(std::max(nc, cap), ceiling);
        voter.resize(nc); cand.resize(nc); value.resize(nc);
        size_t slots = 2;
        while (slots < 2 * (size_t)nc) slots *= 2;
        tab.assign(slots, -1);
        cap = nc;
        const xh::Store s = store();
        for (long long i = 0; i < c->hdr[swx::H_VCNT]; ++i) xh::reindex_one(i, s);
        ++grows;
    }
};
}  // namespace

extern "C" {
void* xhh_create(int n, const uint32_t* stake, int coin_period, long long cap0, long long ceiling) {
    HCtx* h = new HCtx;
    h->c = (Ctx*)swx_host_create(n, stake, coin_period);
    if (cap0 > 0) h->cap0 = cap0;
    if (ceiling > 0) h->ceiling = ceiling;
    return h;
}
void xhh_destroy(void* p) { HCtx* h = (HCtx*)p; swx_host_destroy(h->c); delete h; }
void* xhh_base(void* p) { return ((HCtx*)p)->c; }
int xhh_append(void* p, long long K, const int* cr, const int* sp, const int* op, const double* t, const unsigned char* sig) {
    HCtx* h = (HCtx*)p;
    const int rc = swx_host_append(h->c, K, cr, sp, op, t, sig);
    h->rr.resize(h->c->N); h->cts.resize(h->c->N);
    for (long long i = 0; i < K; ++i) xh::defaults_one(i, h->c->N - K, h->rr.data(), h->cts.data());
    return rc;
}
int xhh_divide(void* p, long long first, long long K) { return swx_host_divide(((HCtx*)p)->c, first, K); }
int xhh_fame(void* p, int* new_rounds, int* n_new) {
    HCtx* h = (HCtx*)p;
    Ctx* c = h->c;
    c->hdr[swx::H_RC] = 0; c->hdr[swx::H_NNEW] = 0;
    const int R = (int)c->hdr[swx::H_R];
    int max_c = 0;
    while (max_c < R && c->cons[max_c]) ++max_c;
    swx::FameScratch x{};
    x.win = std::max(1, R - max_c);
    x.layer = (size_t)c->n * x.win * c->n;
    // every voter round r_ writes at most n voters x (r_ - max_c) candidate rounds x n candidates
    const long long w = R - max_c;
    h->reserve(c->hdr[swx::H_VCNT] + (long long)c->n * c->n * (w * (w - 1) / 2));
    x.hist = h->store();
    std::vector<signed char> votes(2 * x.layer);
    std::vector<unsigned char> s_m(c->np), done(c->Rcap);
    std::vector<int> nr(c->Rcap);
    x.votes = votes.data(); x.s_m = s_m.data(); x.done = done.data(); x.new_rounds = nr.data();
    int rc = 0;
    const swx::State st = c->state();
    run([&] { const int r = swx::decide_fame(st, x); if (r) rc = r; });
    *n_new = (int)c->hdr[swx::H_NNEW];
    for (int i = 0; i < *n_new; ++i) new_rounds[i] = nr[i];
    return rc;
}
int xhh_order(void* p, const int* rounds, int n_rounds, int* out, long long* n_out) {
    HCtx* h = (HCtx*)p;
    Ctx* c = h->c;
    c->hdr[swx::H_RC] = 0; c->hdr[swx::H_NOUT] = 0;
    std::vector<int> rs(rounds, rounds + n_rounds);
    std::sort(rs.begin(), rs.end());
    swx::OrderScratch x{};
    std::vector<int> queue(c->N + 1), fw(c->np), items_ev(c->N + 1), items_rr(c->N + 1);
    std::vector<unsigned char> visited(c->N + 1, 0), sflag(c->np), white(64);
    std::vector<double> times(c->np), tsort(c->np), items_ts(c->N + 1);
    x.queue = queue.data(); x.visited = visited.data(); x.fw = fw.data(); x.sflag = sflag.data(); x.times = times.data();
    x.tsort = tsort.data(); x.white = white.data(); x.items_ev = items_ev.data(); x.items_ts = items_ts.data();
    x.items_rr = items_rr.data();
    int rc = 0;
    const swx::State st = c->state();
    run([&] { const int r = swx::find_order(st, x, rs.data(), n_rounds); if (r) rc = r; });
    *n_out = c->hdr[swx::H_NOUT];
    if (rc) { *n_out = 0; return rc; }   // a failed call records nothing, as it appends nothing to `transactions`
    for (long long i = 0; i < *n_out; ++i) {
        out[i] = items_ev[i]; h->tx.push_back(items_ev[i]);
        xh::record_one(i, items_ev.data(), (const unsigned long long*)items_ts.data(), items_rr.data(), h->rr.data(), h->cts.data());
    }
    return rc;
}
// store: count, overflow word, capacity, growths; then the log
void xhh_store_stats(void* p, long long* out4) {
    HCtx* h = (HCtx*)p;
    out4[0] = h->c->hdr[swx::H_VCNT]; out4[1] = h->c->hdr[swx::H_VOVF]; out4[2] = h->cap; out4[3] = h->grows;
}
void xhh_store_get(void* p, int* voter, int* cand, signed char* value) {
    HCtx* h = (HCtx*)p;
    const long long k = h->c->hdr[swx::H_VCNT];
    memcpy(voter, h->voter.data(), k * sizeof(int)); memcpy(cand, h->cand.data(), k * sizeof(int)); memcpy(value, h->value.data(), k);
}
void xhh_lookup(void* p, long long K, const int* voter, const int* cand, signed char* out) {
    HCtx* h = (HCtx*)p;
    const xh::Store s = h->store();
    for (long long i = 0; i < K; ++i) {
        if (s.tab) xh::lookup_one(i, s, h->c->N, voter, cand, out);
        else out[i] = -1;
    }
}
void xhh_consensus_get(void* p, int* rr, unsigned long long* cts) {
    HCtx* h = (HCtx*)p;
    memcpy(rr, h->rr.data(), h->c->N * sizeof(int)); memcpy(cts, h->cts.data(), h->c->N * 8);
}
}
