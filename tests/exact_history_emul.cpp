// Stand-alone host program — TEST INFRASTRUCTURE (tests/test_exact_history_kernels_host.py builds it with AddressSanitizer
// and UBSan and runs it): the kernels of csrc/exact_history.hip.h thread by thread, and the flush of exact.hip.h with one
// lane, each case checked here against a std::map / a plain loop.  Exit status 0 = every check of the named case held.
//   exact_history_emul grow | overflow | expand <n> | tables
#define SW_EXACT_HOST 1
#include "../py-swirld_amd/csrc/exact.hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace {

typedef unsigned long long u64;

struct Rng {
    u64 s;
    explicit Rng(u64 seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    u64 next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
    int below(int m) { return (int)(next() % (u64)m); }
};

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// the host side of the store, as the library keeps it: grown before a flush, index rebuilt one thread per entry
struct HostStore {
    std::vector<int> voter, cand, tab;
    std::vector<signed char> value;
    long long cap = 0, ceiling, grows = 0;
    explicit HostStore(long long ceil_) : ceiling(ceil_) {}
    xh::Store view() {
        xh::Store s{};
        s.voter = voter.data(); s.cand = cand.data(); s.value = value.data(); s.tab = tab.data(); s.cap = cap; s.tmask = (unsigned)tab.size() - 1;
        return s;
    }
    void reserve(long long need, long long count, long long cap0) {
        if (need > ceiling) need = ceiling;
        if (need <= cap && !tab.empty()) return;
        long long nc = cap0;
        while (nc < need) nc *= 2;
        if (nc > ceiling) nc = ceiling;
        if (nc < cap) nc = cap;
        voter.resize(nc); cand.resize(nc); value.resize(nc);
        size_t slots = 2;
        while (slots < 2 * (size_t)nc) slots *= 2;
        tab.assign(slots, -1);
        cap = nc;
        const xh::Store s = view();
        for (long long i = 0; i < count; ++i) xh::reindex_one(i, s);
        ++grows;
    }
};

// A witness table of R rounds x n members with distinct events, voter rounds flushed one after the other, every layer
// twice (the second time with other values: every key exists and is overwritten).
int run_flush(long long cap0, long long ceiling, bool expect_overflow) {
    const int n = 5, np = 64, R = 9, max_c = 2;
    Rng rng(11);
    std::vector<int> wit((size_t)R * np, -1);
    int next_ev = 0;
    for (int r = 0; r < R; ++r)
        for (int c = 0; c < n; ++c)
            if (r < 2 || rng.below(5)) { wit[(size_t)r * np + c] = next_ev; next_ev += 1 + rng.below(3); }
    long long hdr[swx::H_WORDS] = {0};
    swx::State s{};
    s.n = n; s.npad = np; s.wit = wit.data(); s.hdr = hdr;
    swx::FameScratch x{};
    x.win = R - max_c;
    x.layer = (size_t)n * x.win * n;
    std::vector<signed char> cur(x.layer);
    HostStore hs(ceiling);
    std::map<std::pair<int, int>, int> ref;
    std::vector<std::pair<int, int>> first_order;
    long long collisions = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (int r_ = max_c + 1; r_ < R; ++r_) {
            std::fill(cur.begin(), cur.end(), (signed char)-1);
            long long fresh = 0;
            for (int cy = 0; cy < n; ++cy) {
                if (wit[(size_t)r_ * np + cy] < 0) continue;
                for (int r = max_c; r < r_; ++r)
                    for (int cx = 0; cx < n; ++cx) {
                        if (wit[(size_t)r * np + cx] < 0 || !rng.below(4)) continue;
                        const int v = rng.below(2);
                        cur[(size_t)cy * x.win * n + (size_t)(r - max_c) * n + cx] = (signed char)v;
                        const std::pair<int, int> key(wit[(size_t)r_ * np + cy], wit[(size_t)r * np + cx]);
                        if (!hdr[swx::H_VOVF]) {
                            if (!ref.count(key)) { first_order.push_back(key); ++fresh; }
                            ref[key] = v;
                        }
                    }
            }
            hs.reserve(hdr[swx::H_VCNT] + fresh, hdr[swx::H_VCNT], cap0);
            x.hist = hs.view();
            swx::flush_votes(s, x, cur.data(), r_, max_c);
            CHECK(hdr[swx::H_VCNT] <= hs.cap, "count %lld beyond the capacity %lld", hdr[swx::H_VCNT], hs.cap);
        }
    const xh::Store st = hs.view();
    const long long count = hdr[swx::H_VCNT];
    if (expect_overflow) {
        CHECK(hdr[swx::H_VOVF] == 1, "the overflow word is %lld", hdr[swx::H_VOVF]);
        CHECK(count <= ceiling && hs.cap == ceiling, "count %lld, capacity %lld, ceiling %lld", count, hs.cap, ceiling);
        // a later flush stores nothing more
        x.hist = st;
        swx::flush_votes(s, x, cur.data(), R - 1, max_c);
        CHECK(hdr[swx::H_VCNT] == count, "a flush behind the overflow stored entries");
    } else {
        CHECK(hdr[swx::H_VOVF] == 0, "overflow word set");
        CHECK(count == (long long)ref.size(), "%lld entries, expected %zu", count, ref.size());
        CHECK(hs.grows >= 4, "the store grew %lld times only", hs.grows);
        for (long long i = 0; i < count; ++i) {
            const std::pair<int, int> key(st.voter[i], st.cand[i]);
            CHECK(key == first_order[i], "entry %lld is not in first-insertion order", i);
            CHECK(st.value[i] == ref[key], "entry %lld has value %d", i, st.value[i]);
            CHECK(xh::find(st, key.first, key.second) == (int)i, "entry %lld is not found through the index", i);
            if (st.tab[xh::key_hash(key.first, key.second) & st.tmask] != (int)i) ++collisions;   // its home slot was taken
        }
        CHECK(collisions > 0, "no entry left its home slot: the case must hold colliding hashes");
    }
    // the look-up kernel: stored pairs, absent pairs, pairs outside the events
    std::vector<int> qy, qx;
    for (int i = 0; i < 300; ++i) { qy.push_back(rng.below(next_ev + 4) - 2); qx.push_back(rng.below(next_ev + 4) - 2); }
    for (long long i = 0; i < count; ++i) { qy.push_back(st.voter[i]); qx.push_back(st.cand[i]); }
    std::vector<signed char> out(qy.size(), 7);
    for (size_t i = 0; i < qy.size(); ++i) xh::lookup_one((long long)i, st, next_ev, qy.data(), qx.data(), out.data());
    for (size_t i = 0; i < qy.size(); ++i) {
        int want = -1;
        for (long long k = 0; k < count; ++k) if (st.voter[k] == qy[i] && st.cand[k] == qx[i]) want = st.value[k];
        CHECK(out[i] == want, "look-up %zu (%d, %d): %d, expected %d", i, qy[i], qx[i], out[i], want);
    }
    return 0;
}

// the table of votes.hip.h (rows with member bitmasks) -> entries, the row offsets by the three phases of k_votes_offsets
int run_expand(int n, int T) {
    const int np = (n + 63) / 64 * 64, nwo = (n + 63) / 64, R = 6;
    Rng rng(100 + n);
    std::vector<int> wit((size_t)R * np, -1);
    for (int r = 0; r < R; ++r) for (int c = 0; c < n; ++c) wit[(size_t)r * np + c] = 1000 * r + c;
    const long long rows = 37;
    std::vector<int> row_voter(rows), row_rc(rows);
    std::vector<u64> exists((size_t)rows * nwo, 0), value((size_t)rows * nwo, 0);
    std::vector<int> ry, rx, rv;
    for (long long row = 0; row < rows; ++row) {
        row_voter[row] = 5000 + (int)row / 3;
        row_rc[row] = (int)row % 3 + ((int)row / 3) % 3;   // distinct per voter
        if (row % 7 == 3) continue;   // an empty row
        for (int mc = 0; mc < n; ++mc) {
            const bool last_word = mc / 64 == nwo - 1;
            if (!(last_word ? rng.below(2) : !rng.below(3))) continue;
            const int v = rng.below(2);
            exists[(size_t)row * nwo + mc / 64] |= 1ull << (mc % 64);
            if (v) value[(size_t)row * nwo + mc / 64] |= 1ull << (mc % 64);
            ry.push_back(row_voter[row]); rx.push_back(wit[(size_t)row_rc[row] * np + mc]); rv.push_back(v);
        }
    }
    u64 last = 0;
    for (long long row = 0; row < rows; ++row) last |= exists[(size_t)row * nwo + nwo - 1];
    CHECK(last != 0 && (n % 64 == 0 || (last >> (n % 64)) == 0), "the case needs bits in the last, partial word and none behind member n");
    std::vector<long long> cnt(rows + 1, -1), part(T + 1, -1);
    for (long long r = 0; r < rows; ++r) xh::row_count_one(r, exists.data(), nwo, cnt.data());
    for (int t = 0; t < T; ++t) xh::offsets_phase1(t, T, rows, cnt.data(), part.data());
    for (int t = 0; t < T; ++t) xh::offsets_phase2(t, T, part.data());
    for (int t = 0; t < T; ++t) xh::offsets_phase3(t, T, rows, cnt.data(), part.data());
    CHECK(cnt[rows] == (long long)ry.size(), "total %lld, expected %zu", cnt[rows], ry.size());
    const long long base = 3;   // entries the log holds already
    HostStore hs(1ll << 40);
    hs.reserve(base + cnt[rows], 0, 4);
    xh::Store st = hs.view();
    for (int i = 0; i < base; ++i) { st.voter[i] = 1 + i; st.cand[i] = 2 + i; st.value[i] = 1; }
    const xh::TableIn in{row_voter.data(), row_rc.data(), exists.data(), value.data(), nwo, wit.data(), np, n};
    for (long long r = 0; r < rows; ++r) xh::expand_one(r, in, cnt.data(), base, st);
    const long long count = base + cnt[rows];
    for (long long i = 0; i < count; ++i) xh::reindex_one(i, st);
    for (size_t i = 0; i < ry.size(); ++i) {
        CHECK(st.voter[base + i] == ry[i] && st.cand[base + i] == rx[i] && st.value[base + i] == rv[i], "entry %zu differs", i);
        CHECK(xh::find(st, ry[i], rx[i]) == (int)(base + i), "entry %zu is not found through the index", i);
    }
    CHECK(xh::find(st, 1, 2) == 0 && xh::find(st, 4999, 0) == -1, "entries in front of the import");
    return 0;
}

// normalise, defaults, record — zero produced items included
int run_tables() {
    const int n = 6;
    const long long N = 700;
    Rng rng(77);
    std::vector<int> cr(N), seq(N), ordpos(n), cnt(n, 0), rr(N), want_rr(N);
    std::vector<u64> cts(N), want_cts(N);
    for (long long e = 0; e < N; ++e) { cr[e] = rng.below(n); seq[e] = cnt[cr[e]]++; rr[e] = 40 + rng.below(9); cts[e] = rng.next(); }
    for (int c = 0; c < n; ++c) ordpos[c] = c == 2 ? 0 : rng.below(cnt[c] + 1);
    for (long long e = 0; e < N; ++e) {
        const bool ordered = seq[e] < ordpos[cr[e]];
        want_rr[e] = ordered ? rr[e] : -1;
        want_cts[e] = ordered ? cts[e] : xh::QNAN_BITS;
    }
    for (long long e = 0; e < N; ++e) xh::normalise_one(e, seq.data(), cr.data(), ordpos.data(), rr.data(), cts.data());
    CHECK(rr == want_rr && cts == want_cts, "normalise");
    // events appended later
    const long long K = 45;
    rr.resize(N + K, 5); cts.resize(N + K, 5); want_rr.resize(N + K, -1); want_cts.resize(N + K, xh::QNAN_BITS);
    for (long long i = 0; i < K; ++i) xh::defaults_one(i, N, rr.data(), cts.data());
    CHECK(rr == want_rr && cts == want_cts, "defaults");
    // a call that produced nothing: no thread runs, the arrays may be absent
    for (long long i = 0; i < 0; ++i) xh::record_one(i, nullptr, nullptr, nullptr, rr.data(), cts.data());
    CHECK(rr == want_rr && cts == want_cts, "record of zero items");
    // a call that produced the events that were not ordered, in two rounds
    std::vector<int> items_ev, items_rr;
    std::vector<u64> items_ts;
    for (long long e = N + K - 1; e >= 0; --e)
        if (want_rr[e] < 0 && rng.below(2)) {
            items_ev.push_back((int)e); items_rr.push_back(items_ev.size() < 100 ? 50 : 53);
            double t = 1.7e9 + 0.013 * (double)e;
            u64 bits; memcpy(&bits, &t, 8);
            items_ts.push_back(bits);
            want_rr[e] = items_rr.back(); want_cts[e] = bits;
        }
    for (size_t i = 0; i < items_ev.size(); ++i) xh::record_one((long long)i, items_ev.data(), items_ts.data(), items_rr.data(), rr.data(), cts.data());
    CHECK(rr == want_rr && cts == want_cts, "record");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "grow") return run_flush(4, 1ll << 40, false);
    if (what == "overflow") return run_flush(4, 24, true);
    if (what == "expand" && argc > 2) { const int n = atoi(argv[2]); return run_expand(n, xh::SCAN_THREADS) || run_expand(n, 7); }
    if (what == "tables") return run_tables();
    fprintf(stderr, "usage: %s grow | overflow | expand <n> | tables\n", argv[0]);
    return 2;
}
