// What the exact (forked-hashgraph) path computes beyond the bare order, kept (sw_set_exact_history):
//   * round received and consensus timestamp of every event find_order produces (swirld.py:283, 305), into the same
//     per-event tables the fast path fills (consensus.hip.h), and the order into the same device copy of `transactions`;
//   * Node.votes (swirld.py:60-61, 256-272) KEYED BY EVENT: with forks a voter may be a witness a later sibling replaced
//     in the (round, member) table, so the table form of votes.hip.h cannot name it.
//
// THE VOTE STORE.  An append-only log of entries (voter event y, candidate event x, value) in first-insertion order, and an
// open-addressing index from the 64-bit key (y, x) to the log slot: `tab` holds a log slot or -1, a power-of-two number of
// slots >= 2 x the log's capacity (load factor <= 1/2), linear probing, the key of a slot read from the log.  Assignment is
// the dict's: a new key appends, an existing key has its value overwritten in place.  The log is what the readers give out;
// its order is import order, then first insertion — not the reference's dict order.
//
//   flush (swx::flush_votes in exact.hip.h)   the ONE wavefront of k_exact_fame, at the end of every voter round: lanes
//                        stride over the round's vote layer, look every entry up, claim log slots for the new keys by a
//                        ballot / popcount prefix (one wave: one counter, no global atomic for the append) and insert
//                        them with one compare-and-swap per probed slot.
//   k_votes_reindex      after the host grew the store: one thread per log entry inserts it into the emptied index.
//   k_votes_row_counts / k_votes_offsets / k_votes_expand
//                        the fast path's table (votes.hip.h: rows (voter, candidate round) with member bitmasks) expanded
//                        into entries: set bits per row, their exclusive scan by ONE workgroup, then one thread per row
//                        writes its entries; the candidate of bit mc in a row of round rc is wit[rc][mc].
//   k_votes_lookup       one thread per asked pair: its value, -1 = no entry.
//   k_history_normalise  entering the exact path: every event outside the fast path's ordered chain prefixes gets
//                        rr = -1, cts = the quiet NaN of consensus.hip.h, so that afterwards the tables answer as they are.
//   k_history_defaults   the same two defaults for a range of events (appended on the exact path; sw_rewind).
//   k_history_record     one thread per item find_order produced: rr[ev] = round, cts[ev] = ts (a 64-bit word).
// Plain vector loads and stores and ordinary atomics; no kernel waits for another workgroup; every probe loop is bounded by
// the table's size.  Every index comes from the context's own tables; the pairs of k_votes_lookup are range-checked.
//
// Each kernel body is a per-thread function (or a sequence of per-thread phases with a barrier between them):
// tests/exact_history_emul.cpp runs the same functions thread by thread on the host, under sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) && !defined(SW_EXACT_HOST) && !defined(XH_HOST_EMULATION)
#define XH_HD __device__ __forceinline__
#define XH_DEVICE 1
#else
#define XH_HD inline
#define XH_DEVICE 0
#endif

namespace xh {

typedef unsigned long long u64;

constexpr int THREADS = 256;
constexpr int SCAN_THREADS = 1024;
constexpr u64 QNAN_BITS = 0x7ff8000000000000ull;   // cns::QNAN_BITS: "not ordered yet" of a consensus time

// The store as a kernel sees it.  All zero (the `x{}` of a FameScratch) = record nothing.
struct Store {
    int* voter;           // the log [cap]: voter event y
    int* cand;            //                candidate event x
    signed char* value;   //                votes[y][x], 0 / 1
    int* tab;             // the index: tmask + 1 slots, each a log slot or -1
    long long cap;        // entries the log has room for
    unsigned tmask;
};

XH_HD unsigned key_hash(int y, int x) {
    u64 k = ((u64)(unsigned)y << 32) | (unsigned)x;
    k *= 0x9E3779B97F4A7C15ull;
    return (unsigned)(k >> 32);
}

XH_HD int tab_cas(int* p, int expected, int desired) {
#if XH_DEVICE
    return atomicCAS(p, expected, desired);
#else
    return __sync_val_compare_and_swap(p, expected, desired);
#endif
}

// the log slot of key (y, x), -1 = no entry.  Nothing may write the index meanwhile.
XH_HD int find(const Store& s, int y, int x) {
    unsigned h = key_hash(y, x) & s.tmask;
    for (unsigned step = 0; step <= s.tmask; ++step) {
        const int slot = s.tab[h];
        if (slot < 0) return -1;
        if (s.voter[slot] == y && s.cand[slot] == x) return slot;
        h = (h + 1) & s.tmask;
    }
    return -1;
}

// key (y, x), which the index does not hold and no other thread inserts, -> log slot `slot`.  Concurrent inserts of other
// keys are fine: a slot is taken by exactly one compare-and-swap.  false: no free slot (never with load <= 1/2).
XH_HD bool insert(const Store& s, int y, int x, int slot) {
    unsigned h = key_hash(y, x) & s.tmask;
    for (unsigned step = 0; step <= s.tmask; ++step) {
        if (tab_cas(&s.tab[h], -1, slot) == -1) return true;
        h = (h + 1) & s.tmask;
    }
    return false;
}

// ---- k_votes_reindex: log entry i into the (emptied) index
XH_HD void reindex_one(long long i, const Store& s) { insert(s, s.voter[i], s.cand[i], (int)i); }

// ---- k_votes_lookup: pair i
XH_HD void lookup_one(long long i, const Store& s, long long n_events, const int* voter, const int* cand, signed char* out) {
    const int y = voter[i], x = cand[i];
    int slot = -1;
    if (y >= 0 && x >= 0 && y < n_events && x < n_events) slot = find(s, y, x);
    out[i] = slot < 0 ? (signed char)-1 : s.value[slot];
}

// ---- the table of votes.hip.h -> entries
XH_HD int popc64(u64 v) {
#if XH_DEVICE
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}

// k_votes_row_counts: entries of row `row` (the set bits of its exists words)
XH_HD void row_count_one(long long row, const u64* exists, int nwo, long long* cnt) {
    long long c = 0;
    for (int j = 0; j < nwo; ++j) c += popc64(exists[(size_t)row * nwo + j]);
    cnt[row] = c;
}

// k_votes_offsets, ONE workgroup of T threads over `rows` counts, in place: cnt[row] becomes the exclusive prefix,
// cnt[rows] the total.  Thread t owns the rows [t * per, (t + 1) * per), per = ceil(rows / T).
XH_HD void offsets_phase1(int t, int T, long long rows, const long long* cnt, long long* part) {
    const long long per = (rows + T - 1) / T;
    long long s = 0;
    for (long long r = (long long)t * per; r < rows && r < (long long)(t + 1) * per; ++r) s += cnt[r];
    part[t] = s;
}
XH_HD void offsets_phase2(int t, int T, long long* part) {   // thread 0: exclusive scan of the T partial sums; part[T] = total
    if (t != 0) return;
    long long run = 0;
    for (int i = 0; i < T; ++i) { const long long v = part[i]; part[i] = run; run += v; }
    part[T] = run;
}
XH_HD void offsets_phase3(int t, int T, long long rows, long long* cnt, const long long* part) {
    const long long per = (rows + T - 1) / T;
    long long run = part[t];
    for (long long r = (long long)t * per; r < rows && r < (long long)(t + 1) * per; ++r) { const long long v = cnt[r]; cnt[r] = run; run += v; }
    if (t == 0) cnt[rows] = part[T];
}

struct TableIn {           // the rows sw_export_votes_device writes
    const int* row_voter;
    const int* row_cand_round;
    const u64* exists;
    const u64* value;
    int nwo;               // words per row: ceil(n / 64)
    const int* wit;        // [R][np]
    int np, n;
};

// k_votes_expand: the entries of row `row` to log slots base + off[row] ...; bits at and beyond n are ignored
XH_HD void expand_one(long long row, const TableIn& in, const long long* off, long long base, const Store& s) {
    long long at = base + off[row];
    const int y = in.row_voter[row], rc = in.row_cand_round[row];
    for (int j = 0; j < in.nwo; ++j) {
        u64 ex = in.exists[(size_t)row * in.nwo + j];
        const u64 val = in.value[(size_t)row * in.nwo + j];
        while (ex) {
#if XH_DEVICE
            const int b = __ffsll((long long)ex) - 1;
#else
            const int b = __builtin_ctzll(ex);
#endif
            ex &= ex - 1;
            const int mc = j * 64 + b;
            if (mc >= in.n || at >= s.cap) continue;
            s.voter[at] = y;
            s.cand[at] = in.wit[(size_t)rc * in.np + mc];
            s.value[at] = (signed char)((val >> b) & 1ull);
            ++at;
        }
    }
}

// ---- per-event tables
// k_history_normalise: event e of a context that leaves the fast path — ordered there iff it lies inside its creator's
// ordered chain prefix (consensus.hip.h, k_consensus_events)
XH_HD void normalise_one(long long e, const int* seq, const int* cr, const int* ordpos, int* rr, u64* cts) {
    if (seq[e] < ordpos[cr[e]]) return;
    rr[e] = -1;
    cts[e] = QNAN_BITS;
}
// k_history_defaults: event first + i is not ordered
XH_HD void defaults_one(long long i, long long first, int* rr, u64* cts) {
    rr[first + i] = -1;
    cts[first + i] = QNAN_BITS;
}
// k_history_record: item i of the call's output (every event is produced once, so no two threads write one entry)
XH_HD void record_one(long long i, const int* items_ev, const u64* items_ts, const int* items_rr, int* rr, u64* cts) {
    const int e = items_ev[i];
    rr[e] = items_rr[i];
    cts[e] = items_ts[i];
}

#if XH_DEVICE
__global__ void __launch_bounds__(THREADS) k_votes_reindex(Store s, long long count) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i < count) reindex_one(i, s);
}
__global__ void __launch_bounds__(THREADS)
k_votes_lookup(Store s, long long n_events, long long K, const int* __restrict__ voter, const int* __restrict__ cand, signed char* out) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i < K) lookup_one(i, s, n_events, voter, cand, out);
}
__global__ void __launch_bounds__(THREADS) k_votes_row_counts(long long rows, const u64* __restrict__ exists, int nwo, long long* cnt) {
    const long long r = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (r < rows) row_count_one(r, exists, nwo, cnt);
}
__global__ void __launch_bounds__(SCAN_THREADS) k_votes_offsets(long long rows, long long* cnt) {
    __shared__ long long part[SCAN_THREADS + 1];
    const int t = (int)threadIdx.x;
    offsets_phase1(t, SCAN_THREADS, rows, cnt, part);
    __syncthreads();
    offsets_phase2(t, SCAN_THREADS, part);
    __syncthreads();
    offsets_phase3(t, SCAN_THREADS, rows, cnt, part);
}
__global__ void __launch_bounds__(THREADS) k_votes_expand(long long rows, TableIn in, const long long* __restrict__ off, long long base, Store s) {
    const long long r = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (r < rows) expand_one(r, in, off, base, s);
}
__global__ void __launch_bounds__(THREADS)
k_history_normalise(long long n_events, const int* __restrict__ seq, const int* __restrict__ cr, const int* __restrict__ ordpos, int* rr, u64* cts) {
    const long long e = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (e < n_events) normalise_one(e, seq, cr, ordpos, rr, cts);
}
__global__ void __launch_bounds__(THREADS) k_history_defaults(long long first, long long K, int* rr, u64* cts) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i < K) defaults_one(i, first, rr, cts);
}
__global__ void __launch_bounds__(THREADS)
k_history_record(long long n_items, const int* __restrict__ items_ev, const u64* __restrict__ items_ts, const int* __restrict__ items_rr, int* rr, u64* cts) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i < n_items) record_one(i, items_ev, items_ts, items_rr, rr, cts);
}
#endif

}  // namespace xh
