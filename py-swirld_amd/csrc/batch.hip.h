// Many small hashgraphs at once (DESIGN.md "Batches of small hashgraphs"): B independent hashgraphs of one member count,
// one wavefront each, one launch.  A hashgraph of a batch runs the functions of exact.hip.h — the reference's own
// statements, forks included — on its own slab of one allocation (batch_layout.h); swb::step is a whole step of the
// reference's main loop (swirld.py:325-328: divide_rounds(new), decide_fame(), find_order(new_c)) inside one wavefront,
// with no host in between: decide_fame leaves sorted(new_c) in FameScratch::new_rounds and its length in hdr[H_NNEW],
// which is exactly what find_order takes.
//
// Like exact.hip.h the file compiles for the host (g++ -DSW_EXACT_HOST, one lane or cooperative fibers): the CPU suite runs
// swb::step itself against the reference's fixtures and the oracle (tests/batch_host.cpp, tests/test_batch_host.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "batch_layout.h"
#include "exact.hip.h"

namespace swb {

using swx::Wave;

// per-hashgraph summary words (int64, device): written by lane 0 at the end of a step, read back once per step
enum { S_DIVIDED = 0, S_ROUNDS, S_ORDERED, S_NNEW, S_NOUT, S_STAGE, S_CODE, S_EVENT };
static_assert(S_EVENT + 1 == swb_layout::SUMMARY_WORDS, "summary words");
static_assert(swx::H_WORDS == swb_layout::HDR_WORDS, "hdr words");

// where a hashgraph stopped (S_STAGE; 0 = healthy).  A hashgraph with a stage is FROZEN: later steps skip it.
enum { STAGE_NONE = 0, STAGE_DIVIDE = 1, STAGE_FAME = 2, STAGE_ORDER = 3 };

// what a launch does: PH_HEAD clears the per-step words, PH_TAIL goes on to decide_fame and find_order.  A step whose
// hashgraphs have at most 8192 new events each is one launch with both; a longer one has divide-only launches in front.
enum { PH_HEAD = 1, PH_TAIL = 2 };
constexpr long long MAX_DIVIDE_PER_LAUNCH = 8192;

struct RecFields {
    swx::State s;
    swx::FameScratch fx;    // win / layer are set per step from the undecided rounds (capacity: cap_rounds)
    swx::OrderScratch ox;
    int* log_ev;            // the transaction log: event, round received, consensus timestamp
    int* log_rr;
    double* log_ts;
    long long* sum;         // [SUMMARY_WORDS]
    long long cap_events;
};
static_assert(sizeof(RecFields) < swb_layout::REC_BYTES, "swb::Rec outgrew its slot (batch_layout.h: REC_BYTES)");
// One hashgraph: built once at create, lives in device memory.  Padded to the slot of the layout, so that the records
// of a batch are an ARRAY of Rec: recs[b] is the record at Layout::rec_at(b).
struct Rec : RecFields {
    unsigned char pad[swb_layout::REC_BYTES - sizeof(RecFields)];
};
static_assert(sizeof(Rec) == swb_layout::REC_BYTES, "recs[b] must be the record at Layout::rec_at(b)");

// The record of hashgraph b over an allocation that starts at `base` (a device or a host address: arithmetic only).
inline Rec bind(unsigned char* base, const swb_layout::Layout& l, uint64_t b, int coin_period, uint64_t tot) {
    using namespace swb_layout;
    unsigned char* p = base + l.slab_at(b);
    auto at = [&](int seg) { return (void*)(p + l.off[seg]); };
    Rec r{};
    swx::State& s = r.s;
    s.n = (int)l.n; s.npad = (int)l.npad; s.coin_period = coin_period; s.tot = tot;
    s.stake = (const uint32_t*)at(SEG_STAKE);
    s.cr = (const int*)at(SEG_CR); s.sp = (const int*)at(SEG_SP); s.op = (const int*)at(SEG_OP); s.ht = (const int*)at(SEG_HT);
    s.t = (const double*)at(SEG_T); s.sig = (const unsigned char*)at(SEG_SIG);
    s.round = (int*)at(SEG_ROUND); s.L = (int*)at(SEG_L); s.tbd = (unsigned char*)at(SEG_TBD); s.fam_ev = (signed char*)at(SEG_FAM_EV);
    s.Rcap = (int)l.cap_rounds;
    s.wit = (int*)at(SEG_WIT); s.worder = (int*)at(SEG_WORDER); s.wcnt = (int*)at(SEG_WCNT); s.cons = (unsigned char*)at(SEG_CONS);
    s.fam_slot = (signed char*)at(SEG_FAM_SLOT); s.hdr = (long long*)at(SEG_HDR);
    r.fx.votes = (signed char*)at(SEG_VOTES); r.fx.win = 1; r.fx.layer = (size_t)(l.n * l.n);
    r.fx.s_m = (unsigned char*)at(SEG_SM); r.fx.done = (unsigned char*)at(SEG_DONE); r.fx.new_rounds = (int*)at(SEG_NEW_ROUNDS);
    // (fx.hist stays all zero: a batch keeps no event-keyed vote log)
    swx::OrderScratch& o = r.ox;
    o.queue = (int*)at(SEG_QUEUE); o.visited = (unsigned char*)at(SEG_VISITED); o.fw = (int*)at(SEG_FW);
    o.sflag = (unsigned char*)at(SEG_SFLAG); o.times = (double*)at(SEG_TIMES); o.tsort = (double*)at(SEG_TSORT);
    o.white = (unsigned char*)at(SEG_WHITE); o.items_ev = (int*)at(SEG_ITEMS_EV); o.items_ts = (double*)at(SEG_ITEMS_TS);
    o.items_rr = (int*)at(SEG_ITEMS_RR);
    r.log_ev = (int*)at(SEG_LOG_EV); r.log_rr = (int*)at(SEG_LOG_RR); r.log_ts = (double*)at(SEG_LOG_TS);
    r.sum = (long long*)(base + l.summary_at(b));
    r.cap_events = (long long)l.cap_events;
    return r;
}

// An empty hashgraph: no witness, no round, nothing visited, nothing ordered; the stake row.  Per-event defaults are the
// scatter's business, so an untouched event slot costs nothing here.
SWX_HD inline void init_slab(const Rec& r, const uint32_t* stake) {
    const swx::State& s = r.s;
    const int lane = Wave::lane();
    const size_t rows = (size_t)s.Rcap * s.npad;
    for (size_t i = lane; i < rows; i += Wave::nl) { s.wit[i] = -1; s.worder[i] = 0; s.fam_slot[i] = -1; }
    for (int i = lane; i < s.Rcap; i += Wave::nl) { s.wcnt[i] = 0; s.cons[i] = 0; }
    for (long long i = lane; i <= r.cap_events; i += Wave::nl) r.ox.visited[i] = 0;
    for (int i = lane; i < s.npad; i += Wave::nl) ((uint32_t*)s.stake)[i] = stake[i];
    for (int i = lane; i < swx::H_WORDS; i += Wave::nl) s.hdr[i] = 0;
    for (int i = lane; i < swb_layout::SUMMARY_WORDS; i += Wave::nl) r.sum[i] = 0;
}

// One step of the reference's main loop for one hashgraph, by one wavefront: divide_rounds over the events
// [first, first + K), then (PH_TAIL) decide_fame() and find_order(new_c); the ordered items go to the end of the log.
// The step's new_rounds stay in fx.new_rounds, its counts in S_NNEW / S_NOUT, until the next step.  A non-OK code of any
// phase freezes the hashgraph: (stage, code, H_ERR_AT) into the summary, and every later step returns at once.  What the
// reference has changed by the time it raises stays changed here too: rounds and witnesses of the divided events, the
// fame and consensus decide_fame settled, tbd of the events received so far, the log of the rounds of new_c that completed.
SWX_HD inline void step(const Rec& r, long long first, long long K, int phases) {
    const swx::State& s = r.s;
    const int lane = Wave::lane();
    if (r.sum[S_STAGE] != STAGE_NONE) return;   // frozen (written only behind the last sync of an earlier step or launch)
    if (phases & PH_HEAD) {
        if (lane == 0) {
            s.hdr[swx::H_RC] = swx::X_OK; s.hdr[swx::H_NNEW] = 0; s.hdr[swx::H_NOUT] = 0; s.hdr[swx::H_ERR_AT] = -1;
            r.sum[S_NNEW] = 0; r.sum[S_NOUT] = 0;
        }
        Wave::sync();
    }
    int stage = STAGE_DIVIDE;
    int rc = swx::divide(s, first, K);
    Wave::sync();
    if (rc == swx::X_OK && lane == 0) { r.sum[S_DIVIDED] = first + K; r.sum[S_ROUNDS] = s.hdr[swx::H_R]; }
    if (rc == swx::X_OK && (phases & PH_TAIL)) {
        stage = STAGE_FAME;
        swx::FameScratch fx = r.fx;   // the window of this call: the rounds from the first undecided one on
        const int R = (int)s.hdr[swx::H_R];
        int max_c = 0;
        while (max_c < R && s.cons[max_c]) ++max_c;
        fx.win = R - max_c > 1 ? R - max_c : 1;
        fx.layer = (size_t)s.n * fx.win * s.n;
        rc = swx::decide_fame(s, fx);
        Wave::sync();
        if (rc == swx::X_OK) {
            stage = STAGE_ORDER;
            // find_order(new_c) round by round, as the reference's loop appends every round's `final` to the transactions
            // (swirld.py:307-309 are inside the loop over rounds): a call that raises in a later round of new_c has
            // appended the rounds before it, and so has the log of the hashgraph it freezes.
            const int n_new = (int)s.hdr[swx::H_NNEW];
            const long long at = r.sum[S_ORDERED];
            long long total = 0;
            for (int ir = 0; ir < n_new; ++ir) {
                rc = swx::find_order(s, r.ox, fx.new_rounds + ir, 1);
                Wave::sync();
                if (rc != swx::X_OK) break;
                const long long n_out = s.hdr[swx::H_NOUT];
                for (long long i = lane; i < n_out; i += Wave::nl) {
                    r.log_ev[at + total + i] = r.ox.items_ev[i];
                    r.log_rr[at + total + i] = r.ox.items_rr[i];
                    r.log_ts[at + total + i] = r.ox.items_ts[i];
                }
                total += n_out;
                Wave::sync();   // the items and H_NOUT are read before the next round rewrites them
            }
            if (lane == 0) { r.sum[S_NNEW] = n_new; r.sum[S_NOUT] = total; r.sum[S_ORDERED] = at + total; }
        }
    }
    if (rc != swx::X_OK && lane == 0) {
        r.sum[S_CODE] = rc; r.sum[S_EVENT] = s.hdr[swx::H_ERR_AT]; r.sum[S_ROUNDS] = s.hdr[swx::H_R];
        r.sum[S_STAGE] = stage;
    }
}

}  // namespace swb

#if SWX_DEVICE
// ---- kernels ---------------------------------------------------------------------------------------
// One workgroup of one wavefront per PARTICIPATING hashgraph: blockIdx.x indexes a compact list, so a hashgraph that sits
// a step out, or is frozen, costs no workgroup.  Workgroups never wait for one another: a grid larger than what is
// resident simply runs in turns.
__global__ void __launch_bounds__(64) k_batch_step(const swb::Rec* recs, const int* who, const long long* first, const long long* K, int phases) {
    const swb::Rec r = recs[who[blockIdx.x]];
    swb::step(r, first[blockIdx.x], K[blockIdx.x], phases);
}

__global__ void __launch_bounds__(64) k_batch_init(const swb::Rec* recs, const uint32_t* stake) {
    const swb::Rec r = recs[blockIdx.x];
    swb::init_slab(r, stake + (size_t)blockIdx.x * r.s.npad);
}

// Appended events of the whole batch, concatenated (hashgraph b owns [off[b], off[b + 1]) and stores them from its event
// base[b] on), into the slabs: four threads per event, each one 16 bytes of the signature; the first of the four also
// writes creator, parents, height, timestamp and the per-event defaults (round -1, tbd 1, fam_ev -1).
__global__ void __launch_bounds__(256) k_batch_scatter(const swb::Rec* recs, long long B, const long long* off, const long long* base,
                                                       const int* cr, const int* sp, const int* op, const int* ht, const double* t,
                                                       const uint4* sig) {
    const long long total = off[B];
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long i = tid >> 2;
    const int q = (int)(tid & 3);
    if (i >= total) return;
    long long lo = 0, hi = B;   // the hashgraph of event i: the last b with off[b] <= i
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    const swb::Rec& r = recs[lo];
    const long long e = base[lo] + (i - off[lo]);
    if (e < 0 || e >= r.cap_events) return;   // (the host has checked the capacity: never taken)
    uint4 v = make_uint4(0, 0, 0, 0);
    if (sig) v = sig[4 * i + q];
    ((uint4*)r.s.sig)[4 * e + q] = v;   // the signatures of a slab start on a 64-byte boundary
    if (q == 0) {
        ((int*)r.s.cr)[e] = cr[i]; ((int*)r.s.sp)[e] = sp[i]; ((int*)r.s.op)[e] = op[i]; ((int*)r.s.ht)[e] = ht[i];
        ((double*)r.s.t)[e] = t ? t[i] : 0.0;
        r.s.round[e] = -1; r.s.tbd[e] = 1; r.s.fam_ev[e] = -1;
    }
}
#endif
