// Host side of the C-ABI (include/swirld_hip.h): owns the HBM-resident hashgraph state of one
// Node view and drives the kernels of kernels.hip.h on one HIP stream.
//
// Path (reference file:line):  Node.add_event swirld.py:114-120 -> sw_append_events;
// Node.divide_rounds swirld.py:187-222 -> sw_divide_rounds; Node.decide_fame
// swirld.py:224-277 -> sw_decide_fame; Node.find_order swirld.py:280-311 -> sw_find_order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/swirld_hip.h"
#include "entry_plan.h"
#include "owned.h"
#include "kernels.hip.h"
#define SW_PROV_ROWS 16   // sub-batches of one divide_rounds call that can be swept in chunks
#define SW_RANGE_SLOTS 16 // event ranges swept by sw_cansee_range between two rewinds
#include "crypto.hip.h"
#include "validate.hip.h"
#include "pack.hip.h"
#include "sign.hip.h"
#include "data.hip.h"
#include "exact.hip.h"
#include "batch.hip.h"
#include "ingest.hip.h"
#include "resolve.hip.h"
#include "gossip.hip.h"
#include "walk.hip.h"
#include "wire.hip.h"
#include "turn.hip.h"
#include "consensus.hip.h"
#include "votes.hip.h"

namespace {

std::string g_create_error;

using owned::DBuf;
using owned::Event;
using owned::Pinned;
using owned::Stream;

// growable int32 array in pinned host memory: the ordered events (Node.transactions) — device copies land in it directly
struct PinnedVec {
    Pinned<int32_t> buf;
    size_t n = 0;
    size_t size() const { return n; }
    int32_t* data() { return buf.p; }
    int32_t& operator[](size_t i) { return buf.p[i]; }
    void clear() { n = 0; }
    bool resize(size_t m) {   // (only while nothing is in flight into the array)
        if (m > buf.cap) {
            Pinned<int32_t> q;
            if (!q.reserve(std::max(m, buf.cap + buf.cap / 2 + 4096))) return false;
            if (n) memcpy(q.p, buf.p, n * sizeof(int32_t));
            buf = std::move(q);
        }
        n = m;
        return true;
    }
};

}  // namespace

// can_see table under HIP virtual memory management (windowed mode, sw_set_window): ONE reserved address
// range for the whole table, physical chunks mapped as events arrive and recycled from below the
// eviction horizon — every kernel keeps the same base pointer and the same row arithmetic.
struct VmTable {
    bool active = false;
    char* base = nullptr;
    size_t va_bytes = 0, chunk = 0;
    std::vector<hipMemGenericAllocationHandle_t> handle;  // per chunk slot of the address range
    std::vector<char> mapped;
    std::vector<hipMemGenericAllocationHandle_t> pool;    // physical chunks unmapped by evictions, ready for reuse
    size_t hi = 0;        // chunk slots [lo, hi) are mapped
    size_t lo = 0;
    int64_t evictions = 0;
};

// ONE hashgraph's round loop over several linked contexts (sw_split_link; kernels.hip.h SplitDst): what the host threads of
// the parts share.  Every part runs its own sw_divide_rounds (same events, same call); inside an iteration of the round loop
// its stream waits, at both kernel boundaries, for the other parts' kernels of that boundary — an event per (part, boundary,
// iteration), waited for only after its owner has RECORDED it (`rec`: the producer's packet is then in front of the
// waiter's wherever the runtime maps the streams).
struct SplitGroup {
    int parts = 0;
    sw_ctx* ctx[SW_MAX_PARTS] = {nullptr};
    std::atomic<long long> rec[2][SW_MAX_PARTS];   // iterations whose band / tally event the part has recorded
    std::atomic<int> abort{0};                     // a part failed: the others stop waiting for it
    hipEvent_t ev[2][SW_MAX_PARTS][64] = {};
};

struct sw_ctx {
    // Every stream, event, device buffer and pinned buffer below is a member of an owning type (owned.h): ~sw_ctx gives them
    // back, in reverse order of declaration — so the streams come first and go last.  sw_destroy has drained the device.
    Stream stream;
    Stream stream_cs;    // can_see sweeps run here, ahead of the round loop
    Stream stream_aux;   // per-sub-batch finalize + voter masks run here, behind the round loop
    Stream stream_io;    // payload (timestamps, signatures) uploads of bulk appends
    Stream stream_ord;   // bulk find_order: the samples of group g run here beside the walk of group g + 1 ...
    Stream stream_srt[2];   // ... and its sort (one workgroup per round: ~0.2 ms whatever the number of rounds) and read-back here, groups alternating
    int n = 0, nw = 0, npad = 0, coin_period = 6, device = 0;
    SplitGroup* split = nullptr;   // linked with other contexts (sw_split_link)
    int split_part = 0;
    long long split_iter = 0;      // iterations of the round loop enqueued since the link
    bool split_failed = false;     // a meeting of the parts failed (a part gave up): the call reports it
    DBuf<SplitDst> d_split;        // device copies of the SplitDst the split kernels read: [0] this part's (linked), [q] part q's (SW_SPLIT_EMULATE)
    SplitDst split_up[SW_MAX_PARTS] = {};   // ... and what was uploaded last
    int split_saved[4] = {0, 0, 0, 0};   // tally choice of the context before the link pinned the one-wave-per-slot tally (restored by the unlink)
    int split_emulate = 0;         // SW_SPLIT_EMULATE (measurement): this many parts played by this one context, one behind the other
    VmTable vm;
    int64_t first_resident = 0;   // can_see rows below this event index have been evicted (windowed mode)
    int64_t window_lapse = 0;     // sw_set_window_lapse: a member silent for more than this many events no longer holds the window back (0 = never)
    std::vector<char> lapsed;     // ... and is marked here: its further events are refused (SW_ERANGE) until a rewind / reset
    bool vm_scratch_ok = false;   // windowed mode: the halo scratch rows behind row `cap` are mapped (the sweep may run in chunks)
    DBuf<int32_t> d_ordpos;       // per member: chain positions already ordered (find_order's search bound)
    // exact path for forked hashgraphs (exact.hip.h): entered at the first forked event, left by sw_reset
    bool exact = false;
    int forks_mode = 1;           // 1: accept forks (exact path), 0: refuse them (SW_ENOTSUP, nothing stored)
    // Its rewind is exact_rewind, not a member here: the tables are device state, refilled on the stream, and the one host
    // value, fc_base, is set there from the context's fc_seen.  sw_reset keeps the buffers for the next forked hashgraph.
    struct ExactState {
        DBuf<int32_t> worder, wcnt, newr, queue, fw, items_ev, rounds;
        DBuf<signed char> fam_ev, votes;
        DBuf<unsigned char> tbd, sm, done, visited, sflag, white;
        DBuf<double> times, tsort, items_ts;
        DBuf<long long> hdr;
        int Rcap = 0;               // rows of worder / wcnt / done / newr
        int64_t cap = 0;            // events of fam_ev / tbd / queue / visited / items_*
        FameCounters fc_base{};     // fame counters of the fast path at the switch (the exact path counts from zero)
    } ex;
    // what the exact path computes beyond the order, kept (sw_set_exact_history; exact_history.hip.h): round
    // received / consensus time into cons.d_rr / d_cts / d_tx, and Node.votes keyed by event in a log + index on the device
    struct HistoryState {
        bool on = false;              // the switch: set before the first event, kept by sw_reset
        bool votes_ok = true;         // false: the store is incomplete (overflow, KeyError, votes the fast path could not hand over) until sw_rewind / sw_reset
        const char* why = "";         // ... and the reason, for the message
        DBuf<int32_t> d_voter, d_cand, d_tab, d_items_rr, d_q;
        DBuf<signed char> d_value, d_qout;
        DBuf<long long> d_off;        // row offsets of an import
        int64_t count = 0;            // entries of the log (host copy of hdr[H_VCNT])
        int64_t cap = 0;              // entries the log has room for
        size_t slots = 0;             // slots of the index in use (a power of two >= 2 cap)
        int64_t cap0 = 4096;          // SW_VOTE_STORE_INIT (history_knobs): the first capacity
        int64_t ceiling = (int64_t)1 << 24;   // SW_VOTE_STORE_MAX (history_knobs): the most entries; beyond it votes become unavailable
        int64_t grows = 0, imported = 0, lookups = 0, exported = 0;   // sw_get_vote_store_stats (imported: the hand-over at the first fork)
        int64_t table_calls = -1, table_divided = -1;   // fork-free context: the decide_fame calls and divided events the store was filled from (-1: not filled)
        // sw_rewind: a store filled from the fast path's table is stale (no decide_fame call stands); on the exact path
        // exact_rewind empties the store on the stream.  sw_reset: nothing more — the switch and the buffers stay.
        void rewind() { table_calls = table_divided = -1; }
        void reset() {}
    } hist;
    bool unit_stake = true;
    uint32_t tot = 0;
    std::vector<uint32_t> stake_h;
    FameCounters fc_seen{};            // device fame counters already added to ctr
    std::vector<Event> cs_events;
    int pipe = 5;                       // sub-batches per divide_rounds call behind the short first one (pipelining depth)
    std::string err;

    // host mirror of the DAG (validation, height, chains)
    std::vector<int32_t> cr, sp, op, ht;
    std::vector<int32_t> head;      // latest event per member (-1 none)
    std::vector<int32_t> first_ev;  // first event (root) per member (-1 none)
    std::vector<int32_t> nev;       // events per member so far (next chain position)
    bool pool_h_valid = true;       // chain_ev_h mirrors the device pool (bulk appends invalidate it)
    bool poisoned = false;          // a HIP failure left the context half-updated: every later call fails
    Event ev_payload;               // the payload uploads of bulk appends (stream_io) are complete (find_order / coin bits wait for it)
    bool payload_pending = false;
    std::vector<int32_t> seq_h;     // chain position of every event (host mirror: small appends pack creator(op) | seq(op))
    Pinned<SmallRec> h_small;       // pinned staging of small appends (one packed record per event)
    Event ev_small;                 // ... and the completion of its last upload
    bool small_pending = false;
    Pinned<char> h_pin;             // pinned staging of bulk appends
    int max_height = 0;
    int64_t N = 0, cap = 0, divided = 0;
    // device-side ingest (sw_append_events_device; ingest.hip.h)
    struct IngestState {
        DBuf<int32_t> d_tab;          // [4 + 3 npad]: verdict word (64 bits), pad; then [nev | head | first] of the members
        DBuf<int32_t> d_hist;         // [tiles][npad] creators per tile, then chain position of each member at the head of each tile
        DBuf<int32_t> d_ht_stat;      // k_ingest_heights: [error, largest height, {min, max} per 4096-event block of the batch]
        std::vector<int32_t> stage;   // host staging of d_tab (persistent: uploaded and read back without a copy of a local)
        Event ev_ht;                  // the heights kernel of the last device append (it runs on stream_io, behind the call)
        bool ht_pending = false;      // ... has not been waited for yet: d_ht, max_height, blk_hmin / blk_hmax lack its events
        int64_t ht_first = 0, ht_K = 0;   // ... which are these
        int64_t ht_dev_upto = 0;      // events below this index and beyond the host mirror (sp.size()) have their height in d_ht
        int64_t dev_batches = 0, dev_events = 0, fallback = 0, host_ht = 0;   // sw_get_ingest_stats
        // sw_rewind keeps it (the events and their heights stay); sw_reset, which has drained stream_io, forgets the heights
        void rewind() {}
        void reset() { ht_pending = false; ht_dev_upto = 0; }
    } ing;
    // id index (sw_set_event_ids, sw_ingest_payload[_device]; resolve.hip.h): allocated on first use
    struct IdState {
        DBuf<unsigned char> d_id;     // 32 B per event that has an id, in dense order
        DBuf<int32_t> d_idtab;        // id -> dense index: 1 << idtab_log slots, load <= 1/2, rebuilt from d_id when it grows
        int idtab_log = 0;            // (0: no table yet)
        int64_t n_ids = 0;            // events [0, n_ids) have ids; the index is COMPLETE when n_ids == N
        DBuf<int32_t> d_idflag;       // [4] duplicate flag of an insert
        DBuf<unsigned char> d_pl;     // scratch of a payload call
        DBuf<unsigned char> d_pl_in;  // ... and the staged arrays of the host-array forms
        Pinned<int32_t> h_plcnt;      // pinned: per-wave counts of one batch of waves
        int64_t pl_calls = 0, pl_waves = 0, pl_accepted = 0, pl_rebuilds = 0;   // sw_get_payload_stats (waves, accepted: the last call's)
        double pl_ms[4] = {0, 0, 0, 0};   // ... host time of its phases under sw_set_profiling: resolve, waves, sort + gather, append + commit
        // sw_rewind keeps it (the events stay); sw_reset forgets it: the ids go with the events — the table keeps its size,
        // and sw_reset empties it on the stream
        void rewind() {}
        void reset() { n_ids = 0; }
    } ids;
    // answering a sync on the device (sw_export_payload[_device], sw_sync_pull; gossip.hip.h): scratch, a knob and counters
    // that sw_rewind / sw_reset leave alone
    struct ExportState {
        DBuf<int32_t> d;              // [2: the total, 64 bits][npad + 1: offsets of the members' ranges][npad: chain pool base per member]
        DBuf<unsigned char> d_out;    // the exported arrays of the host-array form and of sw_sync_pull
        int64_t calls = 0, events = 0;   // sw_get_export_stats
        double ms[2] = {0, 0};        // ... host time of the most recent call's phases under sw_set_profiling: ranges + count, gather
        int lanes = 16;               // SW_EXPORT_LANES (measurement knob, read at sw_create): lanes of a wave that share one output slot — 4, 8 or 16
    } xp;
    // Node.votes in bulk (csrc/votes.hip.h; sw_export_votes[_device])
    struct VotesState {
        DBuf<unsigned char> d_sched, d_plan, d_work, d_out;   // call schedule, per-call plan, scratch, the host form's table
        int sched_calls = -1;               // number of decide_fame calls d_sched holds (-1: stale)
        std::vector<unsigned char> sched_stage, plan_stage;   // persistent host staging: uploaded without a sync
        DBuf<unsigned long long> d_cnt;     // vts::C_WORDS counters: rows and entries of the running call, levels replayed since sw_create
        int64_t calls = 0, rows = 0, entries = 0;             // sw_get_votes_stats
        double ms[2] = {0, 0};              // ... under sw_set_profiling: plan + existence + count, rows + values
        // sw_rewind: no decide_fame call stands, the schedule is stale; sw_reset: nothing more
        void rewind() { sched_calls = -1; }
        void reset() {}
    } votes;
    // answering a sync by the pruned walk, forked hashgraphs included (sw_sync_walk, sw_export_walk[_device], sw_sync_pull_walk,
    // sw_get_fork_trunks; walk.hip.h)
    struct WalkState {
        DBuf<int32_t> d;              // [wlk::H_WORDS: the header][npad: the asker's heights][npad: the cap]
        DBuf<unsigned> d_bits;        // the visited bitmap: head + 1 bits
        DBuf<int32_t> d_q;            // the queue of the frontiers: head + 1 entries
        DBuf<int32_t> d_list;         // the ascending list: head + 1 entries
        DBuf<int32_t> d_trunk;        // [npad: trunk per member][npad: roots per member], as of trunk_N events
        DBuf<int32_t> d_children;     // children per self-parent (scratch of k_fork_trunks)
        int64_t trunk_N = -1;         // events d_trunk was computed from (-1: never)
        int threads = 1024;           // SW_WALK_THREADS (read at sw_create): workgroup size of k_walk_bfs, a multiple of 64 up to 1024
        int64_t calls = 0, events = 0, levels = 0;   // sw_get_walk_stats (levels: the last call's)
        double ms[3] = {0, 0, 0};     // ... host time of the most recent call's phases under sw_set_profiling: walk + count, list, gather
        // sw_rewind keeps the trunks (the events stay); sw_reset forgets them: the trunk heights were those of the forgotten events
        void rewind() {}
        void reset() { trunk_N = -1; }
    } walk;
    // what find_order decided per event, kept (sw_get_round_received, sw_get_consensus_time, sw_export_ordered[_device];
    // consensus.hip.h): allocated by the first find_order call that orders something
    struct ConsensusState {
        DBuf<int32_t> d_rr;           // per event: round received (swirld.py:283); entries of events that are not ordered are unspecified
        DBuf<double> d_cts;           // per event: consensus timestamp (swirld.py:305); likewise
        DBuf<int32_t> d_tx;           // device copy of `transactions` ...
        int64_t tx_len = 0;           // ... and its length
        DBuf<int32_t> d_ordpos;       // npad: the ordered prefixes as of now, uploaded by a getter (sw_ctx::d_ordpos holds those at the head of the last call)
        DBuf<unsigned char> d_out;    // the arrays of the host-array forms
        int64_t record_calls = 0, recorded = 0, export_calls = 0, exported = 0;   // sw_get_consensus_stats
        // sw_rewind: nothing is ordered any more (d_rr / d_cts need nothing: no event is inside an ordered prefix); sw_reset:
        // nothing more
        void rewind() { tx_len = 0; }
        void reset() {}
    } cons;
    // validation of payloads against the member keys (sw_set_member_keys, sw_validate_payload[_device]; validate.hip.h):
    // nothing here belongs to the hashgraph, so sw_rewind / sw_reset leave it alone
    struct ValidateState {
        std::vector<uint8_t> keys, usable;   // host copies: n x 32 key bytes, n flags (empty: no keys set)
        DBuf<unsigned char> d_keys;   // [n x 32 key bytes][n usable flags]
        DBuf<unsigned char> d_tab;    // (n + 1) rows of swv::ROW entries: the members' multiples of -A, then the base point's
        DBuf<unsigned char> d_in;     // the staged arrays of the host-array form
        int64_t calls = 0, events = 0, accepted = 0, builds = 0;   // sw_get_validate_stats
        double ms[2] = {0, 0};        // ... host time under sw_set_profiling: the last table build, the last validation
    } val;
    // the signed bytes of events built on the device (sw_pack_events[_device], sw_sync_pull_validated; pack.hip.h): like the
    // keys, a setting and scratch that sw_rewind / sw_reset leave alone
    struct PackState {
        std::string mod = "swirld", qual = "Event";   // module and qualified name of the Event class (sw_set_event_class)
        bool hdr_stale = true;        // d_hdr does not hold the class header of mod / qual yet
        std::vector<uint8_t> hdr;     // host copy of the header as uploaded (it must outlive the asynchronous copy)
        DBuf<unsigned char> d_hdr;    // the class header of the whole stream (pck::HDR_MAX bytes)
        DBuf<unsigned char> d;        // tile sums of the scan
        DBuf<unsigned char> d_in;     // the staged arrays and streams of the host-array form
        DBuf<unsigned char> d_out;    // sw_sync_pull_validated: offsets, streams, flags, verdicts, the count
        Pinned<int32_t> h_cnt;        // pinned: the count of valid events of sw_sync_pull_validated
        int64_t calls = 0, events = 0, bytes = 0;   // sw_get_pack_stats
        double ms[2] = {0, 0};        // ... host time under sw_set_profiling: lengths and scan, the two writers
    } pack;
    // the data of events (sw_set_event_data[_device], sw_gather_event_data[_device], sw_ingest_payload_data[_device],
    // sw_sync_pull_data; data.hip.h): allocated on first use
    struct DataState {
        DBuf<unsigned char> d_arena;  // the arena: 256-byte aligned, at least dat::SLACK readable bytes behind `used`
        DBuf<long long> d_off;        // [n_data + 1] absolute offsets into the arena, contiguous; [0] = 0
        DBuf<unsigned char> d_none;   // per event that has data: nonzero = None
        int64_t n_data = 0;           // events [0, n_data) have data; the store is COMPLETE when n_data == N
        int64_t used = 0;             // bytes of the arena in use
        DBuf<unsigned char> d;        // scratch of a call: scanned offsets + the bad-slot count, none flags, tile sums, slots, folded ok
        DBuf<unsigned char> d_in;     // the staged arrays of the host-array forms
        DBuf<unsigned char> d_out;    // the gathered data: of the host-array gather, and of sw_sync_pull_data's exported events (in the answering context)
        int64_t store_calls = 0, gather_calls = 0, gather_bytes = 0;   // sw_get_data_stats
        double ms[2] = {0, 0};        // ... host time under sw_set_profiling: lengths + scan, the copy
        // sw_rewind keeps it (the events stay); sw_reset forgets it: the data goes with the events (the arena keeps its size)
        void rewind() {}
        void reset() { n_data = 0; used = 0; }
    } data;
    // the wire bytes of a sync answer (sw_pack_message[_device], sw_unpack_message[_device], sw_export_message[_device],
    // sw_ingest_message[_device]; wire.hip.h): settings derived from the event class and the member keys, and scratch —
    // like those, left alone by sw_rewind / sw_reset
    struct WireState {
        std::string mod, qual;        // the class d_set's prefix was built for (empty: none yet)
        std::vector<uint8_t> pre;     // host copy of the bytes in front of the table's length field, as uploaded
        std::vector<uint8_t> keys, skeys;   // the member keys the sorted table was built from; the sorted keys as uploaded
        std::vector<int32_t> sperm;         // ... and the member each belongs to
        DBuf<unsigned char> d_set;    // [wir::PRE_MAX prefix][n x 32 sorted keys][n members][8 words: K, refusal flag, verdict, data bytes, length]
        DBuf<unsigned char> d;        // scratch of a call: record offsets, tile sums, the first unencodable event; data positions
        DBuf<unsigned char> d_in;     // the staged arrays and the message of the host-array forms
        DBuf<unsigned char> d_out;    // the message of sw_export_message; the unpacked arrays of sw_ingest_message
        int blocks = 4096;            // SW_WIRE_BLOCKS (measurement and test knob, read at sw_create): the most workgroups of k_wire_write
        int64_t pack_calls = 0, pack_events = 0, pack_bytes = 0, unpack_calls = 0, unpack_events = 0, refused = 0;   // sw_get_wire_stats
    } wire;
    // creating signed events (sw_set_signing_keys, sw_sign_events[_device], sw_create_events[_device]; sign.hip.h): like the
    // member keys a setting that sw_rewind / sw_reset leave alone; sw_set_member_keys drops it
    struct SignState {
        std::vector<uint8_t> has;     // n flags: the members this context may sign for (empty: no signing key set)
        DBuf<unsigned char> d_keys;   // [n secrets of 64 B][n flags]: the ONLY copy of the secrets, never read back
        DBuf<unsigned char> d;        // scratch of a call: verdict block, levels, level counts and offsets, cursors, sorted events
        DBuf<unsigned char> d_in;     // the staged arrays of the host-array forms; the signed arrays of sw_create_events
        int64_t calls = 0, events = 0, levels = 0, keysets = 0;   // sw_get_sign_stats (levels: the last call's)
        double ms[3] = {0, 0, 0};     // ... host time under sw_set_profiling: levels + sort, signing, commit
    } sign;
    // one event signed by one wavefront, and the gossip turn around it (sw_create_event, sw_gossip_turn; turn.hip.h): counters
    // that sw_rewind / sw_reset leave alone
    struct TurnState {
        int64_t calls = 0, events = 0, turns = 0, profiled = 0;   // sw_get_turn_stats: sw_create_event calls, events the wave signed, turns, stamped launches
        unsigned long long stamps[8] = {0};   // wall_clock64() at the phase boundaries of the last stamped launch (swt::ST_COUNT)
    } turn;

    // device: events
    DBuf<int32_t> d_cr, d_sp, d_op, d_ht, d_seq, d_round, d_L, d_chain_ev;
    DBuf<unsigned char> d_coin, d_sig;
    DBuf<double> d_t;
    DBuf<u64> d_S;
    DBuf<int32_t> d_finlist;   // events k_finalize_check found without a round from the band pass (one entry per event at most)
    DBuf<unsigned> d_fin;      // [0] length of that list for the launch in flight, [2..3] running total (u64)
    DBuf<int32_t> d_chain_start;  // npad: offset of each member's segment in the chain pool
    DBuf<int32_t> d_chain_cnt;    // npad: events per member (segments have slack: geometric growth)
    DBuf<int4> d_cdesc;           // pool-indexed chain descriptors of the dataflow can_see sweep (same indexing as chain_ev)
    DBuf<int32_t> d_bounds;       // [cuts][npad] chain positions of the sub-batch cuts of the running divide_rounds call
    DBuf<long long> d_cuts;
    // chunk-parallel can_see sweep (k_cansee_chunks): per chunked sub-batch 2G + 2 rows of chain positions
    // {w_0, a_0, w_1, a_1, ..., end, end}, the halo rows' scratch table, provisional-entry counters (inside d_rb)
    DBuf<int32_t> d_cbnd;
    DBuf<long long> d_ccuts;
    int chunks = 4;               // SW_CHUNKS: chunks swept concurrently per sub-batch (1 = the unchunked k_cansee_flow)
    int chunk_cfg = 0;            // SW_CHUNK_CFG: 0 = 4 columns per lane, FIFO 8, ring 8; 1 = 2 columns, 8 / 16; 2 = 4 columns, 4 / 8
    int64_t halo = 0;             // SW_HALO: events recomputed in front of a chunk (default 32 x npad: ~2.4x the age of a row's oldest entry at uniform gossip)
    int64_t chunk_min = 8192;     // SW_CHUNK_MIN: smallest chunk worth a halo (round 5: 16384 -> 8192, the short first sub-batch — the one sweep nothing hides — goes out as 4 chunks instead of 3: 6.03 -> 5.98 ms, profiles/r05n_knobs_256x1M.log)
    bool chunks_off = false;      // set when a call had to sweep chunks twice (members silent for longer than the halo): unchunked from then on
    struct ChunkPlan { int G = 0; int row0 = 0; int64_t a[SW_MAX_CHUNKS + 1]; int64_t w[SW_MAX_CHUNKS]; };
    std::vector<ChunkPlan> chunk_plan;   // per sub-batch of the running call
    std::vector<long long> ccuts_stage;  // host staging of the chunk cuts (persistent: uploaded without a sync)
    // multi-GPU split of the can_see table by event ranges (sw_cansee_range / sw_import_rows): the ranges swept here,
    // the rows present in the table without having been divided yet, their cut tables and counters
    struct RangeRec { int64_t first = 0, K = 0; ChunkPlan pl; int row0 = 0; int slot = 0; bool repaired = false; };
    std::vector<RangeRec> ranges;
    std::vector<std::pair<int64_t, int64_t>> present;   // [a, b) rows present, sorted, merged
    DBuf<int32_t> d_rbnd;
    DBuf<long long> d_rcuts;
    std::vector<long long> rcuts_stage;
    DBuf<unsigned> d_rprov;           // [SW_RANGE_SLOTS][SW_MAX_CHUNKS + 1]: provisional entries per chunk, repaired entries
    Event ev_user;                    // between a caller's stream and ours (UserStream), and between two contexts: made on first use
    std::vector<int32_t> chain_cap;   // per member: capacity of its segment
    int64_t pool_used = 0;             // ints of the chain pool handed out
    DBuf<int32_t> d_chain_len;    // [3][npad]: events per member visible to the running round loop, by iteration parity (the gated
                                  // loop's grow), then at the end of the call
    std::vector<int32_t> blk_hmin, blk_hmax;  // height span per 4096-event block (ingest-time index)
    std::vector<int32_t> divided_head;
    DBuf<uint32_t> d_stake;       // npad

    // device: levels
    DBuf<int32_t> d_lev_cnt, d_lev_start, d_lev_cursor;
    DBuf<int32_t> d_lev_cback, d_lev_pinbase, d_lev_pos;   // level sweep: the back cursors, pinned events in front of each level, descriptor position per event
    DBuf<uint8_t> d_lev_pin;     // level sweep: events whose row slice a child looks for after it has left the ring (k_level_hist)
    DBuf<int4> d_desc;

    // device: rounds
    int Rcap = 0;  // rows allocated in lo/lopos/wit/fam/cons/newc
    int R = 0;     // max round + 1
    DBuf<int32_t> d_lo, d_lopos, d_wit;
    DBuf<signed char> d_fam;
    DBuf<int32_t> d_dec_call, d_dec_by;  // per witness slot: the decide_fame() call that decided it and the deciding voter (Node.votes bookkeeping)
    struct FameCall { int max_c, R; int64_t divided; };
    std::vector<FameCall> fame_calls;    // one record per decide_fame() call
    bool votes_partial = false;          // a partitioned commit left dec_call / dec_by of other parts' witnesses unset: no Node.votes
    std::vector<int32_t> cons_call;      // per round: the call that added it to `consensus` (-1: not yet)
    DBuf<unsigned char> d_cons, d_newc;
    DBuf<u64> d_Sw;
    int Sw_rows = 0;
    bool debug_timing = false;   // SW_DEBUG_TIMING=1
    double stage_us[8] = {0};    // sw_divide_rounds host stages: sweeps enqueued, loop set-up, round loop, front rows, aux launches, final syncs
    int64_t stage_calls = 0;
    DBuf<unsigned long long> d_dbg;       // SW_DEBUG_CLOCKS=1: phase stamps of the round-loop kernels
    DBuf<unsigned long long> d_dbg_blk;        // SW_DEBUG_CLOCKS=3: end time of every workgroup of the loop kernels, per iteration
    int64_t dbg_iter_base = 0;            // round_iterations at the last rewind: the phase stamps are indexed by the iterations since
    int dbg_minor = 1;                    // SW_DEBUG_CLOCKS=2: only the entry / band start / end stamps (the others drain the wave)
    DBuf<unsigned char> d_small;   // device copy of the packed records of the current small append
    Event ev_aux_done, ev_cs_done, ev_main_mark, ev_bounds, ev_loop_done;   // (ev_bounds: made on first use)
    std::vector<int32_t> divided_cnt;   // per member: events already divided (chain positions below `divided`)
    std::vector<int32_t> bounds_stage;  // host staging of the cut table (persistent: uploaded without a sync)
    DBuf<int32_t> d_evalround, d_evalpos, d_lo_r, d_cur, d_unres, d_lo_next, d_pos_next, d_farslot, d_force, d_cand, d_gallop;
    DBuf<u64> d_Mb;
    DBuf<int32_t> d_Pc;    // [MCAP + 1] popcounts of the band masks (row 0 = 0, like d_Mb): the cheap bounds of k_tally_bits<., FILT>.
                           // INVARIANT: whoever writes a row of d_Mb writes its popcount here (k_resolve_band's band pass is the only writer of both,
                           // in its plain and its split form): a `sure` verdict of the filtered tally never looks at the mask itself
    DBuf<int32_t> d_rsc;   // [R][3] round-level agreement of k_elections_tiled: open witnesses, decided flag, arrival ticket
    DBuf<u64> d_found64;   // [2][npad] {event << 32 | slot << 26 | look-ahead} of the members' first passing candidates (LoopBufs::found64)
    // one device block read back with ONE copy per round-loop shot: loop state (x2), sweep error flag, per-member
    // front rounds; and its pinned host mirror
    DBuf<unsigned char> d_rb;
    Pinned<unsigned char> h_rb_all;       // SW_PROV_ROWS pinned slots: the loops of a call's sub-batches are read back one behind the other
    std::vector<Event> rb_events;        // per slot: read-back complete
    // pointers INTO another allocation (nothing to free): the pieces of d_rb, the header of d_newc, a slot of h_rb_all
    RState* d_state = nullptr;
    int* d_flow_err = nullptr;            // set by k_cansee_flow when a polling loop gives up (protocol bug)
    struct { int32_t* p = nullptr; } d_front;   // the members' front rounds
    int32_t* d_treecnt = nullptr;         // tallies evaluated per member in the running loop (k_tally_tree)
    unsigned* d_prov = nullptr;           // [SW_PROV_ROWS][SW_MAX_CHUNKS] provisional entries per chunk of the chunk-parallel sweep, then [SW_PROV_ROWS] repaired entries
    FameCounters* d_fc = nullptr;         // header of d_newc: the fame counters travel with the new_c flags in one copy
    unsigned char* h_rb = nullptr;        // the read-back slot that was read last
    int gate_lag = 0, gate_step = 1;   // SW_GATE_LAG / SW_GATE_STEP (test hook): the gated loop's stages published by the host, `gate_step` more every `gate_lag` iterations (0: by the sweep stream)
    int gated = 1;   // SW_GATED: one round loop per large call, gated on the device by the sweep's progress (0: one loop per sub-batch)
    int shot_pct = 100, shot_extra = 2;   // SW_SHOT_PCT / SW_SHOT_EXTRA: a loop's first shot = predicted iterations x pct / 100 + extra (tests: 50 makes every loop top up)
    size_t rb_bytes = 0;
    Pinned<unsigned char> h_fame;     // pinned: [FameCounters][newc flags]
    std::vector<int32_t> front;       // per member: max r with lo[r][c] finite (-1 none); the device keeps it (d_front), the host mirror follows
    std::vector<int32_t> front_dev;   // read-back buffer of d_front
    std::vector<int32_t> lo0_h;       // host copy of lo[0][.] (chain starts)
    std::vector<unsigned char> cons_h;  // host mirror of consensus
    int sw_dirty_from = 1;            // voter masks of rounds >= this must be (re)built

    // tuning
    int skip = 1;         // SW_SKIP: window offset of a fresh round (0 = off); 1 measured best at 256 members (310 vs 326 iterations)
    int gallop_after = 2; // SW_GALLOP: strided candidate windows after this many windows without a passing candidate (0 = never); 2 costs uniform gossip nothing (the first window passes there) and cuts hot-member hashgraphs from 2756 to ~200 iterations
    int elect_impl = 1; // 1: NW threads per candidate (k_elections_tiled, 128 members and more), 0: one thread per candidate
    int elect_cg = 128; // SW_ELECT_CG (256 members): candidates per workgroup of k_elections_tiled — 64, 128 or 256
    int K = 28;        // candidates per member per tally launch: 7 waves per SIMD (the 8th slot is
                       // taken by the concurrent can_see sweep; 29+ costs a second wave generation)
    int MCAP = 0;      // largest band (events) the mask table can hold
    int NEARCAP = 0;   // band cap at round entry (doubles up to MCAP when a far candidate needs a tally)
    int BATCH = 24;    // loop iterations between host checks
    int cansee_impl = 6;  // 6 = dataflow sweep (no levels, no barriers: k_cansee_chunks / k_cansee_flow); 2 / 3 = level-bucketed sweep (k_cansee_stream: the default beyond 256 members; one kernel since round 6, both values select it)
    int ring_H_req = 0;   // SW_RING_H override (0 = automatic)
    int flow_cfg = 1;     // SW_FLOW_CFG: FIFO / ring depths of the dataflow sweep: 0 = 16/32, 1 = 8/16, 2 = 16/16, 3 = 8/32
    int tally_impl = 1;   // 0 = column-lane tally, 1 = bit-sliced, one wave per slot (unit stake only), 2 = bit-sliced two-level search (k_tally_tree)
    bool tally_auto = true;   // SW_TALLY_IMPL not set: large calls of ~256-member hashgraphs without strongly skewed activity use 2
    bool K_auto = true;       // SW_TALLY_K not set: 28 slots for the flat tally, 32 for the tree
    int K_flat = 28;
    int eval_src = 0;      // which half of d_evalround / d_evalpos the last round-loop run left the members' exhaustion marks in
    int band_blocks = 512; // workgroups of the resolve+band kernel
    int fin_blocks = 1024; // SW_FIN_BLOCKS: workgroups of a k_finalize_events launch that runs beside a round loop (profiles/r04q_*: 8192 of them
                           // slow the loop's gathers down; 1024 with the early finalize below: 7.30 -> 7.16 ms per pass at 256 x 1 M, 69.7 -> 66.9 ms at 10 M)
    int mid_pct = 0;       // SW_MID_PCT: where the last sub-batch's round loop is interrupted once for an early finalize (0 = never: with
                           // SW_FIN_BAND=1 there is nothing left to hide; 88 was the default of the row-reading finalize)
    int fin_band = 1;      // SW_FIN_BAND: round[] and the sees-masks come from the round loop's band pass, the finalize launch only checks (1) / every event from its row (0)
    int band_fast = 1;     // SW_BAND_FAST: k_resolve_band takes full groups of 8 band events through a path with fixed indices and compile-time offsets
                           // (round 5, profiles/r05a_*: band phase 2.66 -> 1.90 us, 7.00 -> 6.72 ms per pass at 256 members / 1 M events; 0 = the generic path only)
    int tally_filter = 0;  // SW_TALLY_FILTER: the one-wave-per-slot tally bounds a verdict by the popcounts of the hop masks before it gathers the masks
                           // (round 5, profiles/r05e_*: default beyond 256 members, where the tally is bound by the bytes it gathers — 1024 members / 2 M
                           // events 34.8 -> 32.7 ms, 57.4 -> 61.2 M events/s; at 256 members the one-wave-per-slot kernel is bound by its 8 192 wave launches,
                           // with or without the gathers: 6.58 -> 6.34 ms, the two-level search 6.08)
    int tally_pf = 1;      // SW_TALLY_PF: the first waves of every XCD touch the band-mask table at the head of k_tally_bits (+1 %)

    // round-loop graph
    struct GraphKey { int Rcap; int64_t N; void* lo; void* L; void* chain; void* S; void* round; int K, tally_impl, BATCH, MCAP, variant; };
    bool use_graph = true;
    hipGraph_t loop_graph[4] = {nullptr, nullptr, nullptr, nullptr};
    hipGraphExec_t loop_exec[4] = {nullptr, nullptr, nullptr, nullptr};
    int graph_big = 64;    // SW_GRAPH_BIG: iterations of the largest replayable graph (0 = none beyond 24).  Every graph boundary costs
                           // the loop ≈ 8 us (profiles/r04y_loop_phases_256x1M.txt: iterations 23, 47, 71, ... are the slow ones)
    GraphKey loop_key{};
    int64_t stat_iters = 0, stat_events = 0;  // iterations-per-event history (first-shot sizing)
    // iterations-per-event history of the gated loop, kept apart from the per-sub-batch loops' (first-shot sizing).  It counts
    // the iterations that waited for the sweep too: the first shot has to cover them, or the call ends on host top-ups.
    int64_t gstat_iters = 0, gstat_events = 0;

    // profiling
    bool profiling = false;
    sw_timings tm{};
    sw_counters ctr{};
    std::vector<Event> ev_pool;
    size_t ev_used = 0;
    // find_order state (swirld.py:53-57): ordered events are a prefix of every member's chain
    PinnedVec transactions;
    std::vector<int32_t> ord_pos;            // per member: chain positions already ordered
    std::vector<unsigned char> sig_h;        // host copy of the signatures (whitening, sort key)
    std::vector<int32_t> chain_start_h, chain_ev_h;
    DBuf<int32_t> d_q, d_acc_ev, d_acc_ri, d_sorted, d_hostflag;
    // find_order, tables of a call (order.hip.h): the rounds asked for, f_w per entry as a member-indexed row, ordered prefixes per entry,
    // [start | length | offset] of the newly ordered chain segments per (entry, member), events per entry, the block that is read back
    // ([OrderInfo][new ordered prefixes: npad][acc_off: entries + 1]), per-group tables of the bulk kernels
    DBuf<int32_t> d_ord_rounds, d_fwm, d_ordat, d_rowsum, d_grp;
    DBuf<long long> d_oblk;
    Pinned<char> h_ord;              // pinned staging of a find_order call (rounds and ordered prefixes up, the block and the host-sort flags down)
    std::vector<Event> ord_events;   // bulk find_order, per group: table walked / table consumed; then the ends of the three side streams (stream_ord, stream_srt)
    Pinned<int32_t> h_ord_stage;     // pinned: the [i0, i1) round-entry bounds of the groups of a bulk call
    DBuf<int32_t> d_big_ri, d_sk_ev;     // find_order: rounds too large for the LDS sort and their scratch keys (k_order_sort_big)
    DBuf<long long> d_big_off;
    DBuf<double> d_sk_ts;
    DBuf<u64> d_sk_k8;
    DBuf<int32_t> d_seg;
    DBuf<int32_t> d_fd;    // bulk find_order: first-descendant table of one group of round entries, [member][chain][position] (k_order_walk)
    DBuf<unsigned char> d_white;
    DBuf<double> d_ts;
    DBuf<double> d_tch;    // bulk find_order: timestamps in chain-pool order (k_order_tchain)
    DBuf<int> d_err;
    DBuf<u64> d_flow_dbg;        // SW_DEBUG_TIMING: counters of the dataflow sweep (column 0)
};

namespace {

int fail(sw_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

#define HIPCHK(c, expr)                                                                  \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return fail(c, SW_EIO, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                             \
    } while (0)

#define CHK(expr)                 \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != SW_OK) return rc_; \
    } while (0)

// ... and behind the commit point of an append: from there on a failure leaves the context half-updated, so it is poisoned
#define PCHK(expr) do { int rc_ = (expr); if (rc_ != SW_OK) { c->poisoned = true; return rc_; } } while (0)
#define PHIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { c->poisoned = true; \
        return fail(c, SW_EIO, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } } while (0)

// debugging aid (SW_POISON=<byte>): fresh device memory is filled with that byte, so that a read of
// memory no kernel has written shows up in any test instead of depending on what the heap held before
int poison_byte() {
    static const int v = [] { const char* e = getenv("SW_POISON"); return e && *e ? (int)(strtol(e, nullptr, 0) & 0xff) : -1; }();
    return v;
}
void poison(void* p, size_t bytes) {
    if (poison_byte() >= 0 && p && bytes) { (void)hipMemset(p, poison_byte(), bytes); (void)hipDeviceSynchronize(); }
}

// grow a device buffer to >= need elements, preserving the first `keep` elements
template <class T>
int dgrow(sw_ctx* c, DBuf<T>& b, size_t need, size_t keep) {
    if (need <= b.cap) return SW_OK;
    size_t nc = b.cap ? b.cap : 1;
    while (nc < need) nc = nc + nc / 2 + 64;
    if (b.cap == 0) nc = need;  // first allocation: exact (reserve() gives the final size)
    T* q = nullptr;
    hipError_t e = hipMalloc((void**)&q, nc * sizeof(T));
    if (e != hipSuccess) return fail(c, SW_ENOMEM, "hipMalloc(%zu bytes) failed: %s", nc * sizeof(T), hipGetErrorString(e));
    poison(q, nc * sizeof(T));
    if (b.p) {
        // the old buffer may still be in use on any of the context's streams (calls return without a
        // host synchronisation): drain the device before it is copied and freed — reallocation is rare
        HIPCHK(c, hipDeviceSynchronize());
        if (keep) {
            const hipError_t ec = hipMemcpy(q, b.p, keep * sizeof(T), hipMemcpyDeviceToDevice);
            if (ec != hipSuccess) { (void)hipFree(q); return fail(c, SW_EIO, "hipMemcpy into a grown buffer failed: %s", hipGetErrorString(ec)); }
        }
    }
    b.adopt(q, nc);   // (frees the old block)
    return SW_OK;
}

// an event made on first use
int ensure_event(sw_ctx* c, Event& e) {
    HIPCHK(c, (hipError_t)e.ensure(hipEventDisableTiming));
    return SW_OK;
}

// ---- the entry protocol of the call forms (entry_plan.h) --------------------------------------------------------
using entry::Arg;
using entry::Carve;
using entry::Stage;

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// device memory of the context's device?  (For plain host memory the query itself fails on ROCm: that is the answer,
// and the error is cleared so that it does not surface in a later check.)
bool on_ctx_device(const sw_ctx* c, const void* p, size_t bytes) {
    const char* ends[2] = {(const char*)p, (const char*)p + (bytes ? bytes - 1 : 0)};
    for (const char* q : ends) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, q) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (at.type != hipMemoryTypeDevice || at.device != c->device) return false;
    }
    return true;
}

int misaligned(sw_ctx* c, const char* what, unsigned align) {
    return fail(c, SW_EINVAL, "%s: an array that must be %u-byte aligned is not (ids, signatures and byte streams 16, offsets and timestamps 8, indices 4)",
                what, align);
}

// The arrays of a device-array form, behind the form's *_pre checks: alignment, the context's device made current, residency.
// A row that is NULL or empty is skipped (entry_plan.h).
int device_args(sw_ctx* c, const char* what, std::initializer_list<Arg> rows) {
    const int bad = entry::first_misaligned(rows.begin(), (int)rows.size());
    if (bad >= 0) return misaligned(c, what, rows.begin()[bad].align);
    HIPCHK(c, hipSetDevice(c->device));
    for (const Arg& a : rows)
        if (!entry::skipped(a) && !on_ctx_device(c, a.p, a.bytes))
            return fail(c, SW_EINVAL, "%s: every array must lie in memory of device %d (a host pointer, or another device's)", what, c->device);
    return SW_OK;
}

// A call between the caller's stream and one of ours: join() puts our stream behind what the caller has enqueued (the producers
// of its arrays, earlier readers of its outputs); leave() puts the caller's stream behind what the call enqueued, so that
// whatever it enqueues next reads complete arrays and may reuse its own.  A call that returns between the two, for whatever
// reason, hands the caller's stream back all the same (the destructor, errors ignored and cleared: the call's own error stands).
struct UserStream {
    sw_ctx* c = nullptr;
    hipStream_t user = nullptr, ours = nullptr;
    bool joined = false;
    int join(sw_ctx* ctx, hipStream_t user_stream, hipStream_t our_stream = nullptr) {
        c = ctx;
        user = user_stream;
        ours = our_stream ? our_stream : ctx->stream;
        CHK(ensure_event(c, c->ev_user));
        HIPCHK(c, hipEventRecord(c->ev_user, user));
        HIPCHK(c, hipStreamWaitEvent(ours, c->ev_user, 0));
        joined = true;
        return SW_OK;
    }
    int leave() {
        joined = false;
        HIPCHK(c, hipEventRecord(c->ev_user, ours));
        HIPCHK(c, hipStreamWaitEvent(user, c->ev_user, 0));
        return SW_OK;
    }
    void drained() { joined = false; }   // our stream has been synchronised: there is nothing left to wait for
    ~UserStream() {
        if (joined && (hipEventRecord(c->ev_user, ours) != hipSuccess || hipStreamWaitEvent(user, c->ev_user, 0) != hipSuccess)) (void)hipGetLastError();
    }
};

// The staging buffer of a host-array form, grown to the plan, and the uploads on the context's stream ...
int stage_up(sw_ctx* c, DBuf<unsigned char>& buf, const Stage& st, unsigned char** base) {
    if (st.full) return fail(c, SW_EIO, "a staging plan of more than %d copies (internal error)", Stage::MAX_ROWS);
    CHK(dgrow(c, buf, st.total() + 256, 0));
    *base = buf.p;
    for (int i = 0; i < st.n_up; ++i)
        HIPCHK(c, hipMemcpyAsync(buf.p + st.up[i].off, st.up[i].src, st.up[i].bytes, hipMemcpyHostToDevice, c->stream));
    return SW_OK;
}
// ... and the downloads with the ONE synchronisation behind them.  A row is brought back once: a second call brings what has
// been sized (Stage::out_bytes) since the first.
int stage_down(sw_ctx* c, Stage& st, const unsigned char* base) {
    for (int i = 0; i < st.n_down; ++i) {
        Stage::Copy& d = st.down[i];
        if (d.bytes) HIPCHK(c, hipMemcpyAsync(d.dst, base + d.off, d.bytes, hipMemcpyDeviceToHost, c->stream));
        d.bytes = 0;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

int fill_i32(sw_ctx* c, int32_t* p, size_t n, int v) {
    if (!n) return SW_OK;
    int blocks = (int)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_fill_i32, dim3(blocks), dim3(256), 0, c->stream, p, n, v);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    return SW_OK;
}

// ---- windowed can_see table (VmTable) ----------------------------------------------------------
int vm_map_slot(sw_ctx* c, size_t slot) {
    VmTable& v = c->vm;
    if (v.mapped[slot]) return SW_OK;
    hipMemGenericAllocationHandle_t h;
    if (!v.pool.empty()) { h = v.pool.back(); v.pool.pop_back(); }
    else {
        hipMemAllocationProp prop{};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = c->device;
        hipError_t e = hipMemCreate(&h, v.chunk, &prop, 0);
        if (e != hipSuccess) return fail(c, SW_ENOMEM, "hipMemCreate(%zu bytes) failed: %s", v.chunk, hipGetErrorString(e));
    }
    hipError_t e = hipMemMap(v.base + slot * v.chunk, v.chunk, 0, h, 0);
    if (e != hipSuccess) { v.pool.push_back(h); return fail(c, SW_EIO, "hipMemMap failed: %s", hipGetErrorString(e)); }
    hipMemAccessDesc acc{};
    acc.location.type = hipMemLocationTypeDevice;
    acc.location.id = c->device;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    HIPCHK(c, hipMemSetAccess(v.base + slot * v.chunk, v.chunk, &acc, 1));
    poison(v.base + slot * v.chunk, v.chunk);
    v.handle[slot] = h;
    v.mapped[slot] = 1;
    return SW_OK;
}

// After hipMemUnmap the GPU's translation caches may still hold the old address -> chunk translation
// (measured: profiles/microbench/vmm_remap.hip; the unmap of the virtual-memory-management path does
// not invalidate them, the driver's map / unmap of an ordinary allocation does).  A recycled chunk
// or a re-used address would then be written through the stale entry.  Every batch of unmaps is
// therefore followed by one ordinary 4 MB allocation + free (above the runtime's sub-allocator
// threshold, so it reaches the driver).  SW_VM_FLUSH=0 switches this off (experiments only).
int vm_flush_translations(sw_ctx* c) {
    static const bool on = [] { const char* e = getenv("SW_VM_FLUSH"); return !(e && atoi(e) == 0); }();
    if (!on) return SW_OK;
    void* t = nullptr;
    HIPCHK(c, hipMalloc(&t, (size_t)4 << 20));
    HIPCHK(c, hipFree(t));
    return SW_OK;
}

// make the table resident up to `bytes` (from the first resident chunk)
int vm_ensure(sw_ctx* c, size_t bytes) {
    VmTable& v = c->vm;
    if (bytes > v.va_bytes) return fail(c, SW_ERANGE, "the windowed can_see table is limited to %zu GB of address space", v.va_bytes >> 30);
    const size_t need_hi = (bytes + v.chunk - 1) / v.chunk;
    for (size_t s_ = std::max(v.hi, v.lo); s_ < need_hi; ++s_) CHK(vm_map_slot(c, s_));
    v.hi = std::max(v.hi, need_hi);
    return SW_OK;
}

// unmap every chunk entirely below `bytes`; the physical chunks go to the pool
int vm_evict_below(sw_ctx* c, size_t bytes) {
    VmTable& v = c->vm;
    const size_t new_lo = std::min(bytes / v.chunk, v.hi);
    if (new_lo <= v.lo) return SW_OK;
    HIPCHK(c, hipDeviceSynchronize());  // nothing in flight may still read those rows
    for (size_t s_ = v.lo; s_ < new_lo; ++s_) {
        if (!v.mapped[s_]) continue;
        HIPCHK(c, hipMemUnmap(v.base + s_ * v.chunk, v.chunk));
        v.pool.push_back(v.handle[s_]);
        v.mapped[s_] = 0;
    }
    v.lo = new_lo;
    v.evictions++;
    return vm_flush_translations(c);
}

void vm_destroy(sw_ctx* c) {
    VmTable& v = c->vm;
    if (!v.active) return;
    for (size_t s_ = 0; s_ < v.mapped.size(); ++s_)
        if (v.mapped[s_]) { (void)hipMemUnmap(v.base + s_ * v.chunk, v.chunk); (void)hipMemRelease(v.handle[s_]); }
    for (auto h : v.pool) (void)hipMemRelease(h);
    if (v.base) (void)hipMemAddressFree(v.base, v.va_bytes);
    v = VmTable{};
    (void)vm_flush_translations(c);
}

// elements of the (non-windowed) can_see table for `cap` events: the rows, and behind the last row the scratch rows
// of the chunk-parallel sweep's halos (k_cansee_chunks: SW_MAX_CHUNKS x halo rows).  ONE place decides the size:
// ensure_events and sw_set_window(0) both allocate through it, and the chunk planner checks it.
size_t table_elems(const sw_ctx* c, int64_t cap) {
    return (size_t)(cap + (c->npad <= 256 ? SW_MAX_CHUNKS * c->halo : 0)) * c->npad;
}

// Windowed table: the halo scratch rows of the chunk-parallel sweep live behind row `cap` of the SAME address range
// (one base pointer, as in the plain table): the chunks that hold rows [cap, cap + SW_MAX_CHUNKS * halo) are mapped
// by the first call that is large enough to sweep in chunks (evictions work from the bottom and never reach them; when
// the capacity grows the old scratch chunks simply become table rows and the new ones are mapped on demand).
int vm_map_scratch(sw_ctx* c) {
    VmTable& v = c->vm;
    c->vm_scratch_ok = false;
    if (!v.active || c->npad > 256) return SW_OK;
    const size_t rowbytes = (size_t)c->npad * sizeof(int32_t);
    const size_t a = (size_t)c->cap * rowbytes, b = ((size_t)c->cap + (size_t)c->chunks * (size_t)c->halo) * rowbytes;   // (chunk k uses block k)
    if (b > v.va_bytes) return SW_OK;   // (no room in the reservation: the sweep stays unchunked)
    for (size_t s_ = a / v.chunk; s_ <= (b - 1) / v.chunk; ++s_) CHK(vm_map_slot(c, s_));
    c->vm_scratch_ok = true;
    return SW_OK;
}

// The heights kernel of a device append runs behind the call (stream_io).  Whoever reads d_ht, max_height or the
// block spans, or moves the event arrays, waits for it here and folds its read-back into the host tables.
int heights_ready(sw_ctx* c) {
    if (!c->ing.ht_pending) return SW_OK;
    c->ing.ht_pending = false;
    const int64_t blk0 = c->ing.ht_first >> 12, nblk = ((c->ing.ht_first + c->ing.ht_K - 1) >> 12) - blk0 + 1;
    std::vector<int32_t> st((size_t)(2 + 2 * nblk));
    hipError_t e_ = hipEventSynchronize(c->ing.ev_ht);
    if (e_ == hipSuccess) e_ = hipMemcpy(st.data(), c->ing.d_ht_stat.p, st.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e_ != hipSuccess) { c->poisoned = true; return fail(c, SW_EIO, "heights of a device append: %s", hipGetErrorString(e_)); }
    if (st[0] != 0) {
        c->poisoned = true;
        return fail(c, SW_EIO, "heights of a device append: a tile did not settle within its trip bound (internal)");
    }
    c->max_height = std::max(c->max_height, st[1]);
    c->blk_hmin.resize((size_t)(blk0 + nblk), 0x7fffffff);
    c->blk_hmax.resize((size_t)(blk0 + nblk), -1);
    for (int64_t b = 0; b < nblk; ++b) {
        c->blk_hmin[blk0 + b] = std::min(c->blk_hmin[blk0 + b], st[2 + 2 * b]);
        c->blk_hmax[blk0 + b] = std::max(c->blk_hmax[blk0 + b], st[3 + 2 * b]);
    }
    return SW_OK;
}

int ensure_events(sw_ctx* c, int64_t need) {
    if (need <= c->cap) return SW_OK;
    CHK(heights_ready(c));   // (the event arrays move: a device append's heights kernel may still be writing d_ht)
    int64_t nc = c->cap ? c->cap : 0;
    if (nc == 0) nc = need;
    while (nc < need) nc = nc + nc / 2 + 1024;
    const size_t keep = (size_t)c->N;
    CHK(dgrow(c, c->d_cr, nc, keep));
    CHK(dgrow(c, c->d_sp, nc, keep));
    CHK(dgrow(c, c->d_op, nc, keep));
    CHK(dgrow(c, c->d_ht, nc, keep));
    CHK(dgrow(c, c->d_seq, nc, keep));
    CHK(dgrow(c, c->d_round, nc, keep));
    CHK(dgrow(c, c->d_finlist, nc, 0));
    CHK(dgrow(c, c->d_coin, nc, keep));
    CHK(dgrow(c, c->d_t, nc, keep));
    CHK(dgrow(c, c->d_sig, (size_t)nc * 64, keep * 64));
    CHK(dgrow(c, c->d_S, (size_t)nc * c->nw, keep * c->nw));
    // (windowed table: chunks are mapped per append.)  Behind the last row: the scratch rows of the chunk-parallel
    // sweep's halos (k_cansee_chunks), SW_MAX_CHUNKS x halo rows
    if (!c->vm.active) CHK(dgrow(c, c->d_L, table_elems(c, nc), keep * c->npad));
    c->cap = nc;
    c->vm_scratch_ok = false;   // (windowed table: the scratch rows sit behind row `cap`: mapped again on demand)
    return SW_OK;
}

// rows of the per-round tables; new rows are initialised (lo = INF, wit = -1, fam = -1)
int ensure_rounds(sw_ctx* c, int need) {
    if (need <= c->Rcap) return SW_OK;
    int nc = c->Rcap ? c->Rcap : 256;
    while (nc < need) nc *= 2;
    // (the loop kernels address lo / lopos with 32-bit offsets)
    if ((int64_t)nc * c->npad >= (1ll << 31)) return fail(c, SW_ERANGE, "round table of %d rounds x %d columns exceeds 2^31 entries", nc, c->npad);
    // the per-round tables move: nothing may still be writing the old ones (the aux stream fills
    // witness rows behind the round loop)
    if (c->stream_aux) HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    if (c->stream_cs) HIPCHK(c, hipStreamSynchronize(c->stream_cs));
    const size_t np = c->npad;
    const size_t keep = (size_t)c->Rcap * np;
    CHK(dgrow(c, c->d_lo, (size_t)nc * np, keep));
    CHK(dgrow(c, c->d_lopos, (size_t)nc * np, keep));
    CHK(dgrow(c, c->d_wit, (size_t)nc * np, keep));
    CHK(dgrow(c, c->d_fam, (size_t)nc * np, keep));
    CHK(dgrow(c, c->d_dec_call, (size_t)nc * np, keep));
    CHK(dgrow(c, c->d_dec_by, (size_t)nc * np, keep));
    CHK(dgrow(c, c->d_cons, nc, c->Rcap));
    CHK(dgrow(c, c->d_newc, (size_t)nc + sizeof(FameCounters), c->d_newc.p ? sizeof(FameCounters) : 0));
    if (!c->d_fc) HIPCHK(c, hipMemset(c->d_newc.p, 0, sizeof(FameCounters)));
    c->d_fc = reinterpret_cast<FameCounters*>(c->d_newc.p);
    if (!c->h_fame.reserve((size_t)nc + sizeof(FameCounters))) return fail(c, SW_ENOMEM, "hipHostMalloc for the fame read-back failed");
    const size_t fresh = (size_t)(nc - c->Rcap) * np;
    CHK(fill_i32(c, c->d_lo.p + keep, fresh, SW_INF));
    CHK(fill_i32(c, c->d_lopos.p + keep, fresh, 0));
    CHK(fill_i32(c, c->d_wit.p + keep, fresh, -1));
    CHK(fill_i32(c, c->d_dec_call.p + keep, fresh, -1));
    CHK(fill_i32(c, c->d_dec_by.p + keep, fresh, -1));
    HIPCHK(c, hipMemsetAsync(c->d_fam.p + keep, 0xff, fresh, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_cons.p + c->Rcap, 0, nc - c->Rcap, c->stream));
    c->cons_h.resize(nc, 0);
    c->cons_call.resize(nc, -1);
    c->Rcap = nc;
    return SW_OK;
}

hipEvent_t next_event(sw_ctx* c) {
    if (c->ev_used == c->ev_pool.size()) {
        Event e;
        if (e.ensure(hipEventDefault) != hipSuccess) return nullptr;
        c->ev_pool.push_back(std::move(e));
    }
    return c->ev_pool[c->ev_used++];
}

struct Span {
    hipEvent_t a = nullptr, b = nullptr;
};
Span span_begin(sw_ctx* c, hipStream_t strm = nullptr) {
    Span s;
    if (c->profiling) {
        s.a = next_event(c);
        s.b = next_event(c);
        if (s.a) (void)hipEventRecord(s.a, strm ? strm : c->stream);
    }
    return s;
}
void span_end(sw_ctx* c, Span& s, hipStream_t strm = nullptr) {
    if (c->profiling && s.b) (void)hipEventRecord(s.b, strm ? strm : c->stream);
}
float span_ms(const Span& s) {
    float ms = 0.f;
    if (s.a && s.b) (void)hipEventElapsedTime(&ms, s.a, s.b);
    return ms;
}

// Per-member self-parent chains (index order == chain order for a fork-free DAG): every member
// owns a segment of a pool, chain_ev[chain_start[m] + p] = its p-th event.  Segments have slack
// and grow geometrically (a full segment moves to the end of the pool), so appending events
// costs O(new events), not O(all events); bulk appends rebuild the pool compactly.
// Chain pool entries and chain descriptors of the events [first, first + K): one device pass over
// cr / sp / op / seq with the CURRENT segment offsets (no host loop, no pool upload).
int scatter_chains(sw_ctx* c, int64_t first, int64_t K) {
    if (K <= 0) return SW_OK;
    hipLaunchKernelGGL(k_chain_scatter, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream, (const int*)c->d_cr.p,
                       (const int*)c->d_sp.p, (const int*)c->d_op.p, (const int*)c->d_seq.p, (const int*)c->d_chain_start.p,
                       (int)first, (int)K, c->d_chain_ev.p, c->d_cdesc.p);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    return SW_OK;
}

// Bulk layout: every member gets a fresh segment sized from its event count `cnt` (with slack), and
// the whole pool is re-scattered on the device.  The host copy of the pool becomes stale.
int rebuild_chains(sw_ctx* c, const std::vector<int32_t>& cnt, int64_t n_events) {
    const int np = c->npad, n = c->n;
    std::vector<int32_t> start(np, 0), cap(n, 0);
    int64_t off = 0;
    for (int m = 0; m < n; ++m) {
        start[m] = (int32_t)off;
        cap[m] = cnt[m] + cnt[m] / 4 + 16;
        off += cap[m];
    }
    if (off > 0x7fffffff) return fail(c, SW_ERANGE, "chain pool exceeds 2^31 entries");
    CHK(dgrow(c, c->d_chain_ev, (size_t)off + (size_t)off / 2 + 1024, 0));
    CHK(dgrow(c, c->d_cdesc, c->d_chain_ev.cap, 0));
    c->chain_start_h.swap(start);
    c->chain_cap.swap(cap);
    c->pool_used = off;
    c->pool_h_valid = false;
    std::vector<int32_t> cntp(np, 0);
    std::copy(cnt.begin(), cnt.end(), cntp.begin());
    HIPCHK(c, hipMemcpyAsync(c->d_chain_start.p, c->chain_start_h.data(), np * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_chain_cnt.p, cntp.data(), np * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the staging vectors above are locals)
    return scatter_chains(c, 0, n_events);
}

// ---- lazily fetched host mirrors: the device arrays are the source of truth -------------------
// self / other parents and heights (swirld.py:117-120) of all events: needed by sw_get_height and
// by the level-bucketed can_see kernels only

int ensure_dag_h(sw_ctx* c) {
    CHK(heights_ready(c));
    const int64_t have = (int64_t)c->sp.size();
    if (have >= c->N) return SW_OK;
    const int64_t K = c->N - have;
    // events [have, dev) were appended from device memory: their heights are in d_ht already and are downloaded;
    // those behind came through a bulk host append, and the host loop below computes theirs
    const int64_t dev = std::min(std::max(c->ing.ht_dev_upto, have), c->N);
    c->sp.resize(c->N); c->op.resize(c->N); c->ht.resize(c->N);
    HIPCHK(c, hipMemcpyAsync(c->sp.data() + have, c->d_sp.p + have, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->op.data() + have, c->d_op.p + have, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (dev > have) HIPCHK(c, hipMemcpyAsync(c->ht.data() + have, c->d_ht.p + have, (size_t)(dev - have) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->blk_hmin.resize((size_t)((c->N + 4095) >> 12), 0x7fffffff);
    c->blk_hmax.resize((size_t)((c->N + 4095) >> 12), -1);
    if (dev >= c->N) return SW_OK;
    c->ing.host_ht += c->N - dev;
    for (int64_t e = dev; e < c->N; ++e) {
        const int32_t s_ = c->sp[e], o_ = c->op[e];
        const int32_t h = s_ < 0 ? 0 : std::max(c->ht[s_], c->ht[o_]) + 1;  // swirld.py:117-120
        c->ht[e] = h;
        c->max_height = std::max(c->max_height, h);
        c->blk_hmin[e >> 12] = std::min(c->blk_hmin[e >> 12], h);
        c->blk_hmax[e >> 12] = std::max(c->blk_hmax[e >> 12], h);
    }
    HIPCHK(c, hipMemcpyAsync(c->d_ht.p + dev, c->ht.data() + dev, (size_t)(c->N - dev) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

// host copy of the chain pool (find_order's segment lists)
int ensure_pool_h(sw_ctx* c) {
    if (c->pool_h_valid) return SW_OK;
    c->chain_ev_h.resize((size_t)c->pool_used);
    if (c->pool_used) {
        HIPCHK(c, hipMemcpyAsync(c->chain_ev_h.data(), c->d_chain_ev.p, (size_t)c->pool_used * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->pool_h_valid = true;
    return SW_OK;
}

// host copy of the signatures (find_order's host-sort fallback, sw_get_vote's coin bits)
int ensure_sig_h(sw_ctx* c) {
    const int64_t have = (int64_t)(c->sig_h.size() / 64);
    if (have >= c->N) return SW_OK;
    if (c->payload_pending) { HIPCHK(c, hipEventSynchronize(c->ev_payload)); c->payload_pending = false; }
    c->sig_h.resize((size_t)c->N * 64);
    HIPCHK(c, hipMemcpyAsync(c->sig_h.data() + (size_t)have * 64, c->d_sig.p + (size_t)have * 64, (size_t)(c->N - have) * 64,
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

// geometry of the level-bucketed can_see kernel for this member count: CB columns per workgroup (one thread per event of a
// level, the CB values of a row slice as one vector), npad threads, the deepest per-member ring that fits beside the staging ring
struct CanseeCfg { int CB, H, chs; size_t lds; };
CanseeCfg cansee_cfg(int npad, int want_H) {
    CanseeCfg g{};
    g.CB = npad <= 512 ? 2 : 4;     // >= 160 workgroups up to 512 members, 256 at 1024
    int ch = 256;
    g.chs = 8;
    while (ch < npad) { ch <<= 1; g.chs++; }
    int H = 16;
    auto bytes = [&](int h) { return (size_t)4 * ch * 16 + ((size_t)npad * h + 1 + SW_LEVEL_SIDE) * (g.CB + 1) * sizeof(int) + SW_LEVEL_SIDE * sizeof(int) + 16; };
    while (H > 1 && bytes(H) > 158u * 1024u) H >>= 1;
    if (want_H >= 1 && want_H <= H && (want_H & (want_H - 1)) == 0) H = want_H;
    g.H = H;
    g.lds = bytes(H);
    return g;
}

template <int CB>
int launch_cansee_stream(sw_ctx* c, int nlev, const CanseeCfg& g, int64_t first_event) {
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)k_cansee_stream<CB>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            (void)hipGetLastError();
        attr_set = true;
    }
    hipLaunchKernelGGL((k_cansee_stream<CB>), dim3(c->npad / CB), dim3(c->npad), g.lds, c->stream_cs,
                       (const int4*)c->d_desc.p, (const int*)c->d_lev_start.p, (const int*)c->d_lev_pinbase.p, nlev, c->d_L.p, c->npad, g.H, g.chs, (int)first_event);
    return SW_OK;
}

template <int NW>
int launch_cansee(sw_ctx* c, int nlev, int64_t first_event) {
    // the level-bucketed kernel (the default beyond 256 members; SW_CANSEE_IMPL = 2 / 3 selects it below)
    const CanseeCfg g = cansee_cfg(c->npad, c->ring_H_req);
    if (g.CB == 2) CHK((launch_cansee_stream<2>(c, nlev, g, first_event)));
    else CHK((launch_cansee_stream<4>(c, nlev, g, first_event)));
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    return SW_OK;
}

// dataflow can_see sweep of the sub-batch whose chain positions are bounds rows i and i + 1
template <int NW, int MPL, int F, int H, bool WIDE, bool DBG>
int launch_cansee_flow_t(sw_ctx* c, int i, int64_t first_event) {
    constexpr int npad = 64 * NW;
    const size_t lds = (size_t)npad * ((size_t)F * 16 + (size_t)H * 8 + 8);
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)k_cansee_flow<NW, MPL, F, H, WIDE, DBG>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            (void)hipGetLastError();
        attr_set = true;
    }
    hipLaunchKernelGGL((k_cansee_flow<NW, MPL, F, H, WIDE, DBG>), dim3(npad), dim3(npad / MPL + 64), lds, c->stream_cs,
                       (const int4*)c->d_cdesc.p, (const int*)c->d_chain_start.p,
                       (const int*)c->d_bounds.p + (size_t)i * npad, (const int*)c->d_bounds.p + (size_t)(i + 1) * npad,
                       (const int*)c->d_chain_ev.p, (int)first_event, c->d_L.p, c->d_flow_err, c->d_flow_dbg.p);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    return SW_OK;
}

// chunk-parallel dataflow sweep (k_cansee_chunks) of one plan: all chunks in ONE launch (`sweep_all`), then per
// chunk k >= k_from the repair of its provisional entries and the second sweep — both always enqueued, both gated
// on the device by the count the sweep left (nothing to read back, no host decision on the sweep stream).
// `a0_all`: rows below it are final in memory; a parent in [a0_all, w_k) is a leaf.  A sub-batch of
// sw_divide_rounds passes its first event (chunk 0 has no halo, repairs start at chunk 1); an event range of the
// multi-GPU split (sw_cansee_range) passes 0: nothing below its halo is on this device yet, and its repair
// (sw_cansee_repair, chunk 0 included) runs once the rows below it have been imported.
template <int NW, int C, int F, int H>
int launch_cansee_chunks_t(sw_ctx* c, const sw_ctx::ChunkPlan& pl, const int* bnd, unsigned* prov, unsigned* fixed,
                           int a0_all, bool sweep_all, int k_from, int k_to) {
    constexpr int npad = 64 * NW;
    constexpr int NCG = npad / C;
    const size_t lds = (size_t)npad * ((size_t)F * 16 + (size_t)(C / 2) * H * 16 + 8);
    const bool wide = ((size_t)c->cap + (size_t)SW_MAX_CHUNKS * (size_t)c->halo) * (size_t)npad * sizeof(int32_t) >= (1ull << 32);
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)k_cansee_chunks<NW, C, F, H, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) (void)hipGetLastError();
        if (hipFuncSetAttribute((const void*)k_cansee_chunks<NW, C, F, H, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) (void)hipGetLastError();
        attr_set = true;
    }
    ChunkEv ce{};
    for (int k = 0; k < pl.G; ++k) { ce.w[k] = (int)pl.w[k]; ce.a[k] = (int)pl.a[k]; }
    hipStream_t cs = c->stream_cs;
    auto sweep = [&](int grid, int exact_chunk, unsigned limit) {
        if (wide)
            hipLaunchKernelGGL((k_cansee_chunks<NW, C, F, H, true>), dim3(grid), dim3(npad + 64), lds, cs,
                               (const int4*)c->d_cdesc.p, (const int*)c->d_chain_start.p, (const int*)c->d_chain_ev.p, bnd, ce,
                               a0_all, exact_chunk, c->n, c->d_L.p, (int)c->cap, (int)c->halo, prov, limit, c->d_flow_err);
        else
            hipLaunchKernelGGL((k_cansee_chunks<NW, C, F, H, false>), dim3(grid), dim3(npad + 64), lds, cs,
                               (const int4*)c->d_cdesc.p, (const int*)c->d_chain_start.p, (const int*)c->d_chain_ev.p, bnd, ce,
                               a0_all, exact_chunk, c->n, c->d_L.p, (int)c->cap, (int)c->halo, prov, limit, c->d_flow_err);
        c->ctr.kernel_launches++;
    };
    if (sweep_all) {
        sweep(pl.G * NCG, -1, 0u);
        c->ctr.chunk_sweeps += pl.G;
    }
    for (int k = k_from; k < k_to; ++k) {
        const int64_t len = pl.a[k + 1] - pl.a[k];
        // repair by gathers up to 1/32 of the chunk's entries, a second (dependent) sweep beyond (the sweep counts
        // provisional STORES of C columns each)
        const unsigned limit = (unsigned)std::min<int64_t>((len * c->n) / (32 * C), 0x7fffffff);
        const int blocks = (int)std::min<int64_t>((len + 3) / 4, 2048);
        hipLaunchKernelGGL(k_cansee_fixup<NW>, dim3(blocks), dim3(256), 0, cs, (const int*)c->d_chain_start.p, (const int*)c->d_chain_ev.p,
                           bnd + (size_t)(2 * k) * npad, a0_all, (int)pl.w[k], (int)pl.a[k], (int)pl.a[k + 1], c->n, c->d_L.p,
                           (const unsigned*)(prov + k), limit, fixed);
        c->ctr.kernel_launches++;
        sweep(NCG, k, limit);
    }
    HIPCHK(c, hipGetLastError());
    return SW_OK;
}

template <int NW>
int launch_cansee_plan(sw_ctx* c, const sw_ctx::ChunkPlan& pl, const int* bnd, unsigned* prov, unsigned* fixed,
                       int a0_all, bool sweep_all, int k_from, int k_to) {
    if constexpr (NW <= 4) {
        switch (c->chunk_cfg) {
            case 1: return launch_cansee_chunks_t<NW, 2, 8, 16>(c, pl, bnd, prov, fixed, a0_all, sweep_all, k_from, k_to);
            case 2: return launch_cansee_chunks_t<NW, 4, 4, 8>(c, pl, bnd, prov, fixed, a0_all, sweep_all, k_from, k_to);
            default: return launch_cansee_chunks_t<NW, 4, 8, 8>(c, pl, bnd, prov, fixed, a0_all, sweep_all, k_from, k_to);
        }
    }
    return fail(c, SW_EINVAL, "chunked sweep: more than 256 members");
}

// the chunked sweep of sub-batch i of the running sw_divide_rounds call
template <int NW>
int launch_cansee_chunks(sw_ctx* c, int i) {
    const sw_ctx::ChunkPlan& pl = c->chunk_plan[i];
    return launch_cansee_plan<NW>(c, pl, (const int*)c->d_cbnd.p + (size_t)pl.row0 * c->npad, c->d_prov + (size_t)i * SW_MAX_CHUNKS,
                                  c->d_prov + (size_t)SW_PROV_ROWS * SW_MAX_CHUNKS + i, (int)pl.a[0], true, 1, pl.G);
}

template <int NW, int MPL, int F, int H>
int launch_cansee_flow_g(sw_ctx* c, int i, int64_t first_event) {
    // 32-bit row offsets while the can_see table stays below 4 GB
    const bool wide = (size_t)c->cap * (size_t)(64 * NW) * sizeof(int32_t) >= (1ull << 32);
    if (c->d_flow_dbg.p) return wide ? launch_cansee_flow_t<NW, MPL, F, H, true, true>(c, i, first_event)
                                   : launch_cansee_flow_t<NW, MPL, F, H, false, true>(c, i, first_event);
    return wide ? launch_cansee_flow_t<NW, MPL, F, H, true, false>(c, i, first_event)
                : launch_cansee_flow_t<NW, MPL, F, H, false, false>(c, i, first_event);
}

template <int NW>
int launch_cansee_flow(sw_ctx* c, int i, int64_t first_event) {
    if constexpr (NW <= 4) {
        // LDS footprint matters beyond this kernel: the round-loop kernels share the CU with it, and a
        // 133 KB workgroup leaves room for fewer of their workgroups (SW_FLOW_CFG: FIFO / ring depths)
        switch (c->flow_cfg) {
            case 0: return launch_cansee_flow_g<NW, 1, 16, 32>(c, i, first_event);
            case 2: return launch_cansee_flow_g<NW, 1, 16, 16>(c, i, first_event);
            case 3: return launch_cansee_flow_g<NW, 1, 8, 32>(c, i, first_event);
            default: return launch_cansee_flow_g<NW, 1, 8, 16>(c, i, first_event);
        }
    }
    else if constexpr (NW == 8) return launch_cansee_flow_g<8, 2, 8, 16>(c, i, first_event);   // 256 lanes x 2 chains
    else return launch_cansee_flow_g<16, 4, 4, 8>(c, i, first_event);                          // 256 lanes x 4 chains
}

LoopBufs loop_bufs(sw_ctx* c) {
    LoopBufs B;
    B.st = c->d_state;
    B.lo_r = c->d_lo_r.p; B.cur = c->d_cur.p; B.unres = c->d_unres.p; B.lo_next = c->d_lo_next.p;
    B.pos_next = c->d_pos_next.p; B.evalround = c->d_evalround.p; B.evalpos = c->d_evalpos.p;
    B.found64 = c->d_found64.p;
    B.farslot = c->d_farslot.p;
    B.force = c->d_force.p;
    B.cand = c->d_cand.p;
    B.gallop = c->d_gallop.p;
    B.front = c->d_front.p;
    B.treecnt = c->d_treecnt;
    B.dbg = c->d_dbg.p;
    B.dbg_minor = c->dbg_minor;
    B.dbg_blk = c->d_dbg_blk.p;
    return B;
}

// one iteration of the round loop = (resolve + band masks) -> tally; both kernels guard on the
// device-side state, so extra iterations after `done` are no-ops.  `par` = iteration parity
// (which half of the double-buffered loop state is read / written).
// the tables of every part of a split, as the split kernels take them
SplitDst split_dst(const sw_ctx* c) {
    SplitDst d{};
    const SplitGroup* g = c->split;
    d.part = c->split_part;
    d.parts = g->parts;
    d.ndst = g->parts;
    for (int q = 0; q < g->parts; ++q) {
        const sw_ctx* o = g->ctx[q];
        d.Mb[q] = o->d_Mb.p + o->nw;
        d.Pc[q] = o->d_Pc.p + 1;
        d.S[q] = o->d_S.p;
        d.round[q] = o->d_round.p;
        d.found64[q] = o->d_found64.p;
        d.farslot[q] = o->d_farslot.p;
    }
    return d;
}

// the device copy of a SplitDst (slot 0: the linked part's; slot q: part q of an emulated split), uploaded when it changed
const SplitDst* split_dev(sw_ctx* c, int slot, const SplitDst& d) {
    if (!c->d_split.p) {
        if (dgrow(c, c->d_split, SW_MAX_PARTS, 0) != SW_OK) { (void)hipGetLastError(); return nullptr; }
        memset((void*)c->split_up, 0xff, sizeof c->split_up);
    }
    if (memcmp(&c->split_up[slot], &d, sizeof d) != 0) {
        c->split_up[slot] = d;
        if (hipMemcpyAsync(c->d_split.p + slot, &c->split_up[slot], sizeof d, hipMemcpyHostToDevice, c->stream) != hipSuccess) return nullptr;
    }
    return c->d_split.p + slot;
}

// One boundary of a split iteration: this part's kernel of the boundary is enqueued — record its event, tell the others, and
// make this part's stream wait for theirs (each waited for only once its owner has recorded it).  false: a part gave up.
bool split_meet(sw_ctx* c, int which, long long it) {
    SplitGroup* g = c->split;
    const int p = c->split_part, slot = (int)(it & 63);
    if (hipEventRecord(g->ev[which][p][slot], c->stream) != hipSuccess) { g->abort.store(1); return false; }
    g->rec[which][p].store(it + 1, std::memory_order_release);
    for (int q = 0; q < g->parts; ++q) {
        if (q == p) continue;
        const auto t0 = std::chrono::steady_clock::now();
        long spins = 0;
        while (g->rec[which][q].load(std::memory_order_acquire) < it + 1) {
            if (g->abort.load()) return false;
            if ((++spins & 1023) == 0) {
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(30)) { g->abort.store(1); return false; }   // (a part that never entered the call)
                std::this_thread::yield();
            }
        }
        if (hipStreamWaitEvent(c->stream, g->ev[which][q][slot], 0) != hipSuccess) { g->abort.store(1); return false; }
    }
    return true;
}

// an iteration of a linked context (sw_split_link): its share of the band events, the meeting, its share of the members, the meeting
template <int NW>
void enqueue_iteration_split(sw_ctx* c, int par) {
    const int np = c->npad, K = c->K;
    const int bt = std::max(np, 256);
    const uint32_t tot2 = 2u * c->tot;
    const LoopBufs B = loop_bufs(c);
    const SplitDst sd = split_dst(c);
    const SplitDst* sdp = split_dev(c, 0, sd);
    if (!sdp) { c->split->abort.store(1); c->split_failed = true; return; }
    const long long it = c->split_iter++;
    hipLaunchKernelGGL((k_resolve_band<NW, false, true>), dim3(c->band_blocks), dim3(bt), 0, c->stream, B, par, np, K, c->gallop_after, c->skip,
                       c->NEARCAP, c->MCAP, c->Rcap, (const int*)c->d_chain_start.p, c->d_chain_len.p,
                       (const int*)c->d_chain_ev.p, c->d_lo.p, c->d_lopos.p,
                       (const int*)c->d_L.p, (const int*)c->d_cr.p, (const int*)c->d_op.p, c->d_Mb.p + NW, c->d_round.p, c->d_S.p, c->d_Pc.p + 1, sdp);
    if (!split_meet(c, 0, it)) { c->split_failed = true; return; }
    const int members_here = (np - sd.part + sd.parts - 1) / sd.parts;
    const int tally_blocks = (members_here * K + 3) / 4;
    auto tally_bits = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(tally_blocks), dim3(256), 0, c->stream, B, par, K, c->skip, 0,
                           (const int*)c->d_chain_start.p, (const int*)c->d_chain_len.p, (const int*)c->d_chain_ev.p,
                           (const int*)c->d_L.p, (const int*)c->d_cr.p, (const int*)c->d_sp.p, (const int*)c->d_op.p,
                           (const uint32_t*)c->d_Mb.p, tot2, np, (const int*)c->d_Pc.p, sdp);
    };
    if (c->tally_filter) tally_bits(k_tally_bits<NW, true, true>);
    else tally_bits(k_tally_bits<NW, false, true>);
    if (!split_meet(c, 1, it)) { c->split_failed = true; return; }
    c->ctr.kernel_launches += 2;
}

// SW_SPLIT_EMULATE=<parts> (measurement): ONE unlinked context plays the parts of a split one behind the other — the band
// kernel of every part, then the tally kernel of every part, all storing into its own tables.  Results are those of the plain
// loop; every launch is exactly what one GPU of a `parts`-GPU node runs per iteration, alone on the chip
// (profiles/split_pieces.py reads their durations from the kernel trace).
template <int NW>
void enqueue_iteration_emulated(sw_ctx* c, int par, int parts) {
    const int np = c->npad, K = c->K;
    const int bt = std::max(np, 256);
    const uint32_t tot2 = 2u * c->tot;
    const LoopBufs B = loop_bufs(c);
    SplitDst sd{};
    sd.parts = parts; sd.ndst = 1;
    sd.Mb[0] = c->d_Mb.p + NW; sd.Pc[0] = c->d_Pc.p + 1; sd.S[0] = c->d_S.p; sd.round[0] = c->d_round.p;
    sd.found64[0] = c->d_found64.p; sd.farslot[0] = c->d_farslot.p;
    const SplitDst* sdq[SW_MAX_PARTS];
    for (int q = 0; q < parts; ++q) { sd.part = q; sdq[q] = split_dev(c, q, sd); if (!sdq[q]) { c->split_failed = true; return; } }
    for (int q = 0; q < parts; ++q) {
        hipLaunchKernelGGL((k_resolve_band<NW, false, true>), dim3(c->band_blocks), dim3(bt), 0, c->stream, B, par, np, K, c->gallop_after, c->skip,
                           c->NEARCAP, c->MCAP, c->Rcap, (const int*)c->d_chain_start.p, c->d_chain_len.p,
                           (const int*)c->d_chain_ev.p, c->d_lo.p, c->d_lopos.p,
                           (const int*)c->d_L.p, (const int*)c->d_cr.p, (const int*)c->d_op.p, c->d_Mb.p + NW, c->d_round.p, c->d_S.p, c->d_Pc.p + 1, sdq[q]);
    }
    for (int q = 0; q < parts; ++q) {
        const int members_here = (np - q + parts - 1) / parts;
        const int tally_blocks = (members_here * K + 3) / 4;
        if (c->tally_filter)
            hipLaunchKernelGGL((k_tally_bits<NW, true, true>), dim3(tally_blocks), dim3(256), 0, c->stream, B, par, K, c->skip, 0,
                               (const int*)c->d_chain_start.p, (const int*)c->d_chain_len.p, (const int*)c->d_chain_ev.p,
                               (const int*)c->d_L.p, (const int*)c->d_cr.p, (const int*)c->d_sp.p, (const int*)c->d_op.p,
                               (const uint32_t*)c->d_Mb.p, tot2, np, (const int*)c->d_Pc.p, sdq[q]);
        else
            hipLaunchKernelGGL((k_tally_bits<NW, false, true>), dim3(tally_blocks), dim3(256), 0, c->stream, B, par, K, c->skip, 0,
                               (const int*)c->d_chain_start.p, (const int*)c->d_chain_len.p, (const int*)c->d_chain_ev.p,
                               (const int*)c->d_L.p, (const int*)c->d_cr.p, (const int*)c->d_sp.p, (const int*)c->d_op.p,
                               (const uint32_t*)c->d_Mb.p, tot2, np, (const int*)c->d_Pc.p, sdq[q]);
    }
    c->ctr.kernel_launches += 2 * parts;
}

template <int NW>
void enqueue_iteration(sw_ctx* c, int par, std::vector<Span>* tally_spans, std::vector<Span>* resolve_spans = nullptr) {
    if (c->split) { enqueue_iteration_split<NW>(c, par); return; }
    if (c->split_emulate > 0 && c->unit_stake && c->tally_impl == 1) { enqueue_iteration_emulated<NW>(c, par, c->split_emulate); return; }
    const int np = c->npad, K = c->K;
    const int tally_blocks = np * K / 4;
    const int bt = std::max(np, 256);
    const int band_blocks = c->band_blocks;
    const uint32_t tot2 = 2u * c->tot;
    const LoopBufs B = loop_bufs(c);
    Span sr{};
    if (resolve_spans) sr = span_begin(c);
    auto resolve_band = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(band_blocks), dim3(bt), 0, c->stream, B, par, np, K, c->gallop_after, c->skip,
                           c->NEARCAP, c->MCAP, c->Rcap, (const int*)c->d_chain_start.p, c->d_chain_len.p,
                           (const int*)c->d_chain_ev.p, c->d_lo.p, c->d_lopos.p,
                           (const int*)c->d_L.p, (const int*)c->d_cr.p, (const int*)c->d_op.p, c->d_Mb.p + NW, c->d_round.p, c->d_S.p, c->d_Pc.p + 1, (const SplitDst*)nullptr);
    };
    if constexpr (NW <= 4) {
        if (c->band_fast) resolve_band(k_resolve_band<NW, true>);
        else resolve_band(k_resolve_band<NW, false>);
    } else resolve_band(k_resolve_band<NW, false>);
    if (resolve_spans) { span_end(c, sr); resolve_spans->push_back(sr); }
    Span s{};
    if (tally_spans) s = span_begin(c);
    if (c->unit_stake && c->tally_impl == 2)
        hipLaunchKernelGGL(k_tally_tree<NW>, dim3(np), dim3(512), 0, c->stream, B, par, K, c->skip, c->tally_pf,
                           (const int*)c->d_L.p, (const int*)c->d_sp.p, (const int*)c->d_op.p, (const uint32_t*)c->d_Mb.p, tot2, np);
    else if (c->unit_stake && c->tally_impl >= 1) {
        auto tally_bits = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(tally_blocks), dim3(256), 0, c->stream, B, par, K, c->skip, c->tally_pf,
                               (const int*)c->d_chain_start.p, (const int*)c->d_chain_len.p, (const int*)c->d_chain_ev.p,
                               (const int*)c->d_L.p, (const int*)c->d_cr.p, (const int*)c->d_sp.p, (const int*)c->d_op.p,
                               (const uint32_t*)c->d_Mb.p, tot2, np, (const int*)c->d_Pc.p, (const SplitDst*)nullptr);
        };
        if (c->tally_filter) tally_bits(k_tally_bits<NW, true>);
        else tally_bits(k_tally_bits<NW, false>);
    }
    else if (c->unit_stake)
        hipLaunchKernelGGL((k_tally_candidates<NW, true>), dim3(tally_blocks), dim3(256), 0, c->stream, B, par, K,
                           (const int*)c->d_chain_start.p, (const int*)c->d_chain_len.p, (const int*)c->d_chain_ev.p,
                           (const int*)c->d_L.p, (const int*)c->d_cr.p, (const int*)c->d_sp.p, (const int*)c->d_op.p,
                           (const u64*)(c->d_Mb.p + NW), (const uint32_t*)c->d_stake.p, tot2, np);
    else
        hipLaunchKernelGGL((k_tally_candidates<NW, false>), dim3(tally_blocks), dim3(256), 0, c->stream, B, par, K,
                           (const int*)c->d_chain_start.p, (const int*)c->d_chain_len.p, (const int*)c->d_chain_ev.p,
                           (const int*)c->d_L.p, (const int*)c->d_cr.p, (const int*)c->d_sp.p, (const int*)c->d_op.p,
                           (const u64*)(c->d_Mb.p + NW), (const uint32_t*)c->d_stake.p, tot2, np);
    if (tally_spans) { span_end(c, s); tally_spans->push_back(s); }
    c->ctr.kernel_launches += 2;
}

// the loop body as replayable hipGraphs of [SW_GRAPH_BIG /] 24 / 8 / 2 iterations (2 kernel nodes each); the
// kernel arguments are frozen at capture, so the graphs are rebuilt when any of them changes.
// Iteration counts are even because the loop state is double-buffered by iteration parity.
constexpr int kGraphSizesBase[4] = {0, 24, 8, 2};

template <int NW>
int launch_iterations(sw_ctx* c, int n_iters, std::vector<Span>* tally_spans, std::vector<Span>* resolve_spans = nullptr) {
    // short shots (a Node's small calls): plain launches — the first hipGraphLaunch of a call costs ~200 us
    if (!c->use_graph || tally_spans || n_iters <= 8 || c->split || c->split_emulate) {   // (split: the meetings of the parts are host calls between the kernels)
        for (int it = 0; it < n_iters; ++it) enqueue_iteration<NW>(c, it & 1, tally_spans, resolve_spans);
        return SW_OK;
    }
    sw_ctx::GraphKey key;
    memset(&key, 0, sizeof key);
    key.Rcap = c->Rcap; key.N = c->N; key.lo = (void*)c->d_lo.p; key.L = (void*)c->d_L.p;
    key.chain = (void*)c->d_chain_ev.p; key.K = c->K; key.tally_impl = c->tally_impl;
    key.S = (void*)c->d_S.p; key.round = (void*)c->d_round.p;
    key.BATCH = c->band_blocks + 4096 * c->skip; key.MCAP = c->MCAP + 7 * c->NEARCAP; key.variant = c->band_fast + 2 * c->tally_filter;
    if (memcmp(&key, &c->loop_key, sizeof key) != 0) {
        for (int g = 0; g < 4; ++g) {
            if (c->loop_exec[g]) { (void)hipGraphExecDestroy(c->loop_exec[g]); c->loop_exec[g] = nullptr; }
            if (c->loop_graph[g]) { (void)hipGraphDestroy(c->loop_graph[g]); c->loop_graph[g] = nullptr; }
        }
        c->loop_key = key;
    }
    int left = n_iters;
    const int kGraphSizes[4] = {c->graph_big, kGraphSizesBase[1], kGraphSizesBase[2], kGraphSizesBase[3]};
    for (int g = 0; g < 4; ++g) {
        if (kGraphSizes[g] <= 0) continue;
        while (left >= kGraphSizes[g]) {
            if (!c->loop_exec[g]) {
                HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
                const int64_t launches_before = c->ctr.kernel_launches;
                for (int it = 0; it < kGraphSizes[g]; ++it) enqueue_iteration<NW>(c, it & 1, nullptr);
                c->ctr.kernel_launches = launches_before;
                HIPCHK(c, hipStreamEndCapture(c->stream, &c->loop_graph[g]));
                HIPCHK(c, hipGraphInstantiate(&c->loop_exec[g], c->loop_graph[g], nullptr, nullptr, 0));
            }
            HIPCHK(c, hipGraphLaunch(c->loop_exec[g], c->stream));
            c->ctr.kernel_launches += 2 * kGraphSizes[g];
            left -= kGraphSizes[g];
        }
    }
    return SW_OK;
}

// round numbers and sees-masks of the events [first, first + K) on `ax`, table rows 0 .. R-1 final: with the band pass
// writing them (SW_FIN_BAND=1) a check of one thread per event + the listed leftovers from their rows, else every event
// from its row.  `blocks` = workgroups of the row-reading launch.
template <int NW>
int launch_finalize(sw_ctx* c, hipStream_t ax, int64_t first, int64_t K, int R, int blocks) {
    const int np = c->npad;
    if (K <= 0) return SW_OK;
    if (!c->fin_band) {
        hipLaunchKernelGGL(k_finalize_events<NW>, dim3((unsigned)std::min<int64_t>((K + 3) / 4, blocks)), dim3(256), 0, ax, (const int*)c->d_L.p,
                           (const int*)c->d_cr.p, (const int*)c->d_lo.p, R, (int)first, (int)K, c->d_round.p, c->d_S.p, np);
        c->ctr.kernel_launches++;
        return SW_OK;
    }
    if (!c->d_fin.p) {
        CHK(dgrow(c, c->d_fin, 4, 0));
        HIPCHK(c, hipMemset(c->d_fin.p, 0, 16));
    }
    HIPCHK(c, hipMemsetAsync(c->d_fin.p, 0, sizeof(unsigned), ax));
    hipLaunchKernelGGL(k_finalize_check, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, ax, (const int*)c->d_cr.p, (const int*)c->d_lo.p, R,
                       (int)first, (int)K, (const int*)c->d_round.p, np, c->d_finlist.p, c->d_fin.p);
    hipLaunchKernelGGL(k_finalize_listed<NW>, dim3((unsigned)std::min<int64_t>((K + 3) / 4, std::min(blocks, 1024))), dim3(256), 0, ax, (const int*)c->d_L.p,
                       (const int*)c->d_cr.p, (const int*)c->d_lo.p, R, (const int*)c->d_finlist.p, c->d_fin.p, c->d_round.p, c->d_S.p, np);
    c->ctr.kernel_launches += 2;
    return SW_OK;
}

// first shot of a round loop: the predicted number of iterations for this many events (from the iterations-per-event rate of
// earlier runs); without a measured rate about one round per 11.7 n events (SURVEY.md §8 probe) plus the round in progress —
// a small call must not pay for a long first shot
inline int predict_shot(const sw_ctx* c, int64_t n_new_events, bool gated = false) {
    int shot = std::min<int64_t>(c->BATCH, 2 + (n_new_events / (12 * (int64_t)c->n) + 1) * 2);
    const int64_t si = gated ? c->gstat_iters : c->stat_iters, se = gated ? c->gstat_events : c->stat_events;
    if (si > 0 && se > 0) {
        const double pred = (double)si / (double)se * (double)n_new_events;
        shot = std::max(2, (int)(pred * c->shot_pct / 100.0) + c->shot_extra);
    }
    return std::min(shot, 4096) & ~1;
}

template <int NW>
int launch_voter_masks(sw_ctx* c, int r0, int R, hipStream_t strm) {
    const int np = c->npad;
    if (R > c->Sw_rows) {
        int nr = c->Sw_rows ? c->Sw_rows : 256;
        while (nr < R) nr *= 2;
        u64* q = nullptr;
        hipError_t e = hipMalloc((void**)&q, (size_t)nr * np * NW * sizeof(u64));
        if (e != hipSuccess) return fail(c, SW_ENOMEM, "hipMalloc(Sw) failed: %s", hipGetErrorString(e));
        poison(q, (size_t)nr * np * NW * sizeof(u64));
        HIPCHK(c, hipStreamSynchronize(c->stream_aux));
        if (c->Sw_rows && c->d_Sw.p)
            HIPCHK(c, hipMemcpy(q, c->d_Sw.p, (size_t)c->Sw_rows * np * NW * sizeof(u64), hipMemcpyDeviceToDevice));
        c->d_Sw.adopt(q, (size_t)nr * np * NW);   // (frees the old block)
        c->Sw_rows = nr;
    }
    r0 = std::max(1, r0);
    if (R <= r0) return SW_OK;
    const uint32_t tot2 = 2u * c->tot;
    const int total = (R - r0) * np;
    if (c->unit_stake && c->tally_impl >= 1)
        hipLaunchKernelGGL(k_voter_masks_bits<NW>, dim3((total + 3) / 4), dim3(256), 0, strm,
                           (const int*)c->d_wit.p, (const int*)c->d_L.p, (const int*)c->d_lo.p, (const uint32_t*)c->d_S.p,
                           tot2, r0, R, np, (uint32_t*)c->d_Sw.p, c->d_fc);
    else if (c->unit_stake)
        hipLaunchKernelGGL((k_voter_masks<NW, true>), dim3((total + 3) / 4), dim3(256), 0, strm,
                           (const int*)c->d_wit.p, (const int*)c->d_L.p, (const int*)c->d_lo.p, (const u64*)c->d_S.p,
                           (const uint32_t*)c->d_stake.p, tot2, r0, R, np, c->d_Sw.p, c->d_fc);
    else
        hipLaunchKernelGGL((k_voter_masks<NW, false>), dim3((total + 3) / 4), dim3(256), 0, strm,
                           (const int*)c->d_wit.p, (const int*)c->d_L.p, (const int*)c->d_lo.p, (const u64*)c->d_S.p,
                           (const uint32_t*)c->d_stake.p, tot2, r0, R, np, c->d_Sw.p, c->d_fc);
    c->ctr.kernel_launches++;
    return SW_OK;
}

// Heights of the 4096-event blocks that hold a cut, for events the host mirror lacks (heights_for_spans).
struct EdgeHeights {
    std::vector<int64_t> start;               // first event of each fetched piece
    std::vector<std::vector<int32_t>> h;
    int32_t at(int64_t e) const {
        for (size_t i = 0; i < start.size(); ++i)
            if (e >= start[i] && e < start[i] + (int64_t)h[i].size()) return h[i][(size_t)(e - start[i])];
        return 0;   // (not reached: every partial block beyond the mirror has been fetched)
    }
};

// height span of the events [a, b): from the ingest-time block index, edges by scanning
void height_span(const sw_ctx* c, int64_t a, int64_t b, int* hmin, int* hmax, const EdgeHeights& edge) {
    int lo = 0x7fffffff, hi = -1;
    int64_t e = a;
    const int64_t have = (int64_t)c->ht.size();
    while (e < b) {
        if ((e & 4095) == 0 && e + 4096 <= b) {
            lo = std::min(lo, c->blk_hmin[e >> 12]);
            hi = std::max(hi, c->blk_hmax[e >> 12]);
            e += 4096;
        } else {
            const int32_t h = e < have ? c->ht[e] : edge.at(e);
            lo = std::min(lo, h);
            hi = std::max(hi, h);
            ++e;
        }
    }
    *hmin = lo;
    *hmax = hi;
}

// What the level sweep's sizing reads on the host.  Events appended from device memory have their heights in d_ht and
// their block spans in blk_hmin / blk_hmax without the full host mirror: when every event beyond the mirror is such an
// event, only the blocks that hold a cut are fetched; otherwise the mirror is completed (ensure_dag_h).
int heights_for_spans(sw_ctx* c, const std::vector<int64_t>& cut, EdgeHeights& edge) {
    CHK(heights_ready(c));
    const int64_t have = (int64_t)c->sp.size();
    if (have >= c->N) return SW_OK;
    if (c->ing.ht_dev_upto < c->N) return ensure_dag_h(c);
    for (size_t i = 0; i < cut.size(); ++i) {
        const int64_t x = cut[i];
        const int64_t a = std::max<int64_t>(x & ~(int64_t)4095, have), b = std::min<int64_t>((x | (int64_t)4095) + 1, c->N);
        if ((x & 4095) == 0 || b <= a) continue;
        edge.start.push_back(a);
        edge.h.emplace_back((size_t)(b - a));
        HIPCHK(c, hipMemcpyAsync(edge.h.back().data(), c->d_ht.p + a, (size_t)(b - a) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

// host-side stage clock of sw_divide_rounds (SW_DEBUG_TIMING=1: averages printed by sw_destroy)
struct StageClock {
    bool on;
    std::chrono::steady_clock::time_point last;
    explicit StageClock(bool on_) : on(on_) { if (on) last = std::chrono::steady_clock::now(); }
    void mark(double* acc) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        *acc += std::chrono::duration<double, std::micro>(now - last).count();
        last = now;
    }
};

// ==== sw_divide_rounds, host side =================================================================
// do_divide (at the end of this section) calls the phases below in order; DESIGN.md §4 maps every phase to its
// function and to the stream it enqueues on.

// The finalize / witness-row / voter-mask launches of a finished sub-batch.  The rounds of every event below its limit are
// final (later sub-batches only add lo entries that compare greater than every existing event), so they are produced on a
// third stream, overlapping the round loop of the next sub-batch — and ENQUEUED behind that loop's first shot
// (flush_tail): armed by after_loop, they must wait for the finished loop's kernels, which the aux stream learns from an
// event recorded behind them.
struct DeferredTail {
    bool armed;
    int i, r_start, R;      // the sub-batch, the start round of its loop, the rounds behind it
    int64_t a0, k0;         // its events that no early finalize has taken: [a0, a0 + k0)
    hipEvent_t loop_done;   // recorded behind its loop
};

// one sw_divide_rounds call: what its phases hand on to each other (scratch that outlives the call — bounds_stage,
// ccuts_stage, chunk_plan — stays in sw_ctx)
struct DivideCall {
    const int64_t first, K;
    // sub-batches: the can_see sweep of sub-batch i+1 (stream_cs) overlaps the round loop of sub-batch i (main stream);
    // a kernel boundary separates producer and consumer of a row
    std::vector<int64_t> cut;      // [S + 1] event limits of the sub-batches
    int S = 0;
    bool flow = false;             // the dataflow sweep (else the level-bucketed one)
    bool preswept = false;         // the rows are already in the table: no sweep
    bool gated = false;            // one device-gated round loop for the whole call (run_gated)
    std::vector<int> hmins, nlevs; // level-bucketed sweep: lowest height and levels per sub-batch
    bool bounds_pending = false;   // the cut table is still on its way back (ev_bounds)
    std::vector<int32_t> clen_prev, clen;   // members' visible chain lengths before and after the sub-batch in hand: rows of the cut table
    int64_t fin_from = 0;          // events of the running loop's sub-batch below this one were finalized beside the loop
    DeferredTail tail{};
    StageClock clk;
    // profiling
    Span sp_total, sp_rl;
    hipEvent_t cs_t0 = nullptr, cs_t1 = nullptr, fin_t0 = nullptr;
    float tally_ms = 0.f;
    int tally_launches = 0;
    std::vector<Span> cansee_spans;
    DivideCall(const sw_ctx* c, int64_t first_, int64_t K_) : first(first_), K(K_), clk(c->debug_timing) {}
};

LoopGate* loop_gate(sw_ctx* c) { return reinterpret_cast<LoopGate*>(c->d_rb.p + SW_GATE_OFF); }

// ---- phase: cut plan
void plan_cuts(const sw_ctx* c, DivideCall& d) {
    const int64_t first = d.first, K = d.K;
    std::vector<int64_t>& cut = d.cut;
    cut.assign(1, first);
    if (const char* cs_ = getenv("SW_CUTS"); cs_ && K >= 65536) {  // tuning hook: cut points as fractions of K
        for (const char* q = cs_; *q;) {
            char* end = nullptr;
            const double f = strtod(q, &end);
            if (end == q) break;
            const int64_t bnd = ((first + (int64_t)(f * (double)K)) >> 12) << 12;
            if (bnd > cut.back() && bnd < first + K) cut.push_back(bnd);
            q = *end ? end + 1 : end;
        }
    } else if (K >= 65536 && c->pipe > 1) {
        // a short first sub-batch (its sweep is the only one nothing overlaps), then `pipe` parts.  Round 5: the parts are
        // GRADUATED — weights 0.5, 0.9, 1.2, 1, 1, ... — because a loop now consumes events almost as fast as a sweep produces
        // them (the loop of an even second part waited 0.17 ms for its sweep; profiles/r05l_knobs_256x1M.log: 6.09 -> 5.99 ms)
        const int64_t head = K / 16;
        const int P = c->pipe;
        double w[SW_PROV_ROWS], tot = 0.0;
        for (int s_ = 0; s_ < P; ++s_) { w[s_] = P < 4 ? 1.0 : (s_ == 0 ? 0.5 : s_ == 1 ? 0.9 : s_ == 2 ? 1.2 : 1.0); tot += w[s_]; }
        double acc = 0.0;
        for (int s_ = 0; s_ < P; ++s_) {
            const int64_t at = head + (int64_t)((double)(K - head) * (acc / tot));
            acc += w[s_];
            const int64_t bnd = ((first + at) >> 12) << 12;
            if (bnd > cut.back() && bnd < first + K) cut.push_back(bnd);
        }
    }
    cut.push_back(first + K);
    d.S = (int)cut.size() - 1;
    d.flow = c->cansee_impl >= 6;
}

// ---- phase: which tally (round 4, profiles/r04l_*): the two-level search with a window of 32 wins on 256-member hashgraphs whose
// members are about equally active — uniform gossip +2.6 %, two cliques +18 %, stale other-parents +16 %, 4 M events
// +4.7 %, mild skew +5 % — and loses where a third of the members is 50 times less active (-9 %) and at 64 / 128
// members (-8 / -10 %).  Decided per large call from the members' event counts; SW_TALLY_IMPL / SW_TALLY_K pin it.
void choose_tally(sw_ctx* c, const DivideCall& d) {
    if (!c->tally_auto || !c->unit_stake) return;
    int impl = 1;
    if (c->npad == 256 && c->n > 200 && d.K >= 65536) {
        int32_t lo_ = 0x7fffffff, hi_ = 0;
        for (int m = 0; m < c->n; ++m) { lo_ = std::min(lo_, c->nev[m]); hi_ = std::max(hi_, c->nev[m]); }
        if (lo_ > 0 && (int64_t)hi_ <= 8 * (int64_t)lo_) impl = 2;
    }
    c->tally_impl = impl;
    if (c->K_auto) c->K = impl == 2 ? 32 : c->K_flat;
}

// ---- phase: rows already in the table (event-range split: swept by sw_cansee_range or imported): no sweep, the round
// loop still waits for whatever the sweep stream has in flight (imports, repairs)
int test_preswept(sw_ctx* c, DivideCall& d) {
    const int64_t first = d.first, K = d.K;
    for (const auto& pr : c->present) {
        if (first >= pr.first && first + K <= pr.second) d.preswept = true;
        else if (first < pr.second && first + K > pr.first)
            return fail(c, SW_EINVAL, "divide_rounds [%lld, %lld) straddles the rows [%lld, %lld) already present (sw_cansee_range / sw_import_rows)",
                        (long long)first, (long long)(first + K), (long long)pr.first, (long long)pr.second);
    }
    return SW_OK;
}

// ---- phase: level tables of the level-bucketed sweep
int size_level_tables(sw_ctx* c, DivideCall& d) {
    d.hmins.assign(d.S, 0);
    d.nlevs.assign(d.S, 0);
    if (d.flow || d.preswept) return SW_OK;
    int max_nlev = 1;
    int64_t max_k = 1;
    EdgeHeights edge;
    CHK(heights_for_spans(c, d.cut, edge));  // the level-bucketed kernels need the heights (swirld.py:117-120)
    for (int i = 0; i < d.S; ++i) {
        int hmax;
        height_span(c, d.cut[i], d.cut[i + 1], &d.hmins[i], &hmax, edge);
        d.nlevs[i] = hmax - d.hmins[i] + 1;
        max_nlev = std::max(max_nlev, d.nlevs[i]);
        max_k = std::max(max_k, d.cut[i + 1] - d.cut[i]);
        c->ctr.levels += d.nlevs[i];
    }
    CHK(dgrow(c, c->d_lev_cnt, max_nlev, 0));
    CHK(dgrow(c, c->d_lev_start, max_nlev + 1, 0));
    CHK(dgrow(c, c->d_lev_cursor, max_nlev, 0));
    CHK(dgrow(c, c->d_desc, max_k, 0));
    CHK(dgrow(c, c->d_lev_pin, max_k, 0));
    CHK(dgrow(c, c->d_lev_pos, max_k, 0));
    CHK(dgrow(c, c->d_lev_cback, max_nlev, 0));
    CHK(dgrow(c, c->d_lev_pinbase, max_nlev + 1, 0));
    return SW_OK;
}

// ---- phase: the sweep stream opens behind whatever the main stream still has in flight (a small append returns without a
// host synchronisation); decides whether the call runs gated
int open_sweep_stream(sw_ctx* c, DivideCall& d) {
    while ((int)c->cs_events.size() < d.S) {
        c->cs_events.emplace_back();
        CHK(ensure_event(c, c->cs_events.back()));
    }
    hipStream_t cs = c->stream_cs;
    HIPCHK(c, hipEventRecord(c->ev_main_mark, c->stream));
    HIPCHK(c, hipStreamWaitEvent(cs, c->ev_main_mark, 0));
    // ONE round loop for the whole call, gated on the device by the sweep's progress (SW_GATED=1): the dataflow sweep of a
    // plain table, not the split loop (its meetings are host calls), not preswept ranges, not the windowed table
    d.gated = c->gated && d.S > 1 && d.S <= SW_PROV_ROWS && d.flow && !d.preswept && !c->split && !c->split_emulate && !c->vm.active && c->npad <= 256;
    if (d.gated) hipLaunchKernelGGL(k_set_stage, dim3(1), dim3(64), 0, cs, loop_gate(c), 0);   // (the previous loop is done: cs waited for it)
    if (c->profiling) { d.cs_t0 = next_event(c); d.cs_t1 = next_event(c); (void)hipEventRecord(d.cs_t0, cs); }
    if (c->profiling) { c->tm.resolve_ms = 0.f; c->tm.resolve_launches = 0; }
    return SW_OK;
}

// ---- phase: chain positions of the cuts: bounds[i][m] = events of member m below cut[i].  One cut pair that
// ends at the last appended event (a Node's call) is known on the host: chain lengths at the last
// divide and now.  Otherwise device binary searches over the chain pool.
int build_bounds(sw_ctx* c, DivideCall& d) {
    const int np = c->npad, S = d.S;
    hipStream_t cs = c->stream_cs;
    std::vector<int32_t>& bounds_h = c->bounds_stage;
    bounds_h.resize((size_t)(S + 1) * np);
    CHK(dgrow(c, c->d_bounds, (size_t)(S + 1) * np, 0));
    if (S == 1 && d.first + d.K == c->N) {
        std::copy(c->divided_cnt.begin(), c->divided_cnt.end(), bounds_h.begin());
        std::fill(bounds_h.begin() + np, bounds_h.end(), 0);
        std::copy(c->nev.begin(), c->nev.end(), bounds_h.begin() + np);
        HIPCHK(c, hipMemcpyAsync(c->d_bounds.p, bounds_h.data(), bounds_h.size() * sizeof(int32_t), hipMemcpyHostToDevice, cs));
        return SW_OK;
    }
    CHK(dgrow(c, c->d_cuts, S + 1, 0));
    std::vector<long long> cuts_ll(d.cut.begin(), d.cut.end());
    HIPCHK(c, hipMemcpyAsync(c->d_cuts.p, cuts_ll.data(), (S + 1) * sizeof(long long), hipMemcpyHostToDevice, cs));
    hipLaunchKernelGGL(k_chain_bounds, dim3(S + 1), dim3(np), 0, cs, (const int*)c->d_chain_start.p, (const int*)c->d_chain_cnt.p,
                       (const int*)c->d_chain_ev.p, (const long long*)c->d_cuts.p, np, c->d_bounds.p);
    c->ctr.kernel_launches++;
    // (read back behind the kernel; the host needs the table only for the round loops: do_divide waits for
    // `ev_bounds` after every sweep has been enqueued — the GPU starts sweeping ~0.1 ms earlier)
    HIPCHK(c, hipMemcpyAsync(bounds_h.data(), c->d_bounds.p, bounds_h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, cs));
    CHK(ensure_event(c, c->ev_bounds));
    HIPCHK(c, hipEventRecord(c->ev_bounds, cs));
    d.bounds_pending = true;
    return SW_OK;
}

// ---- phase: chunk plan: a sub-batch long enough is cut into G chunks that are swept concurrently, each from
// `halo` events before its start (k_cansee_chunks); their chain positions come from one more search kernel
int plan_chunks(sw_ctx* c, const DivideCall& d) {
    const int np = c->npad, S = d.S;
    const std::vector<int64_t>& cut = d.cut;
    hipStream_t cs = c->stream_cs;
    c->chunk_plan.assign(S, sw_ctx::ChunkPlan{});
    bool may_chunk = d.flow && !d.preswept && np <= 256 && c->chunks > 1 && !c->chunks_off && S <= SW_PROV_ROWS;
    if (c->debug_timing && S > SW_PROV_ROWS)   // (only the SW_CUTS tuning hook can ask for that many sub-batches)
        fprintf(stderr, "[sw] %d sub-batches: more than %d, swept unchunked\n", S, SW_PROV_ROWS);
    if (may_chunk && c->vm.active && !c->vm_scratch_ok) {   // windowed table: the scratch rows are mapped by the first call that can use them
        bool any = false;
        for (int i = 0; i < S; ++i) any = any || (cut[i + 1] - cut[i]) / c->chunk_min >= 2;
        if (any) CHK(vm_map_scratch(c));
    }
    // (the halo scratch rows must exist: they live behind the table's last row)
    if (!may_chunk || !(c->vm.active ? c->vm_scratch_ok : c->d_L.cap >= table_elems(c, c->cap))) return SW_OK;
    std::vector<long long>& ccuts = c->ccuts_stage;
    ccuts.clear();
    for (int i = 0; i < S; ++i) {
        const int64_t a = cut[i], len = cut[i + 1] - cut[i];
        const int G = (int)std::min<int64_t>(c->chunks, len / c->chunk_min);
        if (G < 2) continue;
        sw_ctx::ChunkPlan& pl = c->chunk_plan[i];
        pl.G = G;
        pl.row0 = (int)ccuts.size();
        for (int k = 0; k <= G; ++k) pl.a[k] = a + len * k / G;
        for (int k = 0; k < G; ++k) {
            pl.w[k] = k == 0 ? a : std::max(a, pl.a[k] - c->halo);
            ccuts.push_back(pl.w[k]);
            ccuts.push_back(pl.a[k]);
        }
        ccuts.push_back(pl.a[G]);   // rows 2G and 2G + 1: the end, twice — chunk k ends at row 2k + 3 for every k
        ccuts.push_back(pl.a[G]);
    }
    if (ccuts.empty()) return SW_OK;
    CHK(dgrow(c, c->d_ccuts, ccuts.size(), 0));
    CHK(dgrow(c, c->d_cbnd, ccuts.size() * (size_t)np, 0));
    // (pageable source: the copy is staged before the call returns)
    HIPCHK(c, hipMemcpyAsync(c->d_ccuts.p, ccuts.data(), ccuts.size() * sizeof(long long), hipMemcpyHostToDevice, cs));
    hipLaunchKernelGGL(k_chain_bounds, dim3((unsigned)ccuts.size()), dim3(np), 0, cs, (const int*)c->d_chain_start.p,
                       (const int*)c->d_chain_cnt.p, (const int*)c->d_chain_ev.p, (const long long*)c->d_ccuts.p, np, c->d_cbnd.p);
    HIPCHK(c, hipMemsetAsync(c->d_prov, 0, (size_t)SW_PROV_ROWS * (SW_MAX_CHUNKS + 1) * sizeof(unsigned), cs));
    c->ctr.kernel_launches++;
    return SW_OK;
}

// the level-bucketed sweep of the events [a, a + k): histogram of the heights, the levels' offsets, the events' descriptors
// scattered by level, then the sweep itself (`scs`: the span of that last kernel)
template <int NW>
int launch_cansee_levels(sw_ctx* c, int64_t a, int64_t k, int hmin, int nlev, Span* scs) {
    const int np = c->npad;
    hipStream_t cs = c->stream_cs;
    HIPCHK(c, hipMemsetAsync(c->d_lev_cnt.p, 0, nlev * sizeof(int32_t), cs));
    HIPCHK(c, hipMemsetAsync(c->d_lev_pin.p, 0, (size_t)k, cs));
    const int eb = (int)((k + 255) / 256);
    const int ringH = cansee_cfg(np, c->ring_H_req).H;
    hipLaunchKernelGGL(k_level_hist, dim3(eb), dim3(256), 0, cs, (const int*)c->d_ht.p, (int)a, (int)k, hmin, c->d_lev_cnt.p,
                       (const int*)c->d_cr.p, (const int*)c->d_op.p, (const int*)c->d_seq.p, (const int*)c->d_chain_start.p,
                       (const int*)c->d_chain_cnt.p, (const int*)c->d_chain_ev.p, ringH, c->d_lev_pin.p);
    hipLaunchKernelGGL(k_level_scan, dim3(1), dim3(1024), 0, cs, (const int*)c->d_lev_cnt.p, nlev, c->d_lev_start.p, c->d_lev_cursor.p);
    HIPCHK(c, hipMemsetAsync(c->d_lev_cback.p, 0, nlev * sizeof(int32_t), cs));
    hipLaunchKernelGGL(k_level_scatter, dim3(eb), dim3(256), 0, cs, (const int*)c->d_ht.p, (const int*)c->d_cr.p,
                       (const int*)c->d_sp.p, (const int*)c->d_op.p, (const int*)c->d_seq.p, (int)a, (int)k, hmin,
                       (const int*)c->d_lev_start.p, c->d_lev_cursor.p, c->d_lev_cback.p, c->d_desc.p, ringH, np,
                       (const unsigned char*)c->d_lev_pin.p, c->d_lev_pos.p);
    // pinned events in front of every level (the front cursors' exclusive scan), then the children's descriptors
    hipLaunchKernelGGL(k_level_scan, dim3(1), dim3(1024), 0, cs, (const int*)c->d_lev_cursor.p, nlev, c->d_lev_pinbase.p, c->d_lev_cback.p);
    hipLaunchKernelGGL(k_level_patch, dim3(eb), dim3(256), 0, cs, (const int*)c->d_ht.p, (const int*)c->d_cr.p, (const int*)c->d_op.p,
                       (const int*)c->d_seq.p, (int)a, (int)k, hmin, (const int*)c->d_lev_start.p, (const int*)c->d_lev_pinbase.p,
                       c->d_desc.p, ringH, np, (const int*)c->d_chain_start.p, (const int*)c->d_chain_cnt.p, (const int*)c->d_chain_ev.p,
                       (const int*)c->d_lev_pos.p);
    c->ctr.kernel_launches += 5;
    *scs = span_begin(c, cs);
    return launch_cansee<NW>(c, nlev, a);
}

// ---- phase: every can_see sweep of the call, enqueued on the sweep stream; behind sweep i its event and, in a gated call,
// the stage the round loop may advance to
template <int NW>
int enqueue_sweeps(sw_ctx* c, DivideCall& d) {
    hipStream_t cs = c->stream_cs;
    for (int i = 0; i < d.S; ++i) {
        const int64_t a = d.cut[i], k = d.cut[i + 1] - d.cut[i];
        Span scs{};
        if (d.preswept) {
            scs = span_begin(c, cs);
        } else if (d.flow && c->chunk_plan[i].G >= 2) {
            scs = span_begin(c, cs);
            CHK(launch_cansee_chunks<NW>(c, i));
        } else if (d.flow) {
            scs = span_begin(c, cs);
            CHK(launch_cansee_flow<NW>(c, i, a));
        } else {
            CHK(launch_cansee_levels<NW>(c, a, k, d.hmins[i], d.nlevs[i], &scs));
        }
        span_end(c, scs, cs);
        if (c->profiling) d.cansee_spans.push_back(scs);
        if (d.gated && !c->gate_lag) { hipLaunchKernelGGL(k_set_stage, dim3(1), dim3(64), 0, cs, loop_gate(c), i + 1); c->ctr.kernel_launches++; }
        HIPCHK(c, hipEventRecord(c->cs_events[i], cs));
    }
    if (c->profiling) (void)hipEventRecord(d.cs_t1, cs);
    return SW_OK;
}

// ---- round loops: what a loop needs in front of it and leaves behind it

// In front of a loop that adds the events up to sub-batch i.  Its start round = the smallest front round among the members
// it adds events to; a member's first event (swirld.py:195-198) opens round 0 for it: lo[0][m], chain position 0, uploaded
// in front of the loop.  Mutates c->front / c->lo0_h and fills d.clen from row i + 1 of the cut table (d.clen_prev is the
// row the loop before it ended at).  On the main stream: the wait for sweep `i_sweep`, then row 0 of the round table and the
// members' front rounds if a root is among the events.
int begin_loop(sw_ctx* c, DivideCall& d, int i, int i_sweep, int* r_start_out) {
    const int np = c->npad;
    int r_start = 0x7fffffff;
    bool row0_dirty = false;
    std::copy(c->bounds_stage.begin() + (size_t)(i + 1) * np, c->bounds_stage.begin() + (size_t)(i + 2) * np, d.clen.begin());
    for (int m = 0; m < c->n; ++m) {
        if (d.clen[m] > d.clen_prev[m]) {  // member touched by this sub-batch
            if (c->front[m] < 0) {         // its root (swirld.py:195-198): lo[0][m], chain position 0
                c->lo0_h[m] = c->first_ev[m];
                c->front[m] = 0;
                row0_dirty = true;
            }
            r_start = std::min(r_start, c->front[m]);
        }
    }
    *r_start_out = r_start == 0x7fffffff ? std::max(c->R - 1, 0) : r_start;
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->cs_events[i_sweep], 0));
    if (row0_dirty) {
        HIPCHK(c, hipMemcpyAsync(c->d_lo.p, c->lo0_h.data(), np * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        std::copy(c->front.begin(), c->front.end(), c->front_dev.begin());
        HIPCHK(c, hipMemcpyAsync(c->d_front.p, c->front_dev.data(), np * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    d.clk.mark(&c->stage_us[1]);
    return SW_OK;
}

// the chunk counters of sub-batch i's sweep, from the read-back slot read last
void chunk_check(sw_ctx* c, int i) {
    const sw_ctx::ChunkPlan& pl = c->chunk_plan[i];
    if (pl.G < 2) return;
    // the sweep of this sub-batch is complete (the loop waited for it) and its counters came back with the
    // loop state: provisional entries per chunk, entries the repair changed.  (A loop never reports SW_OK
    // without at least one read-back behind a shot that waited for cs_events[i]: h_rb is this sub-batch's or a later one.)
    const unsigned* pv = reinterpret_cast<const unsigned*>(c->h_rb + ((unsigned char*)c->d_prov - c->d_rb.p));
    for (int k = 1; k < pl.G; ++k) {
        const unsigned cnt = pv[(size_t)i * SW_MAX_CHUNKS + k];
        const int64_t len = pl.a[k + 1] - pl.a[k];
        c->ctr.chunk_provisional += cnt;
        if (cnt > (unsigned)std::min<int64_t>((len * c->n) / (32 * (c->chunk_cfg == 1 ? 2 : 4)), 0x7fffffff)) {
            c->ctr.chunk_resweeps++;
            c->chunks_off = true;   // this hashgraph has members silent for longer than the halo: sweep unchunked from now on
        }
    }
    c->ctr.chunk_repaired += pv[(size_t)SW_PROV_ROWS * SW_MAX_CHUNKS + i];
}

// what follows a finished loop i (its state is in c->h_rb): the chunk counters of its sweep — the gated loop's: of every
// sweep, all complete since the loop ended at the last stage, all against the slot read last —, the host mirror of the
// front rounds, and the tail of its sub-batch, armed here and enqueued by the next flush_tail
int after_loop(sw_ctx* c, DivideCall& d, int i, int r_start) {
    d.clk.mark(&c->stage_us[2]);
    HIPCHK(c, hipEventRecord(c->ev_loop_done, c->stream));
    for (int k = d.gated ? 0 : i; k <= i; ++k) chunk_check(c, k);
    // host mirror of the per-member front round (kept by the resolve kernel, read back with the loop state)
    for (int m = 0; m < c->n; ++m) c->front[m] = std::max(c->front[m], c->front_dev[m]);
    d.clen_prev.swap(d.clen);
    d.clk.mark(&c->stage_us[3]);
    CHK(ensure_rounds(c, c->R + 2));
    // (the early part of the sub-batch, below fin_from, is done)
    d.tail = DeferredTail{true, i, r_start, c->R, d.fin_from, d.cut[i + 1] - d.fin_from, c->ev_loop_done};
    d.clk.mark(&c->stage_us[4]);
    return SW_OK;
}

// the armed tail, if any, goes to the aux stream: round numbers and sees-masks of the sub-batch's remaining events, its
// witness rows, its voter masks.  Called behind the first shot of the next loop — host work that is off the critical path:
// the GPU is already busy with that shot — and once more at the end of the call, for the last sub-batch's.
template <int NW>
int flush_tail(sw_ctx* c, DivideCall& d) {
    DeferredTail& t = d.tail;
    if (!t.armed) return SW_OK;
    t.armed = false;
    const int np = c->npad;
    hipStream_t ax = c->stream_aux;
    HIPCHK(c, hipStreamWaitEvent(ax, t.loop_done, 0));
    if (t.i == 0 && c->profiling) { d.fin_t0 = next_event(c); (void)hipEventRecord(d.fin_t0, ax); }
    // (a finalize that runs beside the next round loop is throttled: fewer workgroups, less pressure on the loop's gathers;
    // the last one has nothing to hide behind and takes the whole GPU)
    const int blocks = (int)std::min<int64_t>((t.k0 + 3) / 4, t.i == d.S - 1 ? 8192 : c->fin_blocks);
    CHK(launch_finalize<NW>(c, ax, t.a0, t.k0, t.R, blocks));
    const int total = (t.R - t.r_start) * np;
    if (total > 0)
        hipLaunchKernelGGL(k_witness_table, dim3((total + 255) / 256), dim3(256), 0, ax,
                           (const int*)c->d_lo.p, t.R, t.r_start, np, c->d_wit.p);
    c->ctr.kernel_launches += 1;
    return launch_voter_masks<NW>(c, t.r_start, t.R, ax);
}

// ---- round loops: the mechanics both drivers share

// one round loop as the host follows it
struct LoopRun {
    RState st{};        // the loop state read back last
    int launched = 0;   // iterations enqueued
    int pieces = 0;     // gated loop: pieces enqueued in front of the top-ups (SW_DEBUG_TIMING)
    bool spans = false; // profiling: a span around every kernel of the loop (plain launches, no graphs)
    std::vector<Span> tally_spans, resolve_spans;
    // SW_DEBUG_TIMING: when the loop's set-up was enqueued, when the stream had drained the wait for the sweep in front of it
    std::chrono::steady_clock::time_point t_wait, t_loop;
    int64_t iters_before = 0;
    double waited_ms() const { return std::chrono::duration<double, std::milli>(t_loop - t_wait).count(); }
    double loop_ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_loop).count(); }
};

// the loop's k_loop_init on the main stream.  `fin_from`: the band pass writes the rounds of events from this one on
// (SW_FIN_BAND; none without it); `stages` > 0: the gated loop over that many rows of the cut table
void loop_start(sw_ctx* c, LoopRun& L, bool timed, int r_start, int64_t limit, const int32_t* visible_len, int64_t fin_from, int stages) {
    L.t_wait = std::chrono::steady_clock::now();
    L.iters_before = c->ctr.round_iterations;
    if (timed) (void)hipStreamSynchronize(c->stream);   // separates "waiting for the sweep" from the loop itself
    L.t_loop = std::chrono::steady_clock::now();
    const int np = c->npad;
    hipLaunchKernelGGL(k_loop_init, dim3(1), dim3(std::min(2 * np, 1024)), 0, c->stream, loop_bufs(c), np, r_start,
                       (int)limit, c->NEARCAP, (const int*)visible_len, c->d_chain_len.p, c->eval_src,
                       (int)std::min<int64_t>(c->fin_band ? fin_from : 0x7fffffff, 0x7fffffff),
                       (int)std::min<int64_t>(c->ctr.round_iterations - c->dbg_iter_base, 0x7fffffff),
                       stages, stages ? (const int*)c->d_bounds.p : (const int*)nullptr, stages ? (const long long*)c->d_cuts.p : (const long long*)nullptr);
    c->eval_src = 0;
    c->ctr.kernel_launches++;
}

// pinned read-back slot j of the call; -1: the slot that was read last
unsigned char* rb_slot(sw_ctx* c, int j) { return j < 0 ? c->h_rb : c->h_rb_all.p + (size_t)j * c->rb_bytes; }

// `n_it` more iterations on the main stream and behind them loop state, sweep error flag, the members' front rounds,
// tree-tally and chunk counters: ONE copy into pinned slot j, its event recorded behind the copy (j >= 0)
template <int NW>
int enqueue_shot(sw_ctx* c, LoopRun& L, int n_it, int j) {
    CHK(launch_iterations<NW>(c, n_it, L.spans ? &L.tally_spans : nullptr, L.spans ? &L.resolve_spans : nullptr));
    L.launched += n_it;
    if (c->split_failed) { c->poisoned = true; return fail(c, SW_EIO, "split round loop: a linked context did not arrive at iteration %lld (sw_split_link: every part calls sw_divide_rounds)", c->split_iter); }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(rb_slot(c, j), c->d_rb.p, c->rb_bytes, hipMemcpyDeviceToHost, c->stream));
    if (j >= 0) HIPCHK(c, hipEventRecord(c->rb_events[j], c->stream));
    return SW_OK;
}

// wait for slot j (its event; j < 0: the main stream) and decode it.  The front rounds are copied at every read-back;
// nothing reads front_dev before the loop has ended (after_loop), so the copies before the last one are only spare work.
int take_read_back(sw_ctx* c, LoopRun& L, int j) {
    if (j >= 0) HIPCHK(c, hipEventSynchronize(c->rb_events[j]));
    else HIPCHK(c, hipStreamSynchronize(c->stream));
    c->h_rb = rb_slot(c, j);
    memcpy(&L.st, c->h_rb, sizeof L.st);
    int ferr = 0;
    memcpy(&ferr, c->h_rb + 2 * sizeof(RState), sizeof ferr);
    memcpy(c->front_dev.data(), c->h_rb + 256, c->npad * sizeof(int32_t));
    if (ferr) return fail(c, SW_EIO, "can_see sweep gave up polling (code %d): internal protocol error", ferr);
    if (L.st.err) return fail(c, SW_ERANGE, "round table capacity exceeded (internal)");
    return SW_OK;
}

// rounds <= DAG height + 1, retries <= N / K: anything beyond that is a bug, not work.  `slack`: iterations the caller
// enqueues whatever the loop reports (a gated loop's predicted total, the SW_GATE_LAG schedule's forced waits)
int check_terminates(sw_ctx* c, const LoopRun& L, int64_t slack, int lag = 0) {
    if ((int64_t)L.launched <= (int64_t)c->max_height + 2 + c->N / c->K + 4096 + slack) return SW_OK;
    if (lag) return fail(c, SW_EIO, "round loop did not terminate after %d iterations (r=%d, SW_GATE_LAG=%d)", L.launched, L.st.r, lag);
    return fail(c, SW_EIO, "round loop did not terminate after %d iterations (r=%d)", L.launched, L.st.r);
}

// short top-ups behind the predicted iterations, until the loop reports done
inline int top_up_shot(int launched) { return launched < 8 ? 2 : (launched < 48 ? 8 : 4); }

// Early finalize beside a running loop, from a read-back `st` of it: the events below the band of the round in progress,
// [d.fin_from, upto), have their final round (round <= st.r - 1; rows 0 .. st.r of the table are committed and final: a round
// commits only when every member has its next-round event or is exhausted at the last stage).  `slot_read`: the event the
// aux stream waits for, if the host has not waited for the main stream itself.
template <int NW>
int early_finalize(sw_ctx* c, DivideCall& d, const RState& st, int64_t upto, hipEvent_t slot_read) {
    if (st.iter <= 0 || upto < d.fin_from + 16384) return SW_OK;
    if (slot_read) {
        HIPCHK(c, hipStreamWaitEvent(c->stream_aux, slot_read, 0));
        if (c->profiling && !d.fin_t0) { d.fin_t0 = next_event(c); (void)hipEventRecord(d.fin_t0, c->stream_aux); }
    }
    CHK(ensure_rounds(c, st.r + 2));   // (never grows in the gated loop: run_gated has ensured the rows of every iteration it enqueues)
    CHK(launch_finalize<NW>(c, c->stream_aux, d.fin_from, upto - d.fin_from, st.r + 1, c->fin_blocks));
    d.fin_from = upto;
    return SW_OK;
}

// the books of a finished loop over `n_events` new events (its last read-back is in c->h_rb)
void account_loop(sw_ctx* c, DivideCall& d, const LoopRun& L, int64_t n_events, bool gated) {
    const RState& st = L.st;
    // keep the rate estimate to runs where it means something (and, gated, to real schedules)
    if (n_events >= 4096 && !(gated && c->gate_lag)) {
        (gated ? c->gstat_iters : c->stat_iters) += st.iter;
        (gated ? c->gstat_events : c->stat_events) += n_events;
    }
    // the per-member exhaustion marks persist across runs; the next run reads half 0: its k_loop_init moves them there
    // (two small device copies here sat in the gap between two sub-batches' loops)
    c->eval_src = st.iter & 1;
    c->R = st.max_round + 1;
    if (c->unit_stake && c->tally_impl == 2) {   // the tree search counts the tallies it really evaluated (per member, read back with the state)
        const int32_t* tc = reinterpret_cast<const int32_t*>(c->h_rb + ((unsigned char*)c->d_treecnt - c->d_rb.p));
        for (int m = 0; m < c->npad; ++m) c->ctr.tally_evals += tc[m];
    } else
    c->ctr.tally_evals += (int64_t)st.evals;
    c->ctr.far_hops += (int64_t)st.far_hops;
    c->ctr.round_iterations += st.iter;   // (every iteration the loop executed; those of a gated loop that waited for the sweep also in gated_idle_iterations)
    if (gated) {
        c->ctr.gated_calls += 1;
        c->ctr.gated_idle_iterations += st.idle;
    }
    c->ctr.band_events += (int64_t)st.band_events;
    if (c->profiling) {
        float ms = 0.f;
        int cnt = 0;
        // only the launches that did work (iterations before `done`)
        for (size_t i = 0; i < L.tally_spans.size() && (int)i < st.iter - 1; ++i) { ms += span_ms(L.tally_spans[i]); ++cnt; }
        d.tally_ms += ms;
        d.tally_launches += cnt;
        for (size_t i = 0; i < L.resolve_spans.size() && (int)i < st.iter; ++i) { c->tm.resolve_ms += span_ms(L.resolve_spans[i]); c->tm.resolve_launches++; }
    }
}

// ---- driver: one round loop per sub-batch, over the events visible behind sweep i.  First shot: the predicted number of
// iterations (predict_shot), then short top-ups until the loop reports done; the host waits for every shot.
template <int NW>
int run_round_loop(sw_ctx* c, DivideCall& d, int i) {
    const int np = c->npad;
    const int64_t limit = d.cut[i + 1], n_new_events = d.cut[i + 1] - d.cut[i];
    int r_start = 0;
    CHK(begin_loop(c, d, i, i, &r_start));
    const bool dbg_t = c->debug_timing && d.K >= 65536;
    LoopRun L;
    L.spans = c->profiling && !c->split;
    d.fin_from = d.cut[i];
    loop_start(c, L, dbg_t, r_start, limit, c->d_bounds.p + (size_t)(i + 1) * np, d.cut[i], 0);
    int shot = predict_shot(c, n_new_events);
    // SW_MID_PCT (the last sub-batch of a large call has no later loop to hide its finalize behind): the first shot stops
    // `mid_pct` % of the way, the host looks at the loop state once and finalizes the events below the band of the round in
    // progress beside the rest of the loop instead of behind it; the rest of the prediction follows
    int rest = 0;
    if (i == d.S - 1 && n_new_events >= 65536 && shot >= 64 && c->mid_pct > 0) {
        const int head = std::max(2, (int)((int64_t)shot * c->mid_pct / 100) & ~1);
        rest = std::max(2, (shot - head) & ~1);
        shot = head;
    }
    for (;;) {
        CHK(ensure_rounds(c, c->R + L.launched + shot + 4));
        CHK(enqueue_shot<NW>(c, L, shot, -1));
        if (L.launched == shot) CHK(flush_tail<NW>(c, d));   // the previous sub-batch's, behind this one's first shot
        CHK(take_read_back(c, L, -1));
        if (L.st.done) break;
        CHK(check_terminates(c, L, 0));
        if (rest) {
            CHK(flush_tail<NW>(c, d));   // (the previous sub-batch's launches go first: same stream, same order as without the early part)
            CHK(early_finalize<NW>(c, d, L.st, std::min<int64_t>(L.st.mlo, limit), nullptr));
            shot = rest;
            rest = 0;
        } else
        shot = top_up_shot(L.launched);
    }
    account_loop(c, d, L, n_new_events, false);
    if (dbg_t) {
        const double l = L.loop_ms();
        const int64_t its = c->ctr.round_iterations - L.iters_before;
        fprintf(stderr, "[sw] sub-batch %d: %lld events, waited %.3f ms for the sweep, loop %.3f ms, %lld iterations (%.1f us each)\n",
                i, (long long)n_new_events, L.waited_ms(), l, (long long)its, its ? l * 1e3 / (double)its : 0.0);
    }
    return after_loop(c, d, i, r_start);
}

// ---- driver: the gated loop (SW_GATED=1): ONE round loop over the whole call.  The sweep stream publishes how many sub-batches it
// has swept (k_set_stage) and the resolve step latches that one iteration late: no seam between sub-batches (host round
// trip, read-back, k_loop_init, first-shot logic), no round searched twice, a member at the end of its visible chain waits
// in its round.  The predicted iterations of the whole call go out in pieces of about one sub-batch, each read back into
// its own pinned slot: the host waits for the previous piece while the next one runs, and finalizes the events below the
// band of the round in progress beside the loop; witness rows and voter masks follow the loop, as the last sub-batch's did.

// the piece read back into slot j, with the loop still running behind it: decode, then the early finalize (the aux stream
// waits for that read-back)
template <int NW>
int take_piece(sw_ctx* c, DivideCall& d, LoopRun& L, int j) {
    CHK(take_read_back(c, L, j));
    const RState& st = L.st;
    if (!c->fin_band || st.done) return SW_OK;
    return early_finalize<NW>(c, d, st, std::min<int64_t>(std::min(st.mlo, st.N), d.first + d.K), c->rb_events[j]);
}

// the schedule of a gated loop: `total` predicted iterations in P pieces, the host one piece behind the GPU; then top-ups,
// one read-back each
template <int NW>
int gated_schedule(sw_ctx* c, DivideCall& d, LoopRun& L, int total) {
    const int P = std::min(d.S, SW_PROV_ROWS);
    const int piece = std::max(2, (total / P) & ~1);
    int left = total, j = 0;
    bool taken_last = false;
    for (; left > 0 && j < P; ++j) {
        const int n_it = j == P - 1 ? left : std::min(left, piece);
        CHK(enqueue_shot<NW>(c, L, n_it, j));
        left -= n_it;
        if (j > 0) {   // (the GPU has piece j queued behind the one the host waits for)
            CHK(take_piece<NW>(c, d, L, j - 1));
            if (L.st.done) { taken_last = true; break; }
        }
    }
    L.pieces = j;
    if (!taken_last) CHK(take_read_back(c, L, j - 1));
    while (!L.st.done) {
        CHK(check_terminates(c, L, total));
        const int shot = top_up_shot(L.launched);
        CHK(ensure_rounds(c, c->R + L.launched + shot + 4));
        CHK(enqueue_shot<NW>(c, L, shot, 0));
        CHK(take_read_back(c, L, 0));
    }
    return SW_OK;
}

// SW_GATE_LAG (test hook): the stage schedule fixed by the ORDER OF LAUNCHES on the loop stream instead of by the race
// with the sweep stream.  Pieces of exactly `lag` iterations; behind each the loop stream waits for the sweeps of the
// next `gate_step` sub-batches and publishes them itself with the same k_set_stage: iteration t loads
// vis = min(S, 1 + (t / lag) * gate_step).  Nothing on the device waits for `vis`, every publication is enqueued
// behind a sweep already in the queue, and the iteration bound ends a loop that does not finish.  The pinned
// slots are reused in turn (the host is one piece behind, as in gated_schedule).
template <int NW>
int gated_schedule_lag(sw_ctx* c, DivideCall& d, LoopRun& L, int total) {
    const int lag = c->gate_lag, S = d.S;
    int pub = 1;   // (stage 1 is the loop's own start: k_loop_init)
    for (int j = 0;; ++j) {
        CHK(check_terminates(c, L, total + (int64_t)lag * S, lag));
        CHK(ensure_rounds(c, c->R + L.launched + lag + 4));
        CHK(enqueue_shot<NW>(c, L, lag, j % SW_PROV_ROWS));
        if (pub < S) {
            const int v = std::min(S, pub + c->gate_step);
            for (int i = pub; i < v; ++i) HIPCHK(c, hipStreamWaitEvent(c->stream, c->cs_events[i], 0));
            hipLaunchKernelGGL(k_set_stage, dim3(1), dim3(64), 0, c->stream, loop_gate(c), v);
            c->ctr.kernel_launches++;
            pub = v;
        }
        if (j > 0) {
            CHK(take_piece<NW>(c, d, L, (j - 1) % SW_PROV_ROWS));
            L.pieces = j;
            if (L.st.done) return SW_OK;
        }
    }
}

template <int NW>
int run_gated(sw_ctx* c, DivideCall& d) {
    const int np = c->npad, S = d.S;
    int r_start = 0;
    CHK(begin_loop(c, d, S - 1, 0, &r_start));   // (clen_prev is row 0: every member the call adds events to; the loop starts behind the first sweep)
    LoopRun L;
    L.spans = c->profiling;
    d.fin_from = d.first;
    loop_start(c, L, c->debug_timing, r_start, d.cut[1], c->d_bounds.p + np, d.first, S);
    const int total = predict_shot(c, d.K, true);
    CHK(ensure_rounds(c, c->R + total + 8));
    if (c->gate_lag > 0) CHK(gated_schedule_lag<NW>(c, d, L, total));
    else CHK(gated_schedule<NW>(c, d, L, total));
    account_loop(c, d, L, d.K, true);
    if (c->debug_timing) {
        fprintf(stderr, "[sw] gated loop: %d sub-batches, %lld events, waited %.3f ms for the first sweep, loop %.3f ms, %lld iterations + %d waiting, %d launched in %d pieces\n",
                S, (long long)d.K, L.waited_ms(), L.loop_ms(), (long long)(c->ctr.round_iterations - L.iters_before - L.st.idle), L.st.idle, L.launched, L.pieces);
    }
    return after_loop(c, d, S - 1, r_start);   // one tail for the whole call
}

// ---- phase: the three streams join, the books of the call
int finish_call(sw_ctx* c, DivideCall& d) {
    const int np = c->npad, S = d.S, R = c->R;
    const int64_t first = d.first, K = d.K;
    hipEvent_t fin_t1 = nullptr;
    if (c->profiling) { fin_t1 = next_event(c); (void)hipEventRecord(fin_t1, c->stream_aux); }
    // Everything later calls enqueue goes to the main stream (getters, decide_fame, find_order): it
    // waits for the other two streams ON THE DEVICE; the host returns without a synchronisation
    // (a Node makes one such call per gossip step — every host sync costs it ~15 us).
    HIPCHK(c, hipEventRecord(c->ev_aux_done, c->stream_aux));
    HIPCHK(c, hipEventRecord(c->ev_cs_done, c->stream_cs));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_aux_done, 0));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_cs_done, 0));
    span_end(c, d.sp_total);
    if (c->profiling || c->debug_timing) {
        HIPCHK(c, hipStreamSynchronize(c->stream_aux));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream_cs));
    }
    HIPCHK(c, hipGetLastError());
    std::copy(c->bounds_stage.begin() + (size_t)S * np, c->bounds_stage.begin() + (size_t)(S + 1) * np, c->divided_cnt.begin());
    d.clk.mark(&c->stage_us[5]);
    c->sw_dirty_from = std::max(R, 1);  // voter masks are up to date
    if (first + K == c->N) std::copy(c->head.begin(), c->head.end(), c->divided_head.begin());
    else for (int64_t e = first; e < first + K; ++e) c->divided_head[c->cr[e]] = (int32_t)e;
    c->divided = first + K;
    c->ctr.events_divided += K;
    c->ctr.rounds = R;
    if (c->profiling) {
        float ms = 0.f;
        if (d.cs_t0 && d.cs_t1) (void)hipEventElapsedTime(&ms, d.cs_t0, d.cs_t1);
        c->tm.can_see_ms = ms;   // on its own stream: overlaps rounds_ms
        c->tm.rounds_ms = span_ms(d.sp_rl);
        c->tm.tally_ms = d.tally_ms;
        c->tm.tally_launches = d.tally_launches;
        { float fm = 0.f; if (d.fin_t0 && fin_t1) (void)hipEventElapsedTime(&fm, d.fin_t0, fin_t1); c->tm.finalize_ms = fm; }  // aux stream span (overlaps)
        c->tm.total_ms = span_ms(d.sp_total);
        c->tm.cansee_kernel_ms = 0.f;
        c->tm.cansee_launches = (int32_t)d.cansee_spans.size();
        for (const Span& s_ : d.cansee_spans) c->tm.cansee_kernel_ms += span_ms(s_);
    }
    return SW_OK;
}

template <int NW>
int do_divide(sw_ctx* c, int64_t first, int64_t K) {
    const int np = c->npad;
    c->ev_used = 0;
    DivideCall d(c, first, K);
    c->stage_calls += 1;
    d.sp_total = span_begin(c);
    plan_cuts(c, d);
    choose_tally(c, d);
    CHK(test_preswept(c, d));
    CHK(size_level_tables(c, d));
    // ---- sweep stream: every can_see sweep of the call, behind the tables it reads
    CHK(open_sweep_stream(c, d));
    CHK(build_bounds(c, d));
    CHK(plan_chunks(c, d));
    CHK(enqueue_sweeps<NW>(c, d));
    d.clk.mark(&c->stage_us[0]);

    // ---- main stream: the round loops, each over the events visible so far; aux stream: the tails behind them
    if (d.bounds_pending) HIPCHK(c, hipEventSynchronize(c->ev_bounds));
    CHK(ensure_rounds(c, std::max(c->R, 1) + c->BATCH + 4));
    d.sp_rl = span_begin(c);
    d.clen_prev.assign(c->bounds_stage.begin(), c->bounds_stage.begin() + np);
    d.clen.assign(np, 0);
    if (d.gated) CHK(run_gated<NW>(c, d));
    else for (int i = 0; i < d.S; ++i) CHK(run_round_loop<NW>(c, d, i));
    CHK(flush_tail<NW>(c, d));   // the last sub-batch's
    span_end(c, d.sp_rl);
    return finish_call(c, d);
}

// first round not in `consensus` (swirld.py:226-228)
int first_undecided_round(const sw_ctx* c) {
    int max_c = 0;
    while (max_c < c->R && c->cons_h[max_c]) ++max_c;
    return max_c;
}

// voter masks (if stale) + the elections of the candidate rounds max_c + part, max_c + part + nparts, ...
template <int NW>
int fame_launch(sw_ctx* c, int max_c, int part, int nparts, Span* sp_el) {
    const int np = c->npad, R = c->R;
    if (c->payload_pending) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_payload, 0));  // coin bits of a bulk append
    // voter masks: normally already produced by divide_rounds (per sub-batch, overlapped)
    const uint32_t tot2 = 2u * c->tot;
    if (c->sw_dirty_from < R || R > c->Sw_rows) CHK(launch_voter_masks<NW>(c, std::min(c->sw_dirty_from, R), R, c->stream));
    c->sw_dirty_from = std::max(R, 1);
    const bool tiled = NW >= 2 && c->elect_impl == 1;
    if (tiled) CHK(dgrow(c, c->d_rsc, (size_t)3 * c->Rcap, 0));
    hipLaunchKernelGGL(k_fame_prep, dim3(std::max(1, std::min(64, (3 * R + 255) / 256))), dim3(256), 0, c->stream, c->d_newc.p + sizeof(FameCounters), R,
                       tiled ? c->d_rsc.p : nullptr, tiled ? 3 * R : 0);
    const int nblk = R - max_c - part > 0 ? (R - max_c - part + nparts - 1) / nparts : 0;
    const int call_idx = (int)c->fame_calls.size();
    if (sp_el) *sp_el = span_begin(c);
    if (nblk > 0) {
        bool split_done = false;
#define SW_ELECT_ARGS (const int*)c->d_wit.p, (const u64*)c->d_Sw.p, (const unsigned char*)c->d_coin.p, (const uint32_t*)c->d_stake.p, \
                      tot2, c->coin_period, max_c, R, np, c->d_fam.p, c->d_cons.p, c->d_newc.p + sizeof(FameCounters), c->d_fc, c->d_dec_call.p, c->d_dec_by.p, call_idx, part, nparts
        if constexpr (NW >= 2) {  // NW threads per candidate, a round as 64 NW / CG workgroups of CG candidates (k_elections_tiled)
            if (c->elect_impl == 1) {
#define SW_ELECT_TILED(CG_)                                                                                                             \
    do {                                                                                                                                \
        if (c->unit_stake) hipLaunchKernelGGL((k_elections_tiled<NW, true, CG_>), dim3(nblk * (64 * NW / (CG_))), dim3((CG_) * NW), 0, c->stream, SW_ELECT_ARGS, c->d_rsc.p);  \
        else hipLaunchKernelGGL((k_elections_tiled<NW, false, CG_>), dim3(nblk * (64 * NW / (CG_))), dim3((CG_) * NW), 0, c->stream, SW_ELECT_ARGS, c->d_rsc.p);                \
    } while (0)
                if constexpr (NW == 2) SW_ELECT_TILED(128);
                else if constexpr (NW == 4) {
                    if (c->elect_cg == 64) SW_ELECT_TILED(64);
                    else if (c->elect_cg == 256) SW_ELECT_TILED(256);
                    else SW_ELECT_TILED(128);
                } else if constexpr (NW == 8) SW_ELECT_TILED(128);
                else SW_ELECT_TILED(64);
#undef SW_ELECT_TILED
                split_done = true;
            }
        }
        if (!split_done) {
            if (c->unit_stake) hipLaunchKernelGGL((k_elections<NW, true>), dim3(nblk), dim3(np), 0, c->stream, SW_ELECT_ARGS);
            else hipLaunchKernelGGL((k_elections<NW, false>), dim3(nblk), dim3(np), 0, c->stream, SW_ELECT_ARGS);
        }
#undef SW_ELECT_ARGS
        c->ctr.kernel_launches++;
    }
    if (sp_el) span_end(c, *sp_el);
    HIPCHK(c, hipGetLastError());
    return SW_OK;
}

void fame_counters(sw_ctx* c, const FameCounters& fc) {
    c->ctr.voter_evals += (int64_t)(fc.voter_evals - c->fc_seen.voter_evals);
    c->ctr.majority_evals += (int64_t)(fc.majority_evals - c->fc_seen.majority_evals);
    c->ctr.coin_votes += (int64_t)(fc.coin_votes - c->fc_seen.coin_votes);
    c->ctr.coin_flips += (int64_t)(fc.coin_flips - c->fc_seen.coin_flips);
    c->fc_seen = fc;
}

template <int NW>
int do_fame(sw_ctx* c, int32_t* new_rounds, int cap, int* n_new) {
    const int R = c->R;
    c->ev_used = 0;
    Span sp = span_begin(c), sp_el{};
    const int max_c = first_undecided_round(c);
    CHK(fame_launch<NW>(c, max_c, 0, 1, &sp_el));
    // fame counters + new_c flags: one copy into pinned memory
    HIPCHK(c, hipMemcpyAsync(c->h_fame.p, c->d_newc.p, sizeof(FameCounters) + (size_t)R, hipMemcpyDeviceToHost, c->stream));
    span_end(c, sp);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    FameCounters fc;
    memcpy(&fc, c->h_fame.p, sizeof fc);
    const unsigned char* newc = c->h_fame.p + sizeof(FameCounters);
    const int call_idx = (int)c->fame_calls.size();
    c->fame_calls.push_back({max_c, R, c->divided});
    int cnt = 0;
    for (int r = 0; r < R; ++r)
        if (newc[r]) {
            c->cons_h[r] = 1;
            c->cons_call[r] = call_idx;
            if (cnt < cap && new_rounds) new_rounds[cnt] = r;
            ++cnt;
        }
    if (n_new) *n_new = cnt;
    fame_counters(c, fc);
    if (c->profiling) { c->tm.fame_ms = span_ms(sp); c->tm.elections_ms = span_ms(sp_el); }
    if (cnt > cap) return fail(c, SW_ERANGE, "new_rounds capacity %d < %d", cap, cnt);
    return SW_OK;
}

// Candidate-partitioned decide_fame (multi-GPU row (e)): this part's share of the elections; the
// context's own tables receive this part's decisions only, nothing enters `consensus` yet.
template <int NW>
int do_fame_partial(sw_ctx* c, int part, int nparts, int8_t* famous, uint8_t* decided) {
    const int np = c->npad, n = c->n, R = c->R;
    const int max_c = first_undecided_round(c);
    CHK(fame_launch<NW>(c, max_c, part, nparts, nullptr));
    std::vector<signed char> fam((size_t)R * np);
    HIPCHK(c, hipMemcpyAsync(c->h_fame.p, c->d_newc.p, sizeof(FameCounters) + (size_t)R, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(fam.data(), c->d_fam.p, fam.size(), hipMemcpyDeviceToHost, c->stream));
    // the kernel marks the rounds it completed in the device-side consensus flags; they become
    // official in sw_commit_fame, for every part alike
    HIPCHK(c, hipStreamSynchronize(c->stream));
    FameCounters fc;
    memcpy(&fc, c->h_fame.p, sizeof fc);
    const unsigned char* newc = c->h_fame.p + sizeof(FameCounters);
    for (int r = 0; r < R; ++r) {
        decided[r] = newc[r];
        const bool mine = r >= max_c && (r - max_c) % nparts == part;
        for (int m = 0; m < n; ++m) famous[(size_t)r * n + m] = (r < max_c || mine) ? fam[(size_t)r * np + m] : (signed char)-1;
    }
    fame_counters(c, fc);
    return SW_OK;
}

template <class T>
int get_round_rows(sw_ctx* c, const T* src, int r0, int r1, T* out, T absent) {
    if (!c || !out) return SW_EINVAL;
    if (r0 < 0 || r1 < r0) return fail(c, SW_ERANGE, "bad round range");
    const int np = c->npad, n = c->n;
    HIPCHK(c, hipSetDevice(c->device));
    const int rr = std::min(r1, c->R);
    std::vector<T> tmp((size_t)std::max(rr - r0, 0) * np);
    if (!tmp.empty()) {
        HIPCHK(c, hipMemcpyAsync(tmp.data(), src + (size_t)r0 * np, tmp.size() * sizeof(T), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    for (int r = r0; r < r1; ++r)
        for (int m = 0; m < n; ++m)
            out[(size_t)(r - r0) * n + m] = r < rr ? tmp[(size_t)(r - r0) * np + m] : absent;
    return SW_OK;
}


// Windowed mode: evict every can_see row no later call can read.  Rows still needed: every member's
// latest event (the self-parent row of its next event; recent other-parents), every member's first
// not-yet-ordered event and what follows it (find_order's chain searches start at the ordered
// prefix), and everything from the thresholds lo[r][.] of the oldest round still in play — the first
// round not in `consensus` or the oldest front round of a member, whichever is older (band rows,
// witness rows, voter masks, famous witnesses of rounds yet to be ordered).  A silent member pins
// the horizon at its last event; the reference keeps every row forever (swirld.py:69-72).
int window_evict(sw_ctx* c) {
    if (!c->vm.active || c->divided != c->N || c->N == 0) return SW_OK;
    const int n = c->n, np = c->npad;
    int64_t horizon = c->N;
    int fmin = 0x7fffffff;
    CHK(ensure_pool_h(c));
    // members that have LAPSED (sw_set_window_lapse; the reference has no such notion: it keeps every row): silent for more
    // than `window_lapse` events.  Their latest row, their unordered tail and their front round stop holding the window
    // back; in exchange their further events are refused — waking one would restart the round loop at its old front
    // round, whose band begins at thresholds long evicted.  No other path reads their old rows: a round's band and
    // tally only follow members with a witness in it, find_order only chains with a famous witness in the rounds it orders.
    if (c->window_lapse > 0) {
        if ((int)c->lapsed.size() != n) c->lapsed.assign(n, 0);
        for (int m = 0; m < n; ++m)
            if (c->head[m] >= 0 && (int64_t)c->head[m] < c->N - c->window_lapse) c->lapsed[m] = 1;
    }
    auto is_lapsed = [&](int m) { return c->window_lapse > 0 && c->lapsed[m]; };
    for (int m = 0; m < n; ++m) {
        if (is_lapsed(m)) continue;
        if (c->head[m] >= 0) horizon = std::min<int64_t>(horizon, c->head[m]);
        if (c->ord_pos[m] < c->nev[m]) horizon = std::min<int64_t>(horizon, c->chain_ev_h[(size_t)c->chain_start_h[m] + c->ord_pos[m]]);
        if (c->front[m] >= 0) fmin = std::min(fmin, c->front[m]);
    }
    const int rmin = std::min(first_undecided_round(c), fmin == 0x7fffffff ? 0 : fmin);
    if (rmin < c->R) {
        std::vector<int32_t> row(np);
        HIPCHK(c, hipMemcpyAsync(row.data(), c->d_lo.p + (size_t)rmin * np, np * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int m = 0; m < n; ++m) if (row[m] != SW_INF && !is_lapsed(m)) horizon = std::min<int64_t>(horizon, row[m]);
    } else horizon = 0;
    const size_t rowbytes = (size_t)np * sizeof(int32_t);
    CHK(vm_evict_below(c, (size_t)std::max<int64_t>(horizon, 0) * rowbytes));
    c->first_resident = (int64_t)((c->vm.lo * c->vm.chunk + rowbytes - 1) / rowbytes);
    return SW_OK;
}

// ==== sw_find_order, host side ====================================================================
// do_find_order (at the end of this section) calls the phases below in order; DESIGN.md §5 maps every phase to its
// function, to the stream it enqueues on and to what the host waits for.

// pinned staging of a find_order call (laid out by stage_order_call)
int ensure_order_host(sw_ctx* c, size_t bytes) {
    if (bytes <= c->h_ord.cap) return SW_OK;
    if (c->h_ord.p) HIPCHK(c, hipDeviceSynchronize());
    const size_t nc = bytes + bytes / 2 + 4096;
    if (!c->h_ord.reserve(nc)) return fail(c, SW_ENOMEM, "hipHostMalloc(%zu bytes) for find_order failed", nc);
    return SW_OK;
}

// pinned staging of the group bounds of a bulk find_order call
int ensure_order_stage(sw_ctx* c, size_t ints) {
    if (ints <= c->h_ord_stage.cap) return SW_OK;
    if (c->h_ord_stage.p) HIPCHK(c, hipDeviceSynchronize());
    if (!c->h_ord_stage.reserve(ints * 2 + 256)) return fail(c, SW_ENOMEM, "hipHostMalloc for find_order's group table failed");
    return SW_OK;
}

// ---- round received and consensus timestamp of the ordered events, kept on the device (consensus.hip.h) ----
// room for `tx_total` ordered events and for every stored event's two values; earlier records survive a growth
int consensus_reserve(sw_ctx* c, size_t tx_total) {
    const size_t ev = (size_t)std::max<int64_t>(c->cap, c->N);
    CHK(dgrow(c, c->cons.d_rr, ev, c->cons.d_rr.cap));
    CHK(dgrow(c, c->cons.d_cts, ev, c->cons.d_cts.cap));
    CHK(dgrow(c, c->cons.d_tx, tx_total, (size_t)c->cons.tx_len));
    return SW_OK;
}

int consensus_record_enqueue(sw_ctx* c, int64_t n_acc, size_t tx_at, int nr, const long long* acc_off, const int32_t* hostflag, const int32_t* sorted) {
    hipLaunchKernelGGL(cns::k_consensus_record, dim3((unsigned)((n_acc + cns::THREADS - 1) / cns::THREADS)), dim3(cns::THREADS), 0, c->stream,
                       (const int*)c->d_acc_ev.p, (const int*)c->d_acc_ri.p, (const int*)c->d_ord_rounds.p, (const unsigned long long*)c->d_ts.p,
                       (long long)n_acc, c->cons.d_rr.p, (unsigned long long*)c->cons.d_cts.p);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->cons.d_tx.p + tx_at, c->d_sorted.p, (size_t)n_acc * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    bool patched = false;
    for (int i = 0; i < nr; ++i) {
        const int64_t len = acc_off[i + 1] - acc_off[i];
        if (!hostflag[i] || !len) continue;
        HIPCHK(c, hipMemcpyAsync(c->cons.d_tx.p + tx_at + acc_off[i], sorted + acc_off[i], (size_t)len * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        patched = true;
    }
    if (patched) HIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

// The end of a find_order call that keeps its result: the two values of its n_acc events into the per-event tables, its part
// of the order behind d_tx[tx_at).  Enqueued on c->stream behind the call's last synchronisation and NOT waited for: the next
// find_order call synchronises c->stream (its lap "tables") before any of its side streams writes d_acc_ev, d_acc_ri, d_ts or
// d_sorted again, a dgrow of one of them drains the device, and every reader of the tables runs on c->stream.  Only a call
// with host-sorted rounds (rare) waits: their slices come from `sorted`, pinned memory the next call may move.
int consensus_record(sw_ctx* c, int64_t n_acc, size_t tx_at, int nr, const long long* acc_off, const int32_t* hostflag, const int32_t* sorted) {
    const int rc = consensus_record_enqueue(c, n_acc, tx_at, nr, acc_off, hostflag, sorted);
    if (rc != SW_OK) { c->poisoned = true; return rc; }   // (the host's order is extended, the device's is not)
    c->cons.tx_len = (int64_t)tx_at + n_acc;
    c->cons.record_calls++;
    c->cons.recorded += n_acc;
    return SW_OK;
}

constexpr int order_tile(int NW) { return NW <= 8 ? 16 : 8; }   // positions per tile of k_order_median: 16 KB of LDS at 256 members (8 workgroups per CU)
constexpr int order_cw(int NW) { return NW >= 4 ? 256 : 64 * NW; }   // columns per workgroup of k_order_walk

// the SW_ORDER_* switches of one call (read per call: the tests force either path between two calls of one process)
struct OrderKnobs {
    int64_t bulk_min;   // SW_ORDER_BULK: events from which a call takes the first-descendant table (0 = never) [16384]
    int64_t slab_mb;    // SW_ORDER_SLAB_MB: table per group [256 per 256 columns: 4 groups per 1 M events — 128 and 512 are both 0.15-0.3 ms slower, profiles/r06_measured_and_dropped.txt]
    int S;              // SW_ORDER_S: stretches per (member, column group) of the walk [enough for 1024 workgroups], 1..64
    bool one_stream;    // SW_ORDER_ONE_STREAM: one slab, everything on the main stream
    bool sort_inline;   // SW_ORDER_SORT_INLINE: a group's sort behind its samples, on their stream
    bool late_copy;     // SW_ORDER_LATE_COPY: the caller's copy in one piece at the end
    bool host;          // SW_ORDER_HOST: test hook: every round sorted by the host
    bool big_host;      // SW_ORDER_BIG_HOST: test hook: oversize rounds to the host, as before round 4
    bool timing;        // SW_DEBUG_TIMING: the laps below
};

OrderKnobs read_order_knobs(const sw_ctx* c) {
    OrderKnobs k;
    const char* e;
    k.bulk_min = (e = getenv("SW_ORDER_BULK")) ? atoll(e) : 16384;
    k.slab_mb = (e = getenv("SW_ORDER_SLAB_MB")) ? atoll(e) : 256 * std::max(1, c->nw / 4);
    const int wgs = c->n * (c->npad / order_cw(c->nw));   // workgroups of the walk per stretch
    k.S = std::min(std::max((e = getenv("SW_ORDER_S")) ? atoi(e) : (1024 + wgs - 1) / wgs, 1), 64);
    k.one_stream = getenv("SW_ORDER_ONE_STREAM") != nullptr;
    k.sort_inline = getenv("SW_ORDER_SORT_INLINE") != nullptr;
    k.late_copy = getenv("SW_ORDER_LATE_COPY") != nullptr;
    k.host = getenv("SW_ORDER_HOST") != nullptr;
    k.big_host = getenv("SW_ORDER_BIG_HOST") != nullptr;
    k.timing = getenv("SW_DEBUG_TIMING") != nullptr;
    return k;
}

// host laps of one call under SW_DEBUG_TIMING, each behind a synchronisation of the main stream (profiles/order_laps.py)
struct OrderLaps {
    bool on;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    void lap(sw_ctx* c, const char* what, hipStream_t side = nullptr) {   // side: a side stream to wait for first
        if (!on) return;
        if (side) (void)hipStreamSynchronize(side);
        (void)hipStreamSynchronize(c->stream);
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[find_order] %-10s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - last).count());
        last = t;
    }
};

// The read-back block of a call, d_oblk on the device and its image in the pinned block: [OrderInfo][ord_new: npad ints]
// [acc_off: nr + 1 long long], fetched with ONE copy (and its OrderInfo once more at the end of the call).
struct OrderBlock {
    OrderInfo* info = nullptr;
    int32_t* ordnew = nullptr;       // members' ordered prefixes behind this call
    long long* acc_off = nullptr;    // [nr + 1] first ordered event of every round entry
    OrderBlock() = default;
    OrderBlock(void* base, int np) : info(static_cast<OrderInfo*>(base)), ordnew(reinterpret_cast<int32_t*>(info + 1)), acc_off(reinterpret_cast<long long*>(ordnew + np)) {}
    static size_t bytes(int np, int nr) { return sizeof(OrderInfo) + (size_t)np * 4 + ((size_t)nr + 1) * 8; }
};
static_assert(sizeof(OrderInfo) % 8 == 0, "acc_off follows OrderInfo and an even number of ints");

struct OrderSpan { int i0, i1; };   // the round entries [i0, i1) of a group

// one sw_find_order call: what its phases hand on to each other (buffers that outlive the call stay in sw_ctx)
struct OrderCall {
    const OrderKnobs k;
    const std::vector<int32_t> rounds;   // sorted, unique: the round entries
    const int nr;
    int32_t* const out_events;           // the caller's array (may be NULL) and its capacity
    const int64_t cap;
    // views into the pinned block (stage_order_call)
    int32_t *h_rounds = nullptr, *h_ordpos = nullptr, *hostflag = nullptr;   // hostflag[i]: the host sorts round entry i
    OrderInfo* h_init = nullptr;
    OrderBlock h;                        // the read-back block
    // views into d_oblk, d_seg, d_fwm
    OrderBlock d;
    int32_t *d_seg_start = nullptr, *d_seg_len = nullptr, *d_seg_off = nullptr, *d_fwseq = nullptr;
    int64_t n_acc = 0;                   // events the call orders
    size_t tx_at = 0;                    // ... behind this many of earlier calls
    int32_t* sorted = nullptr;           // transactions + tx_at: the device-sorted order lands in place
    // rounds too large for the LDS sort (plan_order_sorts)
    std::vector<int32_t> big_ri;
    std::vector<long long> big_off{0};
    bool fetch_early = false;            // every sort is followed by the copy of its part of the order to the host
    bool bulk = false;                   // the first-descendant table (else one search per (event, famous witness))
    // groups and slabs of a bulk call (plan_order_groups)
    std::vector<OrderSpan> groups;
    int64_t stride = 0;                  // entries between two members' planes of a slab
    bool two = false;                    // two slabs, side streams
    hipStream_t s1 = nullptr;            // the stream of the table's consumers
    hipStream_t tail = nullptr;          // the stream the last kernels of the call are on
    bool copied_early = false;           // out_events already holds the order as the device sorted it
    bool any_host_sorted = false;        // the host re-sorted rounds of it
    std::vector<int32_t> acc_ev;         // host copies, fetched only for the rounds the host has to sort
    std::vector<double> ts;
    std::vector<unsigned char> white_h;
    int64_t produced = 0;
    OrderLaps clk;
    OrderCall(sw_ctx* c, std::vector<int32_t>&& rounds_, int32_t* out_events_, int64_t cap_)
        : k(read_order_knobs(c)), rounds(std::move(rounds_)), nr((int)rounds.size()), out_events(out_events_), cap(cap_), tx_at(c->transactions.size()), tail(c->stream), clk{k.timing} {}
};

// the call's part of `transactions`: from its growth (order_reserve) on, every return that does not keep the call's result
// gives it back, so that sw_num_ordered, sw_get_transactions, ord_pos and the device's tables go on agreeing.  The device is
// drained first: after a HIP error in the middle of the groups, copies into that part may still be in flight on the sort
// streams, and the next call may grow (and move) the array.
struct OrderRollback {
    sw_ctx* c;
    const OrderCall& o;
    bool armed;
    ~OrderRollback() { if (armed) { (void)hipDeviceSynchronize(); c->transactions.resize(o.tx_at); } }
};

// ---- phase: the rounds argument, shared with exact_order: sorted(new_c), swirld.py:283, every round once and known
int order_rounds_arg(sw_ctx* c, std::vector<int32_t>& rounds) {
    std::sort(rounds.begin(), rounds.end());
    rounds.erase(std::unique(rounds.begin(), rounds.end()), rounds.end());
    if (!rounds.empty() && (rounds.front() < 0 || rounds.back() >= c->R))
        return fail(c, SW_ERANGE, "find_order: round outside [0, %d) (KeyError in the reference)", c->R);
    return SW_OK;
}

// ---- phase: staging and the table buffers.  The pinned block is [rounds: nr][ordpos: npad][OrderInfo init][read-back block]
// [hostflag: nr], every part on a 64-byte boundary; this function alone knows the offsets.  The tables of
// the call are all on the device: f_w (:284), q (:288-293), ordered prefixes per entry, segment offsets.
int stage_order_call(sw_ctx* c, OrderCall& o) {
    const int np = c->npad, nr = o.nr;
    if ((int64_t)(nr + 1) * np >= (1ll << 31)) return fail(c, SW_ERANGE, "find_order: %d rounds x %d columns exceed 2^31 table entries", nr, np);
    const size_t blk = OrderBlock::bytes(np, nr);
    const size_t ordpos_off = ((size_t)nr * 4 + 63) & ~(size_t)63, init_off = ordpos_off + (size_t)np * 4, blk_off = init_off + 64,
                 flag_off = blk_off + ((blk + 63) & ~(size_t)63);
    CHK(ensure_order_host(c, flag_off + (size_t)nr * 4));
    o.h_rounds = reinterpret_cast<int32_t*>(c->h_ord.p);
    o.h_ordpos = reinterpret_cast<int32_t*>(c->h_ord.p + ordpos_off);
    o.h_init = reinterpret_cast<OrderInfo*>(c->h_ord.p + init_off);
    o.h = OrderBlock(c->h_ord.p + blk_off, np);
    o.hostflag = reinterpret_cast<int32_t*>(c->h_ord.p + flag_off);
    std::copy(o.rounds.begin(), o.rounds.end(), o.h_rounds);
    std::fill(o.h_ordpos, o.h_ordpos + np, 0);
    std::copy(c->ord_pos.begin(), c->ord_pos.end(), o.h_ordpos);
    *o.h_init = OrderInfo{0, 0x7fffffff, 0, {0, 0, 0, 0}};
    CHK(dgrow(c, c->d_ord_rounds, nr, 0));
    CHK(dgrow(c, c->d_fwm, (size_t)2 * nr * np, 0));   // [famous witness | its chain position] per (entry, member)
    CHK(dgrow(c, c->d_q, (size_t)nr * np, 0));
    CHK(dgrow(c, c->d_ordat, (size_t)(nr + 1) * np, 0));
    CHK(dgrow(c, c->d_seg, (size_t)3 * nr * np, 0));
    CHK(dgrow(c, c->d_rowsum, nr, 0));
    CHK(dgrow(c, c->d_oblk, blk / 8, 0));
    CHK(dgrow(c, c->d_ordpos, np, 0));
    o.d = OrderBlock(c->d_oblk.p, np);
    o.d_seg_start = c->d_seg.p; o.d_seg_len = c->d_seg.p + (size_t)nr * np; o.d_seg_off = c->d_seg.p + (size_t)2 * nr * np;
    o.d_fwseq = c->d_fwm.p + (size_t)nr * np;
    HIPCHK(c, hipMemcpyAsync(c->d_ord_rounds.p, o.h_rounds, (size_t)nr * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_ordpos.p, o.h_ordpos, (size_t)np * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(o.d.info, o.h_init, sizeof(OrderInfo), hipMemcpyHostToDevice, c->stream));
    return SW_OK;
}

// ---- phase: the tables.  Five kernels, ONE read-back (events per entry, error words, new prefixes) and the first of the
// call's two synchronisations: all the host sees before it sizes the bulk kernels.
template <int NW>
int order_tables(sw_ctx* c, OrderCall& o) {
    const int np = c->npad, n = c->n, nr = o.nr;
    hipLaunchKernelGGL(k_order_prep, dim3(nr), dim3(np), 0, c->stream, (const int*)c->d_ord_rounds.p, (const int*)c->d_wit.p,
                       (const signed char*)c->d_fam.p, (const int*)c->d_seq.p, n, np, c->d_fwm.p, o.d_fwseq, o.d.info);
    hipLaunchKernelGGL(k_order_bounds<NW>, dim3(nr, NW), dim3(64 * NW), 0, c->stream, (const int*)c->d_fwm.p, (const int*)c->d_L.p,
                       (const int*)c->d_seq.p, (const uint32_t*)c->d_stake.p, c->tot, (const int*)c->d_chain_start.p,
                       (const int*)c->d_chain_cnt.p, (const int*)c->d_chain_ev.p, n, (int)(c->N - 1), c->d_q.p);
    hipLaunchKernelGGL(k_order_runmax, dim3(1), dim3(np), 0, c->stream, (const int*)c->d_q.p, (const int*)c->d_ordpos.p, nr, np,
                       c->d_ordat.p, o.d_seg_start, o.d_seg_len, o.d.ordnew);
    hipLaunchKernelGGL(k_order_rowscan, dim3(nr), dim3(np), 0, c->stream, (const int*)o.d_seg_len, np, o.d_seg_off, c->d_rowsum.p);
    hipLaunchKernelGGL(k_order_offsets, dim3(1), dim3(1024), 0, c->stream, (const int*)c->d_rowsum.p, nr, o.d.acc_off, o.d.info);
    c->ctr.kernel_launches += 5;
    HIPCHK(c, hipMemcpyAsync(o.h.info, o.d.info, OrderBlock::bytes(np, nr), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    o.clk.lap(c, "tables");
    if (o.h.info->undecided_ri != 0x7fffffff)
        return fail(c, SW_EINVAL, "find_order: round %d has an undecided witness (KeyError on self.famous[w], swirld.py:284)", o.rounds[o.h.info->undecided_ri]);
    o.n_acc = o.h.info->n_acc;
    if (o.n_acc > 0x7ffffff0ll) return fail(c, SW_ERANGE, "find_order: more than 2^31 events in one call");
    return SW_OK;
}

// ---- phase: room for the call's events: its part of `transactions` (from here on OrderRollback gives it back), the
// per-event buffers, the consensus tables
int order_reserve(sw_ctx* c, OrderCall& o) {
    const int nr = o.nr;
    const int64_t n_acc = o.n_acc;
    std::fill(o.hostflag, o.hostflag + nr, 0);
    if (!c->transactions.resize(o.tx_at + (size_t)n_acc)) return fail(c, SW_ENOMEM, "pinned host memory for the ordered events");   // the device-sorted order lands in place
    o.sorted = c->transactions.data() + o.tx_at;
    if (!n_acc) return SW_OK;
    CHK(dgrow(c, c->d_acc_ev, n_acc, 0));
    CHK(dgrow(c, c->d_acc_ri, n_acc, 0));
    CHK(dgrow(c, c->d_ts, n_acc, 0));
    CHK(dgrow(c, c->d_white, (size_t)nr * 64, 0));
    CHK(dgrow(c, c->d_sorted, n_acc, 0));
    CHK(dgrow(c, c->d_hostflag, nr, 0));
    CHK(consensus_reserve(c, o.tx_at + (size_t)n_acc));
    return SW_OK;
}

// ---- phase: which sorts, which samples
void plan_order_sorts(const sw_ctx* c, OrderCall& o) {
    // rounds too large for the LDS sort: the same network over global scratch, one workgroup per such round (behind everything else)
    for (int i = 0; i < o.nr; ++i) {
        const int64_t len = o.h.acc_off[i + 1] - o.h.acc_off[i];
        if (len <= SORT_CAP || o.k.big_host) continue;
        int64_t m = 1;
        while (m < len) m <<= 1;
        o.big_ri.push_back(i);
        o.big_off.push_back(o.big_off.back() + m);
    }
    o.fetch_early = o.big_ri.empty();   // (oversize rounds are sorted last: then the whole order travels at the end)
    // A call that orders many events: the first-descendant table (k_order_walk) instead of one binary search per
    // (event, famous witness) pair.  Same samples, by construction and by test (SW_ORDER_BULK=<events> moves the
    // threshold, 0 = never).
    // Beyond 512 members every call takes the table: the search kernel's 16-word instance keeps ~90 wave masks alive around
    // its divergent chain searches, the compiler spills them, and the timestamps came back wrong AND different from run
    // to run (1024 members x 100 k events, profiles/r06_order_search_16_words.txt) — it is not built.
    o.bulk = c->nw > 8 || (o.k.bulk_min > 0 && o.n_acc >= o.k.bulk_min);
}

// ---- phase: groups and slabs of a bulk call.
// The table is built for GROUPS of consecutive round entries whose events fit SW_ORDER_SLAB_MB
// of table — a slab that stays allocated instead of one table as large as the can_see rows of everything the call
// orders — and there are TWO slabs: the samples, the sort and the read-back of group g run on a second stream
// beside the walk of group g + 1 (the walk is bound by its stores, the samples by their selection loops).
int plan_order_groups(sw_ctx* c, OrderCall& o) {
    const int np = c->npad, n = c->n, nr = o.nr, P = order_tile(c->nw);
    const long long* acc_off = o.h.acc_off;
    const int64_t pad = (int64_t)P * np;   // every chain rounds its positions up to whole tiles
    const int64_t slab_pos = std::max<int64_t>(2 * pad, (o.k.slab_mb << 20) / ((int64_t)n * 4));
    int64_t stride = 0;
    for (int i0 = 0; i0 < nr;) {
        int i1 = i0 + 1;
        while (i1 < nr && acc_off[i1 + 1] - acc_off[i0] + pad <= slab_pos) ++i1;
        if (acc_off[i1] > acc_off[i0]) { o.groups.push_back({i0, i1}); stride = std::max<int64_t>(stride, acc_off[i1] - acc_off[i0] + pad); }
        i0 = i1;
    }
    // the planes of the members sit `stride` entries apart and are read / written at the same offsets at the same
    // time: 4 KB x odd + 256 B between them, so that they spread over the memory channels whatever the interleaving
    // granule (a power of two — 131 072 entries for a full slab — put all 256 planes' lines on one channel)
    o.stride = (((stride + 1023) >> 10) | 1) * 1024 + 64;
    const size_t ng = o.groups.size();
    o.two = ng > 1 && !o.k.one_stream;
    CHK(dgrow(c, c->d_fd, (size_t)o.stride * n * (o.two ? 2 : 1), 0));
    CHK(dgrow(c, c->d_grp, (OrderGroup::ints(np) + 2) * std::max<size_t>(ng, 1), 0));
    int32_t* d_gbounds = c->d_grp.p + OrderGroup::ints(np) * ng;
    CHK(ensure_order_stage(c, ng * 2));
    for (size_t gi = 0; gi < ng; ++gi) { c->h_ord_stage.p[2 * gi] = o.groups[gi].i0; c->h_ord_stage.p[2 * gi + 1] = o.groups[gi].i1; }
    HIPCHK(c, hipMemcpyAsync(d_gbounds, c->h_ord_stage.p, ng * 2 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_order_group, dim3((unsigned)ng), dim3(np), 0, c->stream, (const int*)c->d_ordat.p, (const int*)c->d_fwm.p,
                       (const int*)c->d_chain_start.p, (const int*)c->d_chain_cnt.p, (const int*)c->d_chain_ev.p, (const int*)d_gbounds, n, np, P, c->d_grp.p);
    c->ctr.kernel_launches++;
    if (o.two) {
        for (Stream* st : {&c->stream_ord, &c->stream_srt[0], &c->stream_srt[1]})
            if (!*st) {
                hipStream_t made = nullptr;
                HIPCHK(c, hipStreamCreateWithFlags(&made, hipStreamNonBlocking));
                st->reset(made);
            }
        while (c->ord_events.size() < 3 * ng + 3) {   // per group: table walked / table consumed / order on the host; then the ends of the three side streams
            c->ord_events.emplace_back();
            CHK(ensure_event(c, c->ord_events.back()));
        }
    }
    o.s1 = o.two ? c->stream_ord : c->stream;
    return SW_OK;
}

// ---- phase: what only the consumers of the table need (the ordered events round-major, the whitening keys, cleared flags):
// enqueued on THEIR stream, beside the first walk (the tables it reads are complete: the host has waited for them)
int consumer_preamble(sw_ctx* c, const OrderCall& o, hipStream_t st) {
    const int np = c->npad, nr = o.nr;
    HIPCHK(c, hipMemsetAsync(c->d_hostflag.p, 0, nr * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_order_segments, dim3((unsigned)(((size_t)nr * np + 255) / 256)), dim3(256), 0, st, (const int*)o.d_seg_start,
                       (const int*)o.d_seg_len, (const int*)o.d_seg_off, (const long long*)o.d.acc_off, (const int*)c->d_chain_start.p,
                       (const int*)c->d_chain_ev.p, np, nr * np, c->d_acc_ev.p, c->d_acc_ri.p);
    hipLaunchKernelGGL(k_order_white, dim3(nr), dim3(1024), 0, st, (const int*)c->d_fwm.p, c->n, np,
                       (const unsigned char*)c->d_sig.p, c->d_white.p);
    c->ctr.kernel_launches += 2;
    return SW_OK;
}

// ... and, for the samples of a bulk call, the timestamps in chain order from the position in front of every member's first
// unordered event on
int enqueue_tchain(sw_ctx* c, const OrderCall& o) {
    const int n = c->n;
    CHK(dgrow(c, c->d_tch, c->d_chain_ev.cap, 0));
    int longest = 1;
    for (int m = 0; m < n; ++m) longest = std::max(longest, c->nev[m] - c->ord_pos[m] + 1);
    hipLaunchKernelGGL(k_order_tchain, dim3(n, (unsigned)std::min(64, (longest + 255) / 256)), dim3(256), 0, o.s1, (const int*)c->d_chain_start.p,
                       (const int*)c->d_chain_cnt.p, (const int*)c->d_chain_ev.p, (const int*)c->d_ordpos.p, (const double*)c->d_t.p, c->d_tch.p);
    c->ctr.kernel_launches++;
    return SW_OK;
}

// device sort of the round entries [i0, i1) by (ts, first 8 whitened key bytes), then their part of the order to the host
int sort_and_fetch(sw_ctx* c, const OrderCall& o, hipStream_t st, int i0, int i1) {
    hipLaunchKernelGGL(k_order_sort, dim3(i1 - i0), dim3(1024), 0, st, (const int*)c->d_acc_ev.p,
                       (const long long*)o.d.acc_off, (const double*)c->d_ts.p, (const unsigned char*)c->d_sig.p,
                       (const unsigned char*)c->d_white.p, i0, c->d_sorted.p, c->d_hostflag.p);
    c->ctr.kernel_launches++;
    const int64_t a0 = o.h.acc_off[i0], na = o.h.acc_off[i1] - a0;
    if (o.fetch_early && na) HIPCHK(c, hipMemcpyAsync(o.sorted + a0, c->d_sorted.p + a0, na * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    return SW_OK;
}

// ---- phase: one group: its walk on the main stream into the slab of its parity, its samples on s1, its sort and the
// read-back of its part of the order on a sort stream of its parity.  Events 3 gi / 3 gi + 1 / 3 gi + 2: table walked /
// table consumed / order on the host.
template <int NW>
int enqueue_group(sw_ctx* c, OrderCall& o, size_t gi) {
    constexpr int P = order_tile(NW), CW = order_cw(NW);
    const int np = c->npad, n = c->n, ncg = np / CW, S = o.k.S;
    const OrderSpan& g = o.groups[gi];
    const bool two = o.two;
    hipStream_t s1 = o.s1;
    int* grp = c->d_grp.p + OrderGroup::ints(np) * gi;
    int* fd = c->d_fd.p + (two && (gi & 1) ? (size_t)o.stride * n : 0);
    const int64_t na = o.h.acc_off[g.i1] - o.h.acc_off[g.i0];
    if (two && gi >= 2) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ord_events[3 * (gi - 2) + 1], 0));   // the slab's last reader
    hipLaunchKernelGGL(k_order_walk<CW>, dim3((unsigned)((size_t)n * ncg * S)), dim3(CW), 0, c->stream, (const int*)c->d_L.p,
                       (const int*)c->d_seq.p, (const int*)c->d_chain_start.p, (const int*)c->d_chain_ev.p, (const int*)c->d_ordat.p,
                       g.i0, g.i1, (const int*)grp, np, S, P, (long long)o.stride, fd);
    o.clk.lap(c, "walk", s1);
    if (two) {
        HIPCHK(c, hipEventRecord(c->ord_events[3 * gi], c->stream));
        HIPCHK(c, hipStreamWaitEvent(s1, c->ord_events[3 * gi], 0));
    }
    hipLaunchKernelGGL((k_order_median<NW, P>), dim3((unsigned)(na / P + n)), dim3(256), 0, s1, (const int*)fd,
                       (long long)o.stride, (const int*)grp, (const int*)c->d_ordat.p, g.i0, g.i1, n, (const int*)o.d_fwseq,
                       (const long long*)o.d.acc_off, (const int*)o.d_seg_off, (const int*)c->d_chain_start.p, (const double*)c->d_tch.p,
                       c->d_ts.p, o.d.info);
    o.clk.lap(c, "median", s1);
    hipStream_t s2 = s1;
    if (two) {
        HIPCHK(c, hipEventRecord(c->ord_events[3 * gi + 1], s1));
        if (!o.k.sort_inline) {
            s2 = c->stream_srt[gi & 1];
            HIPCHK(c, hipStreamWaitEvent(s2, c->ord_events[3 * gi + 1], 0));
        }
    }
    c->ctr.kernel_launches += 2;
    CHK(sort_and_fetch(c, o, s2, g.i0, g.i1));
    if (two && o.fetch_early) HIPCHK(c, hipEventRecord(c->ord_events[3 * gi + 2], s2));
    return SW_OK;
}

// ---- phase: the side streams join the main one (round entries that order nothing keep their zeroed flag and have nothing to
// sort), then the early copy to the caller
int join_and_copy_early(sw_ctx* c, OrderCall& o) {
    if (!o.two) return SW_OK;
    hipStream_t side[3] = {c->stream_ord, c->stream_srt[0], c->stream_srt[1]};
    for (int k = 0; k < 3; ++k) {
        hipEvent_t e = c->ord_events[3 * o.groups.size() + k];
        HIPCHK(c, hipEventRecord(e, side[k]));
        HIPCHK(c, hipStreamWaitEvent(c->stream, e, 0));
    }
    // the caller's copy of the order, group by group as it arrives, while the device works on the later groups
    if (!(o.fetch_early && o.out_events && !o.k.host && !o.k.late_copy)) return SW_OK;
    for (size_t gi = 0; gi < o.groups.size(); ++gi) {
        HIPCHK(c, hipEventSynchronize(c->ord_events[3 * gi + 2]));
        const int64_t a0 = o.h.acc_off[o.groups[gi].i0], a1 = std::min<int64_t>(o.h.acc_off[o.groups[gi].i1], o.cap);
        if (a1 > a0) memcpy(o.out_events + a0, o.sorted + a0, (size_t)(a1 - a0) * sizeof(int32_t));
    }
    o.copied_early = true;
    return SW_OK;
}

// ---- phase: a small call: one search per (event, famous witness) pair and one sort, all on the main stream
template <int NW>
int order_small_call(sw_ctx* c, const OrderCall& o) {
    CHK(consumer_preamble(c, o, c->stream));
    if constexpr (NW <= 8) {
        hipLaunchKernelGGL(k_order_times<NW>, dim3((unsigned)((o.n_acc + 3) / 4)), dim3(256), 0, c->stream,
                           (const int*)c->d_acc_ev.p, (const int*)c->d_acc_ri.p, (int)o.n_acc, (const int*)c->d_fwm.p,
                           (const int*)c->d_L.p, (const int*)c->d_cr.p, (const int*)c->d_seq.p,
                           (const double*)c->d_t.p, (const int*)c->d_chain_start.p, (const int*)c->d_chain_ev.p,
                           (const int*)c->d_ordpos.p, c->d_ts.p, o.d.info);
        c->ctr.kernel_launches++;
    }
    return sort_and_fetch(c, o, c->stream, 0, o.nr);
}

// ---- phase: the oversize rounds, sorted over global scratch behind everything else; then the whole order travels at once
int sort_big_rounds(sw_ctx* c, const OrderCall& o) {
    if (o.big_ri.empty()) return SW_OK;
    CHK(dgrow(c, c->d_big_ri, o.big_ri.size(), 0));
    CHK(dgrow(c, c->d_big_off, o.big_off.size(), 0));
    CHK(dgrow(c, c->d_sk_ts, (size_t)o.big_off.back(), 0));
    CHK(dgrow(c, c->d_sk_k8, (size_t)o.big_off.back(), 0));
    CHK(dgrow(c, c->d_sk_ev, (size_t)o.big_off.back(), 0));
    // (pageable sources: the copies are staged before the call returns)
    HIPCHK(c, hipMemcpyAsync(c->d_big_ri.p, o.big_ri.data(), o.big_ri.size() * sizeof(int32_t), hipMemcpyHostToDevice, o.tail));
    HIPCHK(c, hipMemcpyAsync(c->d_big_off.p, o.big_off.data(), o.big_off.size() * sizeof(long long), hipMemcpyHostToDevice, o.tail));
    hipLaunchKernelGGL(k_order_sort_big, dim3((unsigned)o.big_ri.size()), dim3(1024), 0, o.tail, (const int*)c->d_big_ri.p,
                       (const long long*)c->d_big_off.p, (const int*)c->d_acc_ev.p, (const long long*)o.d.acc_off,
                       (const double*)c->d_ts.p, (const unsigned char*)c->d_sig.p, (const unsigned char*)c->d_white.p,
                       c->d_sk_ts.p, c->d_sk_k8.p, c->d_sk_ev.p, c->d_sorted.p, c->d_hostflag.p);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipMemcpyAsync(o.sorted, c->d_sorted.p, o.n_acc * sizeof(int32_t), hipMemcpyDeviceToHost, o.tail));
    return SW_OK;
}

// ---- phase: the final read-back and the second of the call's two synchronisations: OrderInfo again (the samples' error
// word), the rounds the device left to the host; only for those a third one, behind the copies their host sort needs
int order_read_back(sw_ctx* c, OrderCall& o) {
    const int nr = o.nr;
    HIPCHK(c, hipMemcpyAsync(o.h.info, o.d.info, sizeof(OrderInfo), hipMemcpyDeviceToHost, o.tail));
    HIPCHK(c, hipMemcpyAsync(o.hostflag, c->d_hostflag.p, nr * sizeof(int32_t), hipMemcpyDeviceToHost, o.tail));
    HIPCHK(c, hipStreamSynchronize(o.tail));
    HIPCHK(c, hipGetLastError());
    if (o.h.info->index_err)   // (nothing of this call is kept)
        return fail(c, SW_ERANGE, "find_order: an event is seen by a single famous witness (IndexError at swirld.py:305)");
    if (o.k.host) std::fill(o.hostflag, o.hostflag + nr, 1);  // test hook: host sort
    for (int i = 0; i < nr; ++i) { o.any_host_sorted = o.any_host_sorted || o.hostflag[i]; c->ctr.order_rounds_host_sorted += o.hostflag[i] ? 1 : 0; }
    if (!o.any_host_sorted) return SW_OK;
    // rare: oversize round or a (ts, 8-byte key) tie: the host needs ts, the whitening keys and the signatures
    o.acc_ev.resize((size_t)o.n_acc);
    o.ts.resize((size_t)o.n_acc);
    o.white_h.resize((size_t)nr * 64);
    HIPCHK(c, hipMemcpyAsync(o.ts.data(), c->d_ts.p, o.n_acc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(o.acc_ev.data(), c->d_acc_ev.p, o.n_acc * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(o.white_h.data(), c->d_white.p, o.white_h.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    CHK(ensure_sig_h(c));
    return SW_OK;
}

// ---- phase: the final order inside each round the device left to the host: (consensus timestamp, whitened signature), swirld.py:306
void host_sort_rounds(const sw_ctx* c, OrderCall& o) {
    struct Item { double ts; uint64_t k8; int32_t ev; };
    const unsigned char* sig = c->sig_h.data();
    std::vector<Item> items;
    for (int i = 0; i < o.nr; ++i) {
        if (!o.n_acc || !o.hostflag[i]) {  // sorted on the device: already in `transactions`
            o.produced += o.h.acc_off[i + 1] - o.h.acc_off[i];
            continue;
        }
        const unsigned char* white = o.white_h.data() + (size_t)i * 64;  // swirld.py:285
        items.clear();
        for (int64_t a = o.h.acc_off[i]; a < o.h.acc_off[i + 1]; ++a) {
            Item it{o.ts[a], 0, o.acc_ev[a]};
            const unsigned char* sg = sig + (size_t)o.acc_ev[a] * 64;
            for (int b = 0; b < 8; ++b) it.k8 = (it.k8 << 8) | (unsigned char)(white[b] ^ sg[b]);
            items.push_back(it);
        }
        std::sort(items.begin(), items.end(), [sig, white](const Item& x, const Item& y) {
            if (x.ts != y.ts) return x.ts < y.ts;
            if (x.k8 != y.k8) return x.k8 < y.k8;
            const unsigned char* sx = sig + (size_t)x.ev * 64;
            const unsigned char* sy = sig + (size_t)y.ev * 64;
            for (int b = 8; b < 64; ++b) {
                const unsigned char kx = white[b] ^ sx[b], ky = white[b] ^ sy[b];
                if (kx != ky) return kx < ky;
            }
            return x.ev < y.ev;
        });
        for (const Item& it : items) o.sorted[o.produced++] = it.ev;   // swirld.py:307-309
    }
}

// ---- phase: the end of a call, which keeps its result from here on (SW_ERANGE for a short out_events included; a failure inside
// consensus_record poisons the context instead): the caller's copy in one piece, the device's copy of the order and its
// two values per event, the members' ordered prefixes, the window.  Who copies the order to the caller: join_and_copy_early, group
// by group, when the call has two slabs, no oversize round and neither SW_ORDER_HOST nor SW_ORDER_LATE_COPY; the copy here
// otherwise — and AGAIN after an early copy when the host re-sorted a round, which the early copy took as the device left it.
int finish_order(sw_ctx* c, OrderCall& o, int64_t* n_out) {
    if (o.out_events && o.n_acc && !(o.copied_early && !o.any_host_sorted)) memcpy(o.out_events, o.sorted, (size_t)std::min<int64_t>(o.n_acc, o.cap) * sizeof(int32_t));
    o.clk.lap(c, "sort");
    if (o.n_acc) CHK(consensus_record(c, o.n_acc, o.tx_at, o.nr, o.h.acc_off, o.hostflag, o.sorted));
    std::copy(o.h.ordnew, o.h.ordnew + c->n, c->ord_pos.begin());
    CHK(window_evict(c));
    if (n_out) *n_out = o.produced;
    if (o.produced > o.cap) return fail(c, SW_ERANGE, "find_order: out_events capacity %lld < %lld", (long long)o.cap, (long long)o.produced);
    return SW_OK;
}

template <int NW>
int do_find_order(sw_ctx* c, std::vector<int32_t> rounds, int32_t* out_events, int64_t cap, int64_t* n_out) {
    if (rounds.empty()) return SW_OK;
    if (c->payload_pending) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_payload, 0));  // timestamps / signatures of a bulk append
    CHK(order_rounds_arg(c, rounds));
    OrderCall o(c, std::move(rounds), out_events, cap);
    CHK(stage_order_call(c, o));
    CHK(order_tables<NW>(c, o));
    OrderRollback undo{c, o, true};
    CHK(order_reserve(c, o));
    if (o.n_acc) {
        plan_order_sorts(c, o);
        if (o.bulk) {
            CHK(plan_order_groups(c, o));
            o.clk.lap(c, "group");
            CHK(consumer_preamble(c, o, o.s1));
            o.clk.lap(c, "preamble", o.s1);
            CHK(enqueue_tchain(c, o));
            for (size_t gi = 0; gi < o.groups.size(); ++gi) CHK(enqueue_group<NW>(c, o, gi));
            CHK(join_and_copy_early(c, o));
            o.clk.lap(c, "walk+median");
        } else {
            CHK(order_small_call<NW>(c, o));
        }
        CHK(sort_big_rounds(c, o));
        o.clk.lap(c, "sort kernels");
        CHK(order_read_back(c, o));
    }
    o.clk.lap(c, "read-back");
    host_sort_rounds(c, o);
    undo.armed = false;
    return finish_order(c, o, n_out);
}


// the history of the exact path (sw_set_exact_history; exact_history.hip.h): what exact_* calls
static_assert(xh::QNAN_BITS == cns::QNAN_BITS, "one quiet NaN for 'not ordered'");
// SW_VOTE_STORE_INIT / SW_VOTE_STORE_MAX (measurement and test knobs), read at sw_create and again by sw_rewind / sw_reset,
// where the store is empty: its first capacity and its ceiling, in entries
void history_knobs(sw_ctx* c) {
    c->hist.cap0 = 4096;
    c->hist.ceiling = (int64_t)1 << 24;
    if (const char* e_ = getenv("SW_VOTE_STORE_INIT")) { const long long w = atoll(e_); if (w >= 1 && w <= ((long long)1 << 29)) c->hist.cap0 = w; }
    if (const char* e_ = getenv("SW_VOTE_STORE_MAX")) { const long long w = atoll(e_); if (w >= 1 && w <= ((long long)1 << 29)) c->hist.ceiling = w; }
}

xh::Store history_store(sw_ctx* c) {
    auto& h = c->hist;
    xh::Store s{};
    s.voter = h.d_voter.p; s.cand = h.d_cand.p; s.value = h.d_value.p; s.tab = h.d_tab.p;
    s.cap = h.cap; s.tmask = (unsigned)(h.slots - 1);
    return s;
}

void history_votes_lost(sw_ctx* c, const char* why) {
    c->hist.votes_ok = false;
    c->hist.why = why;
}

// Room for `need` entries in all — at most the ceiling: what does not fit makes the kernel set the overflow word.  The log
// keeps its entries (dgrow copies them), the index is emptied and rebuilt by k_votes_reindex, one thread per entry.
int history_store_reserve(sw_ctx* c, int64_t need) {
    auto& h = c->hist;
    need = std::min(need, h.ceiling);
    if (need <= h.cap && h.slots) return SW_OK;
    int64_t nc = std::max<int64_t>(h.cap0, 1);
    while (nc < need) nc *= 2;
    nc = std::min(std::max(nc, h.cap), h.ceiling);
    size_t slots = 2;
    while (slots < 2 * (size_t)nc) slots *= 2;
    const size_t keep = (size_t)h.count;
    CHK(dgrow(c, h.d_voter, (size_t)nc, keep));
    CHK(dgrow(c, h.d_cand, (size_t)nc, keep));
    CHK(dgrow(c, h.d_value, (size_t)nc, keep));
    CHK(dgrow(c, h.d_tab, slots, 0));
    h.cap = nc;
    h.slots = slots;
    HIPCHK(c, hipMemsetAsync(h.d_tab.p, 0xff, slots * sizeof(int32_t), c->stream));
    if (h.count) {
        hipLaunchKernelGGL(xh::k_votes_reindex, dim3((unsigned)((h.count + xh::THREADS - 1) / xh::THREADS)), dim3(xh::THREADS), 0, c->stream, history_store(c), (long long)h.count);
        c->ctr.kernel_launches++;
        HIPCHK(c, hipGetLastError());
    }
    h.grows++;
    return SW_OK;
}

int history_defaults(sw_ctx* c, int64_t first, int64_t K) {
    if (!K) return SW_OK;
    hipLaunchKernelGGL(xh::k_history_defaults, dim3((unsigned)((K + xh::THREADS - 1) / xh::THREADS)), dim3(xh::THREADS), 0, c->stream, (long long)first, (long long)K,
                       c->cons.d_rr.p, (xh::u64*)c->cons.d_cts.p);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    return SW_OK;
}

// Behind a successful exact_order: the two values of its `produced` items into the per-event tables, the items behind the
// device copy of the order.  (A call that failed returned before this and records nothing.)
int history_record(sw_ctx* c, int64_t produced) {
    if (!produced) return SW_OK;
    const size_t at = (size_t)c->cons.tx_len;
    CHK(consensus_reserve(c, at + (size_t)produced));
    hipLaunchKernelGGL(xh::k_history_record, dim3((unsigned)((produced + xh::THREADS - 1) / xh::THREADS)), dim3(xh::THREADS), 0, c->stream, (long long)produced,
                       (const int*)c->ex.items_ev.p, (const xh::u64*)c->ex.items_ts.p, (const int*)c->hist.d_items_rr.p, c->cons.d_rr.p, (xh::u64*)c->cons.d_cts.p);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->cons.d_tx.p + at, c->ex.items_ev.p, (size_t)produced * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (the next call may overwrite the items)
    c->cons.tx_len = (int64_t)at + produced;
    c->cons.record_calls++;
    c->cons.recorded += produced;
    return SW_OK;
}

// The one declaration ahead of its definition, for a true cycle: exact_enter ends in history_enter, and history_enter
// writes the exact path's header (exact_set_hdr) and expands the table of the votes export, both defined behind exact_*.
int history_enter(sw_ctx* c);

}  // namespace

// ====================================================================================
//                                     C-ABI
// ====================================================================================
extern "C" {

int sw_version(void) { return 7; }

const char* sw_last_error(const sw_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int sw_create(int n_members, const uint64_t* stake, int coin_period, int device, sw_ctx** out) {
    if (!out) return fail(nullptr, SW_EINVAL, "out is NULL");
    *out = nullptr;
    if (n_members < 1 || n_members > SW_MAX_MEMBERS) return fail(nullptr, SW_EINVAL, "n_members must be in [1, %d]", SW_MAX_MEMBERS);
    if (!stake) return fail(nullptr, SW_EINVAL, "stake is NULL");
    if (coin_period < 1) return fail(nullptr, SW_EINVAL, "coin_period must be >= 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, SW_ENODEV, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, SW_ENODEV, "device %d out of range (%d devices)", device, ndev);
    uint64_t tot = 0;
    bool unit = true;
    for (int i = 0; i < n_members; ++i) {
        if (stake[i] > (1ull << 30)) return fail(nullptr, SW_EOVERFLOW, "stake[%d] too large for the 32-bit tally", i);
        tot += stake[i];
        unit = unit && stake[i] == 1;
    }
    if (tot >= (1ull << 30)) return fail(nullptr, SW_EOVERFLOW, "total stake %llu >= 2^30", (unsigned long long)tot);
    sw_ctx* c = new sw_ctx();
    c->n = n_members;
    int nw = 1;
    while (nw * 64 < n_members) nw *= 2;
    c->nw = nw;
    c->npad = nw * 64;
    c->coin_period = coin_period;
    c->device = device;
    c->unit_stake = unit;
    c->tot = (uint32_t)tot;
    c->stake_h.assign(c->npad, 0);
    for (int i = 0; i < n_members; ++i) c->stake_h[i] = (uint32_t)stake[i];
    c->head.assign(n_members, -1);
    c->first_ev.assign(n_members, -1);
    c->front.assign(n_members, -1);
    c->front_dev.assign(c->npad, -1);
    c->divided_head.assign(c->npad, -1);
    c->ord_pos.assign(n_members, 0);
    c->lo0_h.assign(c->npad, SW_INF);
    c->NEARCAP = std::max(64 * c->npad, 4096);
    c->MCAP = std::max(1024 * c->npad, 65536);
    if (c->npad > 512) {
        // 1024 members: the tally runs at the L2 roofline (n^2 / 8 bytes of hop masks per evaluation), so fewer
        // evaluations per round pay: a round ends >= 10-11 chain positions behind its start there, a window of 12
        // slots from offset 10 finds it in 1.1 iterations per round at uniform gossip (41.3 -> 48.7 M ev/s at
        // 2 M events; coin-round stress +8 %, two cliques -5 %: profiles/r03y_*)
        c->K = 12;
        c->skip = 10;
    }
    // Tuning / diagnostic switches (environment, read here once per context).  None changes results; every one is
    // VALIDATED: a value that is not an integer inside the documented range fails sw_create with SW_EINVAL naming
    // the variable, instead of being silently clamped or read as 0.
    std::string knob_err;
    auto knob = [&](const char* name, long long lo, long long hi, auto* dst) {
        const char* s = getenv(name);
        if (!s || !*s) return;
        char* end = nullptr;
        const long long v = strtoll(s, &end, 10);
        if (*end != 0 || v < lo || v > hi) {
            if (knob_err.empty()) { char b[160]; snprintf(b, sizeof b, "%s=%s: an integer in [%lld, %lld]", name, s, lo, hi); knob_err = b; }
            return;
        }
        *dst = static_cast<std::remove_pointer_t<decltype(dst)>>(v);
    };
    int graph = c->use_graph ? 1 : 0;
    c->K_auto = !(getenv("SW_TALLY_K") && *getenv("SW_TALLY_K"));
    c->tally_auto = !(getenv("SW_TALLY_IMPL") && *getenv("SW_TALLY_IMPL"));
    knob("SW_TALLY_K", 1, 63, &c->K);             // (rounded to a multiple of 4 and capped at 60 below: a member's row of the candidate table has 64 columns)
    knob("SW_BAND", 64, 1 << 28, &c->NEARCAP);
    knob("SW_BAND_MAX", 64, 1 << 28, &c->MCAP);
    c->MCAP = std::max(c->MCAP, c->NEARCAP);
    knob("SW_BATCH", 1, 4096, &c->BATCH);
    knob("SW_GRAPH", 0, 1, &graph);
    knob("SW_GRAPH_BIG", 0, 512, &c->graph_big);
    c->graph_big &= ~1;
    c->use_graph = graph != 0;
    // 1024-thread workgroups (1024 members): one per CU is resident, 512 would run as two shifts (profiles/r04n_*: 41.4 -> 40.1 ms at 1024 x 2 M)
    if (c->npad >= 1024) c->band_blocks = 256;
    knob("SW_BAND_BLOCKS", 1, 4096, &c->band_blocks);
    knob("SW_TALLY_PF", 0, 1, &c->tally_pf);
    knob("SW_MID_PCT", 0, 99, &c->mid_pct);
    knob("SW_FIN_BAND", 0, 1, &c->fin_band);
    knob("SW_FIN_BLOCKS", 64, 8192, &c->fin_blocks);
    // beyond 512 members the sweep is the level-bucketed kernel (1024-thread workgroups, one per CU) and the loop kernels are
    // throughput-bound: side by side they cost each other more than the overlap hides (round 6, profiles/r06_pipe_1024.txt: 1024
    // members / 2 M events 32.55 -> 31.49 ms, 8 M events 125.4 -> 124.0, coin-round stress 44.5 -> 38.9; at 512 members the opposite,
    // 20.7 -> 26.3): every sweep of a call first, then ONE loop
    if (c->npad > 512) c->pipe = 1;
    knob("SW_PIPE", 1, SW_PROV_ROWS - 1, &c->pipe);   // (head + pipe sub-batches: every one of them has a row of chunk counters)
    if (c->npad > 256) c->cansee_impl = 3;  // wide member counts: the level-bucketed streaming kernel is faster than the dataflow sweep there
    knob("SW_CANSEE_IMPL", 2, 6, &c->cansee_impl);
    if (c->cansee_impl == 4 || c->cansee_impl == 5) knob_err = "SW_CANSEE_IMPL: 6 (dataflow sweep), 2 or 3 (level-bucketed sweep)";
    knob("SW_TALLY_IMPL", 0, 2, &c->tally_impl);   // 0 column-lane, 1 bit-sliced (one wave per slot), 2 bit-sliced two-level search (one workgroup per member)
    knob("SW_FLOW_CFG", 0, 3, &c->flow_cfg);
    knob("SW_CHUNKS", 1, SW_MAX_CHUNKS, &c->chunks);
    knob("SW_CHUNK_CFG", 0, 2, &c->chunk_cfg);
    knob("SW_BAND_FAST", 0, 1, &c->band_fast);
    if (c->npad > 256) c->tally_filter = 1;
    knob("SW_TALLY_FILTER", 0, 1, &c->tally_filter);
    knob("SW_SPLIT_EMULATE", 0, SW_MAX_PARTS, &c->split_emulate);   // (measurement: the parts of a split played by one context; pin SW_TALLY_IMPL=1 with it)
    knob("SW_SHOT_PCT", 10, 400, &c->shot_pct);
    knob("SW_GATED", 0, 1, &c->gated);
    knob("SW_GATE_LAG", 0, 256, &c->gate_lag);      // (test hooks, DESIGN.md §4: the gated loop's stage schedule fixed by the host)
    knob("SW_GATE_STEP", 1, SW_PROV_ROWS, &c->gate_step);
    if (c->gate_lag & 1) knob_err = "SW_GATE_LAG: an even number in [0, 256] (iteration parity)";
    knob("SW_SHOT_EXTRA", 0, 64, &c->shot_extra);
    knob("SW_CHUNK_MIN", 64, 1 << 30, &c->chunk_min);
    c->halo = 32 * (int64_t)c->npad;
    knob("SW_HALO", 0, 1 << 24, &c->halo);
    knob("SW_ELECT_IMPL", 0, 1, &c->elect_impl);
    knob("SW_ELECT_CG", 64, 256, &c->elect_cg);
    if (c->elect_cg != 64 && c->elect_cg != 128 && c->elect_cg != 256) knob_err = "SW_ELECT_CG: 64, 128 or 256";
    knob("SW_GALLOP", 0, 255, &c->gallop_after);
    knob("SW_SKIP", 0, 32, &c->skip);
    knob("SW_RING_H", 0, 64, &c->ring_H_req);      // ring depth of the level-bucketed sweep (0 = automatic)
    if (!knob_err.empty()) {
        delete c;
        return fail(nullptr, SW_EINVAL, "%s", knob_err.c_str());
    }
    // a zeroed buffer of 64-bit words for diagnostics: without it (no memory) the context works all the same
    auto debug_buf = [&](auto& b, size_t words) {
        if (dgrow(c, b, words, 0) == SW_OK) (void)hipMemset(b.p, 0, words * 8);
        else { (void)hipGetLastError(); c->err.clear(); }
    };
    c->debug_timing = getenv("SW_DEBUG_TIMING") != nullptr;
    if (c->debug_timing) {
        debug_buf(c->d_flow_dbg, 8);
    }
    if (const char* e_ = getenv("SW_EXPORT_LANES")) { const int g = atoi(e_); if (g == 4 || g == 8) c->xp.lanes = g; }
    if (const char* e_ = getenv("SW_WALK_THREADS")) { const int w = atoi(e_); if (w >= 64 && w <= wlk::MAX_THREADS && w % 64 == 0) c->walk.threads = w; }
    if (const char* e_ = getenv("SW_WIRE_BLOCKS")) { const int w = atoi(e_); if (w >= 1 && w <= 4096) c->wire.blocks = w; }
    history_knobs(c);
    if (getenv("SW_DEBUG_CLOCKS")) {  // diagnostics: phase stamps of the round-loop kernels
        c->dbg_minor = atoi(getenv("SW_DEBUG_CLOCKS")) >= 2 ? 0 : 1;
        if (atoi(getenv("SW_DEBUG_CLOCKS")) == 3) {
            debug_buf(c->d_dbg_blk, (size_t)SW_DBG_MAX_ITERS * 2 * 2048);
        }
        debug_buf(c->d_dbg, (size_t)SW_DBG_MAX_ITERS * 32);
    }
    c->nev.assign(n_members, 0);
    c->BATCH = (c->BATCH + 1) & ~1;  // even: the loop state is double-buffered by iteration parity
    // npad*K waves, 4 per workgroup (npad is a multiple of 64 anyway); a member's row of the candidate
    // table has 64 slots and slot 0 is the window header, so at most 60 candidates after rounding
    c->K = std::min((c->K + 3) & ~3, 60);
    c->K_flat = c->K;
    auto bail = [&](int rc) { g_create_error = c->err; sw_destroy(c); return rc; };
#define CCHK(expr) do { int rc_ = (expr); if (rc_ != SW_OK) return bail(rc_); } while (0)
#define CHIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { fail(c, SW_EIO, "%s: %s", #expr, hipGetErrorString(e_)); return bail(SW_EIO); } } while (0)
    CHIP(hipSetDevice(device));
    {
        // the round loop is the critical path: its stream gets the highest priority, the can_see
        // sweeps (which have slack when pipelined) the lowest
        int least = 0, greatest = 0;
        const char* pe = getenv("SW_PRIO");
        const bool use_prio = !pe || atoi(pe) != 0;
        const bool prio = use_prio && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest;
        if (!prio) (void)hipGetLastError();
        auto make_stream = [&](Stream& st, int priority) {
            hipStream_t made = nullptr;
            const hipError_t e_ = prio ? hipStreamCreateWithPriority(&made, hipStreamNonBlocking, priority) : hipStreamCreateWithFlags(&made, hipStreamNonBlocking);
            if (e_ == hipSuccess) st.reset(made);
            return e_;
        };
        CHIP(make_stream(c->stream, greatest));
        CHIP(make_stream(c->stream_cs, least));
        CHIP(make_stream(c->stream_aux, least));
        CHIP(make_stream(c->stream_io, least));
        // experiment (SW_CS_CUS=<count>): confine the can_see sweeps to the first <count> compute units of
        // the CU mask, so that the round loop's kernels find the others free of polling waves
        if (const char* e = getenv("SW_CS_CUS")) {
            const int cus = atoi(e);
            if (cus > 0 && cus < 256) {
                uint32_t mask[8] = {0};
                for (int i = 0; i < cus; ++i) mask[i >> 5] |= 1u << (i & 31);
                hipStream_t s2 = nullptr;
                if (hipExtStreamCreateWithCUMask(&s2, 8, mask) == hipSuccess) c->stream_cs.reset(s2);
                else (void)hipGetLastError();
            }
        }
        CCHK(ensure_event(c, c->ev_payload));
        CCHK(ensure_event(c, c->ev_small));
    }
    {
        static_assert(2 * sizeof(RState) + sizeof(int) <= SW_GATE_OFF && SW_GATE_OFF % 8 == 0 && SW_GATE_OFF + sizeof(LoopGate) <= 256, "readback block header");
        const size_t tree_off = 256 + (size_t)c->npad * sizeof(int32_t);
        const size_t prov_off = tree_off + (size_t)c->npad * sizeof(int32_t);
        c->rb_bytes = prov_off + (size_t)SW_PROV_ROWS * (SW_MAX_CHUNKS + 1) * sizeof(unsigned);
        CCHK(dgrow(c, c->d_rb, c->rb_bytes, 0));
        CHIP(hipMemset(c->d_rb.p, 0, c->rb_bytes));
        if (!c->h_rb_all.reserve(c->rb_bytes * SW_PROV_ROWS)) { fail(c, SW_ENOMEM, "hipHostMalloc for the read-back slots failed"); return bail(SW_ENOMEM); }
        c->h_rb = c->h_rb_all.p;
        c->rb_events.resize(SW_PROV_ROWS);
        for (Event& e1 : c->rb_events) CCHK(ensure_event(c, e1));
        c->d_state = reinterpret_cast<RState*>(c->d_rb.p);
        c->d_flow_err = reinterpret_cast<int*>(c->d_rb.p + 2 * sizeof(RState));
        c->d_front.p = reinterpret_cast<int32_t*>(c->d_rb.p + 256);
        c->d_treecnt = reinterpret_cast<int32_t*>(c->d_rb.p + tree_off);
        c->d_prov = reinterpret_cast<unsigned*>(c->d_rb.p + prov_off);
    }
    CCHK(dgrow(c, c->d_err, 1, 0));

    const int np = c->npad;
    CCHK(dgrow(c, c->d_stake, np, 0));
    CHIP(hipMemcpy(c->d_stake.p, c->stake_h.data(), np * sizeof(uint32_t), hipMemcpyHostToDevice));
    CCHK(dgrow(c, c->d_evalround, 2 * np, 0));
    CCHK(dgrow(c, c->d_evalpos, 2 * np, 0));
    CCHK(dgrow(c, c->d_lo_r, 2 * np, 0));
    CCHK(dgrow(c, c->d_cur, 2 * np, 0));
    CCHK(dgrow(c, c->d_unres, 2 * np, 0));
    CCHK(dgrow(c, c->d_lo_next, 2 * np, 0));
    CCHK(dgrow(c, c->d_pos_next, 2 * np, 0));
    CCHK(dgrow(c, c->d_found64, 2 * np, 0));
    CCHK(dgrow(c, c->d_farslot, 2 * np, 0));
    CCHK(dgrow(c, c->d_force, 2 * np, 0));
    CCHK(dgrow(c, c->d_cand, (size_t)2 * np * 64, 0));
    CCHK(dgrow(c, c->d_gallop, 2 * np, 0));
    CCHK(fill_i32(c, c->d_front.p, np, -1));
    c->divided_cnt.assign(np, 0);
    for (Event* e1 : {&c->ev_aux_done, &c->ev_cs_done, &c->ev_main_mark, &c->ev_loop_done}) CCHK(ensure_event(c, *e1));
    CCHK(dgrow(c, c->d_chain_len, 3 * np, 0));
    CCHK(dgrow(c, c->d_chain_start, np, 0));
    CCHK(dgrow(c, c->d_chain_cnt, np, 0));
    // band masks; row 0 stays all-zero (the bit-sliced tally points "not a hop" at it), the band
    // proper starts at row 1
    CCHK(dgrow(c, c->d_Mb, ((size_t)c->MCAP + 1) * c->nw, 0));
    CHIP(hipMemset(c->d_Mb.p, 0, (size_t)c->nw * sizeof(u64)));
    CCHK(dgrow(c, c->d_Pc, (size_t)c->MCAP + 1, 0));
    CHIP(hipMemset(c->d_Pc.p, 0, sizeof(int32_t)));
    CCHK(fill_i32(c, c->d_evalround.p, 2 * np, -1));
    CCHK(fill_i32(c, c->d_evalpos.p, 2 * np, 0));
    CCHK(fill_i32(c, c->d_lo_r.p, 2 * np, SW_INF));
    CCHK(fill_i32(c, c->d_cur.p, 2 * np, 0));
    CCHK(fill_i32(c, c->d_lo_next.p, 2 * np, SW_INF));
    CCHK(fill_i32(c, c->d_pos_next.p, 2 * np, 0));
    CHIP(hipMemsetAsync(c->d_found64.p, 0xff, 2 * np * sizeof(u64), c->stream));
    CHIP(hipMemsetAsync(c->d_unres.p, 0, 2 * np * sizeof(int32_t), c->stream));
    CCHK(ensure_rounds(c, 256));
    CHIP(hipStreamSynchronize(c->stream));
#undef CCHK
#undef CHIP
    *out = c;
    return SW_OK;
}

static void split_dissolve(SplitGroup* g) {
    if (!g) return;
    for (int q = 0; q < g->parts; ++q)
        if (g->ctx[q]) {
            sw_ctx* c = g->ctx[q];
            (void)hipStreamSynchronize(c->stream);
            if (c->split == g) { c->tally_impl = c->split_saved[0]; c->tally_auto = c->split_saved[1] != 0; c->K = c->split_saved[2]; c->K_auto = c->split_saved[3] != 0; }   // (what the link pinned)
            c->split = nullptr;
        }
    for (int w = 0; w < 2; ++w)
        for (int q = 0; q < SW_MAX_PARTS; ++q)
            for (auto e : g->ev[w][q]) if (e) (void)hipEventDestroy(e);
    delete g;
}

int sw_destroy(sw_ctx* c) {
    if (c && c->split) split_dissolve(c->split);
    if (!c) return SW_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    if (c->debug_timing && c->d_flow_dbg.p) {
        u64 d[8] = {0};
        (void)hipMemcpy(d, c->d_flow_dbg.p, sizeof d, hipMemcpyDeviceToHost);
        fprintf(stderr, "[sw] dataflow sweep, column 0: %llu events, %llu rows re-read from memory, %llu starved lane-trips, %llu wave-trips over %llu wave runs "
                "(%.1f trips per wave run), loader passes %llu (+%llu idle)\n", d[0], d[1], d[2], d[3], d[6], d[6] ? (double)d[3] / (double)d[6] : 0.0, d[4], d[5]);
    }
    if (c->debug_timing && c->stage_calls > 0) {
        const double k = 1.0 / (double)c->stage_calls;
        fprintf(stderr, "[sw] sw_divide_rounds host stages, us per call over %lld calls: sweeps enqueued %.1f, loop set-up %.1f, "
                "round loop %.1f, front rows %.1f, aux launches %.1f, final syncs %.1f\n", (long long)c->stage_calls,
                c->stage_us[0] * k, c->stage_us[1] * k, c->stage_us[2] * k, c->stage_us[3] * k, c->stage_us[4] * k, c->stage_us[5] * k);
    }
    if (c->vm.active) { vm_destroy(c); c->d_L.release(); }   // (d_L aliased the reservation)
    if (c->sign.d_keys.p) { (void)hipMemset(c->sign.d_keys.p, 0, c->sign.d_keys.cap); (void)hipDeviceSynchronize(); }   // the secrets do not outlive the context
    if (c->stream_io) (void)hipStreamSynchronize(c->stream_io);
    for (int g = 0; g < 4; ++g) {
        if (c->loop_exec[g]) (void)hipGraphExecDestroy(c->loop_exec[g]);
        if (c->loop_graph[g]) (void)hipGraphDestroy(c->loop_graph[g]);
    }
    // everything else is a member of an owning type (owned.h): ~sw_ctx gives it back — the device is idle and current
    delete c;
    return SW_OK;
}

int sw_reserve(sw_ctx* c, int64_t n_events) {
    if (!c || n_events < 0) return SW_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    return ensure_events(c, n_events);
}

int64_t sw_num_events(const sw_ctx* c) { return c ? c->N : 0; }

// Parallel copy of `bytes` bytes (bulk appends stage t / sig in pinned memory so that the upload
// can run behind the call; one thread cannot saturate the host memory system).
static void parallel_memcpy(void* dst, const void* src, size_t bytes) {
    unsigned hw = std::thread::hardware_concurrency();
    int nt = (int)std::min<size_t>(std::max(1u, std::min(hw / 2, 8u)), bytes / (4u << 20) + 1);
    if (nt <= 1) { memcpy(dst, src, bytes); return; }
    std::vector<std::thread> th;
    const size_t per = ((bytes / nt) + 63) & ~(size_t)63;
    for (int i = 0; i < nt; ++i) {
        const size_t a0 = std::min(bytes, per * i), a1 = std::min(bytes, per * (i + 1));
        if (a1 > a0) th.emplace_back([=] { memcpy((char*)dst + a0, (const char*)src + a0, a1 - a0); });
    }
    for (auto& t : th) t.join();
}

// ---- exact path for forked hashgraphs (exact.hip.h) ----------------------------------------------
// The context's own tables are the state (can_see table, round array, witness / fame / consensus
// tables); what the reference keeps beyond the fast path's per-slot view is added here: the dict order
// of every round's witnesses, fame per EVENT, tbd.  Every call is one launch of one wavefront.
swx::State exact_state(sw_ctx* c) {
    swx::State s{};
    s.n = c->n; s.npad = c->npad; s.coin_period = c->coin_period; s.tot = c->tot; s.stake = c->d_stake.p;
    s.cr = c->d_cr.p; s.sp = c->d_sp.p; s.op = c->d_op.p; s.ht = c->d_ht.p; s.t = c->d_t.p; s.sig = c->d_sig.p;
    s.round = c->d_round.p; s.L = c->d_L.p; s.tbd = c->ex.tbd.p; s.fam_ev = c->ex.fam_ev.p;
    s.Rcap = c->Rcap; s.wit = c->d_wit.p; s.worder = c->ex.worder.p; s.wcnt = c->ex.wcnt.p; s.cons = c->d_cons.p;
    s.fam_slot = c->d_fam.p; s.hdr = c->ex.hdr.p;
    return s;
}

// per-event and per-round buffers of the exact path follow the context's capacities
int exact_grow(sw_ctx* c) {
    const size_t np = c->npad;
    if (c->ex.cap < c->cap) {
        const size_t keep = (size_t)c->ex.cap, nc = (size_t)c->cap;
        CHK(dgrow(c, c->ex.fam_ev, nc, keep));
        CHK(dgrow(c, c->ex.tbd, nc, keep));
        CHK(dgrow(c, c->ex.queue, nc + 1, 0));
        CHK(dgrow(c, c->ex.visited, nc + 1, 0));
        CHK(dgrow(c, c->ex.items_ev, nc + 1, 0));
        CHK(dgrow(c, c->ex.items_ts, nc + 1, 0));
        HIPCHK(c, hipMemsetAsync(c->ex.fam_ev.p + keep, 0xff, nc - keep, c->stream));
        HIPCHK(c, hipMemsetAsync(c->ex.tbd.p + keep, 1, nc - keep, c->stream));
        HIPCHK(c, hipMemsetAsync(c->ex.visited.p, 0, c->ex.visited.cap, c->stream));  // all zero between calls
        c->ex.cap = c->cap;
    }
    if (c->hist.on) {   // (asked for on every call: the switch may have been set after a sw_reset that kept the buffers above)
        CHK(dgrow(c, c->hist.d_items_rr, (size_t)c->cap + 1, 0));
        CHK(consensus_reserve(c, (size_t)c->cons.tx_len));   // d_rr / d_cts follow the capacity; what was recorded stays
    }
    if (c->ex.Rcap < c->Rcap) {
        const size_t keep = (size_t)c->ex.Rcap, nc = (size_t)c->Rcap;
        CHK(dgrow(c, c->ex.worder, nc * np, keep * np));
        CHK(dgrow(c, c->ex.wcnt, nc, keep));
        CHK(dgrow(c, c->ex.done, nc, 0));
        CHK(dgrow(c, c->ex.newr, nc, 0));
        HIPCHK(c, hipMemsetAsync(c->ex.wcnt.p + keep, 0, (nc - keep) * sizeof(int32_t), c->stream));
        c->ex.Rcap = c->Rcap;
    }
    return SW_OK;
}

int exact_read_hdr(sw_ctx* c, long long* hdr) {
    HIPCHK(c, hipMemcpyAsync(hdr, c->ex.hdr.p, swx::H_WORDS * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

int exact_set_hdr(sw_ctx* c, int slot, long long v) {
    HIPCHK(c, hipMemcpyAsync(c->ex.hdr.p + slot, &v, sizeof v, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

// The first forked event arrives: hand the fast path's state over (nothing of it is recomputed).
int exact_enter(sw_ctx* c) {
    if (c->vm.active) return fail(c, SW_ENOTSUP, "a forked event in windowed mode: the exact path needs every can_see row");
    HIPCHK(c, hipDeviceSynchronize());
    c->payload_pending = false; c->small_pending = false;
    CHK(ensure_dag_h(c));  // host sp / op / height complete, heights on the device
    CHK(ensure_rounds(c, std::max(c->max_height + 3, c->R + 1)));
    const size_t np = c->npad;
    CHK(dgrow(c, c->ex.hdr, (size_t)swx::H_WORDS, 0));
    CHK(dgrow(c, c->ex.sm, np, 0)); CHK(dgrow(c, c->ex.fw, np, 0)); CHK(dgrow(c, c->ex.sflag, np, 0));
    CHK(dgrow(c, c->ex.times, np, 0)); CHK(dgrow(c, c->ex.tsort, np, 0)); CHK(dgrow(c, c->ex.white, 64, 0));
    CHK(exact_grow(c));
    long long hdr[swx::H_WORDS] = {0};
    hdr[swx::H_R] = c->R;
    HIPCHK(c, hipMemcpyAsync(c->ex.hdr.p, hdr, sizeof hdr, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->ex.wcnt.p, 0, (size_t)c->ex.Rcap * sizeof(int32_t), c->stream));
    c->ex.fc_base = c->fc_seen;
    const long long n_tx = (long long)c->transactions.size();
    if (n_tx) HIPCHK(c, hipMemcpyAsync(c->ex.items_ev.p, c->transactions.data(), (size_t)n_tx * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipLaunchKernelGGL(k_exact_import, dim3(1), dim3(64), 0, c->stream, exact_state(c), (long long)c->N, (const int*)c->ex.items_ev.p, n_tx);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->hist.on) CHK(history_enter(c));
    c->exact = true;
    return SW_OK;
}

// Node.add_event for a context on the exact path (swirld.py:114-120) + the structural half of
// is_valid_event (swirld.py:104-108: 0 or 2 parents, both known, self-parent by the creator,
// other-parent by another member).  Nothing is stored before the whole batch is accepted.
int append_exact(sw_ctx* c, int64_t K, const int32_t* creator, const int32_t* self_parent, const int32_t* other_parent,
                 const double* t, const uint8_t* sig64) {
    const int64_t N0 = c->N;
    const int n = c->n;
    for (int64_t i = 0; i < K; ++i) {
        const int64_t e = N0 + i;
        const int32_t m = creator[i], s = self_parent[i], o = other_parent[i];
        if (m < 0 || m >= n) return fail(c, SW_EINVAL, "event %lld: creator %d out of range", (long long)e, m);
        if ((s < 0) != (o < 0)) return fail(c, SW_EINVAL, "event %lld: must have 0 or 2 parents", (long long)e);
        if (s >= e || o >= e) return fail(c, SW_EINVAL, "event %lld: parent index not earlier (not a topological order)", (long long)e);
        if (s >= 0) {
            if ((s < N0 ? c->cr[s] : creator[s - N0]) != m) return fail(c, SW_EINVAL, "event %lld: self-parent is by another member", (long long)e);
            if ((o < N0 ? c->cr[o] : creator[o - N0]) == m) return fail(c, SW_EINVAL, "event %lld: other-parent is by the same member", (long long)e);
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->exact) CHK(exact_enter(c));
    CHK(ensure_events(c, N0 + K));
    CHK(exact_grow(c));
    std::vector<int32_t> hnew(K);
    int hmax = c->max_height;
    for (int64_t i = 0; i < K; ++i) {  // swirld.py:117-120
        const int32_t s = self_parent[i], o = other_parent[i];
        if (s < 0) { hnew[i] = 0; continue; }
        const int32_t hs = s < N0 ? c->ht[s] : hnew[s - N0], ho = o < N0 ? c->ht[o] : hnew[o - N0];
        hnew[i] = std::max(hs, ho) + 1;
        hmax = std::max(hmax, hnew[i]);
    }
    const size_t b4 = (size_t)K * sizeof(int32_t);
    HIPCHK(c, hipMemcpyAsync(c->d_cr.p + N0, creator, b4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_sp.p + N0, self_parent, b4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_op.p + N0, other_parent, b4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_ht.p + N0, hnew.data(), b4, hipMemcpyHostToDevice, c->stream));
    if (t) HIPCHK(c, hipMemcpyAsync(c->d_t.p + N0, t, (size_t)K * 8, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemsetAsync(c->d_t.p + N0, 0, (size_t)K * 8, c->stream));
    if (sig64) HIPCHK(c, hipMemcpyAsync(c->d_sig.p + (size_t)N0 * 64, sig64, (size_t)K * 64, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemsetAsync(c->d_sig.p + (size_t)N0 * 64, 0, (size_t)K * 64, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_round.p + N0, 0xff, b4, c->stream));
    HIPCHK(c, hipMemsetAsync(c->ex.fam_ev.p + N0, 0xff, (size_t)K, c->stream));
    HIPCHK(c, hipMemsetAsync(c->ex.tbd.p + N0, 1, (size_t)K, c->stream));
    if (c->hist.on) CHK(history_defaults(c, N0, K));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->cr.insert(c->cr.end(), creator, creator + K);
    c->sp.insert(c->sp.end(), self_parent, self_parent + K);
    c->op.insert(c->op.end(), other_parent, other_parent + K);
    c->ht.insert(c->ht.end(), hnew.begin(), hnew.end());
    c->max_height = hmax;
    c->N = N0 + K;
    return SW_OK;
}

int exact_divide(sw_ctx* c, int64_t first, int64_t K) {
    CHK(ensure_rounds(c, c->max_height + 3));  // round <= height: every row a witness can land in exists
    CHK(exact_grow(c));
    CHK(exact_set_hdr(c, swx::H_RC, 0));
    for (int64_t a = first; a < first + K; a += 8192) {  // (bounded launches: one wavefront walks the events in order)
        const int64_t k = std::min<int64_t>(8192, first + K - a);
        hipLaunchKernelGGL(k_exact_divide, dim3(1), dim3(64), 0, c->stream, exact_state(c), (long long)a, (long long)k);
        c->ctr.kernel_launches++;
    }
    HIPCHK(c, hipGetLastError());
    long long hdr[swx::H_WORDS];
    CHK(exact_read_hdr(c, hdr));
    if (hdr[swx::H_RC] != swx::X_OK) { c->poisoned = true; return fail(c, SW_EIO, "exact divide_rounds: a parent of event %lld has no round", hdr[swx::H_ERR_AT]); }
    c->R = (int)hdr[swx::H_R];
    c->divided = first + K;
    c->ctr.events_divided += K;
    c->ctr.rounds = c->R;
    return SW_OK;
}

int exact_fame(sw_ctx* c, int32_t* new_rounds, int cap, int* n_new) {
    const int R = c->R;
    const int max_c = first_undecided_round(c);
    swx::FameScratch x{};
    x.win = std::max(1, R - max_c);
    x.layer = (size_t)c->n * x.win * c->n;
    if (x.layer > ((size_t)4 << 30)) return fail(c, SW_ENOMEM, "exact decide_fame: %d undecided rounds x %d members need %zu GB of vote storage", x.win, c->n, (2 * x.layer) >> 30);
    CHK(exact_grow(c));
    CHK(dgrow(c, c->ex.votes, 2 * x.layer, 0));
    x.votes = c->ex.votes.p; x.s_m = c->ex.sm.p; x.done = c->ex.done.p; x.new_rounds = c->ex.newr.p;
    if (c->hist.on && c->hist.votes_ok) {
        // every voter round r_ stores at most n voters x (r_ - max_c) candidate rounds x n candidates
        const int64_t w = R - max_c;
        CHK(history_store_reserve(c, c->hist.count + (int64_t)c->n * c->n * (w * (w - 1) / 2)));
        x.hist = history_store(c);
    }
    CHK(exact_set_hdr(c, swx::H_RC, 0));
    CHK(exact_set_hdr(c, swx::H_NNEW, 0));
    hipLaunchKernelGGL(k_exact_fame, dim3(1), dim3(64), 0, c->stream, exact_state(c), x);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    long long hdr[swx::H_WORDS];
    CHK(exact_read_hdr(c, hdr));
    if (x.hist.voter) {
        c->hist.count = hdr[swx::H_VCNT];
        if (hdr[swx::H_VOVF] == 1) history_votes_lost(c, "the vote store reached its ceiling (SW_VOTE_STORE_MAX)");
        else if (hdr[swx::H_VOVF]) history_votes_lost(c, "a decide_fame call ended in the reference's KeyError");
    }
    if (hdr[swx::H_RC] != swx::X_OK)
        return fail(c, SW_EINVAL, "exact decide_fame: a voter strongly sees a member without a witness in the previous round, or a vote is missing (KeyError in the reference, swirld.py:253 / 260)");
    const int cnt = (int)hdr[swx::H_NNEW];
    std::vector<int32_t> nr(std::max(cnt, 1));
    if (cnt) {
        HIPCHK(c, hipMemcpyAsync(nr.data(), c->ex.newr.p, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    for (int i = 0; i < cnt; ++i) {
        c->cons_h[nr[i]] = 1;
        if (i < cap && new_rounds) new_rounds[i] = nr[i];
    }
    if (n_new) *n_new = cnt;
    FameCounters fc{};
    fc.voter_evals = (u64)hdr[swx::H_VOTER_EVALS] + c->ex.fc_base.voter_evals;
    fc.majority_evals = (u64)hdr[swx::H_MAJ_EVALS] + c->ex.fc_base.majority_evals;
    fc.coin_votes = (u64)hdr[swx::H_COIN_VOTES] + c->ex.fc_base.coin_votes;
    fc.coin_flips = (u64)hdr[swx::H_COIN_FLIPS] + c->ex.fc_base.coin_flips;
    fame_counters(c, fc);
    if (cnt > cap) return fail(c, SW_ERANGE, "new_rounds capacity %d < %d", cap, cnt);
    return SW_OK;
}

int exact_order(sw_ctx* c, std::vector<int32_t> rounds, int32_t* out_events, int64_t cap, int64_t* n_out) {
    CHK(order_rounds_arg(c, rounds));
    const int nr = (int)rounds.size();
    if (nr == 0) return SW_OK;
    CHK(exact_grow(c));
    CHK(dgrow(c, c->ex.rounds, nr, 0));
    HIPCHK(c, hipMemcpyAsync(c->ex.rounds.p, rounds.data(), (size_t)nr * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    CHK(exact_set_hdr(c, swx::H_RC, 0));
    CHK(exact_set_hdr(c, swx::H_NOUT, 0));
    swx::OrderScratch x{};
    x.queue = c->ex.queue.p; x.visited = c->ex.visited.p; x.fw = c->ex.fw.p; x.sflag = c->ex.sflag.p; x.times = c->ex.times.p;
    x.tsort = c->ex.tsort.p; x.white = c->ex.white.p; x.items_ev = c->ex.items_ev.p; x.items_ts = c->ex.items_ts.p;
    if (c->hist.on) x.items_rr = c->hist.d_items_rr.p;
    hipLaunchKernelGGL(k_exact_order, dim3(1), dim3(64), 0, c->stream, exact_state(c), x, (const int*)c->ex.rounds.p, nr);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    long long hdr[swx::H_WORDS];
    CHK(exact_read_hdr(c, hdr));
    if (hdr[swx::H_RC] == swx::X_EINDEX)
        return fail(c, SW_ERANGE, "find_order: an event is seen by a single famous witness (IndexError at swirld.py:305)");
    if (hdr[swx::H_RC] != swx::X_OK)
        return fail(c, SW_EINVAL, "find_order: a round has an undecided witness (KeyError on self.famous[w], swirld.py:284)");
    const int64_t produced = hdr[swx::H_NOUT];
    const size_t at = c->transactions.size();
    if (!c->transactions.resize(at + (size_t)produced)) return fail(c, SW_ENOMEM, "pinned host memory for the ordered events");
    if (produced) {
        HIPCHK(c, hipMemcpyAsync(c->transactions.data() + at, c->ex.items_ev.p, (size_t)produced * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (c->hist.on) CHK(history_record(c, produced));
    if (n_out) *n_out = produced;
    if (produced > cap) return fail(c, SW_ERANGE, "find_order: out_events capacity %lld < %lld", (long long)cap, (long long)produced);
    if (out_events) memcpy(out_events, c->transactions.data() + at, (size_t)produced * sizeof(int32_t));
    return SW_OK;
}

// state of the exact path back to "nothing divided" (sw_rewind; the events and their forks stay)
int exact_rewind(sw_ctx* c) {
    if (c->N) {
        HIPCHK(c, hipMemsetAsync(c->ex.fam_ev.p, 0xff, (size_t)c->N, c->stream));
        HIPCHK(c, hipMemsetAsync(c->ex.tbd.p, 1, (size_t)c->N, c->stream));
    }
    if (c->ex.Rcap) HIPCHK(c, hipMemsetAsync(c->ex.wcnt.p, 0, (size_t)c->ex.Rcap * sizeof(int32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->ex.hdr.p, 0, swx::H_WORDS * sizeof(long long), c->stream));
    if (c->hist.on) {   // nothing is ordered, no vote has been cast: the store is empty and complete again
        if (c->N) CHK(history_defaults(c, 0, c->N));
        if (c->hist.slots) HIPCHK(c, hipMemsetAsync(c->hist.d_tab.p, 0xff, c->hist.slots * sizeof(int32_t), c->stream));
        c->hist.count = 0;
        c->hist.votes_ok = true;
        c->hist.why = "";
        history_knobs(c);
        if (c->hist.cap > c->hist.ceiling) c->hist.cap = c->hist.ceiling;   // (the buffers stay; the kernel stops at `cap`)
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ex.fc_base = c->fc_seen;
    return SW_OK;
}

// A Node's gossip step appends a handful of events: one packed record per event in pinned memory,
// ONE host-to-device copy, ONE kernel (k_ingest_small), no host synchronisation.  The batch has been
// validated; the per-member tables of the caller (head_t, nev_t, first_t) are committed here.
static int append_small(sw_ctx* c, int64_t K, const int32_t* creator, const int32_t* self_parent, const int32_t* other_parent,
                        const double* t, const uint8_t* sig64, const std::vector<int32_t>& seq, std::vector<int32_t>& head_t,
                        std::vector<int32_t>& nev_t, std::vector<int32_t>& first_t) {
    const int64_t N0 = c->N;
    const int n = c->n, np = c->npad;
    CHK(ensure_dag_h(c));  // parents' heights (complete already unless a bulk append came before)
    if ((size_t)K > c->h_small.cap) {
        if (c->small_pending) { HIPCHK(c, hipEventSynchronize(c->ev_small)); c->small_pending = false; }
        if (!c->h_small.reserve(std::max<size_t>(256, (size_t)K * 2))) return fail(c, SW_ENOMEM, "hipHostMalloc for the small-append staging buffer failed");
    }
    // ---- segments that overflow move to the end of the pool, doubled (device-to-device)
    bool moved = false;
    for (int m = 0; m < n; ++m) {
        if (nev_t[m] <= c->chain_cap[m]) continue;
        int32_t ncap = std::max(16, 2 * c->chain_cap[m]);
        while (ncap < nev_t[m]) ncap *= 2;
        if (c->pool_used + ncap > 0x7fffffff) return fail(c, SW_ERANGE, "chain pool exceeds 2^31 entries");
        const int64_t noff = c->pool_used;
        const int32_t before = c->nev[m];
        CHK(dgrow(c, c->d_chain_ev, (size_t)(noff + ncap) * 2, (size_t)c->pool_used));
        CHK(dgrow(c, c->d_cdesc, c->d_chain_ev.cap, (size_t)c->pool_used));
        if (before) {
            HIPCHK(c, hipMemcpyAsync(c->d_chain_ev.p + noff, c->d_chain_ev.p + c->chain_start_h[m], (size_t)before * sizeof(int32_t),
                                     hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->d_cdesc.p + noff, c->d_cdesc.p + c->chain_start_h[m], (size_t)before * sizeof(int4),
                                     hipMemcpyDeviceToDevice, c->stream));
        }
        if (c->pool_h_valid) {
            c->chain_ev_h.resize((size_t)(noff + ncap), -1);
            std::copy(c->chain_ev_h.begin() + c->chain_start_h[m], c->chain_ev_h.begin() + c->chain_start_h[m] + before, c->chain_ev_h.begin() + noff);
        }
        c->chain_start_h[m] = (int32_t)noff;
        c->chain_cap[m] = ncap;
        c->pool_used = noff + ncap;
        moved = true;
    }
    if (moved) {
        HIPCHK(c, hipMemcpyAsync(c->d_chain_start.p, c->chain_start_h.data(), np * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (rare; keeps the host table free to change)
    }
    // ---- packed records
    if (c->small_pending) { HIPCHK(c, hipEventSynchronize(c->ev_small)); c->small_pending = false; }
    const bool dag_complete = (int64_t)c->sp.size() == N0;  // always, after ensure_dag_h
    if (!dag_complete) return fail(c, SW_EIO, "host mirror of the hashgraph is incomplete (internal)");
    c->cr.reserve(N0 + K); c->sp.reserve(N0 + K); c->op.reserve(N0 + K); c->ht.reserve(N0 + K); c->seq_h.reserve(N0 + K);
    c->blk_hmin.resize((size_t)((N0 + K + 4095) >> 12), 0x7fffffff);
    c->blk_hmax.resize((size_t)((N0 + K + 4095) >> 12), -1);
    const bool sig_complete = (int64_t)(c->sig_h.size() / 64) == N0;
    if (sig_complete) c->sig_h.resize((size_t)(N0 + K) * 64);
    if (c->pool_h_valid && c->chain_ev_h.size() < (size_t)c->pool_used) c->chain_ev_h.resize((size_t)c->pool_used, -1);
    for (int64_t i = 0; i < K; ++i) {
        const int64_t e = N0 + i;
        SmallRec& r = c->h_small.p[i];
        const int32_t m = creator[i], s_ = self_parent[i], o_ = other_parent[i];
        r.cr = m; r.sp = s_; r.op = o_; r.seq = seq[i];
        const int32_t h = s_ < 0 ? 0 : std::max(c->ht[s_], c->ht[o_]) + 1;  // swirld.py:117-120 (parents are earlier: already mirrored)
        r.ht = h;
        r.at = c->chain_start_h[m] + seq[i];
        r.w = o_ < 0 ? 0 : (c->cr[o_] | ((c->seq_h[o_] & 63) << 10));
        r.pad = 0;
        r.t = t ? t[i] : 0.0;
        if (sig64) memcpy(r.sig, sig64 + 64 * i, 64); else memset(r.sig, 0, 64);
        // host mirrors (a later event of this batch may have this one as a parent)
        c->cr.push_back(m); c->sp.push_back(s_); c->op.push_back(o_); c->ht.push_back(h); c->seq_h.push_back(seq[i]);
        c->max_height = std::max(c->max_height, h);
        c->blk_hmin[e >> 12] = std::min(c->blk_hmin[e >> 12], h);
        c->blk_hmax[e >> 12] = std::max(c->blk_hmax[e >> 12], h);
        if (sig_complete) memcpy(c->sig_h.data() + (size_t)e * 64, r.sig, 64);
        if (c->pool_h_valid) c->chain_ev_h[(size_t)r.at] = (int32_t)e;
    }
    // (from here on the host tables are committed; a device failure poisons the context)
    c->head.swap(head_t);
    c->first_ev.swap(first_t);
    c->nev.swap(nev_t);
    c->N = N0 + K;
    CHK(dgrow(c, c->d_small, c->h_small.cap * sizeof(SmallRec), 0));
    hipError_t e1 = hipMemcpyAsync(c->d_small.p, c->h_small.p, (size_t)K * sizeof(SmallRec), hipMemcpyHostToDevice, c->stream);
    if (e1 == hipSuccess) {
        hipLaunchKernelGGL(k_ingest_small, dim3((unsigned)((K + 127) / 128)), dim3(128), 0, c->stream, (const SmallRec*)c->d_small.p, (int)N0, (int)K,
                           c->d_cr.p, c->d_sp.p, c->d_op.p, c->d_seq.p, c->d_ht.p, c->d_t.p, c->d_sig.p, c->d_coin.p, c->d_round.p,
                           c->d_chain_ev.p, c->d_cdesc.p, c->d_chain_cnt.p);
        c->ctr.kernel_launches++;
        e1 = hipGetLastError();
    }
    if (e1 == hipSuccess) e1 = hipEventRecord(c->ev_small, c->stream);
    if (e1 != hipSuccess) { c->poisoned = true; return fail(c, SW_EIO, "small append: %s", hipGetErrorString(e1)); }
    c->small_pending = true;
    return SW_OK;
}

int sw_append_events(sw_ctx* c, int64_t K, const int32_t* creator, const int32_t* self_parent,
                     const int32_t* other_parent, const double* t, const uint8_t* sig64) {
    if (!c) return SW_EINVAL;
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (K < 0 || (K > 0 && (!creator || !self_parent || !other_parent))) return fail(c, SW_EINVAL, "NULL event arrays");
    if (K == 0) return SW_OK;
    if (c->N + K > 0x7ffffff0ll) return fail(c, SW_ERANGE, "more than 2^31 events");
    CHK(heights_ready(c));   // (a device append's heights kernel may still run: the event arrays may move below)
    if (c->exact) return append_exact(c, K, creator, self_parent, other_parent, t, sig64);
    const int64_t N0 = c->N;
    const int n = c->n;
    const bool bulk = K >= 8192 || c->chain_cap.empty() || K * 8 >= N0;
    // ---- 1. host pass: everything of is_valid_event's structural half (swirld.py:104-108) that needs
    // only per-member tables, on COPIES of them — nothing is stored before the whole batch is accepted.
    // Arity; topological order; self-parent = the creator's latest event (which makes it an event
    // of the same creator and refuses forks: the round-synchronous path needs one self-parent chain
    // per member, and a stored fork would make every later sw_divide_rounds fail); chain positions.
    std::vector<int32_t> head_t(c->head), nev_t(c->nev), first_t(c->first_ev), seq(K);
    for (int64_t i = 0; i < K; ++i) {
        const int64_t e = N0 + i;
        const int32_t m = creator[i], s = self_parent[i], o = other_parent[i];
        if (m < 0 || m >= n) return fail(c, SW_EINVAL, "event %lld: creator %d out of range", (long long)e, m);
        if ((s < 0) != (o < 0)) return fail(c, SW_EINVAL, "event %lld: must have 0 or 2 parents", (long long)e);
        if (s >= e || o >= e) return fail(c, SW_EINVAL, "event %lld: parent index not earlier (not a topological order)", (long long)e);
        if (!c->lapsed.empty() && c->lapsed[m])
            return fail(c, SW_ERANGE, "event %lld: member %d was silent for more than %lld events and has lapsed out of the windowed table (sw_set_window_lapse)",
                        (long long)e, m, (long long)c->window_lapse);
        if (s >= 0 && (s < c->first_resident || o < c->first_resident))
            return fail(c, SW_ERANGE, "event %lld: the can_see row of a parent was evicted (windowed mode keeps rows from event %lld on)", (long long)e, (long long)c->first_resident);
        if (head_t[m] != s) {
            if (s >= 0 && (s < N0 ? c->cr[s] : creator[s - N0]) != m)
                return fail(c, SW_EINVAL, "event %lld: self-parent is by another member", (long long)e);
            // a fork (the reference stores it, README.md:84): the context moves to the exact path, which
            // validates the batch again on its own terms
            if (c->forks_mode == 1 && !c->vm.active) return append_exact(c, K, creator, self_parent, other_parent, t, sig64);
            return fail(c, SW_ENOTSUP, "event %lld is a fork (member %d already has %s): forked hashgraphs are outside the "
                        "supported domain; nothing was stored", (long long)e, m, s < 0 ? "a root" : "a later event on that self-parent");
        }
        head_t[m] = (int32_t)e;
        if (first_t[m] < 0) first_t[m] = (int32_t)e;
        seq[i] = nev_t[m]++;
    }
    if (!bulk) {  // small append: the other-parent's creator from the host mirror
        for (int64_t i = 0; i < K; ++i) {
            const int32_t o = other_parent[i];
            if (o >= 0 && (o < N0 ? c->cr[o] : creator[o - N0]) == creator[i])
                return fail(c, SW_EINVAL, "event %lld: other-parent is by the same member", (long long)(N0 + i));
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    // ---- 2. allocations (still nothing committed)
    CHK(ensure_events(c, N0 + K));
    if (c->vm.active) CHK(vm_ensure(c, (size_t)(N0 + K) * c->npad * sizeof(int32_t)));
    if (!bulk) return append_small(c, K, creator, self_parent, other_parent, t, sig64, seq, head_t, nev_t, first_t);
    const size_t b4 = (size_t)K * sizeof(int32_t);
    const bool stage = bulk && (t || sig64) && (size_t)K * 72 <= ((size_t)1 << 30);  // (beyond 1 GiB of payload: plain copies)
    if (stage) {
        const size_t need = (size_t)K * 72;
        if (c->payload_pending) { HIPCHK(c, hipEventSynchronize(c->ev_payload)); c->payload_pending = false; }
        if (!c->h_pin.reserve(need)) return fail(c, SW_ENOMEM, "hipHostMalloc(%zu bytes) for the ingest staging buffer failed", need);
    }
    // ---- 3. parent arrays to the (uncommitted) tail of the device arrays; bulk: device half of the validation
    HIPCHK(c, hipMemcpyAsync(c->d_cr.p + N0, creator, b4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_sp.p + N0, self_parent, b4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_op.p + N0, other_parent, b4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_seq.p + N0, seq.data(), b4, hipMemcpyHostToDevice, c->stream));
    if (bulk) {
        int verdict = 0x7fffffff;
        HIPCHK(c, hipMemcpyAsync(c->d_err.p, &verdict, sizeof verdict, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_validate_other_parent, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream,
                           (const int*)c->d_cr.p, (const int*)c->d_op.p, (int)N0, (int)K, c->d_err.p);
        c->ctr.kernel_launches++;
        HIPCHK(c, hipMemcpyAsync(&verdict, c->d_err.p, sizeof verdict, hipMemcpyDeviceToHost, c->stream));
        // the payload is staged while the device validates
        if (stage) {
            if (t) parallel_memcpy(c->h_pin.p, t, (size_t)K * 8);
            if (sig64) parallel_memcpy(c->h_pin.p + (size_t)K * 8, sig64, (size_t)K * 64);
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (verdict != 0x7fffffff)
            return fail(c, SW_EINVAL, "event %d: other-parent is by the same member", verdict);
    }
    // ---- 4. commit.  From here on a device failure leaves the context inconsistent: it is poisoned.
    c->cr.insert(c->cr.end(), creator, creator + K);
    c->seq_h.insert(c->seq_h.end(), seq.begin(), seq.end());
    // the lazily fetched mirrors stay complete when they were complete (a Node appends a few events per
    // call); after a bulk append they are refilled from the device on demand
    if (!bulk && (int64_t)c->sp.size() == N0) {
        c->sp.insert(c->sp.end(), self_parent, self_parent + K);
        c->op.insert(c->op.end(), other_parent, other_parent + K);
        c->ht.resize(N0 + K);
        c->blk_hmin.resize((size_t)((N0 + K + 4095) >> 12), 0x7fffffff);
        c->blk_hmax.resize((size_t)((N0 + K + 4095) >> 12), -1);
        for (int64_t e = N0; e < N0 + K; ++e) {
            const int32_t s_ = c->sp[e], o_ = c->op[e];
            const int32_t h = s_ < 0 ? 0 : std::max(c->ht[s_], c->ht[o_]) + 1;  // swirld.py:117-120
            c->ht[e] = h;
            c->max_height = std::max(c->max_height, h);
            c->blk_hmin[e >> 12] = std::min(c->blk_hmin[e >> 12], h);
            c->blk_hmax[e >> 12] = std::max(c->blk_hmax[e >> 12], h);
        }
        PHIP(hipMemcpyAsync(c->d_ht.p + N0, c->ht.data() + N0, b4, hipMemcpyHostToDevice, c->stream));
    }
    if (!bulk && (int64_t)(c->sig_h.size() / 64) == N0) {
        c->sig_h.resize((size_t)(N0 + K) * 64);
        if (sig64) memcpy(c->sig_h.data() + (size_t)N0 * 64, sig64, (size_t)K * 64);
        else memset(c->sig_h.data() + (size_t)N0 * 64, 0, (size_t)K * 64);
    }
    c->head.swap(head_t);
    c->first_ev.swap(first_t);
    c->N = N0 + K;
    // payload: timestamps, signatures, coin bits (swirld.py:272) — needed by decide_fame's coin rounds
    // and by find_order only, so a bulk append uploads them behind the call on their own stream
    hipStream_t ps = stage ? c->stream_io : c->stream;
    if (stage) {
        if (t) PHIP(hipMemcpyAsync(c->d_t.p + N0, c->h_pin.p, (size_t)K * 8, hipMemcpyHostToDevice, ps));
        if (sig64) PHIP(hipMemcpyAsync(c->d_sig.p + (size_t)N0 * 64, c->h_pin.p + (size_t)K * 8, (size_t)K * 64, hipMemcpyHostToDevice, ps));
    } else {
        if (t) PHIP(hipMemcpyAsync(c->d_t.p + N0, t, (size_t)K * 8, hipMemcpyHostToDevice, ps));
        if (sig64) PHIP(hipMemcpyAsync(c->d_sig.p + (size_t)N0 * 64, sig64, (size_t)K * 64, hipMemcpyHostToDevice, ps));
    }
    if (!t) PHIP(hipMemsetAsync(c->d_t.p + N0, 0, (size_t)K * 8, ps));
    if (!sig64) PHIP(hipMemsetAsync(c->d_sig.p + (size_t)N0 * 64, 0, (size_t)K * 64, ps));
    hipLaunchKernelGGL(k_coin_bits, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, ps, (const unsigned char*)c->d_sig.p, (int)N0, (int)K, c->d_coin.p);
    c->ctr.kernel_launches++;
    if (stage) { PHIP(hipEventRecord(c->ev_payload, ps)); c->payload_pending = true; }
    PHIP(hipMemsetAsync(c->d_round.p + N0, 0xff, b4, c->stream));
    // per-member chain pool + chain descriptors: part of the ingest-time layout of the hashgraph store
    PCHK(rebuild_chains(c, nev_t, c->N));
    c->nev.swap(nev_t);
    PHIP(hipStreamSynchronize(c->stream));  // caller buffers may be released on return (bulk payload: staged copy)
    return SW_OK;
}

// ---- sw_append_events_device: the same K events from device memory ------------------------------------------------
namespace {

// Everything outside the bulk fork-free fast path: the batch goes to the host and through sw_append_events.
int ingest_fallback(sw_ctx* c, int64_t K, const int32_t* d_creator, const int32_t* d_self_parent, const int32_t* d_other_parent,
                    const double* d_t, const uint8_t* d_sig64, hipStream_t us) {
    c->ing.fallback++;
    std::vector<int32_t> cr((size_t)K), sp((size_t)K), op((size_t)K);
    std::vector<double> t(d_t ? (size_t)K : 0);
    std::vector<uint8_t> sig(d_sig64 ? (size_t)K * 64 : 0);
    const size_t b4 = (size_t)K * sizeof(int32_t);
    HIPCHK(c, hipMemcpyAsync(cr.data(), d_creator, b4, hipMemcpyDeviceToHost, us));
    HIPCHK(c, hipMemcpyAsync(sp.data(), d_self_parent, b4, hipMemcpyDeviceToHost, us));
    HIPCHK(c, hipMemcpyAsync(op.data(), d_other_parent, b4, hipMemcpyDeviceToHost, us));
    if (d_t) HIPCHK(c, hipMemcpyAsync(t.data(), d_t, (size_t)K * 8, hipMemcpyDeviceToHost, us));
    if (d_sig64) HIPCHK(c, hipMemcpyAsync(sig.data(), d_sig64, (size_t)K * 64, hipMemcpyDeviceToHost, us));
    HIPCHK(c, hipStreamSynchronize(us));
    return sw_append_events(c, K, cr.data(), sp.data(), op.data(), d_t ? t.data() : nullptr, d_sig64 ? sig.data() : nullptr);
}

}  // namespace

// The call itself, behind the argument checks: K > 0 events in memory of the context's device, produced on `us`.
// (Also the last step of sw_ingest_payload[_device], with `us` the context's own stream.)
static int append_device_body(sw_ctx* c, int64_t K, const int32_t* d_creator, const int32_t* d_self_parent, const int32_t* d_other_parent,
                              const double* d_t, const uint8_t* d_sig64, hipStream_t us) {
    const size_t b4 = (size_t)K * sizeof(int32_t);
    const int64_t N0 = c->N;
    const int n = c->n, np = c->npad;
    const bool bulk = K >= 8192 || c->chain_cap.empty() || K * 8 >= N0;   // (sw_append_events' predicate)
    if (c->exact || c->vm.active || !bulk || np > ing::MAX_KEYS)
        return ingest_fallback(c, K, d_creator, d_self_parent, d_other_parent, d_t, d_sig64, us);
    // heights of the events so far must be on the device (a bulk HOST append leaves them to ensure_dag_h)
    CHK(heights_ready(c));
    if ((int64_t)c->sp.size() < N0 && c->ing.ht_dev_upto < N0) CHK(ensure_dag_h(c));
    // ---- allocations (nothing committed)
    CHK(ensure_events(c, N0 + K));
    const int tiles = (int)((K + ing::TILE - 1) / ing::TILE);
    const int64_t blk0 = N0 >> 12, nblk = ((N0 + K - 1) >> 12) - blk0 + 1;
    CHK(dgrow(c, c->ing.d_tab, (size_t)4 + 3 * np, 0));
    CHK(dgrow(c, c->ing.d_hist, (size_t)tiles * np, 0));
    CHK(dgrow(c, c->ing.d_ht_stat, (size_t)(2 + 2 * nblk), 0));
    // (the pinned staging buffer may still feed the payload upload of an earlier bulk host append)
    if (c->payload_pending) { HIPCHK(c, hipEventSynchronize(c->ev_payload)); c->payload_pending = false; }
    if (!c->h_pin.reserve((size_t)K * 8)) return fail(c, SW_ENOMEM, "hipHostMalloc(%zu bytes) for the ingest read-back buffer failed", (size_t)K * 8);
    CHK(ensure_event(c, c->ing.ev_ht));
    // ---- the context's stream waits for what the caller enqueued; parent arrays to the (uncommitted) tail
    UserStream bracket;
    CHK(bracket.join(c, us));
    HIPCHK(c, hipMemcpyAsync(c->d_cr.p + N0, d_creator, b4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_sp.p + N0, d_self_parent, b4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_op.p + N0, d_other_parent, b4, hipMemcpyDeviceToDevice, c->stream));
    // ---- verdict word and per-member tables [nev | head | first]
    std::vector<int32_t>& tab = c->ing.stage;
    tab.assign((size_t)4 + 3 * np, 0);
    const unsigned long long none = ing::V_NONE;
    memcpy(tab.data(), &none, sizeof none);
    for (int m = 0; m < np; ++m) {
        tab[4 + m] = m < n ? c->nev[m] : 0;
        tab[4 + np + m] = m < n ? c->head[m] : -1;
        tab[4 + 2 * np + m] = (m < n && c->first_ev[m] >= 0) ? c->first_ev[m] : 0x7fffffff;
    }
    HIPCHK(c, hipMemcpyAsync(c->ing.d_tab.p, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    unsigned long long* d_v = (unsigned long long*)c->ing.d_tab.p;
    int* d_tab = c->ing.d_tab.p + 4;
    int nbits = 0;
    while ((1 << nbits) < np) ++nbits;
    const dim3 ev_grid((unsigned)((K + 255) / 256));
    hipLaunchKernelGGL(ing::k_ingest_local, ev_grid, dim3(256), 0, c->stream, c->d_cr.p, (const int*)c->d_sp.p, (const int*)c->d_op.p,
                       (int)N0, (int)K, n, d_v);
    hipLaunchKernelGGL(ing::k_ingest_hist, dim3(tiles), dim3(ing::THREADS), 0, c->stream, (const int*)c->d_cr.p, (int)N0, (int)K, np,
                       c->ing.d_hist.p, d_tab);
    hipLaunchKernelGGL(ing::k_ingest_scan, dim3((np + 63) / 64), dim3(64), 0, c->stream, c->ing.d_hist.p, tiles, np, d_tab);
    hipLaunchKernelGGL(ing::k_ingest_rank, dim3(tiles), dim3(ing::THREADS), 0, c->stream, (const int*)c->d_cr.p, (int)N0, (int)K, np, nbits,
                       (const int*)c->ing.d_hist.p, c->d_seq.p);
    hipLaunchKernelGGL(ing::k_ingest_links, ev_grid, dim3(256), 0, c->stream, (const int*)c->d_cr.p, (const int*)c->d_sp.p,
                       (const int*)c->d_op.p, (const int*)c->d_seq.p, (int)N0, (int)K, d_v);
    c->ctr.kernel_launches += 5;
    HIPCHK(c, hipGetLastError());
    // ---- one read-back: verdict and tables; the always-complete host mirrors (creator, chain position) ride along
    int32_t* pin_cr = (int32_t*)c->h_pin.p;
    int32_t* pin_seq = pin_cr + K;
    HIPCHK(c, hipMemcpyAsync(tab.data(), c->ing.d_tab.p, tab.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(pin_cr, c->d_cr.p + N0, b4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(pin_seq, c->d_seq.p + N0, b4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    bracket.drained();   // (the commit below drains the stream again before it returns; a failure inside it poisons the context)
    unsigned long long v;
    memcpy(&v, tab.data(), sizeof v);
    if (v != ing::V_NONE) {
        const long long e = (long long)(v >> 8);
        switch ((int)(v & 0xff)) {
            case ing::V_CREATOR: return fail(c, SW_EINVAL, "event %lld: creator out of range", e);
            case ing::V_ARITY: return fail(c, SW_EINVAL, "event %lld: must have 0 or 2 parents", e);
            case ing::V_ORDER: return fail(c, SW_EINVAL, "event %lld: parent index not earlier (not a topological order)", e);
            case ing::V_SELF: return fail(c, SW_EINVAL, "event %lld: self-parent is by another member", e);
            case ing::V_OTHER: return fail(c, SW_EINVAL, "event %lld: other-parent is by the same member", e);
            default:   // a fork: nothing is committed, the host path decides (exact path, or SW_ENOTSUP)
                return ingest_fallback(c, K, d_creator, d_self_parent, d_other_parent, d_t, d_sig64, us);
        }
    }
    // ---- commit.  From here on a device failure leaves the context inconsistent: it is poisoned.
    c->cr.insert(c->cr.end(), pin_cr, pin_cr + K);
    c->seq_h.insert(c->seq_h.end(), pin_seq, pin_seq + K);
    std::vector<int32_t> nev_t(c->nev);
    for (int m = 0; m < n; ++m) {
        nev_t[m] = tab[4 + m];
        c->head[m] = tab[4 + np + m];
        c->first_ev[m] = tab[4 + 2 * np + m] == 0x7fffffff ? -1 : tab[4 + 2 * np + m];
    }
    c->N = N0 + K;
    // payload: device to device on the context's stream (done when the call returns)
    if (d_t) PHIP(hipMemcpyAsync(c->d_t.p + N0, d_t, (size_t)K * 8, hipMemcpyDeviceToDevice, c->stream));
    else PHIP(hipMemsetAsync(c->d_t.p + N0, 0, (size_t)K * 8, c->stream));
    if (d_sig64) PHIP(hipMemcpyAsync(c->d_sig.p + (size_t)N0 * 64, d_sig64, (size_t)K * 64, hipMemcpyDeviceToDevice, c->stream));
    else PHIP(hipMemsetAsync(c->d_sig.p + (size_t)N0 * 64, 0, (size_t)K * 64, c->stream));
    hipLaunchKernelGGL(k_coin_bits, ev_grid, dim3(256), 0, c->stream, (const unsigned char*)c->d_sig.p, (int)N0, (int)K, c->d_coin.p);
    c->ctr.kernel_launches++;
    PHIP(hipMemsetAsync(c->d_round.p + N0, 0xff, b4, c->stream));
    // heights: behind the call, on the payload stream (the parent arrays are in place: the stream was drained above)
    std::vector<int32_t> st0((size_t)(2 + 2 * nblk));
    st0[0] = 0; st0[1] = -1;
    for (int64_t b = 0; b < nblk; ++b) { st0[2 + 2 * b] = 0x7fffffff; st0[3 + 2 * b] = -1; }
    PHIP(hipMemcpy(c->ing.d_ht_stat.p, st0.data(), st0.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(ing::k_ingest_heights, dim3(1), dim3(ing::HT_TILE), 0, c->stream_io, (const int*)c->d_sp.p, (const int*)c->d_op.p,
                       c->d_ht.p, (int)N0, (int)K, (int)blk0, c->ing.d_ht_stat.p);
    c->ctr.kernel_launches++;
    PHIP(hipGetLastError());
    PHIP(hipEventRecord(c->ing.ev_ht, c->stream_io));
    c->ing.ht_pending = true; c->ing.ht_first = N0; c->ing.ht_K = K; c->ing.ht_dev_upto = N0 + K;
    PCHK(rebuild_chains(c, nev_t, c->N));
    c->nev.swap(nev_t);
    PHIP(hipStreamSynchronize(c->stream));  // the caller's arrays may be reused or freed on return
    // ... and the caller's stream may not overwrite them before the copies above are done (they are: drained)
    c->ing.dev_batches++;
    c->ing.dev_events += K;
    return SW_OK;
}

int sw_append_events_device(sw_ctx* c, int64_t K, const int32_t* d_creator, const int32_t* d_self_parent,
                            const int32_t* d_other_parent, const double* d_t, const uint8_t* d_sig64, void* user_stream) {
    if (!c) return SW_EINVAL;
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (K < 0 || (K > 0 && (!d_creator || !d_self_parent || !d_other_parent))) return fail(c, SW_EINVAL, "NULL event arrays");
    if (K == 0) return SW_OK;
    if (c->N + K > 0x7ffffff0ll) return fail(c, SW_ERANGE, "more than 2^31 events");
    const size_t k = (size_t)K;
    CHK(device_args(c, "sw_append_events_device", {{d_creator, k * 4, 1}, {d_self_parent, k * 4, 1}, {d_other_parent, k * 4, 1}, {d_t, k * 8, 1}, {d_sig64, k * 64, 1}}));
    return append_device_body(c, K, d_creator, d_self_parent, d_other_parent, d_t, d_sig64, (hipStream_t)user_stream);
}

int sw_get_ingest_stats(sw_ctx* c, int64_t* device_batches, int64_t* device_events, int64_t* fallback_batches, int64_t* host_height_events) {
    if (!c) return SW_EINVAL;
    if (device_batches) *device_batches = c->ing.dev_batches;
    if (device_events) *device_events = c->ing.dev_events;
    if (fallback_batches) *fallback_batches = c->ing.fallback;
    if (host_height_events) *host_height_events = c->ing.host_ht;
    return SW_OK;
}

// ---- id index and payload ingest by event id (resolve.hip.h) ------------------------------------------------------
}  // extern "C"
namespace {

constexpr int PL_WAVE_BATCH = 32;   // waves launched between two read-backs of their counts

// (re)build the table from the ids the context holds
int idtab_rebuild(sw_ctx* c) {
    HIPCHK(c, hipMemsetAsync(c->ids.d_idtab.p, 0xff, sizeof(int32_t) << c->ids.idtab_log, c->stream));
    if (c->ids.n_ids) {
        hipLaunchKernelGGL(rsv::k_tab_insert, dim3((unsigned)((c->ids.n_ids + 255) / 256)), dim3(256), 0, c->stream, c->ids.d_idtab.p, c->ids.idtab_log,
                           (const unsigned char*)c->ids.d_id.p, 0, (int)c->ids.n_ids, (int*)nullptr);
        c->ctr.kernel_launches++;
        HIPCHK(c, hipGetLastError());
    }
    c->ids.pl_rebuilds++;
    return SW_OK;
}

// room for `count` ids: the id array (contents kept) and a table of load <= 1/2
int idindex_reserve(sw_ctx* c, int64_t count) {
    CHK(dgrow(c, c->ids.d_id, (size_t)count * 32, (size_t)c->ids.n_ids * 32));
    CHK(dgrow(c, c->ids.d_idflag, 4, 0));
    int lg = 10;
    while ((1ll << lg) < 2 * count) ++lg;
    if (lg <= c->ids.idtab_log) return SW_OK;
    CHK(dgrow(c, c->ids.d_idtab, (size_t)1 << lg, 0));
    c->ids.idtab_log = lg;
    return idtab_rebuild(c);
}

// insert the ids of the events [first, first + K) (already in d_id); *flag = 0 fine, 1 an id was present or twice, 2 table full
int idtab_insert(sw_ctx* c, int64_t first, int64_t K, int* flag) {
    HIPCHK(c, hipMemsetAsync(c->ids.d_idflag.p, 0, sizeof(int32_t), c->stream));
    hipLaunchKernelGGL(rsv::k_tab_insert, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream, c->ids.d_idtab.p, c->ids.idtab_log,
                       (const unsigned char*)c->ids.d_id.p, (int)first, (int)K, c->ids.d_idflag.p);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    int32_t f = 0;
    HIPCHK(c, hipMemcpyAsync(&f, c->ids.d_idflag.p, sizeof f, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *flag = f;
    return SW_OK;
}

// The payload call behind the argument checks.  Every array lies in device memory; d_out too.
int payload_core(sw_ctx* c, int64_t K, const uint8_t* d_id32, const uint8_t* d_sp_id32, const uint8_t* d_op_id32, const uint8_t* d_arity,
                 const int32_t* d_creator, const uint8_t* d_ok, const double* d_t, const uint8_t* d_sig64, hipStream_t us, int32_t* d_out,
                 int64_t* n_stored) {
    const int64_t N0 = c->N;
    const bool prof = c->profiling;
    auto t0 = std::chrono::steady_clock::now();
    // ---- allocations (nothing committed): ids and table for every event of the payload, scratch
    CHK(idindex_reserve(c, N0 + K));
    int llog = 4;
    while ((1ll << llog) < 2 * K) ++llog;
    const size_t nctr = (size_t)K + PL_WAVE_BATCH + 2;
    const size_t tiles0 = (size_t)((K + ing::TILE - 1) / ing::TILE);
    Carve cv;
    const size_t o_lslots = cv.take(sizeof(int32_t) << llog), o_wave = cv.take((size_t)K * 4), o_pr = cv.take((size_t)K * 8);
    const size_t o_la = cv.take((size_t)K * 4), o_lb = cv.take((size_t)K * 4), o_pend = cv.take(nctr * 4), o_acc = cv.take(nctr * 4);
    const size_t o_key = cv.take((size_t)K * 4), o_seq = cv.take((size_t)K * 4), o_oa = cv.take((size_t)K * 4), o_ob = cv.take((size_t)K * 4);
    const size_t o_rank = cv.take((size_t)K * 4), o_hist = cv.take(tiles0 * 1024 * 4), o_tab = cv.take(3 * 1024 * 4), o_base = cv.take(1024 * 4);
    const size_t o_gcr = cv.take((size_t)K * 4), o_gsp = cv.take((size_t)K * 4), o_gop = cv.take((size_t)K * 4);
    const size_t o_gt = cv.take(d_t ? (size_t)K * 8 : 0), o_gsig = cv.take(d_sig64 ? (size_t)K * 64 : 0);
    CHK(dgrow(c, c->ids.d_pl, cv.off, 0));
    unsigned char* B = c->ids.d_pl.p;
    int* lslots = (int*)(B + o_lslots); int* wave = (int*)(B + o_wave); int* pr = (int*)(B + o_pr);
    int* lst[2] = {(int*)(B + o_la), (int*)(B + o_lb)};
    int* pend = (int*)(B + o_pend); int* acc = (int*)(B + o_acc);
    int* key = (int*)(B + o_key); int* seq = (int*)(B + o_seq); int* ord[2] = {(int*)(B + o_oa), (int*)(B + o_ob)};
    int* rank_of = (int*)(B + o_rank); int* hist = (int*)(B + o_hist); int* tab = (int*)(B + o_tab); int* base = (int*)(B + o_base);
    int* g_cr = (int*)(B + o_gcr); int* g_sp = (int*)(B + o_gsp); int* g_op = (int*)(B + o_gop);
    double* g_t = d_t ? (double*)(B + o_gt) : nullptr;
    unsigned char* g_sig = d_sig64 ? B + o_gsig : nullptr;
    if (!c->ids.h_plcnt.reserve(2 * PL_WAVE_BATCH + 2)) return fail(c, SW_ENOMEM, "hipHostMalloc for the wave counts failed");
    UserStream bracket;   // (left by the destructor on a failure; a success has drained the stream)
    CHK(bracket.join(c, us));
    // ---- resolve: the payload's own table (lowest position of every id), local checks, parent references
    const dim3 ev_grid((unsigned)((K + 255) / 256));
    HIPCHK(c, hipMemsetAsync(lslots, 0xff, sizeof(int32_t) << llog, c->stream));
    HIPCHK(c, hipMemsetAsync(pend, 0, (o_acc - o_pend) + nctr * 4, c->stream));   // (pend and acc are neighbours)
    hipLaunchKernelGGL(rsv::k_tab_insert, ev_grid, dim3(256), 0, c->stream, lslots, llog, (const unsigned char*)d_id32, 0, (int)K, (int*)nullptr);
    hipLaunchKernelGGL(rsv::k_pl_local, ev_grid, dim3(256), 0, c->stream, (const int*)c->ids.d_idtab.p, N0 ? c->ids.idtab_log : 0,
                       (const unsigned char*)c->ids.d_id.p, (const int*)lslots, llog, (const unsigned char*)d_id32, (const unsigned char*)d_sp_id32,
                       (const unsigned char*)d_op_id32, (const unsigned char*)d_arity, (const int*)d_creator, (const unsigned char*)d_ok, (int)K, c->n,
                       (int*)d_out, wave, pr, lst[0], pend);
    c->ctr.kernel_launches += 2;
    HIPCHK(c, hipGetLastError());
    if (prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->ids.pl_ms[0] = ms_since(t0); t0 = std::chrono::steady_clock::now(); }
    // ---- waves: batches of launches, one read-back of their counts each; ends with the first wave that accepts nothing
    int64_t W = -1, A = 0, ub = K;
    for (int64_t w0 = 0; W < 0; w0 += PL_WAVE_BATCH) {
        if (w0 > K + 1) return fail(c, SW_EIO, "payload waves did not end after %lld waves (internal error)", (long long)w0);
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((ub + 255) / 256, 2048));
        for (int64_t w = w0; w < w0 + PL_WAVE_BATCH; ++w)
            hipLaunchKernelGGL(rsv::k_pl_wave, dim3(grid), dim3(256), 0, c->stream, (int)w, (const int*)lst[w & 1], (const int*)(pend + w), lst[(w + 1) & 1],
                               pend + w + 1, acc + w, (const int*)pr, (const int*)d_creator, (const int*)c->d_cr.p, wave, (int*)d_out);
        c->ctr.kernel_launches += PL_WAVE_BATCH;
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(c->ids.h_plcnt.p, pend + w0, (PL_WAVE_BATCH + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->ids.h_plcnt.p + PL_WAVE_BATCH + 1, acc + w0, PL_WAVE_BATCH * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int j = 0; j < PL_WAVE_BATCH; ++j) {
            const int a = c->ids.h_plcnt.p[PL_WAVE_BATCH + 1 + j];
            if (a == 0) { W = w0 + j; break; }
            A += a;
        }
        ub = c->ids.h_plcnt.p[PL_WAVE_BATCH];
    }
    hipLaunchKernelGGL(rsv::k_pl_leftover, ev_grid, dim3(256), 0, c->stream, (const int*)wave, (int)K, (int*)d_out);
    c->ctr.kernel_launches++;
    c->ids.pl_waves = W;
    c->ids.pl_accepted = A;
    c->ids.pl_calls++;
    if (prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->ids.pl_ms[1] = ms_since(t0); t0 = std::chrono::steady_clock::now(); }
    c->ids.pl_ms[2] = c->ids.pl_ms[3] = 0;
    if (A == 0) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        bracket.drained();
        return SW_OK;
    }
    // ---- dense order: stable sort of the accepted events by wave, LSD in passes of 10 bits through the stable-rank
    // kernels of ingest.hip.h (keys < 1024; an event that was not accepted has key -1 and drops out in pass 0)
    int passes = 1;
    while (passes < 4 && ((W - 1) >> (10 * passes)) > 0) ++passes;
    const int* cur = nullptr;
    for (int p = 0; p < passes; ++p) {
        const int64_t cnt = p == 0 ? K : A;
        const int tiles = (int)((cnt + ing::TILE - 1) / ing::TILE);
        const dim3 g((unsigned)((cnt + 255) / 256));
        int* dst = ord[p & 1];
        HIPCHK(c, hipMemsetAsync(tab, 0, 3 * 1024 * sizeof(int32_t), c->stream));
        hipLaunchKernelGGL(rsv::k_pl_keys, g, dim3(256), 0, c->stream, (const int*)wave, cur, (int)cnt, 10 * p, key);
        hipLaunchKernelGGL(ing::k_ingest_hist, dim3(tiles), dim3(ing::THREADS), 0, c->stream, (const int*)key, 0, (int)cnt, 1024, hist, tab);
        hipLaunchKernelGGL(ing::k_ingest_scan, dim3(1024 / 64), dim3(64), 0, c->stream, hist, tiles, 1024, tab);
        hipLaunchKernelGGL(ing::k_ingest_rank, dim3(tiles), dim3(ing::THREADS), 0, c->stream, (const int*)key, 0, (int)cnt, 1024, 10, (const int*)hist, seq);
        hipLaunchKernelGGL(rsv::k_pl_bases, dim3(1), dim3(1024), 0, c->stream, (const int*)tab, base);
        hipLaunchKernelGGL(rsv::k_pl_scatter, g, dim3(256), 0, c->stream, (const int*)key, (const int*)seq, (const int*)base, cur, (int)cnt, dst);
        c->ctr.kernel_launches += 6;
        HIPCHK(c, hipGetLastError());
        cur = dst;
    }
    const dim3 a_grid((unsigned)((A + 255) / 256));
    hipLaunchKernelGGL(rsv::k_pl_ranks, a_grid, dim3(256), 0, c->stream, cur, (int)A, (int)N0, rank_of, (int*)d_out);
    hipLaunchKernelGGL(rsv::k_pl_gather, a_grid, dim3(256), 0, c->stream, cur, (int)A, (int)N0, (const int*)rank_of, (const int*)pr, (const int*)d_creator,
                       (const unsigned char*)d_id32, d_t, g_cr, g_sp, g_op, g_t, c->ids.d_id.p + (size_t)N0 * 32);
    if (d_sig64)
        hipLaunchKernelGGL(rsv::k_pl_gather_sig, dim3((unsigned)((A * 16 + 255) / 256)), dim3(256), 0, c->stream, cur, (int)A, (const unsigned char*)d_sig64, g_sig);
    c->ctr.kernel_launches += 3;
    HIPCHK(c, hipGetLastError());
    if (prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->ids.pl_ms[2] = ms_since(t0); t0 = std::chrono::steady_clock::now(); }
    // ---- append (bulk device path or its fallbacks; atomic), then — only then — the ids
    CHK(append_device_body(c, A, g_cr, g_sp, g_op, g_t, g_sig, c->stream));
    int flag = 0;
    const int rc = idtab_insert(c, N0, A, &flag);
    if (rc != SW_OK || flag != 0) {
        c->poisoned = true;
        return rc != SW_OK ? rc : fail(c, SW_EIO, "id table insert after the append reported %d (internal error)", flag);
    }
    c->ids.n_ids = N0 + A;
    *n_stored = A;
    if (prof) c->ids.pl_ms[3] = ms_since(t0);
    bracket.drained();   // (idtab_insert has synchronised)
    return SW_OK;
}

int payload_args(sw_ctx* c, int64_t K, const void* id, const void* sp, const void* op, const void* ar, const void* cr, const void* out,
                 int64_t* n_stored, const char* what) {
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (!n_stored) return fail(c, SW_EINVAL, "%s: n_stored is NULL", what);
    *n_stored = 0;
    if (K < 0 || (K > 0 && (!id || !sp || !op || !ar || !cr || !out))) return fail(c, SW_EINVAL, "%s: NULL payload arrays", what);
    if (K > 0x3fffffffll || c->N + K > 0x7ffffff0ll) return fail(c, SW_ERANGE, "%s: more than 2^31 events", what);
    if (c->ids.n_ids != c->N)
        return fail(c, SW_ENOTSUP, "%s: %lld of the %lld stored events have no id (sw_set_event_ids first)", what, (long long)(c->N - c->ids.n_ids), (long long)c->N);
    return SW_OK;
}

}  // namespace
extern "C" {

int sw_set_event_ids(sw_ctx* c, int64_t first, int64_t K, const uint8_t* id32) {
    if (!c) return SW_EINVAL;
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (K < 0 || (K > 0 && !id32)) return fail(c, SW_EINVAL, "sw_set_event_ids: NULL ids");
    if (first != c->ids.n_ids) return fail(c, SW_EINVAL, "sw_set_event_ids must continue at event %lld (got %lld): ids are contiguous from 0", (long long)c->ids.n_ids, (long long)first);
    if (first + K > c->N) return fail(c, SW_ERANGE, "events [%lld, %lld) outside the stored hashgraph", (long long)first, (long long)(first + K));
    if (K == 0) return SW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    CHK(idindex_reserve(c, first + K));
    HIPCHK(c, hipMemcpyAsync(c->ids.d_id.p + (size_t)first * 32, id32, (size_t)K * 32, hipMemcpyHostToDevice, c->stream));
    int flag = 0;
    CHK(idtab_insert(c, first, K, &flag));
    if (flag != 0) {
        CHK(idtab_rebuild(c));   // (the table as it was: from the ids below `first`)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (flag == 1) return fail(c, SW_EINVAL, "sw_set_event_ids: an id is already present, or occurs twice in the call");
        return fail(c, SW_EIO, "sw_set_event_ids: id table full (internal error)");
    }
    c->ids.n_ids = first + K;
    return SW_OK;
}

int sw_get_event_ids(sw_ctx* c, int64_t first, int64_t K, uint8_t* out) {
    if (!c) return SW_EINVAL;
    if (first < 0 || K < 0 || first + K > c->ids.n_ids) return fail(c, SW_ERANGE, "events [%lld, %lld) beyond the %lld events that have ids", (long long)first, (long long)(first + K), (long long)c->ids.n_ids);
    if (K == 0) return SW_OK;
    if (!out) return fail(c, SW_EINVAL, "sw_get_event_ids: NULL output");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->ids.d_id.p + (size_t)first * 32, (size_t)K * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

int sw_lookup_event_ids(sw_ctx* c, int64_t K, const uint8_t* id32, int32_t* index_out) {
    if (!c) return SW_EINVAL;
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (K < 0 || K > 0x3fffffffll || (K > 0 && (!id32 || !index_out))) return fail(c, SW_EINVAL, "sw_lookup_event_ids: NULL arrays");
    if (K == 0) return SW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    Stage st;
    const size_t o_id = st.in(id32, (size_t)K * 32), o_out = st.out(index_out, (size_t)K * 4);
    unsigned char* B = nullptr;
    CHK(stage_up(c, c->ids.d_pl_in, st, &B));
    hipLaunchKernelGGL(rsv::k_tab_lookup, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream, (const int*)c->ids.d_idtab.p, c->ids.n_ids ? c->ids.idtab_log : 0,
                       (const unsigned char*)c->ids.d_id.p, (const unsigned char*)(B + o_id), (int)K, (int*)(B + o_out));
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    return stage_down(c, st, B);
}

int sw_ingest_payload_device(sw_ctx* c, int64_t K, const uint8_t* d_id32, const uint8_t* d_sp_id32, const uint8_t* d_op_id32, const uint8_t* d_arity,
                             const int32_t* d_creator, const uint8_t* d_ok, const double* d_t, const uint8_t* d_sig64, void* user_stream,
                             int32_t* d_index_out, int64_t* n_stored) {
    if (!c) return SW_EINVAL;
    CHK(payload_args(c, K, d_id32, d_sp_id32, d_op_id32, d_arity, d_creator, d_index_out, n_stored, "sw_ingest_payload_device"));
    if (K == 0) return SW_OK;
    const size_t k = (size_t)K;
    CHK(device_args(c, "sw_ingest_payload_device", {{d_id32, k * 32, 8}, {d_sp_id32, k * 32, 8}, {d_op_id32, k * 32, 8}, {d_arity, k, 1}, {d_creator, k * 4, 1},
                                                    {d_index_out, k * 4, 1}, {d_ok, k, 1}, {d_t, k * 8, 1}, {d_sig64, k * 64, 1}}));
    return payload_core(c, K, d_id32, d_sp_id32, d_op_id32, d_arity, d_creator, d_ok, d_t, d_sig64, (hipStream_t)user_stream, d_index_out, n_stored);
}

int sw_ingest_payload(sw_ctx* c, int64_t K, const uint8_t* id32, const uint8_t* sp_id32, const uint8_t* op_id32, const uint8_t* arity,
                      const int32_t* creator, const uint8_t* ok, const double* t, const uint8_t* sig64, int32_t* index_out, int64_t* n_stored) {
    if (!c) return SW_EINVAL;
    CHK(payload_args(c, K, id32, sp_id32, op_id32, arity, creator, index_out, n_stored, "sw_ingest_payload"));
    if (K == 0) return SW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t k = (size_t)K;
    Stage st;
    const size_t o_id = st.in(id32, k * 32), o_sp = st.in(sp_id32, k * 32), o_op = st.in(op_id32, k * 32), o_ar = st.in(arity, k), o_cr = st.in(creator, k * 4);
    const size_t o_ok = st.in(ok, k), o_t = st.in(t, k * 8), o_sig = st.in(sig64, k * 64), o_out = st.out(index_out, k * 4);
    unsigned char* B = nullptr;
    CHK(stage_up(c, c->ids.d_pl_in, st, &B));
    CHK(payload_core(c, K, B + o_id, B + o_sp, B + o_op, B + o_ar, (const int32_t*)(B + o_cr), ok ? B + o_ok : nullptr,
                     t ? (const double*)(B + o_t) : nullptr, sig64 ? B + o_sig : nullptr, c->stream, (int32_t*)(B + o_out), n_stored));
    return stage_down(c, st, B);
}

int sw_get_payload_stats(sw_ctx* c, int64_t* calls, int64_t* waves, int64_t* accepted, int64_t* table_rebuilds, double* phase_ms) {
    if (!c) return SW_EINVAL;
    if (calls) *calls = c->ids.pl_calls;
    if (waves) *waves = c->ids.pl_waves;
    if (accepted) *accepted = c->ids.pl_accepted;
    if (table_rebuilds) *table_rebuilds = c->ids.pl_rebuilds;
    if (phase_ms) for (int i = 0; i < 4; ++i) phase_ms[i] = c->ids.pl_ms[i];
    return SW_OK;
}

int sw_divide_rounds(sw_ctx* c, int64_t first, int64_t K) {
    if (!c) return SW_EINVAL;
    if (K < 0 || first < 0 || first + K > c->N) return fail(c, SW_ERANGE, "events [%lld, %lld) outside the stored hashgraph", (long long)first, (long long)(first + K));
    if (first != c->divided) return fail(c, SW_EINVAL, "divide_rounds must continue at event %lld (got %lld): every event is divided once, in order", (long long)c->divided, (long long)first);
    if (K == 0) return SW_OK;
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->exact) return exact_divide(c, first, K);
    switch (c->nw) {
        case 1: return do_divide<1>(c, first, K);
        case 2: return do_divide<2>(c, first, K);
        case 4: return do_divide<4>(c, first, K);
        case 8: return do_divide<8>(c, first, K);
        case 16: return do_divide<16>(c, first, K);
    }
    return fail(c, SW_EINVAL, "unsupported member count");
}

int sw_decide_fame(sw_ctx* c, int32_t* new_rounds, int cap, int* n_new) {
    if (!c) return SW_EINVAL;
    if (n_new) *n_new = 0;
    if (c->R <= 0) return fail(c, SW_EINVAL, "decide_fame before any witness exists (max() of an empty dict in the reference, swirld.py:225)");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->exact) return exact_fame(c, new_rounds, cap, n_new);
    switch (c->nw) {
        case 1: return do_fame<1>(c, new_rounds, cap, n_new);
        case 2: return do_fame<2>(c, new_rounds, cap, n_new);
        case 4: return do_fame<4>(c, new_rounds, cap, n_new);
        case 8: return do_fame<8>(c, new_rounds, cap, n_new);
        case 16: return do_fame<16>(c, new_rounds, cap, n_new);
    }
    return fail(c, SW_EINVAL, "unsupported member count");
}

int sw_decide_fame_partial(sw_ctx* c, int part, int nparts, int8_t* famous, uint8_t* decided, int r_cap, int* r_out) {
    if (!c || !famous || !decided) return SW_EINVAL;
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (nparts < 1 || part < 0 || part >= nparts) return fail(c, SW_EINVAL, "part %d of %d", part, nparts);
    if (c->exact) return fail(c, SW_ENOTSUP, "sw_decide_fame_partial is not available on the exact (forked-hashgraph) path");
    if (c->R <= 0) return fail(c, SW_EINVAL, "decide_fame before any witness exists (max() of an empty dict in the reference, swirld.py:225)");
    if (r_out) *r_out = c->R;
    if (r_cap < c->R) return fail(c, SW_ERANGE, "famous / decided hold %d rounds, %d needed", r_cap, c->R);
    HIPCHK(c, hipSetDevice(c->device));
    switch (c->nw) {
        case 1: return do_fame_partial<1>(c, part, nparts, famous, decided);
        case 2: return do_fame_partial<2>(c, part, nparts, famous, decided);
        case 4: return do_fame_partial<4>(c, part, nparts, famous, decided);
        case 8: return do_fame_partial<8>(c, part, nparts, famous, decided);
        case 16: return do_fame_partial<16>(c, part, nparts, famous, decided);
    }
    return fail(c, SW_EINVAL, "unsupported member count");
}

int sw_commit_fame(sw_ctx* c, const int8_t* famous, const uint8_t* decided, int R, int32_t* new_rounds, int cap, int* n_new) {
    if (!c || !famous || !decided) return SW_EINVAL;
    if (n_new) *n_new = 0;
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (R != c->R) return fail(c, SW_EINVAL, "merged table has %d rounds, the context %d", R, c->R);
    if (c->exact) return fail(c, SW_ENOTSUP, "sw_commit_fame is not available on the exact (forked-hashgraph) path");
    HIPCHK(c, hipSetDevice(c->device));
    const int np = c->npad, n = c->n;
    const int max_c = first_undecided_round(c);
    std::vector<signed char> fam((size_t)(R - max_c) * np, (signed char)-1);
    std::vector<unsigned char> cons(R - max_c, 0);
    const int call_idx = (int)c->fame_calls.size();
    c->fame_calls.push_back({max_c, R, c->divided});
    c->votes_partial = true;  // the deciding call / voter of witnesses decided by other parts is unknown here: sw_get_vote refuses
    int cnt = 0;
    for (int r = max_c; r < R; ++r) {
        for (int m = 0; m < n; ++m) fam[(size_t)(r - max_c) * np + m] = famous[(size_t)r * n + m];
        if (decided[r]) {
            c->cons_h[r] = 1;
            c->cons_call[r] = call_idx;
            if (cnt < cap && new_rounds) new_rounds[cnt] = r;
            ++cnt;
        }
        cons[r - max_c] = c->cons_h[r];
    }
    if (R > max_c) {
        HIPCHK(c, hipMemcpyAsync(c->d_fam.p + (size_t)max_c * np, fam.data(), fam.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_cons.p + max_c, cons.data(), cons.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (n_new) *n_new = cnt;
    if (cnt > cap) return fail(c, SW_ERANGE, "new_rounds capacity %d < %d", cap, cnt);
    return SW_OK;
}

// ---- multi-GPU split of the can_see table by event ranges -----------------------
static int range_checks(sw_ctx* c, int64_t first, int64_t K, const char* what) {
    if (!c) return SW_EINVAL;
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (c->exact) return fail(c, SW_ENOTSUP, "%s is not available on the exact (forked-hashgraph) path", what);
    if (c->vm.active) return fail(c, SW_ENOTSUP, "%s is not available with the windowed table", what);
    if (c->npad > 256 || c->cansee_impl != 6) return fail(c, SW_ENOTSUP, "%s needs the chunk-parallel dataflow sweep (at most 256 members)", what);
    if (first < 0 || K <= 0 || first + K > c->N) return fail(c, SW_ERANGE, "%s: events [%lld, %lld) outside the stored hashgraph", what, (long long)first, (long long)(first + K));
    if (first < c->divided) return fail(c, SW_EINVAL, "%s: events below %lld are divided already", what, (long long)c->divided);
    return SW_OK;
}

static void mark_present(sw_ctx* c, int64_t a, int64_t b) {
    c->present.push_back({a, b});
    std::sort(c->present.begin(), c->present.end());
    std::vector<std::pair<int64_t, int64_t>> m;
    for (const auto& pr : c->present) {
        if (!m.empty() && pr.first <= m.back().second) m.back().second = std::max(m.back().second, pr.second);
        else m.push_back(pr);
    }
    c->present.swap(m);
}

int sw_row_stride(const sw_ctx* c) { return c ? c->npad : 0; }
int sw_get_tally_impl(const sw_ctx* c) { return c ? (c->unit_stake ? c->tally_impl : 0) : SW_EINVAL; }

}  // extern "C"
template <int NW>
static int do_cansee_range(sw_ctx* c, int64_t first, int64_t K) {
    const int np = c->npad;
    if ((int)c->ranges.size() >= SW_RANGE_SLOTS) return fail(c, SW_ERANGE, "more than %d ranges between two rewinds", SW_RANGE_SLOTS);
    for (const auto& pr : c->present)
        if (first < pr.second && first + K > pr.first) return fail(c, SW_EINVAL, "sw_cansee_range: rows [%lld, %lld) are present already", (long long)pr.first, (long long)pr.second);
    if (!c->d_rprov.p) {
        CHK(dgrow(c, c->d_rprov, (size_t)SW_RANGE_SLOTS * (SW_MAX_CHUNKS + 1), 0));
        CHK(ensure_event(c, c->ev_user));
    }
    if (c->d_L.cap < table_elems(c, c->cap)) return fail(c, SW_EIO, "the can_see table has no halo scratch rows (internal)");
    sw_ctx::RangeRec r;
    r.first = first; r.K = K;
    r.slot = (int)c->ranges.size();
    r.row0 = r.slot * (2 * SW_MAX_CHUNKS + 2);
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>(c->chunks, K / std::max<int64_t>(c->chunk_min, 1)));
    r.pl.G = G;
    std::vector<long long>& cc = c->rcuts_stage;
    cc.assign((size_t)2 * SW_MAX_CHUNKS + 2, first + K);
    for (int k = 0; k <= G; ++k) r.pl.a[k] = first + K * k / G;
    for (int k = 0; k < G; ++k) {
        r.pl.w[k] = std::max<int64_t>(0, r.pl.a[k] - c->halo);   // chunk 0 has a halo too: nothing below the range is here yet
        cc[2 * k] = r.pl.w[k];
        cc[2 * k + 1] = r.pl.a[k];
    }
    cc[2 * G] = cc[2 * G + 1] = r.pl.a[G];
    hipStream_t cs = c->stream_cs;
    // behind whatever the main stream still has in flight (appends return without a host synchronisation)
    HIPCHK(c, hipEventRecord(c->ev_main_mark, c->stream));
    HIPCHK(c, hipStreamWaitEvent(cs, c->ev_main_mark, 0));
    CHK(dgrow(c, c->d_rcuts, (size_t)SW_RANGE_SLOTS * (2 * SW_MAX_CHUNKS + 2), 0));
    CHK(dgrow(c, c->d_rbnd, (size_t)SW_RANGE_SLOTS * (2 * SW_MAX_CHUNKS + 2) * np, 0));
    HIPCHK(c, hipMemcpyAsync(c->d_rcuts.p + r.row0, cc.data(), cc.size() * sizeof(long long), hipMemcpyHostToDevice, cs));
    HIPCHK(c, hipStreamSynchronize(cs));   // (one staging vector per context: reusable on return)
    hipLaunchKernelGGL(k_chain_bounds, dim3((unsigned)cc.size()), dim3(np), 0, cs, (const int*)c->d_chain_start.p,
                       (const int*)c->d_chain_cnt.p, (const int*)c->d_chain_ev.p, (const long long*)(c->d_rcuts.p + r.row0), np,
                       c->d_rbnd.p + (size_t)r.row0 * np);
    unsigned* prov = c->d_rprov.p + (size_t)r.slot * (SW_MAX_CHUNKS + 1);
    HIPCHK(c, hipMemsetAsync(prov, 0, (SW_MAX_CHUNKS + 1) * sizeof(unsigned), cs));
    c->ctr.kernel_launches++;
    CHK(launch_cansee_plan<NW>(c, r.pl, (const int*)c->d_rbnd.p + (size_t)r.row0 * np, prov, prov + SW_MAX_CHUNKS, 0, true, 0, 0));
    c->ranges.push_back(r);
    mark_present(c, first, first + K);
    return SW_OK;
}

extern "C" {
int sw_cansee_range(sw_ctx* c, int64_t first, int64_t K) {
    CHK(range_checks(c, first, K, "sw_cansee_range"));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ensure_events(c, c->N));
    switch (c->nw) {
        case 1: return do_cansee_range<1>(c, first, K);
        case 2: return do_cansee_range<2>(c, first, K);
        case 4: return do_cansee_range<4>(c, first, K);
    }
    return fail(c, SW_ENOTSUP, "sw_cansee_range: more than 256 members");
}

int sw_cansee_repair(sw_ctx* c, int64_t first, int64_t K) {
    CHK(range_checks(c, first, K, "sw_cansee_repair"));
    HIPCHK(c, hipSetDevice(c->device));
    for (auto& r : c->ranges) {
        if (r.first != first || r.K != K) continue;
        if (r.repaired) return SW_OK;
        // every row below the range must be here: the repair reads the rows the provisional entries name
        int64_t covered = c->divided;
        for (const auto& pr : c->present) if (pr.first <= covered) covered = std::max(covered, pr.second);
        if (covered < first) return fail(c, SW_EINVAL, "sw_cansee_repair: the rows [%lld, %lld) below the range are not present yet", (long long)covered, (long long)first);
        const int np = c->npad;
        unsigned* prov = c->d_rprov.p + (size_t)r.slot * (SW_MAX_CHUNKS + 1);
        const int k_from = r.pl.w[0] > 0 ? 0 : 1;   // (a range that starts at event 0 has no halo in front of its first chunk)
        int rc = SW_EINVAL;
        switch (c->nw) {
            case 1: rc = launch_cansee_plan<1>(c, r.pl, (const int*)c->d_rbnd.p + (size_t)r.row0 * np, prov, prov + SW_MAX_CHUNKS, 0, false, k_from, r.pl.G); break;
            case 2: rc = launch_cansee_plan<2>(c, r.pl, (const int*)c->d_rbnd.p + (size_t)r.row0 * np, prov, prov + SW_MAX_CHUNKS, 0, false, k_from, r.pl.G); break;
            case 4: rc = launch_cansee_plan<4>(c, r.pl, (const int*)c->d_rbnd.p + (size_t)r.row0 * np, prov, prov + SW_MAX_CHUNKS, 0, false, k_from, r.pl.G); break;
        }
        CHK(rc);
        r.repaired = true;
        return SW_OK;
    }
    return fail(c, SW_EINVAL, "sw_cansee_repair: [%lld, %lld) is not a range swept by sw_cansee_range", (long long)first, (long long)(first + K));
}

int sw_export_rows(sw_ctx* c, int64_t first, int64_t K, void* dst_device, void* user_stream) {
    if (!c || !dst_device) return SW_EINVAL;
    if (c->exact || c->vm.active) return fail(c, SW_ENOTSUP, "sw_export_rows: fast path with the plain table only");
    if (first < 0 || K <= 0 || first + K > c->N) return fail(c, SW_ERANGE, "sw_export_rows: events [%lld, %lld) outside the stored hashgraph", (long long)first, (long long)(first + K));
    bool ok = first + K <= c->divided;
    for (const auto& pr : c->present) ok = ok || (first >= pr.first && first + K <= pr.second);
    if (!ok) return fail(c, SW_EINVAL, "sw_export_rows: the rows [%lld, %lld) have not been computed here", (long long)first, (long long)(first + K));
    HIPCHK(c, hipSetDevice(c->device));
    // the destination may still be read by work the caller enqueued earlier (a previous collective)
    UserStream bracket;
    CHK(bracket.join(c, (hipStream_t)user_stream, c->stream_cs));
    HIPCHK(c, hipMemcpyAsync(dst_device, c->d_L.p + (size_t)first * c->npad, (size_t)K * c->npad * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream_cs));
    return bracket.leave();
}

int sw_import_rows(sw_ctx* c, int64_t first, int64_t K, const void* src_device, void* user_stream) {
    if (!src_device) return SW_EINVAL;
    CHK(range_checks(c, first, K, "sw_import_rows"));
    for (const auto& pr : c->present)
        if (first < pr.second && first + K > pr.first) return fail(c, SW_EINVAL, "sw_import_rows: rows [%lld, %lld) are present already", (long long)pr.first, (long long)pr.second);
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ensure_events(c, c->N));
    UserStream bracket;   // what the caller enqueued so far (the collective that fills src); it may not reuse src before the copy is done
    CHK(bracket.join(c, (hipStream_t)user_stream, c->stream_cs));
    HIPCHK(c, hipMemcpyAsync(c->d_L.p + (size_t)first * c->npad, src_device, (size_t)K * c->npad * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream_cs));
    CHK(bracket.leave());
    mark_present(c, first, first + K);
    return SW_OK;
}

int sw_get_range_stats(sw_ctx* c, int64_t* provisional, int64_t* repaired, int64_t* resweeps) {
    if (!c) return SW_EINVAL;
    int64_t pv = 0, rp = 0, rs = 0;
    if (c->d_rprov.p && !c->ranges.empty()) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream_cs));
        std::vector<unsigned> h((size_t)SW_RANGE_SLOTS * (SW_MAX_CHUNKS + 1));
        HIPCHK(c, hipMemcpy(h.data(), c->d_rprov.p, h.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
        for (const auto& r : c->ranges) {
            const unsigned* p = h.data() + (size_t)r.slot * (SW_MAX_CHUNKS + 1);
            const int Cc = c->chunk_cfg == 1 ? 2 : 4;
            for (int k = 0; k < r.pl.G; ++k) {
                pv += p[k];
                const int64_t len = r.pl.a[k + 1] - r.pl.a[k];
                if ((k > 0 || r.pl.w[0] > 0) && p[k] > (unsigned)std::min<int64_t>((len * c->n) / (32 * Cc), 0x7fffffff)) ++rs;
            }
            rp += p[SW_MAX_CHUNKS];
        }
    }
    if (provisional) *provisional = pv;
    if (repaired) *repaired = rp;
    if (resweeps) *resweeps = rs;
    return SW_OK;
}

int sw_set_window(sw_ctx* c, int enable, int chunk_mb) {
    if (!c) return SW_EINVAL;
    if (c->N != 0) return fail(c, SW_EINVAL, "sw_set_window must be called before the first event is appended");
    HIPCHK(c, hipSetDevice(c->device));
    if (!enable) {
        if (c->vm.active) {
            HIPCHK(c, hipDeviceSynchronize());
            vm_destroy(c);
            c->d_L.release();
            if (c->cap) CHK(dgrow(c, c->d_L, table_elems(c, c->cap), 0));   // (with the halo scratch rows: ADVICE r3)
        }
        return SW_OK;
    }
    if (c->vm.active) return SW_OK;
    HIPCHK(c, hipDeviceSynchronize());
    c->d_L.reset();
    hipMemAllocationProp prop{};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = c->device;
    size_t gran = 0;
    HIPCHK(c, hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended));
    if (gran == 0) gran = 4096;
    if (chunk_mb <= 0) chunk_mb = 64;
    if (const char* e_ = getenv("SW_VM_CHUNK_MB")) chunk_mb = std::max(1, atoi(e_));
    VmTable& v = c->vm;
    v.chunk = (((size_t)chunk_mb << 20) + gran - 1) / gran * gran;
    const size_t rowbytes = (size_t)c->npad * sizeof(int32_t);
    size_t va = std::min<size_t>((size_t)0x7ffffff0ull * rowbytes, (size_t)4 << 40);  // up to 4 TB of address space
    va = (va + v.chunk - 1) / v.chunk * v.chunk;
    void* base = nullptr;
    hipError_t e = hipMemAddressReserve(&base, va, 0, nullptr, 0);
    if (e != hipSuccess) { v = VmTable{}; return fail(c, SW_ENOMEM, "hipMemAddressReserve(%zu GB) failed: %s", va >> 30, hipGetErrorString(e)); }
    v.base = (char*)base;
    v.va_bytes = va;
    v.handle.assign(va / v.chunk, hipMemGenericAllocationHandle_t{});
    v.mapped.assign(va / v.chunk, 0);
    v.active = true;
    c->d_L.alias((int32_t*)base, va / sizeof(int32_t));
    c->first_resident = 0;
    return SW_OK;
}

int sw_set_window_lapse(sw_ctx* c, int64_t events) {
    if (!c) return SW_EINVAL;
    if (events < 0) return fail(c, SW_EINVAL, "sw_set_window_lapse: a number of events >= 0 (0 = members never lapse)");
    if (!c->vm.active && events > 0) return fail(c, SW_EINVAL, "sw_set_window_lapse needs the windowed table (sw_set_window first)");
    c->window_lapse = events;
    if (events == 0) c->lapsed.clear();
    return SW_OK;
}

int sw_get_window(sw_ctx* c, int64_t* first_resident_event, int64_t* resident_bytes, int64_t* evictions) {
    if (!c) return SW_EINVAL;
    if (first_resident_event) *first_resident_event = c->first_resident;
    if (resident_bytes) {
        if (c->vm.active) { size_t cnt = 0; for (char m_ : c->vm.mapped) cnt += m_ != 0; *resident_bytes = (int64_t)(cnt * c->vm.chunk); }
        else *resident_bytes = (int64_t)(c->d_L.cap * sizeof(int32_t));
    }
    if (evictions) *evictions = c->vm.evictions;
    return SW_OK;
}

int sw_set_forks(sw_ctx* c, int accept) {
    if (!c) return SW_EINVAL;
    if (accept != 0 && accept != 1) return fail(c, SW_EINVAL, "sw_set_forks: 0 (refuse) or 1 (accept)");
    c->forks_mode = accept;
    return SW_OK;
}

int sw_get_exact(sw_ctx* c, int* out) {
    if (!c || !out) return SW_EINVAL;
    *out = c->exact ? 1 : 0;
    return SW_OK;
}

// Members of witnesses[r] in dict insertion order (what iterating self.witnesses[r] yields, swirld.py:234, 240):
// ascending event index of a member's FIRST witness of the round — which is the table entry unless a fork
// sibling replaced it (exact path: kept explicitly).
int sw_get_witness_order(sw_ctx* c, int r, int32_t* members, int* n_out) {
    if (!c || !members || !n_out) return SW_EINVAL;
    *n_out = 0;
    if (r < 0 || r >= c->R) return fail(c, SW_ERANGE, "round %d outside [0, %d)", r, c->R);
    HIPCHK(c, hipSetDevice(c->device));
    const int np = c->npad, n = c->n;
    if (c->exact) {
        int32_t cnt = 0;
        std::vector<int32_t> row(np);
        HIPCHK(c, hipMemcpyAsync(&cnt, c->ex.wcnt.p + r, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(row.data(), c->ex.worder.p + (size_t)r * np, np * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int i = 0; i < cnt; ++i) members[i] = row[i];
        *n_out = cnt;
        return SW_OK;
    }
    std::vector<int32_t> row(np);
    HIPCHK(c, hipMemcpyAsync(row.data(), c->d_wit.p + (size_t)r * np, np * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<std::pair<int32_t, int32_t>> ws;
    for (int m = 0; m < n; ++m) if (row[m] >= 0) ws.push_back({row[m], m});
    std::sort(ws.begin(), ws.end());
    for (size_t i = 0; i < ws.size(); ++i) members[i] = ws[i].second;
    *n_out = (int)ws.size();
    return SW_OK;
}

// What a rewind and a reset do to a subsystem's state is written ONCE, in the rewind() / reset() of its state struct
// (sw_ctx); a struct without them is left alone by both calls.  Here: the list of those calls, the core's own tables,
// and the device work at its place in stream order.
int sw_rewind(sw_ctx* c) {
    if (!c) return SW_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream_cs));   // (calls return without a host synchronisation)
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    const size_t rows = (size_t)c->Rcap * c->npad;
    c->hist.rewind();
    c->votes.rewind();
    c->ing.rewind();
    c->ids.rewind();
    c->data.rewind();
    c->walk.rewind();
    c->fame_calls.clear();
    c->votes_partial = false;
    c->eval_src = 0;
    std::fill(c->cons_call.begin(), c->cons_call.end(), -1);
    {   // every table back to its initial value, one launch (byte tables as 32-bit words: their allocations are padded to 256 B)
        RewindJob J{};
        int nj = 0;
        auto job = [&](void* p_, size_t words, int v) { if (p_ && words) { J.p[nj] = (int*)p_; J.n[nj] = words; J.v[nj] = v; ++nj; } };
        job(c->d_lo.p, rows, SW_INF);
        job(c->d_lopos.p, rows, 0);
        job(c->d_wit.p, rows, -1);
        job(c->d_dec_call.p, rows, -1);
        job(c->d_dec_by.p, rows, -1);
        job(c->d_evalround.p, 2 * (size_t)c->npad, -1);
        job(c->d_evalpos.p, 2 * (size_t)c->npad, 0);
        job(c->d_front.p, c->npad, -1);
        job(c->d_round.p, (size_t)c->N, -1);
        if (rows % 4 == 0) job(c->d_fam.p, rows / 4, -1);
        else HIPCHK(c, hipMemsetAsync(c->d_fam.p, 0xff, rows, c->stream));
        if (c->Rcap % 4 == 0) job(c->d_cons.p, (size_t)c->Rcap / 4, 0);
        else HIPCHK(c, hipMemsetAsync(c->d_cons.p, 0, c->Rcap, c->stream));
        size_t longest = 1;
        for (int i = 0; i < nj; ++i) longest = std::max<size_t>(longest, J.n[i]);
        if (nj) {
            hipLaunchKernelGGL(k_rewind_fill, dim3((unsigned)std::min<size_t>((longest + 1023) / 1024, 1024), nj), dim3(256), 0, c->stream, J);
            c->ctr.kernel_launches++;
            HIPCHK(c, hipGetLastError());
        }
    }
    std::fill(c->front.begin(), c->front.end(), -1);
    std::fill(c->divided_cnt.begin(), c->divided_cnt.end(), 0);
    std::fill(c->lapsed.begin(), c->lapsed.end(), 0);   // (every row is mapped again below: nobody has lapsed)
    if (c->vm.active && c->vm.lo > 0) {
        // every row is recomputed from event 0: the whole table moves to a fresh reservation (made before
        // the old one is given back, so the addresses differ), physical chunks recycled through the pool
        HIPCHK(c, hipDeviceSynchronize());
        VmTable& v = c->vm;
        void* base = nullptr;
        hipError_t e = hipMemAddressReserve(&base, v.va_bytes, 0, nullptr, 0);
        if (e != hipSuccess) { c->poisoned = true; return fail(c, SW_ENOMEM, "hipMemAddressReserve failed on rewind: %s", hipGetErrorString(e)); }
        for (size_t s_ = 0; s_ < v.mapped.size(); ++s_)
            if (v.mapped[s_]) { HIPCHK(c, hipMemUnmap(v.base + s_ * v.chunk, v.chunk)); v.pool.push_back(v.handle[s_]); v.mapped[s_] = 0; }
        HIPCHK(c, hipMemAddressFree(v.base, v.va_bytes));
        CHK(vm_flush_translations(c));
        v.base = (char*)base;
        v.lo = 0; v.hi = 0;
        c->vm_scratch_ok = false;
        c->d_L.alias((int32_t*)base, c->d_L.cap);
        c->first_resident = 0;
        CHK(vm_ensure(c, (size_t)c->N * c->npad * sizeof(int32_t)));
    }
    c->ranges.clear();
    c->present.clear();
    std::fill(c->divided_head.begin(), c->divided_head.end(), -1);
    std::fill(c->lo0_h.begin(), c->lo0_h.end(), SW_INF);
    std::fill(c->cons_h.begin(), c->cons_h.end(), 0);
    c->divided = 0;
    c->R = 0;
    c->sw_dirty_from = 1;
    c->dbg_iter_base = c->ctr.round_iterations;   // (the phase stamps of the loop kernels count from the rewind)
    c->transactions.clear();
    c->cons.rewind();   // (with the host's order, behind the device work: an early return above leaves both as they were)
    std::fill(c->ord_pos.begin(), c->ord_pos.end(), 0);
    if (c->exact) CHK(exact_rewind(c));
    return SW_OK;
}

int sw_reset(sw_ctx* c) {
    if (!c) return SW_EINVAL;
    CHK(sw_rewind(c));
    // forget the events as well; device storage (and the launch graphs keyed on it) stays
    c->cr.clear(); c->sp.clear(); c->op.clear(); c->ht.clear(); c->seq_h.clear();
    std::fill(c->head.begin(), c->head.end(), -1);
    std::fill(c->first_ev.begin(), c->first_ev.end(), -1);
    std::fill(c->nev.begin(), c->nev.end(), 0);
    c->blk_hmin.clear(); c->blk_hmax.clear();
    c->max_height = 0;
    c->N = 0;
    c->sig_h.clear();
    c->chain_cap.clear();
    c->chain_ev_h.clear();
    c->pool_used = 0;
    c->pool_h_valid = true;
    if (c->stream_io) HIPCHK(c, hipStreamSynchronize(c->stream_io));  // a payload upload may still be writing t / sig
    c->payload_pending = false;
    c->hist.reset();
    c->votes.reset();
    c->cons.reset();
    c->ing.reset();    // (the heights kernel of a device append ran on stream_io too)
    c->ids.reset();    // ... and its table is emptied here, on the stream
    c->data.reset();
    c->walk.reset();
    if (c->ids.idtab_log) HIPCHK(c, hipMemsetAsync(c->ids.d_idtab.p, 0xff, sizeof(int32_t) << c->ids.idtab_log, c->stream));
    c->exact = false;  // (a fresh hashgraph starts on the fast path again)
    c->chunks_off = false;  // ... and with the chunked sweep
    return SW_OK;
}

int sw_split_link(sw_ctx* const* ctxs, int parts) {
    if (!ctxs || parts < 2 || parts > SW_MAX_PARTS) return fail(nullptr, SW_EINVAL, "sw_split_link: 2 .. %d contexts", SW_MAX_PARTS);
    sw_ctx* c0 = ctxs[0];
    for (int q = 0; q < parts; ++q) {
        sw_ctx* c = ctxs[q];
        if (!c) return fail(c0, SW_EINVAL, "sw_split_link: context %d is NULL", q);
        for (int o = 0; o < q; ++o) if (ctxs[o] == c) return fail(c, SW_EINVAL, "sw_split_link: context %d given twice", q);
        if (c->poisoned) return fail(c, SW_EIO, "context poisoned by an earlier failure");
        if (c->split) return fail(c, SW_EINVAL, "sw_split_link: context %d is linked already", q);
        if (c->exact || c->vm.active || !c->unit_stake)
            return fail(c, SW_ENOTSUP, "sw_split_link: unit stake, the fast path and the plain can_see table only");
        if (c->n != c0->n || c->N != c0->N || c->divided != c0->divided || c->R != c0->R || c->coin_period != c0->coin_period)
            return fail(c, SW_EINVAL, "sw_split_link: context %d does not hold the same hashgraph, divided to the same point, as context 0", q);
        if (c->MCAP != c0->MCAP || c->NEARCAP != c0->NEARCAP || c->skip != c0->skip || c->gallop_after != c0->gallop_after || c->pipe != c0->pipe)
            return fail(c, SW_EINVAL, "sw_split_link: context %d was created under other tuning knobs than context 0", q);
    }
    SplitGroup* g = new SplitGroup();
    g->parts = parts;
    for (int w = 0; w < 2; ++w) for (int q = 0; q < SW_MAX_PARTS; ++q) g->rec[w][q].store(0);
    for (int q = 0; q < parts; ++q) {
        sw_ctx* c = ctxs[q];
        g->ctx[q] = c;
        if (hipSetDevice(c->device) != hipSuccess) { split_dissolve(g); return fail(c0, SW_EIO, "hipSetDevice(%d) failed", c->device); }
        for (int o = 0; o < parts; ++o)
            if (ctxs[o]->device != c->device) {
                int can = 0;
                (void)hipDeviceCanAccessPeer(&can, c->device, ctxs[o]->device);
                if (!can) { split_dissolve(g); return fail(c0, SW_ENOTSUP, "sw_split_link: device %d cannot map the memory of device %d", c->device, ctxs[o]->device); }
                const hipError_t e = hipDeviceEnablePeerAccess(ctxs[o]->device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); split_dissolve(g); return fail(c0, SW_EIO, "hipDeviceEnablePeerAccess failed: %s", hipGetErrorString(e)); }
                (void)hipGetLastError();
            }
        for (int w = 0; w < 2; ++w)
            for (auto& e : g->ev[w][q])
                if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { split_dissolve(g); return fail(c0, SW_EIO, "hipEventCreate failed"); }
    }
    for (int q = 0; q < parts; ++q) {
        sw_ctx* c = ctxs[q];
        // the split kernels exist for the one-wave-per-slot tally (the default beyond 256 members)
        c->split_saved[0] = c->tally_impl; c->split_saved[1] = c->tally_auto; c->split_saved[2] = c->K; c->split_saved[3] = c->K_auto;
        c->tally_impl = 1; c->tally_auto = false; c->K = c->K_flat; c->K_auto = false;
        c->split_part = q;
        c->split_iter = 0;
        c->split_failed = false;
        c->split = g;
    }
    return SW_OK;
}

int sw_split_unlink(sw_ctx* c) {
    if (!c) return SW_EINVAL;
    if (!c->split) return SW_OK;
    split_dissolve(c->split);
    return SW_OK;
}

int sw_find_order(sw_ctx* c, const int32_t* rounds, int n_rounds, int32_t* out_events, int64_t cap, int64_t* n_out) {
    if (!c) return SW_EINVAL;
    if (n_out) *n_out = 0;
    if (n_rounds < 0 || (n_rounds > 0 && !rounds)) return fail(c, SW_EINVAL, "find_order: NULL rounds");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int32_t> rs(rounds, rounds + n_rounds);
    if (c->exact) return exact_order(c, rs, out_events, cap, n_out);
    switch (c->nw) {
        case 1: return do_find_order<1>(c, rs, out_events, cap, n_out);
        case 2: return do_find_order<2>(c, rs, out_events, cap, n_out);
        case 4: return do_find_order<4>(c, rs, out_events, cap, n_out);
        case 8: return do_find_order<8>(c, rs, out_events, cap, n_out);
        case 16: return do_find_order<16>(c, rs, out_events, cap, n_out);
    }
    return fail(c, SW_EINVAL, "unsupported member count");
}

// ---- getters ----
static int get_i32(sw_ctx* c, const int32_t* src, int64_t first, int64_t K, int32_t* out, int64_t limit) {
    if (!c || !out) return SW_EINVAL;
    if (first < 0 || K < 0 || first + K > limit) return fail(c, SW_ERANGE, "range [%lld, %lld) outside [0, %lld)", (long long)first, (long long)(first + K), (long long)limit);
    if (!K) return SW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, src + first, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

int sw_get_height(sw_ctx* c, int64_t first, int64_t K, int32_t* out) {
    if (!c || !out) return SW_EINVAL;
    if (first < 0 || K < 0 || first + K > c->N) return fail(c, SW_ERANGE, "range outside the stored hashgraph");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ensure_dag_h(c));
    std::copy(c->ht.begin() + first, c->ht.begin() + first + K, out);
    return SW_OK;
}

int sw_get_round(sw_ctx* c, int64_t first, int64_t K, int32_t* out) {
    return get_i32(c, c ? c->d_round.p : nullptr, first, K, out, c ? c->divided : 0);
}

int sw_get_can_see(sw_ctx* c, int64_t first, int64_t K, int32_t* out) {
    if (!c || !out) return SW_EINVAL;
    if (first < 0 || K < 0 || first + K > c->divided) return fail(c, SW_ERANGE, "range outside the divided events");
    if (!K) return SW_OK;
    if (first < c->first_resident) return fail(c, SW_ERANGE, "can_see rows below event %lld were evicted (windowed mode)", (long long)c->first_resident);
    HIPCHK(c, hipSetDevice(c->device));
    const int np = c->npad, n = c->n;
    const int64_t chunk = std::max<int64_t>(1, (64ll << 20) / (np * 4));
    std::vector<int32_t> tmp((size_t)std::min(chunk, K) * np);
    for (int64_t a = 0; a < K; a += chunk) {
        const int64_t m = std::min(chunk, K - a);
        HIPCHK(c, hipMemcpyAsync(tmp.data(), c->d_L.p + (size_t)(first + a) * np, (size_t)m * np * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int64_t i = 0; i < m; ++i) memcpy(out + (size_t)(a + i) * n, tmp.data() + (size_t)i * np, n * sizeof(int32_t));
    }
    return SW_OK;
}

int sw_max_round(sw_ctx* c, int* out) {
    if (!c || !out) return SW_EINVAL;
    *out = c->R - 1;
    return SW_OK;
}

int sw_get_witnesses(sw_ctx* c, int r0, int r1, int32_t* out) {
    return get_round_rows<int32_t>(c, c ? c->d_wit.p : nullptr, r0, r1, out, -1);
}

int sw_get_famous(sw_ctx* c, int r0, int r1, int8_t* out) {
    return get_round_rows<signed char>(c, c ? c->d_fam.p : nullptr, r0, r1, (signed char*)out, (signed char)-1);
}

// Node.famous keyed by EVENT (swirld.py:64): -1 undecided / not a witness, 0 / 1.  On the fast path a
// member has one witness per round for good, so this is the slot table scattered to the events; on the
// exact path a fork sibling may have replaced a decided witness, whose entry the reference keeps.
int sw_get_famous_events(sw_ctx* c, int64_t first, int64_t K, int8_t* out) {
    if (!c || !out) return SW_EINVAL;
    if (first < 0 || K < 0 || first + K > c->N) return fail(c, SW_ERANGE, "range outside the stored events");
    if (!K) return SW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->exact) {
        HIPCHK(c, hipMemcpyAsync(out, c->ex.fam_ev.p + first, (size_t)K, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return SW_OK;
    }
    memset(out, 0xff, (size_t)K);
    const int np = c->npad, R = c->R;
    if (R <= 0) return SW_OK;
    std::vector<int32_t> wit((size_t)R * np);
    std::vector<signed char> fam((size_t)R * np);
    HIPCHK(c, hipMemcpyAsync(wit.data(), c->d_wit.p, wit.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(fam.data(), c->d_fam.p, fam.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < wit.size(); ++i)
        if (wit[i] >= first && wit[i] < first + K) out[wit[i] - first] = fam[i];
    return SW_OK;
}

int sw_get_consensus(sw_ctx* c, int r0, int r1, uint8_t* out) {
    if (!c || !out) return SW_EINVAL;
    if (r0 < 0 || r1 < r0) return fail(c, SW_ERANGE, "bad round range");
    for (int r = r0; r < r1; ++r) out[r - r0] = (r < c->R && r < (int)c->cons_h.size()) ? c->cons_h[r] : 0;
    return SW_OK;
}

int sw_get_sees_mask(sw_ctx* c, int64_t first, int64_t K, uint64_t* out) {
    if (!c || !out) return SW_EINVAL;
    if (first < 0 || K < 0 || first + K > c->divided) return fail(c, SW_ERANGE, "range outside the divided events");
    if (!K) return SW_OK;
    if (c->exact) return fail(c, SW_ENOTSUP, "sw_get_sees_mask is not available on the exact (forked-hashgraph) path");
    HIPCHK(c, hipSetDevice(c->device));
    const int nw = c->nw, nwo = (c->n + 63) / 64;
    std::vector<u64> tmp((size_t)K * nw);
    HIPCHK(c, hipMemcpyAsync(tmp.data(), c->d_S.p + (size_t)first * nw, tmp.size() * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < K; ++i)
        for (int j = 0; j < nwo; ++j) out[(size_t)i * nwo + j] = tmp[(size_t)i * nw + j];
    return SW_OK;
}

// Node.votes[voter][candidate] (swirld.py:60-61, 256-272).  The elections keep votes as per-round
// member bitmasks, so an entry is recomputed on demand — with the reference's FULL semantics, call
// schedule included:
//  * the VALUE of votes[y][x] is a function of the hashgraph alone (y's strongly-seen set, the
//    votes of those witnesses, y's coin bit): the election of x is replayed level by level up to
//    y's round, every witness voting;
//  * whether the ENTRY exists depends on the decide_fame() calls (Appendix A Q8/Q9): y recorded a
//    vote on x iff in some call both were registered witnesses, y was a voter (round(y) > max_c of
//    that call), round(x) was not yet in `consensus`, and x was still undecided when y's turn came
//    — i.e. the call precedes the one that decided x, or is that call and y comes before the
//    deciding voter in voter order (rounds ascending, registration order inside a round); the
//    deciding voter itself stores nothing.  Per call the context keeps (max_c, rounds, events
//    divided), per round the call that put it into `consensus`, per witness the call and the voter
//    that decided it (written by the election kernels).
int sw_get_vote(sw_ctx* c, int rv, int mv, int rc, int mc, int8_t* out) {
    if (!c || !out) return SW_EINVAL;
    *out = -1;
    if (c->exact) return fail(c, SW_ENOTSUP, "sw_get_vote is not available on the exact (forked-hashgraph) path");
    if (c->votes_partial) return fail(c, SW_ENOTSUP, "sw_get_vote is not available after sw_commit_fame (the deciding voters of other parts' witnesses are not recorded)");
    const int np = c->npad, nw = c->nw, n = c->n;
    if (rc < 0 || rv >= c->R || mv < 0 || mv >= n || mc < 0 || mc >= n) return fail(c, SW_ERANGE, "witness slot outside the table");
    if (rv <= rc) return SW_OK;
    if (rv >= c->Sw_rows || c->sw_dirty_from <= rv) return fail(c, SW_EINVAL, "votes are available after decide_fame has seen these rounds");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ensure_sig_h(c));
    const int D = rv - rc;
    std::vector<int32_t> wit((size_t)(D + 1) * np);
    std::vector<u64> Sw((size_t)D * np * nw);
    int32_t dec[2] = {-1, -1};
    HIPCHK(c, hipMemcpyAsync(wit.data(), c->d_wit.p + (size_t)rc * np, wit.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(Sw.data(), c->d_Sw.p + (size_t)(rc + 1) * np * nw, Sw.size() * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&dec[0], c->d_dec_call.p + (size_t)rc * np + mc, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&dec[1], c->d_dec_by.p + (size_t)rc * np + mc, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int32_t x = wit[mc], y = wit[(size_t)D * np + mv];
    if (x < 0 || y < 0) return SW_OK;  // not witnesses: no entry
    // ---- does the entry exist?  calls c0 .. c1 in which y evaluated x
    const int ncalls = (int)c->fame_calls.size();
    const int64_t born = (int64_t)std::max(x, y) + 1;  // both are divided (hence registered) once `divided` >= born
    int c0 = 0;
    while (c0 < ncalls && c->fame_calls[c0].divided < born) ++c0;
    int c1 = ncalls - 1;
    while (c1 >= c0 && c->fame_calls[c1].max_c + 1 > rv) --c1;          // y must be a voter: round(y) >= max_c + 1
    if (c->cons_call[rc] >= 0) c1 = std::min(c1, c->cons_call[rc]);     // rounds in `consensus` are skipped (swirld.py:233)
    if (dec[0] >= 0) {
        int32_t rz = -1;
        HIPCHK(c, hipMemcpy(&rz, c->d_round.p + dec[1], sizeof rz, hipMemcpyDeviceToHost));
        const bool before_decider = y != dec[1] && (rv < rz || (rv == rz && y < dec[1]));
        c1 = std::min(c1, before_decider ? dec[0] : dec[0] - 1);
    }
    if (c1 < c0) return SW_OK;
    // ---- its value: the election of x replayed up to y's level
    std::vector<char> V(n, 0), Vn(n, 0);
    auto sw_bit = [&](int d, int voter, int member) {  // d = 1..D
        return (int)((Sw[((size_t)(d - 1) * np + voter) * nw + (member >> 6)] >> (member & 63)) & 1ull);
    };
    for (int v = 0; v < n; ++v) V[v] = wit[(size_t)1 * np + v] >= 0 ? (char)sw_bit(1, v, mc) : 0;  // x in s (swirld.py:258)
    if (D == 1) { *out = V[mv]; return SW_OK; }
    const uint64_t tot2 = 2ull * c->tot;
    for (int d = 2; d <= D; ++d) {
        const int32_t* wrow = wit.data() + (size_t)d * np;
        const bool coin_round = (d % c->coin_period) == 0;
        for (int v = 0; v < n; ++v) {
            Vn[v] = 0;
            if (wrow[v] < 0) continue;
            uint64_t yes = 0, all = 0;
            for (int m = 0; m < n; ++m)
                if (sw_bit(d, v, m)) { all += c->stake_h[m]; if (V[m]) yes += c->stake_h[m]; }
            const uint64_t no = all - yes;
            const int vote = !(no > yes);            // majority(): tie -> True (swirld.py:24-27)
            const uint64_t tt = vote ? yes : no;
            Vn[v] = (char)vote;
            if (coin_round && !(3 * tt > tot2)) Vn[v] = (char)(c->sig_h[(size_t)wrow[v] * 64] >> 7);  // swirld.py:272
        }
        if (d == D) { *out = Vn[mv]; return SW_OK; }
        V.swap(Vn);
    }
    return SW_OK;
}

// ---- Node.votes in bulk (votes.hip.h): the table of sw_get_vote's answers for whole voter rounds ---------------------------
}  // extern "C"
namespace {

struct VotesCall {
    int rv0 = 0, rv1 = 0, rc0 = 0, nrv = 0;   // voter rounds [rv0, rv1) (rv0 >= 1), candidate rounds from rc0 on
    long long pairs = 0;                      // (voter round, candidate round) pairs the call schedule allows
    vts::Tables t{};
    vts::Sched s{};
    vts::Range g{};
    vts::Work w{};
};

// sw_get_vote's preconditions for the whole range; *empty: nothing to export
int votes_pre(sw_ctx* c, int rv0, int rv1, const char* what, bool* empty) {
    *empty = true;
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (c->exact) return fail(c, SW_ENOTSUP, "%s is not available on the exact (forked-hashgraph) path", what);
    if (c->votes_partial) return fail(c, SW_ENOTSUP, "%s is not available after sw_commit_fame (the deciding voters of other parts' witnesses are not recorded)", what);
    if (rv0 >= rv1) return SW_OK;
    if (rv0 < 0 || rv1 > c->R) return fail(c, SW_ERANGE, "%s: voter rounds [%d, %d) outside the table of %d rounds", what, rv0, rv1, c->R);
    const int seen = c->fame_calls.empty() ? 0 : c->fame_calls.back().R;
    if (rv1 > seen || rv1 > c->Sw_rows || c->sw_dirty_from < rv1)
        return fail(c, SW_EINVAL, "%s: votes are available after decide_fame has seen these rounds (%d so far)", what, seen);
    *empty = rv1 <= 1;
    return SW_OK;
}

// the call schedule on the device, uploaded when decide_fame has been called since
int votes_schedule(sw_ctx* c, VotesCall& v) {
    auto& vs = c->votes;
    const int ncalls = (int)c->fame_calls.size(), R = ncalls ? c->fame_calls.back().R : 0;
    Carve cv;
    const size_t o_maxc = cv.take((size_t)ncalls * 4), o_cons = cv.take((size_t)R * 4), o_div = cv.take((size_t)ncalls * 8);
    if (vs.sched_calls != ncalls) {
        CHK(dgrow(c, vs.d_sched, cv.off + 256, 0));
        vs.sched_stage.assign(cv.off, 0);
        int32_t* maxc = (int32_t*)(vs.sched_stage.data() + o_maxc);
        int32_t* cons = (int32_t*)(vs.sched_stage.data() + o_cons);
        long long* div = (long long*)(vs.sched_stage.data() + o_div);
        for (int i = 0; i < ncalls; ++i) { maxc[i] = c->fame_calls[i].max_c; div[i] = c->fame_calls[i].divided; }
        for (int r = 0; r < R; ++r) cons[r] = c->cons_call[r];
        HIPCHK(c, hipMemcpyAsync(vs.d_sched.p, vs.sched_stage.data(), cv.off, hipMemcpyHostToDevice, c->stream));
        vs.sched_calls = ncalls;
    }
    v.s.call_maxc = (const int*)(vs.d_sched.p + o_maxc);
    v.s.cons_call = (const int*)(vs.d_sched.p + o_cons);
    v.s.call_div = (const long long*)(vs.d_sched.p + o_div);
    v.s.ncalls = ncalls;
    return SW_OK;
}

// Per voter round what the host knows (vts::plan_rounds: the calls that bound its entries, the lowest candidate round they
// leave open), uploaded; the context's tables; and the call's scratch carved out of one allocation.
int votes_plan(sw_ctx* c, VotesCall& v, int rv0, int rv1) {
    auto& vs = c->votes;
    const auto& calls = c->fame_calls;
    const int ncalls = (int)calls.size(), np = c->npad;
    v.rv0 = std::max(rv0, 1);
    v.rv1 = rv1;
    v.nrv = v.rv1 - v.rv0;
    Carve cv;
    const size_t o_lo = cv.take((size_t)v.nrv * 4), o_c1v = cv.take((size_t)v.nrv * 4), o_cf = cv.take((size_t)v.nrv * 4),
                 o_q = cv.take((size_t)(v.nrv + 1) * 8);
    vs.plan_stage.assign(cv.off, 0);
    int32_t* lo = (int32_t*)(vs.plan_stage.data() + o_lo);
    int32_t* c1v = (int32_t*)(vs.plan_stage.data() + o_c1v);
    int32_t* cf = (int32_t*)(vs.plan_stage.data() + o_cf);
    long long* q = (long long*)(vs.plan_stage.data() + o_q);
    std::vector<vts::CallRec> recs(ncalls);
    for (int i = 0; i < ncalls; ++i) recs[i] = vts::CallRec{calls[i].max_c, calls[i].R, (long long)calls[i].divided};
    v.rc0 = vts::plan_rounds(recs.data(), ncalls, c->cons_call.data(), v.rv0, v.rv1, lo, c1v, cf, q);
    v.pairs = q[v.nrv];
    CHK(dgrow(c, vs.d_plan, cv.off + 256, 0));
    HIPCHK(c, hipMemcpyAsync(vs.d_plan.p, vs.plan_stage.data(), cv.off, hipMemcpyHostToDevice, c->stream));
    v.g = vts::Range{v.rv0, v.rv1, v.rc0, (const int*)(vs.d_plan.p + o_lo), (const int*)(vs.d_plan.p + o_c1v), (const int*)(vs.d_plan.p + o_cf),
                     (const long long*)(vs.d_plan.p + o_q)};
    v.t = vts::Tables{c->d_wit.p, (const vts::u64*)c->d_Sw.p, c->d_coin.p, c->d_stake.p, c->d_dec_call.p, c->d_dec_by.p, c->d_round.p, (long long)c->N,
                      c->n, np, c->nw, (c->n + 63) / 64, c->coin_period, 2u * c->tot};
    // scratch
    const size_t NR = (size_t)(v.rv1 - v.rc0), V = (size_t)v.nrv * np;
    Carve wc;
    const size_t o_born = wc.take(NR * np * 4), o_rz = wc.take(NR * np * 4), o_order = wc.take(NR * np * 4), o_rank = wc.take(NR * np * 4),
                 o_nwit = wc.take(NR * 4), o_hr = wc.take(NR * 4), o_hc = wc.take(NR * 4), o_lod = wc.take((size_t)v.nrv * 4),
                 o_mask = wc.take((size_t)v.pairs * c->nw * 8), o_vrows = wc.take(V * 4), o_vent = wc.take(V * 8), o_voff = wc.take(V * 8);
    CHK(dgrow(c, vs.d_work, wc.off + 256, 0));
    if (!vs.d_cnt.p) {
        CHK(dgrow(c, vs.d_cnt, vts::C_WORDS, 0));
        HIPCHK(c, hipMemsetAsync(vs.d_cnt.p, 0, vts::C_WORDS * sizeof(unsigned long long), c->stream));
    }
    unsigned char* B = vs.d_work.p;
    v.w = vts::Work{(int*)(B + o_born), (int*)(B + o_rz), (int*)(B + o_order), (int*)(B + o_rank), (int*)(B + o_nwit), (int*)(B + o_hr), (int*)(B + o_hc),
                    (int*)(B + o_lod), (vts::u64*)(B + o_mask), (int*)(B + o_vrows), (long long*)(B + o_vent), (long long*)(B + o_voff), vs.d_cnt.p};
    if (v.pairs) HIPCHK(c, hipMemsetAsync(B + o_mask, 0, (size_t)v.pairs * c->nw * 8, c->stream));
    return SW_OK;
}

// existence: rows per voter, their scan, and the read-back of the two counts — the call's one synchronisation
int votes_count(sw_ctx* c, VotesCall& v, int64_t* n_rows, int64_t* n_entries) {
    const int np = c->npad;
    const long long V = (long long)v.nrv * np;
    const unsigned vblocks = (unsigned)((V + vts::COUNT_THREADS - 1) / vts::COUNT_THREADS);
    hipLaunchKernelGGL(vts::k_votes_prep, dim3((unsigned)(v.rv1 - v.rc0)), dim3(np), 0, c->stream, v.t, v.s, v.g, v.w);
    hipLaunchKernelGGL(vts::k_votes_lo, dim3((unsigned)((v.nrv + vts::COUNT_THREADS - 1) / vts::COUNT_THREADS)), dim3(vts::COUNT_THREADS), 0, c->stream, v.g, v.w);
    hipLaunchKernelGGL(vts::k_votes_rows<false>, dim3(vblocks), dim3(vts::COUNT_THREADS), 0, c->stream, v.t, v.s, v.g, v.w, vts::Out{});
    hipLaunchKernelGGL(vts::k_votes_scan, dim3(1), dim3(vts::SCAN_THREADS), 0, c->stream, v.w, V);
    c->ctr.kernel_launches += 4;
    HIPCHK(c, hipGetLastError());
    unsigned long long cnt[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(cnt, c->votes.d_cnt.p, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_rows = (int64_t)cnt[vts::C_ROWS];
    *n_entries = (int64_t)cnt[vts::C_ENTRIES];
    return SW_OK;
}

// the rows and their exists words, then the elections replayed for the values
int votes_write(sw_ctx* c, VotesCall& v, const vts::Out& out) {
    const int np = c->npad;
    const long long V = (long long)v.nrv * np;
    const unsigned vblocks = (unsigned)((V + vts::COUNT_THREADS - 1) / vts::COUNT_THREADS);
    hipLaunchKernelGGL(vts::k_votes_rows<true>, dim3(vblocks), dim3(vts::COUNT_THREADS), 0, c->stream, v.t, v.s, v.g, v.w, out);
    const unsigned blocks = (unsigned)(v.rv1 - 1 - v.rc0) * (unsigned)v.t.nwo;   // candidate rounds rc0 .. rv1 - 2
    const size_t lds = ((size_t)64 * c->nw + np) * 8 + (size_t)np * 4 + 16;
    if (blocks) {
        if (c->unit_stake) hipLaunchKernelGGL(vts::k_votes_values<true>, dim3(blocks), dim3(np), lds, c->stream, v.t, v.g, v.w, out);
        else hipLaunchKernelGGL(vts::k_votes_values<false>, dim3(blocks), dim3(np), lds, c->stream, v.t, v.g, v.w, out);
    }
    c->ctr.kernel_launches += 2;
    HIPCHK(c, hipGetLastError());
    return SW_OK;
}

void votes_account(sw_ctx* c, int64_t rows, int64_t entries) {
    c->votes.calls++;
    c->votes.rows += rows;
    c->votes.entries += entries;
}

}  // namespace
extern "C" {

int sw_export_votes_device(sw_ctx* c, int rv0, int rv1, int64_t cap_rows, int32_t* d_row_voter, int32_t* d_row_cand_round, uint64_t* d_exists,
                           uint64_t* d_value, int64_t* n_rows, int64_t* n_entries, void* user_stream) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_export_votes_device";
    if (!n_rows || !n_entries) return fail(c, SW_EINVAL, "%s: n_rows or n_entries is NULL", what);
    *n_rows = *n_entries = 0;
    bool empty = true;
    CHK(votes_pre(c, rv0, rv1, what, &empty));
    if (cap_rows < 0 || (cap_rows > 0 && (!d_row_voter || !d_row_cand_round || !d_exists || !d_value)))
        return fail(c, SW_EINVAL, "%s: NULL output arrays (capacity %lld)", what, (long long)cap_rows);
    // (with capacity 0 the rows are empty and skipped: the alignment of whatever was passed is asked for all the same)
    if (cap_rows == 0 && (((uintptr_t)d_exists | (uintptr_t)d_value) & 15)) return misaligned(c, what, 16);
    const size_t k = (size_t)cap_rows, nwo = (size_t)(c->n + 63) / 64;
    CHK(device_args(c, what, {{d_exists, k * nwo * 8, 16}, {d_value, k * nwo * 8, 16}, {d_row_voter, k * 4, 4}, {d_row_cand_round, k * 4, 4}}));
    if (empty) return SW_OK;
    const bool prof = c->profiling;
    auto t0 = std::chrono::steady_clock::now();
    UserStream bracket;   // earlier readers of the output arrays
    CHK(bracket.join(c, (hipStream_t)user_stream));
    VotesCall v;
    CHK(votes_schedule(c, v));
    CHK(votes_plan(c, v, rv0, rv1));
    CHK(votes_count(c, v, n_rows, n_entries));
    c->votes.ms[0] = prof ? ms_since(t0) : 0;
    c->votes.ms[1] = 0;
    if (*n_rows > cap_rows) return fail(c, SW_ERANGE, "%s: %lld rows to export, capacity %lld (nothing written)", what, (long long)*n_rows, (long long)cap_rows);
    t0 = std::chrono::steady_clock::now();
    if (*n_rows) CHK(votes_write(c, v, vts::Out{d_row_voter, d_row_cand_round, (vts::u64*)d_exists, (vts::u64*)d_value}));
    CHK(bracket.leave());
    if (prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->votes.ms[1] = ms_since(t0); }
    votes_account(c, *n_rows, *n_entries);
    return SW_OK;
}

int sw_export_votes(sw_ctx* c, int rv0, int rv1, int64_t cap_rows, int32_t* row_voter, int32_t* row_cand_round, uint64_t* exists, uint64_t* value,
                    int64_t* n_rows, int64_t* n_entries) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_export_votes";
    if (!n_rows || !n_entries) return fail(c, SW_EINVAL, "%s: n_rows or n_entries is NULL", what);
    *n_rows = *n_entries = 0;
    bool empty = true;
    CHK(votes_pre(c, rv0, rv1, what, &empty));
    if (cap_rows < 0 || (cap_rows > 0 && (!row_voter || !row_cand_round || !exists || !value)))
        return fail(c, SW_EINVAL, "%s: NULL output arrays (capacity %lld)", what, (long long)cap_rows);
    if (empty) return SW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const bool prof = c->profiling;
    auto t0 = std::chrono::steady_clock::now();
    VotesCall v;
    CHK(votes_schedule(c, v));
    CHK(votes_plan(c, v, rv0, rv1));
    CHK(votes_count(c, v, n_rows, n_entries));
    c->votes.ms[0] = prof ? ms_since(t0) : 0;
    c->votes.ms[1] = 0;
    if (*n_rows > cap_rows) return fail(c, SW_ERANGE, "%s: %lld rows to export, capacity %lld (nothing written)", what, (long long)*n_rows, (long long)cap_rows);
    t0 = std::chrono::steady_clock::now();
    if (*n_rows) {
        const size_t k = (size_t)*n_rows, nwo = (size_t)(c->n + 63) / 64;
        Stage st;
        const size_t o_ex = st.out(exists, k * nwo * 8), o_val = st.out(value, k * nwo * 8), o_rv = st.out(row_voter, k * 4), o_rc = st.out(row_cand_round, k * 4);
        unsigned char* B = nullptr;
        CHK(stage_up(c, c->votes.d_out, st, &B));
        CHK(votes_write(c, v, vts::Out{(int*)(B + o_rv), (int*)(B + o_rc), (vts::u64*)(B + o_ex), (vts::u64*)(B + o_val)}));
        CHK(stage_down(c, st, B));
    }
    if (prof) c->votes.ms[1] = ms_since(t0);
    votes_account(c, *n_rows, *n_entries);
    return SW_OK;
}

int sw_get_votes_stats(sw_ctx* c, int64_t* calls, int64_t* rows, int64_t* entries, int64_t* levels, double* phase_ms) {
    if (!c) return SW_EINVAL;
    if (calls) *calls = c->votes.calls;
    if (rows) *rows = c->votes.rows;
    if (entries) *entries = c->votes.entries;
    if (phase_ms) for (int i = 0; i < 2; ++i) phase_ms[i] = c->votes.ms[i];
    if (levels) {
        *levels = 0;
        if (c->votes.d_cnt.p) {
            unsigned long long lv = 0;
            HIPCHK(c, hipSetDevice(c->device));
            HIPCHK(c, hipMemcpyAsync(&lv, c->votes.d_cnt.p + vts::C_LEVELS, sizeof lv, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            *levels = (int64_t)lv;
        }
    }
    return SW_OK;
}

// ---- the history of the exact path (exact_history.hip.h) ---------------------------------------------------
}  // extern "C"
namespace {

// The votes of the fast path — the table of sw_export_votes_device over every voter round decide_fame has seen — as entries
// at the head of the (emptied) store, indexed.  The table's preconditions are the caller's business (votes_pre).
int history_table_import(sw_ctx* c, int seen) {
    auto& h = c->hist;
    h.count = 0;
    if (h.slots) HIPCHK(c, hipMemsetAsync(h.d_tab.p, 0xff, h.slots * sizeof(int32_t), c->stream));
    if (seen <= 1) return SW_OK;
    VotesCall v;
    CHK(votes_schedule(c, v));
    CHK(votes_plan(c, v, 0, seen));
    int64_t rows = 0, entries = 0;
    CHK(votes_count(c, v, &rows, &entries));
    if (!rows) return SW_OK;
    if (entries > h.ceiling) { history_votes_lost(c, "the vote store reached its ceiling (SW_VOTE_STORE_MAX)"); return SW_OK; }
    const size_t k = (size_t)rows, nwo = (size_t)(c->n + 63) / 64;
    Carve cv;
    const size_t o_ex = cv.take(k * nwo * 8), o_val = cv.take(k * nwo * 8), o_rv = cv.take(k * 4), o_rc = cv.take(k * 4);
    CHK(dgrow(c, c->votes.d_out, cv.off + 256, 0));
    unsigned char* B = c->votes.d_out.p;
    CHK(votes_write(c, v, vts::Out{(int*)(B + o_rv), (int*)(B + o_rc), (vts::u64*)(B + o_ex), (vts::u64*)(B + o_val)}));
    CHK(history_store_reserve(c, entries));
    CHK(dgrow(c, h.d_off, k + 1, 0));
    const unsigned blocks = (unsigned)((rows + xh::THREADS - 1) / xh::THREADS);
    const xh::TableIn in{(const int*)(B + o_rv), (const int*)(B + o_rc), (const xh::u64*)(B + o_ex), (const xh::u64*)(B + o_val), (int)nwo, c->d_wit.p, c->npad, c->n};
    hipLaunchKernelGGL(xh::k_votes_row_counts, dim3(blocks), dim3(xh::THREADS), 0, c->stream, (long long)rows, in.exists, (int)nwo, h.d_off.p);
    hipLaunchKernelGGL(xh::k_votes_offsets, dim3(1), dim3(xh::SCAN_THREADS), 0, c->stream, (long long)rows, h.d_off.p);
    hipLaunchKernelGGL(xh::k_votes_expand, dim3(blocks), dim3(xh::THREADS), 0, c->stream, (long long)rows, in, (const long long*)h.d_off.p, 0ll, history_store(c));
    hipLaunchKernelGGL(xh::k_votes_reindex, dim3((unsigned)((entries + xh::THREADS - 1) / xh::THREADS)), dim3(xh::THREADS), 0, c->stream, history_store(c), (long long)entries);
    c->ctr.kernel_launches += 4;
    HIPCHK(c, hipGetLastError());
    h.count = entries;
    return SW_OK;
}

// The end of exact_enter with history on.  Per-event tables: every event outside the fast path's ordered chain prefixes gets
// the "not ordered" defaults, so that from now on the tables answer as they are.  Votes: taken over from the table when it is
// current — nothing divided since the last decide_fame call, no partitioned commit; unavailable otherwise.
int history_enter(sw_ctx* c) {
    auto& h = c->hist;
    CHK(consensus_reserve(c, (size_t)c->cons.tx_len));
    CHK(dgrow(c, c->cons.d_ordpos, c->npad, 0));
    if (c->N) {
        HIPCHK(c, hipMemcpyAsync(c->cons.d_ordpos.p, c->ord_pos.data(), (size_t)c->n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(xh::k_history_normalise, dim3((unsigned)((c->N + xh::THREADS - 1) / xh::THREADS)), dim3(xh::THREADS), 0, c->stream, (long long)c->N,
                           (const int*)c->d_seq.p, (const int*)c->d_cr.p, (const int*)c->cons.d_ordpos.p, c->cons.d_rr.p, (xh::u64*)c->cons.d_cts.p);
        c->ctr.kernel_launches++;
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (ord_pos is pageable memory)
    }
    h.votes_ok = true;
    h.why = "";
    h.count = 0;
    const int seen = c->fame_calls.empty() ? 0 : c->fame_calls.back().R;
    if (c->votes_partial) history_votes_lost(c, "the context forked after sw_commit_fame (the fast path had no votes to hand over)");
    else if (!c->fame_calls.empty() && (c->fame_calls.back().divided != c->divided || seen > c->Sw_rows || c->sw_dirty_from < seen))
        history_votes_lost(c, "rounds were divided that decide_fame had not seen when the first fork arrived (the fast path's voter masks were not current)");
    else {
        CHK(history_table_import(c, seen));
        h.imported += h.count;
    }
    h.table_calls = h.table_divided = -1;
    CHK(exact_set_hdr(c, swx::H_VCNT, h.count));
    return SW_OK;
}

// what the three readers of the store check, and — on a context that is still fork-free — the store filled from the table
int history_votes_pre(sw_ctx* c, const char* what) {
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (!c->hist.on) return fail(c, SW_ENOTSUP, "%s needs sw_set_exact_history(ctx, 1)", what);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->exact) {
        const int seen = c->fame_calls.empty() ? 0 : c->fame_calls.back().R;
        bool empty = true;
        CHK(votes_pre(c, 0, seen, what, &empty));
        // (the table is a function of the decide_fame calls so far: filled once per call schedule, not once per read; what the
        // fill found — the entries, or that they do not fit under the ceiling — stands until the schedule moves on)
        if (c->hist.table_calls != (int64_t)c->fame_calls.size() || c->hist.table_divided != c->divided) {
            c->hist.table_calls = c->hist.table_divided = -1;
            c->hist.votes_ok = true;
            c->hist.why = "";
            CHK(history_table_import(c, seen));
            c->hist.table_calls = (int64_t)c->fame_calls.size();
            c->hist.table_divided = c->divided;
        }
    }
    if (!c->hist.votes_ok) return fail(c, SW_ENOTSUP, "%s: the votes are unavailable until sw_rewind / sw_reset: %s", what, c->hist.why);
    return SW_OK;
}

}  // namespace
extern "C" {

int sw_set_exact_history(sw_ctx* c, int enable) {
    if (!c) return SW_EINVAL;
    if (enable != 0 && enable != 1) return fail(c, SW_EINVAL, "sw_set_exact_history: 0 (off) or 1 (on)");
    if (c->N) return fail(c, SW_EINVAL, "sw_set_exact_history: only before the first event is appended (%lld stored)", (long long)c->N);
    c->hist.on = enable != 0;
    return SW_OK;
}

int sw_get_exact_history(sw_ctx* c, int* enabled, int* votes_available) {
    if (!c) return SW_EINVAL;
    if (enabled) *enabled = c->hist.on ? 1 : 0;
    // fork-free: the table answers unless a partitioned commit left it incomplete, or its last fill (still current) found more
    // entries than the ceiling admits
    const bool filled = c->hist.table_calls == (int64_t)c->fame_calls.size() && c->hist.table_divided == c->divided;
    if (votes_available) *votes_available = c->hist.on && (!c->exact ? !c->votes_partial && !(filled && !c->hist.votes_ok) : c->hist.votes_ok) ? 1 : 0;
    return SW_OK;
}

int sw_get_votes_by_event(sw_ctx* c, int64_t K, const int32_t* voter, const int32_t* cand, int8_t* out) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_get_votes_by_event";
    if (K < 0 || (K > 0 && (!voter || !cand || !out))) return fail(c, SW_EINVAL, "%s: NULL arrays (K = %lld)", what, (long long)K);
    CHK(history_votes_pre(c, what));
    if (!K) return SW_OK;
    auto& h = c->hist;
    if (!h.count) { memset(out, 0xff, (size_t)K); return SW_OK; }
    CHK(dgrow(c, h.d_q, (size_t)2 * K, 0));
    CHK(dgrow(c, h.d_qout, (size_t)K, 0));
    HIPCHK(c, hipMemcpyAsync(h.d_q.p, voter, (size_t)K * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(h.d_q.p + K, cand, (size_t)K * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(xh::k_votes_lookup, dim3((unsigned)((K + xh::THREADS - 1) / xh::THREADS)), dim3(xh::THREADS), 0, c->stream, history_store(c), (long long)c->N,
                       (long long)K, (const int*)h.d_q.p, (const int*)(h.d_q.p + K), h.d_qout.p);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, h.d_qout.p, (size_t)K, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    h.lookups += K;
    return SW_OK;
}

static int vote_entries_range(sw_ctx* c, const char* what, int64_t first, int64_t cap, const void* a, const void* b, const void* v, int64_t* n_total) {
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (!n_total) return fail(c, SW_EINVAL, "%s: n_total is NULL", what);
    *n_total = 0;
    if (first < 0 || cap < 0 || (cap > 0 && (!a || !b || !v))) return fail(c, SW_EINVAL, "%s: NULL output arrays (capacity %lld) or a negative position", what, (long long)cap);
    return SW_OK;
}

int sw_export_vote_entries_device(sw_ctx* c, int64_t first, int64_t cap_entries, int32_t* d_voter, int32_t* d_cand, int8_t* d_value, int64_t* n_total,
                                  void* user_stream) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_export_vote_entries_device";
    int64_t k = 0;
    CHK(vote_entries_range(c, what, first, cap_entries, d_voter, d_cand, d_value, n_total));
    if (!c->hist.on) return fail(c, SW_ENOTSUP, "%s needs sw_set_exact_history(ctx, 1)", what);
    CHK(device_args(c, what, {{d_voter, (size_t)cap_entries * 4, 4}, {d_cand, (size_t)cap_entries * 4, 4}, {d_value, (size_t)cap_entries, 1}}));
    UserStream bracket;   // earlier readers of the output arrays
    CHK(bracket.join(c, (hipStream_t)user_stream));
    CHK(history_votes_pre(c, what));   // (fork-free: the table's count is the one synchronisation; exact: the host knows the count)
    auto& h = c->hist;
    *n_total = h.count;
    k = std::max<int64_t>(0, h.count - first);
    if (k > cap_entries) return fail(c, SW_ERANGE, "%s: %lld entries to export, capacity %lld (nothing written)", what, (long long)k, (long long)cap_entries);
    if (k) {
        HIPCHK(c, hipMemcpyAsync(d_voter, h.d_voter.p + first, (size_t)k * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_cand, h.d_cand.p + first, (size_t)k * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_value, h.d_value.p + first, (size_t)k, hipMemcpyDeviceToDevice, c->stream));
    }
    CHK(bracket.leave());
    h.exported += k;
    return SW_OK;
}

int sw_export_vote_entries(sw_ctx* c, int64_t first, int64_t cap_entries, int32_t* voter, int32_t* cand, int8_t* value, int64_t* n_total) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_export_vote_entries";
    int64_t k = 0;
    CHK(vote_entries_range(c, what, first, cap_entries, voter, cand, value, n_total));
    CHK(history_votes_pre(c, what));
    auto& h = c->hist;
    *n_total = h.count;
    k = std::max<int64_t>(0, h.count - first);
    if (k > cap_entries) return fail(c, SW_ERANGE, "%s: %lld entries to export, capacity %lld (nothing written)", what, (long long)k, (long long)cap_entries);
    if (k) {
        HIPCHK(c, hipMemcpyAsync(voter, h.d_voter.p + first, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(cand, h.d_cand.p + first, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(value, h.d_value.p + first, (size_t)k, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    h.exported += k;
    return SW_OK;
}

int sw_get_vote_store_stats(sw_ctx* c, int64_t* entries, int64_t* capacity, int64_t* bytes, int64_t* grows, int64_t* imported, int64_t* lookups,
                            int64_t* exported) {
    if (!c) return SW_EINVAL;
    if (!c->hist.on) return fail(c, SW_ENOTSUP, "sw_get_vote_store_stats needs sw_set_exact_history(ctx, 1)");
    const auto& h = c->hist;
    if (entries) *entries = h.count;
    if (capacity) *capacity = h.cap;
    if (bytes) *bytes = (int64_t)(h.d_voter.cap * 4 + h.d_cand.cap * 4 + h.d_value.cap + h.d_tab.cap * 4);
    if (grows) *grows = h.grows;
    if (imported) *imported = h.imported;
    if (lookups) *lookups = h.lookups;
    if (exported) *exported = h.exported;
    return SW_OK;
}

int sw_get_known_heights(sw_ctx* c, int64_t head_event, int32_t* out) {
    if (!c || !out) return SW_EINVAL;
    if (head_event < c->first_resident || head_event >= c->divided) return fail(c, SW_ERANGE, "head %lld is not a divided, resident event", (long long)head_event);
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ensure_dag_h(c));  // heights on the device
    const int np = c->npad;
    CHK(dgrow(c, c->d_q, (size_t)3 * np, 0));
    hipLaunchKernelGGL(k_known_heights, dim3(1), dim3(np), 0, c->stream, (const int*)c->d_L.p, (const int*)c->d_ht.p, (int)head_event, np, c->d_q.p);
    c->ctr.kernel_launches++;
    std::vector<int32_t> tmp(np);
    HIPCHK(c, hipMemcpyAsync(tmp.data(), c->d_q.p, np * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::copy(tmp.begin(), tmp.begin() + c->n, out);
    return SW_OK;
}

int sw_sync_diff(sw_ctx* c, int64_t head_event, const int32_t* known_height, int32_t* pos_first, int32_t* pos_end, int64_t* n_events) {
    if (!c || !known_height || !pos_first || !pos_end) return SW_EINVAL;
    if (c->exact) return fail(c, SW_ENOTSUP, "sw_sync_diff is not available on the exact (forked-hashgraph) path");
    if (head_event < c->first_resident || head_event >= c->divided) return fail(c, SW_ERANGE, "head %lld is not a divided, resident event", (long long)head_event);
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ensure_dag_h(c));
    const int np = c->npad, n = c->n;
    CHK(dgrow(c, c->d_q, (size_t)3 * np, 0));
    std::vector<int32_t> kn(np, -1), res((size_t)2 * np);
    std::copy(known_height, known_height + n, kn.begin());
    HIPCHK(c, hipMemcpyAsync(c->d_q.p, kn.data(), np * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_sync_diff, dim3(1), dim3(np), 0, c->stream, (const int*)c->d_L.p, (const int*)c->d_ht.p, (const int*)c->d_seq.p,
                       (const int*)c->d_cr.p, (const int*)c->d_chain_start.p, (const int*)c->d_chain_ev.p, (const int*)c->d_q.p,
                       (int)head_event, np, c->d_q.p + np, c->d_q.p + 2 * np);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipMemcpyAsync(res.data(), c->d_q.p + np, (size_t)2 * np * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int64_t tot = 0;
    for (int m = 0; m < n; ++m) {
        pos_first[m] = res[m];
        pos_end[m] = res[(size_t)np + m];
        tot += pos_end[m] - pos_first[m];
    }
    if (n_events) *n_events = tot;
    return SW_OK;
}

int sw_get_chain_events(sw_ctx* c, int member, int32_t p0, int32_t p1, int32_t* out) {
    if (!c || !out) return SW_EINVAL;
    if (c->exact) return fail(c, SW_ENOTSUP, "sw_get_chain_events is not available on the exact (forked-hashgraph) path");
    if (member < 0 || member >= c->n || p0 < 0 || p1 < p0 || p1 > c->nev[member]) return fail(c, SW_ERANGE, "chain positions [%d, %d) of member %d", p0, p1, member);
    if (p1 == p0) return SW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->d_chain_ev.p + c->chain_start_h[member] + p0, (size_t)(p1 - p0) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

// ---- answering a sync on the device (gossip.hip.h): the diff of sw_sync_diff as the arrays a payload call takes ---------
}  // extern "C"
namespace {

struct ExportArrays { uint8_t *id, *sp_id, *op_id, *arity; int32_t* creator; double* t; uint8_t* sig; int32_t* event; };

// what both forms and sw_sync_pull ask of the answering context
int export_pre(sw_ctx* c, int64_t head, const char* what) {
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (c->exact) return fail(c, SW_ENOTSUP, "%s is not available on the exact (forked-hashgraph) path", what);
    if (c->ids.n_ids != c->N)
        return fail(c, SW_ENOTSUP, "%s: %lld of the %lld stored events have no id (sw_set_event_ids first)", what, (long long)(c->N - c->ids.n_ids), (long long)c->N);
    if (head < c->first_resident || head >= c->divided) return fail(c, SW_ERANGE, "%s: head %lld is not a divided, resident event", what, (long long)head);
    return SW_OK;
}

// d_ht complete on the device.  sw_sync_diff and sw_get_known_heights call ensure_dag_h for this, which also fills the host
// mirrors of parents and heights; nothing here reads those mirrors, so the download is skipped when the device already holds
// every height: events appended from device memory have theirs in d_ht once heights_ready has waited for the kernel
// (ht_dev_upto), and only a bulk HOST append leaves heights to ensure_dag_h's loop — the test append_device_body makes.
int heights_on_device(sw_ctx* c) {
    CHK(heights_ready(c));
    if ((int64_t)c->sp.size() < c->N && c->ing.ht_dev_upto < c->N) CHK(ensure_dag_h(c));
    return SW_OK;
}

// k_sync_diff, the offsets and the count, on the context's stream; ONE synchronisation, for the count.  `known` (n int32,
// may be NULL: nobody known) is copied with `kind`; it is compared with heights and never used as an index.
int export_ranges(sw_ctx* c, int64_t head, const int32_t* known, hipMemcpyKind kind, int64_t* total) {
    CHK(heights_on_device(c));
    const int np = c->npad, n = c->n;
    CHK(dgrow(c, c->d_q, (size_t)3 * np, 0));
    CHK(dgrow(c, c->xp.d, (size_t)2 * np + 8, 0));
    if (c->payload_pending) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_payload, 0));   // timestamps / signatures of a bulk host append
    HIPCHK(c, hipMemsetAsync(c->d_q.p, 0xff, (size_t)np * sizeof(int32_t), c->stream));
    if (known) HIPCHK(c, hipMemcpyAsync(c->d_q.p, known, (size_t)n * sizeof(int32_t), kind, c->stream));
    hipLaunchKernelGGL(k_sync_diff, dim3(1), dim3(np), 0, c->stream, (const int*)c->d_L.p, (const int*)c->d_ht.p, (const int*)c->d_seq.p,
                       (const int*)c->d_cr.p, (const int*)c->d_chain_start.p, (const int*)c->d_chain_ev.p, (const int*)c->d_q.p,
                       (int)head, np, c->d_q.p + np, c->d_q.p + 2 * np);
    hipLaunchKernelGGL(gsp::k_export_offsets, dim3(1), dim3(gsp::SCAN_THREADS), 0, c->stream, (const int*)(c->d_q.p + np), (const int*)(c->d_q.p + 2 * np),
                       (const int*)c->d_chain_start.p, n, c->xp.d.p + 2, c->xp.d.p + 2 + np + 1, (long long*)c->xp.d.p);
    c->ctr.kernel_launches += 2;
    HIPCHK(c, hipGetLastError());
    long long tot = 0;
    HIPCHK(c, hipMemcpyAsync(&tot, c->xp.d.p, sizeof tot, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (tot < 1 || tot > c->N) return fail(c, SW_EIO, "export: the ranges hold %lld events of %lld (internal error)", tot, (long long)c->N);
    *total = tot;
    return SW_OK;
}

// the gather of `total` slots behind export_ranges, on the context's stream (asynchronous)
int export_gather(sw_ctx* c, int64_t total, const ExportArrays& o) {
    const int np = c->npad;
    gsp::ExportIn in{c->xp.d.p + 2, c->xp.d.p + 2 + np + 1, c->d_chain_ev.p, c->d_sp.p, c->d_op.p, c->ids.d_id.p, c->d_sig.p, (const unsigned long long*)c->d_t.p};
    gsp::ExportOut out{o.id, o.sp_id, o.op_id, o.arity, o.creator, (unsigned long long*)o.t, o.sig, o.event};
    const int G = c->xp.lanes;
    const size_t lds = (size_t)(2 * c->n + 1) * sizeof(int);   // off[n + 1] | base[n]
    const dim3 grid((unsigned)std::min<int64_t>(2048, (total * G + gsp::GATHER_THREADS - 1) / gsp::GATHER_THREADS)), block(gsp::GATHER_THREADS);
    if (G == 4) hipLaunchKernelGGL(gsp::k_export_gather<4>, grid, block, lds, c->stream, in, out, c->n, (int)total);
    else if (G == 8) hipLaunchKernelGGL(gsp::k_export_gather<8>, grid, block, lds, c->stream, in, out, c->n, (int)total);
    else hipLaunchKernelGGL(gsp::k_export_gather<16>, grid, block, lds, c->stream, in, out, c->n, (int)total);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    return SW_OK;
}

// the exported arrays for `total` events inside xp.d_out; with `st` and `host` (the host-array forms) stage_down(st, xp.d_out)
// brings them to the caller's arrays
int export_scratch(sw_ctx* c, int64_t total, bool with_t, bool with_sig, bool with_event, ExportArrays* o, Stage* st = nullptr, const ExportArrays& host = {}) {
    const size_t k = (size_t)total;
    Stage own;
    Stage& s = st ? *st : own;
    const size_t o_id = s.out(host.id, k * 32), o_sp = s.out(host.sp_id, k * 32), o_op = s.out(host.op_id, k * 32), o_ar = s.out(host.arity, k), o_cr = s.out(host.creator, k * 4);
    const size_t o_t = s.out(host.t, with_t ? k * 8 : 0), o_sig = s.out(host.sig, with_sig ? k * 64 : 0), o_ev = s.out(host.event, with_event ? k * 4 : 0);
    unsigned char* B = nullptr;
    CHK(stage_up(c, c->xp.d_out, s, &B));
    *o = ExportArrays{B + o_id, B + o_sp, B + o_op, B + o_ar, (int32_t*)(B + o_cr), with_t ? (double*)(B + o_t) : nullptr,
                      with_sig ? B + o_sig : nullptr, with_event ? (int32_t*)(B + o_ev) : nullptr};
    return SW_OK;
}

}  // namespace
extern "C" {

int sw_get_known_heights_device(sw_ctx* c, int64_t head_event, int32_t* d_out, void* user_stream) {
    if (!c || !d_out) return SW_EINVAL;
    if (head_event < c->first_resident || head_event >= c->divided) return fail(c, SW_ERANGE, "head %lld is not a divided, resident event", (long long)head_event);
    CHK(device_args(c, "sw_get_known_heights_device", {{d_out, (size_t)c->n * sizeof(int32_t), 1}}));
    CHK(heights_on_device(c));
    const int np = c->npad;
    CHK(dgrow(c, c->d_q, (size_t)3 * np, 0));
    UserStream bracket;   // (the output may still be read by what the caller enqueued earlier)
    CHK(bracket.join(c, (hipStream_t)user_stream));
    hipLaunchKernelGGL(k_known_heights, dim3(1), dim3(np), 0, c->stream, (const int*)c->d_L.p, (const int*)c->d_ht.p, (int)head_event, np, c->d_q.p);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    // n entries, not npad: the caller's array ends there
    HIPCHK(c, hipMemcpyAsync(d_out, c->d_q.p, (size_t)c->n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    return bracket.leave();
}

int sw_export_payload_device(sw_ctx* c, int64_t head_event, const int32_t* d_known_height, int64_t cap, uint8_t* d_id32, uint8_t* d_sp_id32,
                             uint8_t* d_op_id32, uint8_t* d_arity, int32_t* d_creator, double* d_t, uint8_t* d_sig64, int32_t* d_event,
                             void* user_stream, int64_t* n_out) {
    if (!c) return SW_EINVAL;
    if (!n_out) return fail(c, SW_EINVAL, "sw_export_payload_device: n_out is NULL");
    *n_out = 0;
    CHK(export_pre(c, head_event, "sw_export_payload_device"));
    if (cap < 0 || (cap > 0 && (!d_id32 || !d_sp_id32 || !d_op_id32 || !d_arity || !d_creator)))
        return fail(c, SW_EINVAL, "sw_export_payload_device: NULL output arrays (capacity %lld)", (long long)cap);
    // (with capacity 0 the rows are empty and skipped: the alignment of whatever was passed is asked for all the same)
    if (cap == 0 && (((uintptr_t)d_id32 | (uintptr_t)d_sp_id32 | (uintptr_t)d_op_id32 | (uintptr_t)d_sig64) & 15)) return misaligned(c, "sw_export_payload_device", 16);
    const size_t k = (size_t)cap;
    CHK(device_args(c, "sw_export_payload_device", {{d_id32, k * 32, 16}, {d_sp_id32, k * 32, 16}, {d_op_id32, k * 32, 16}, {d_sig64, k * 64, 16},
                                                    {d_known_height, (size_t)c->n * sizeof(int32_t), 1}, {d_arity, k, 1}, {d_creator, k * 4, 1}, {d_t, k * 8, 1},
                                                    {d_event, k * 4, 1}}));
    const bool prof = c->profiling;
    auto t0 = std::chrono::steady_clock::now();
    UserStream bracket;   // the producer of d_known_height; earlier readers of the output arrays
    CHK(bracket.join(c, (hipStream_t)user_stream));
    int64_t total = 0;
    CHK(export_ranges(c, head_event, d_known_height, hipMemcpyDeviceToDevice, &total));
    *n_out = total;
    c->xp.ms[0] = prof ? ms_since(t0) : 0;
    c->xp.ms[1] = 0;
    if (total > cap) return fail(c, SW_ERANGE, "sw_export_payload_device: %lld events to export, capacity %lld (nothing written)", (long long)total, (long long)cap);
    t0 = std::chrono::steady_clock::now();
    CHK(export_gather(c, total, ExportArrays{d_id32, d_sp_id32, d_op_id32, d_arity, d_creator, d_t, d_sig64, d_event}));
    CHK(bracket.leave());
    if (prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->xp.ms[1] = ms_since(t0); }
    c->xp.calls++;
    c->xp.events += total;
    return SW_OK;
}

int sw_export_payload(sw_ctx* c, int64_t head_event, const int32_t* known_height, int64_t cap, uint8_t* id32, uint8_t* sp_id32, uint8_t* op_id32,
                      uint8_t* arity, int32_t* creator, double* t, uint8_t* sig64, int32_t* event, int64_t* n_out) {
    if (!c) return SW_EINVAL;
    if (!n_out) return fail(c, SW_EINVAL, "sw_export_payload: n_out is NULL");
    *n_out = 0;
    CHK(export_pre(c, head_event, "sw_export_payload"));
    if (cap < 0 || (cap > 0 && (!id32 || !sp_id32 || !op_id32 || !arity || !creator)))
        return fail(c, SW_EINVAL, "sw_export_payload: NULL output arrays (capacity %lld)", (long long)cap);
    HIPCHK(c, hipSetDevice(c->device));
    const bool prof = c->profiling;
    auto t0 = std::chrono::steady_clock::now();
    int64_t total = 0;
    CHK(export_ranges(c, head_event, known_height, hipMemcpyHostToDevice, &total));
    *n_out = total;
    c->xp.ms[0] = prof ? ms_since(t0) : 0;
    c->xp.ms[1] = 0;
    if (total > cap) return fail(c, SW_ERANGE, "sw_export_payload: %lld events to export, capacity %lld (nothing written)", (long long)total, (long long)cap);
    t0 = std::chrono::steady_clock::now();
    ExportArrays d{};
    Stage st;
    CHK(export_scratch(c, total, t != nullptr, sig64 != nullptr, event != nullptr, &d, &st, ExportArrays{id32, sp_id32, op_id32, arity, creator, t, sig64, event}));
    CHK(export_gather(c, total, d));
    CHK(stage_down(c, st, c->xp.d_out.p));
    if (prof) c->xp.ms[1] = ms_since(t0);
    c->xp.calls++;
    c->xp.events += total;
    return SW_OK;
}

int sw_get_export_stats(sw_ctx* c, int64_t* calls, int64_t* events, double* phase_ms) {
    if (!c) return SW_EINVAL;
    if (calls) *calls = c->xp.calls;
    if (events) *events = c->xp.events;
    if (phase_ms) for (int i = 0; i < 2; ++i) phase_ms[i] = c->xp.ms[i];
    return SW_OK;
}

int sw_num_ordered(sw_ctx* c, int64_t* out) {
    if (!c || !out) return SW_EINVAL;
    *out = (int64_t)c->transactions.size();
    return SW_OK;
}

int sw_get_transactions(sw_ctx* c, int64_t first, int64_t K, int32_t* out) {
    if (!c || !out) return SW_EINVAL;
    if (first < 0 || K < 0 || first + K > (int64_t)c->transactions.size()) return fail(c, SW_ERANGE, "range outside the ordered events");
    for (int64_t i = 0; i < K; ++i) out[i] = c->transactions[first + i];
    return SW_OK;
}

// ---- round received and consensus timestamp (consensus.hip.h; swirld.py:283-309) ----------------------------------------
}  // extern "C"
namespace {

int consensus_pre(sw_ctx* c, const char* what) {
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (c->exact && !c->hist.on) return fail(c, SW_ENOTSUP, "%s is not available on the exact (forked-hashgraph) path", what);
    return SW_OK;
}

// both per-event getters: k_consensus_events into context scratch, the wanted array(s) back, one synchronisation
int consensus_events(sw_ctx* c, const char* what, int64_t first, int64_t K, int32_t* rr_out, double* cts_out) {
    CHK(consensus_pre(c, what));
    if (first < 0 || K < 0 || first + K > c->N)
        return fail(c, SW_ERANGE, "%s: range [%lld, %lld) outside [0, %lld)", what, (long long)first, (long long)(first + K), (long long)c->N);
    if (!K || (!rr_out && !cts_out)) return SW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->exact) {
        // (history on) the tables hold -1 / the quiet NaN for every event that is not ordered: they are copied as they are
        if (rr_out) HIPCHK(c, hipMemcpyAsync(rr_out, c->cons.d_rr.p + first, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        if (cts_out) HIPCHK(c, hipMemcpyAsync(cts_out, c->cons.d_cts.p + first, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return SW_OK;
    }
    const int np = c->npad;
    Stage st;
    const size_t o_rr = st.out_opt(rr_out, (size_t)K * 4), o_cts = st.out_opt(cts_out, (size_t)K * 8);
    unsigned char* B = nullptr;
    CHK(stage_up(c, c->cons.d_out, st, &B));
    CHK(dgrow(c, c->cons.d_ordpos, np, 0));
    // (a pageable source: staged before the call returns; every entry below n is written, the kernel reads no other)
    HIPCHK(c, hipMemcpyAsync(c->cons.d_ordpos.p, c->ord_pos.data(), (size_t)c->n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    int32_t* d_rr_out = rr_out ? (int32_t*)(B + o_rr) : nullptr;
    unsigned long long* d_cts_out = cts_out ? (unsigned long long*)(B + o_cts) : nullptr;
    const unsigned grid = (unsigned)std::min<int64_t>(4096, (K + cns::THREADS - 1) / cns::THREADS);
    hipLaunchKernelGGL(cns::k_consensus_events, dim3(grid), dim3(cns::THREADS), 0, c->stream, (long long)first, (long long)K, (const int*)c->d_seq.p,
                       (const int*)c->d_cr.p, (const int*)c->cons.d_ordpos.p, (const int*)c->cons.d_rr.p, (const unsigned long long*)c->cons.d_cts.p, d_rr_out, d_cts_out);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    return stage_down(c, st, B);
}

struct OrderedArrays { int32_t* event; uint8_t* id; int32_t* creator; int32_t* rr; double* t; };

// what both export forms check before anything is enqueued
int ordered_pre(sw_ctx* c, const char* what, int64_t first, int64_t K, bool want_ids) {
    CHK(consensus_pre(c, what));
    if (first < 0 || K < 0 || first + K > c->cons.tx_len)
        return fail(c, SW_ERANGE, "%s: positions [%lld, %lld) outside the %lld ordered events (nothing written)", what, (long long)first, (long long)(first + K), (long long)c->cons.tx_len);
    if (want_ids && c->ids.n_ids != c->N)
        return fail(c, SW_ENOTSUP, "%s: %lld of the %lld stored events have no id (sw_set_event_ids first, or pass no id array)", what, (long long)(c->N - c->ids.n_ids), (long long)c->N);
    return SW_OK;
}

// the gather of K > 0 positions on the context's stream (asynchronous)
int ordered_gather(sw_ctx* c, int64_t first, int64_t K, const OrderedArrays& o) {
    cns::OrderedIn in{c->cons.d_tx.p, c->ids.d_id.p, c->d_cr.p, c->cons.d_rr.p, (const unsigned long long*)c->cons.d_cts.p};
    cns::OrderedOut out{o.event, o.id, o.creator, o.rr, (unsigned long long*)o.t};
    constexpr int G = cns::GATHER_LANES;
    const dim3 grid((unsigned)std::min<int64_t>(2048, (K * G + cns::THREADS - 1) / cns::THREADS)), block(cns::THREADS);
    hipLaunchKernelGGL(cns::k_ordered_gather<G>, grid, block, 0, c->stream, in, out, (long long)first, (long long)K);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    c->cons.export_calls++;
    c->cons.exported += K;
    return SW_OK;
}

}  // namespace
extern "C" {

int sw_get_round_received(sw_ctx* c, int64_t first, int64_t K, int32_t* out) {
    if (!c) return SW_EINVAL;
    return consensus_events(c, "sw_get_round_received", first, K, out, nullptr);
}

int sw_get_consensus_time(sw_ctx* c, int64_t first, int64_t K, double* out) {
    if (!c) return SW_EINVAL;
    return consensus_events(c, "sw_get_consensus_time", first, K, nullptr, out);
}

int sw_export_ordered_device(sw_ctx* c, int64_t first, int64_t K, int32_t* d_event, uint8_t* d_id32, int32_t* d_creator,
                             int32_t* d_round_received, double* d_time, void* user_stream) {
    if (!c) return SW_EINVAL;
    CHK(ordered_pre(c, "sw_export_ordered_device", first, K, d_id32 != nullptr));
    if (!K && ((uintptr_t)d_id32 & 15)) return misaligned(c, "sw_export_ordered_device", 16);   // (asked for K = 0 too, where the row is skipped)
    if (!K || (!d_event && !d_id32 && !d_creator && !d_round_received && !d_time)) return SW_OK;
    const size_t k = (size_t)K;
    CHK(device_args(c, "sw_export_ordered_device", {{d_id32, k * 32, 16}, {d_event, k * 4, 1}, {d_creator, k * 4, 1}, {d_round_received, k * 4, 1}, {d_time, k * 8, 1}}));
    UserStream bracket;   // earlier readers of the output arrays
    CHK(bracket.join(c, (hipStream_t)user_stream));
    CHK(ordered_gather(c, first, K, OrderedArrays{d_event, d_id32, d_creator, d_round_received, d_time}));
    return bracket.leave();
}

int sw_export_ordered(sw_ctx* c, int64_t first, int64_t K, int32_t* event, uint8_t* id32, int32_t* creator, int32_t* round_received, double* time) {
    if (!c) return SW_EINVAL;
    CHK(ordered_pre(c, "sw_export_ordered", first, K, id32 != nullptr));
    if (!K || (!event && !id32 && !creator && !round_received && !time)) return SW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t k = (size_t)K;
    Stage st;
    const size_t o_ev = st.out_opt(event, k * 4), o_id = st.out_opt(id32, k * 32), o_cr = st.out_opt(creator, k * 4),
                 o_rr = st.out_opt(round_received, k * 4), o_t = st.out_opt(time, k * 8);
    unsigned char* B = nullptr;
    CHK(stage_up(c, c->cons.d_out, st, &B));
    const OrderedArrays d{event ? (int32_t*)(B + o_ev) : nullptr, id32 ? B + o_id : nullptr, creator ? (int32_t*)(B + o_cr) : nullptr,
                          round_received ? (int32_t*)(B + o_rr) : nullptr, time ? (double*)(B + o_t) : nullptr};
    CHK(ordered_gather(c, first, K, d));
    return stage_down(c, st, B);
}

int sw_get_consensus_stats(sw_ctx* c, int64_t* record_calls, int64_t* recorded_events, int64_t* export_calls, int64_t* exported_events) {
    if (!c) return SW_EINVAL;
    if (record_calls) *record_calls = c->cons.record_calls;
    if (recorded_events) *recorded_events = c->cons.recorded;
    if (export_calls) *export_calls = c->cons.export_calls;
    if (exported_events) *exported_events = c->cons.exported;
    return SW_OK;
}

// (one counter lives on the device: the events the finalize check sent back to their rows)
static int refresh_device_counters(sw_ctx* c) {
    if (!c->d_fin.p) return SW_OK;
    unsigned long long tot = 0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream_aux));
    HIPCHK(c, hipMemcpy(&tot, c->d_fin.p + 2, sizeof tot, hipMemcpyDeviceToHost));
    c->ctr.finalize_from_rows = (int64_t)tot;
    return SW_OK;
}

int sw_get_counters(sw_ctx* c, sw_counters* out) {
    if (!c || !out) return SW_EINVAL;
    CHK(refresh_device_counters(c));
    *out = c->ctr;
    return SW_OK;
}

int sw_get_counters_sized(sw_ctx* c, void* out, size_t out_bytes) {
    if (!c || !out) return SW_EINVAL;
    CHK(refresh_device_counters(c));
    memcpy(out, &c->ctr, std::min(out_bytes, sizeof(sw_counters)));
    return SW_OK;
}

int sw_set_profiling(sw_ctx* c, int enable) {
    if (!c) return SW_EINVAL;
    c->profiling = enable != 0;
    return SW_OK;
}

int sw_debug_clocks(sw_ctx* c, unsigned long long* out, int64_t cap_words) {
    if (!c || !out) return SW_EINVAL;
    if (!c->d_dbg.p) return fail(c, SW_EINVAL, "sw_debug_clocks: the context was not created with SW_DEBUG_CLOCKS=1");
    const int64_t nw = std::min<int64_t>(cap_words, (int64_t)SW_DBG_MAX_ITERS * 32);
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(out, c->d_dbg.p, (size_t)nw * 8, hipMemcpyDeviceToHost));
    return SW_OK;
}

int sw_debug_live_resources(int64_t* device_bytes, int64_t* pinned_bytes, int64_t* events, int64_t* streams) {
    if (device_bytes) *device_bytes = owned::live.device_bytes.load(std::memory_order_relaxed);
    if (pinned_bytes) *pinned_bytes = owned::live.pinned_bytes.load(std::memory_order_relaxed);
    if (events) *events = owned::live.events.load(std::memory_order_relaxed);
    if (streams) *streams = owned::live.streams.load(std::memory_order_relaxed);
    return SW_OK;
}

int sw_debug_block_clocks(sw_ctx* c, unsigned long long* out, int64_t cap_words) {
    if (!c || !out) return SW_EINVAL;
    if (!c->d_dbg_blk.p) return fail(c, SW_EINVAL, "sw_debug_block_clocks: the context was not created with SW_DEBUG_CLOCKS=3");
    const int64_t nw = std::min<int64_t>(cap_words, (int64_t)SW_DBG_MAX_ITERS * 2 * 2048);
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(out, c->d_dbg_blk.p, (size_t)nw * 8, hipMemcpyDeviceToHost));
    return SW_OK;
}

int sw_get_timings(sw_ctx* c, sw_timings* out) {
    if (!c || !out) return SW_EINVAL;
    *out = c->tm;
    return SW_OK;
}

int sw_synchronize(sw_ctx* c) {
    if (!c) return SW_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

// ---- validation of payloads against the member keys (validate.hip.h) ---------------------------------
}  // extern "C"

namespace {

// the launch behind the argument checks, on the context's stream: every array in device memory
int validate_launch(sw_ctx* c, int64_t K, const swv::Payload& p, uint8_t* d_ok) {
    const int n = c->n;
    const unsigned blocks = (unsigned)((K + 63) / 64);
    hipLaunchKernelGGL(swv::k_validate_payload, dim3(blocks), dim3(64), 0, c->stream, p, (long long)K, n, (const uint8_t*)c->val.d_keys.p,
                       (const uint8_t*)c->val.d_keys.p + (size_t)n * 32, (const swv::niels*)c->val.d_tab.p, d_ok);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    return SW_OK;
}

// the signing keys of the context, overwritten with zeros (sw_clear_signing_keys, sw_set_member_keys, sw_destroy)
int sign_keys_clear(sw_ctx* c) {
    c->sign.has.clear();
    if (!c->sign.d_keys.p) return SW_OK;
    HIPCHK(c, hipMemsetAsync(c->sign.d_keys.p, 0, c->sign.d_keys.cap, c->stream));   // (behind whatever still signs on this stream)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

int validate_pre(sw_ctx* c, int64_t K, const void* msgs, const void* msg_off, int64_t msg_bytes, const void* whole, const void* whole_off,
                 int64_t whole_bytes, const void* sig, const void* creator, const void* id, const void* ok, const char* what) {
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (c->val.keys.empty()) return fail(c, SW_ENOTSUP, "%s: no member keys (sw_set_member_keys first)", what);
    if (K < 0 || msg_bytes < 0 || whole_bytes < 0) return fail(c, SW_EINVAL, "%s: negative count or length", what);
    if (K > 0x7fffffff) return fail(c, SW_ERANGE, "%s: more than 2^31 events", what);
    if (K > 0 && (!msg_off || !sig || !creator || !ok || (msg_bytes > 0 && !msgs))) return fail(c, SW_EINVAL, "%s: NULL arrays", what);
    const bool any_whole = whole || whole_off || whole_bytes;
    if (K > 0 && any_whole && (!whole_off || !id || (whole_bytes > 0 && !whole)))
        return fail(c, SW_EINVAL, "%s: the id check needs whole, whole_off and id32 (or none of the three)", what);
    return SW_OK;
}

}  // namespace

extern "C" {

int sw_set_member_keys(sw_ctx* c, const uint8_t* pk32, int32_t* n_unusable) {
    if (!c) return SW_EINVAL;
    if (n_unusable) *n_unusable = 0;
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (!pk32) return fail(c, SW_EINVAL, "sw_set_member_keys: NULL keys");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->n;
    const auto t0 = std::chrono::steady_clock::now();
    CHK(sign_keys_clear(c));   // signing keys belong to the member keys they were checked against
    CHK(dgrow(c, c->val.d_keys, n * 33, 0));
    CHK(dgrow(c, c->val.d_tab, (n + 1) * swv::ROW * sizeof(swv::niels), 0));
    // (an earlier validation may still be reading the old table on this stream: the build is ordered behind it)
    std::vector<uint8_t> keys(pk32, pk32 + n * 32), usable(n);
    HIPCHK(c, hipMemcpyAsync(c->val.d_keys.p, keys.data(), n * 32, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(swv::k_validate_table, dim3((unsigned)n + 1), dim3(swv::POSITIONS), 0, c->stream, (const uint8_t*)c->val.d_keys.p, (int)n,
                       (swv::niels*)c->val.d_tab.p, (uint8_t*)c->val.d_keys.p + n * 32);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(usable.data(), c->val.d_keys.p + n * 32, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->val.keys.swap(keys);
    c->val.usable.swap(usable);
    c->val.builds++;
    c->val.ms[0] = c->profiling ? ms_since(t0) : 0;
    int32_t bad = 0;
    for (uint8_t u : c->val.usable) bad += !u;
    if (n_unusable) *n_unusable = bad;
    return SW_OK;
}

int sw_get_member_keys(sw_ctx* c, uint8_t* pk32_out, uint8_t* usable_out) {
    if (!c) return SW_EINVAL;
    if (c->val.keys.empty()) return fail(c, SW_ENOTSUP, "sw_get_member_keys: no member keys (sw_set_member_keys first)");
    if (pk32_out) memcpy(pk32_out, c->val.keys.data(), c->val.keys.size());
    if (usable_out) memcpy(usable_out, c->val.usable.data(), c->val.usable.size());
    return SW_OK;
}

int sw_validate_payload_device(sw_ctx* c, int64_t K, const uint8_t* d_msgs, const int64_t* d_msg_off, int64_t msg_bytes, const uint8_t* d_whole,
                               const int64_t* d_whole_off, int64_t whole_bytes, const uint8_t* d_sig64, const int32_t* d_creator,
                               const uint8_t* d_id32, uint8_t* d_ok, void* user_stream) {
    if (!c) return SW_EINVAL;
    CHK(validate_pre(c, K, d_msgs, d_msg_off, msg_bytes, d_whole, d_whole_off, whole_bytes, d_sig64, d_creator, d_id32, d_ok, "sw_validate_payload_device"));
    if (K == 0) return SW_OK;
    const size_t k = (size_t)K;
    const bool idchk = d_whole_off != nullptr;
    // (ids without an id check are never read: their row is skipped, and only their alignment is asked for, as it always was)
    if (!idchk && ((uintptr_t)d_id32 & 7)) return misaligned(c, "sw_validate_payload_device", 8);
    CHK(device_args(c, "sw_validate_payload_device", {{d_id32, idchk ? k * 32 : 0, 8}, {d_msg_off, (k + 1) * 8, 8}, {d_whole_off, (k + 1) * 8, 8},
                                                      {d_msgs, (size_t)msg_bytes, 1}, {d_sig64, k * 64, 1}, {d_creator, k * 4, 1}, {d_ok, k, 1},
                                                      {d_whole, idchk ? (size_t)whole_bytes : 0, 1}}));
    const bool prof = c->profiling;
    const auto t0 = std::chrono::steady_clock::now();
    UserStream bracket;   // the producers of the arrays; earlier readers of d_ok
    CHK(bracket.join(c, (hipStream_t)user_stream));
    // (a zero-length buffer may be NULL: the kernel then only forms pointers it never reads through; `whole` non-NULL is
    // what selects the id check there)
    const uint8_t* anchor = (const uint8_t*)c->val.d_keys.p;
    const swv::Payload p{d_msgs ? d_msgs : anchor, (const long long*)d_msg_off, (long long)msg_bytes, idchk ? (d_whole ? d_whole : anchor) : nullptr,
                         (const long long*)d_whole_off, (long long)whole_bytes, d_sig64, d_creator, d_id32};
    CHK(validate_launch(c, K, p, d_ok));
    CHK(bracket.leave());   // whatever the caller enqueues next reads a complete d_ok
    c->val.ms[1] = 0;
    if (prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->val.ms[1] = ms_since(t0); }
    c->val.calls++;
    c->val.events += K;
    return SW_OK;
}

int sw_validate_payload(sw_ctx* c, int64_t K, const uint8_t* msgs, const int64_t* msg_off, int64_t msg_bytes, const uint8_t* whole,
                        const int64_t* whole_off, int64_t whole_bytes, const uint8_t* sig64, const int32_t* creator, const uint8_t* id32, uint8_t* ok) {
    if (!c) return SW_EINVAL;
    CHK(validate_pre(c, K, msgs, msg_off, msg_bytes, whole, whole_off, whole_bytes, sig64, creator, id32, ok, "sw_validate_payload"));
    if (K == 0) return SW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const bool prof = c->profiling;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t k = (size_t)K, mb = (size_t)msg_bytes, wb = (size_t)whole_bytes;
    const bool idchk = whole_off != nullptr;
    Stage st;   // (an absent buffer takes no room: `whole` and `whole_off` come together or not at all, validate_pre)
    const size_t o_moff = st.in(msg_off, (k + 1) * 8), o_m = st.in(msgs, mb), o_woff = st.in(whole_off, (k + 1) * 8), o_w = st.in(whole, wb);
    const size_t o_sig = st.in(sig64, k * 64), o_cr = st.in(creator, k * 4), o_id = st.in(idchk ? id32 : nullptr, k * 32), o_ok = st.out(ok, k);
    unsigned char* B = nullptr;
    CHK(stage_up(c, c->val.d_in, st, &B));
    const swv::Payload p{B + o_m, (const long long*)(B + o_moff), (long long)msg_bytes, idchk ? B + o_w : nullptr,
                         idchk ? (const long long*)(B + o_woff) : nullptr, (long long)whole_bytes, B + o_sig, (const int32_t*)(B + o_cr),
                         idchk ? B + o_id : nullptr};
    CHK(validate_launch(c, K, p, B + o_ok));
    CHK(stage_down(c, st, B));
    c->val.ms[1] = prof ? ms_since(t0) : 0;
    int64_t acc = 0;
    for (size_t i = 0; i < k; ++i) acc += ok[i] != 0;
    c->val.calls++;
    c->val.events += K;
    c->val.accepted += acc;
    return SW_OK;
}

int sw_get_validate_stats(sw_ctx* c, int64_t* calls, int64_t* events, int64_t* accepted, int64_t* table_builds, double* phase_ms) {
    if (!c) return SW_EINVAL;
    if (calls) *calls = c->val.calls;
    if (events) *events = c->val.events;
    if (accepted) *accepted = c->val.accepted;
    if (table_builds) *table_builds = c->val.builds;
    if (phase_ms) for (int i = 0; i < 2; ++i) phase_ms[i] = c->val.ms[i];
    return SW_OK;
}

// ---- the signed bytes of events built on the device (pack.hip.h) ---------------------------------------
}  // extern "C"

namespace {

struct PackArrays {   // what a pack call reads and writes, every array in device memory
    const uint8_t *sp_id, *op_id, *arity;
    const int32_t* creator;
    const double* t;
    const uint8_t *sig, *data;
    const int64_t* data_off;
    int64_t data_bytes;
    const uint8_t* data_none;
    uint8_t* msgs;
    int64_t* msg_off;
    uint8_t* whole;
    int64_t* whole_off;
    uint8_t* enc;
};

bool utf8_name(const char* s) {   // 1 .. 255 bytes of well-formed UTF-8
    if (!s) return false;
    const size_t len = strlen(s);
    if (len < 1 || len > (size_t)pck::MAX_NAME) return false;
    const unsigned char* p = (const unsigned char*)s;
    for (size_t i = 0; i < len;) {
        const unsigned b = p[i];
        int more;
        unsigned cp;
        if (b < 0x80) { ++i; continue; }
        else if (b >= 0xc2 && b <= 0xdf) { more = 1; cp = b & 0x1f; }
        else if (b >= 0xe0 && b <= 0xef) { more = 2; cp = b & 0x0f; }
        else if (b >= 0xf0 && b <= 0xf4) { more = 3; cp = b & 0x07; }
        else return false;
        if (i + more >= len) return false;
        for (int k = 1; k <= more; ++k) {
            if ((p[i + k] & 0xc0) != 0x80) return false;
            cp = (cp << 6) | (p[i + k] & 0x3f);
        }
        if ((more == 2 && cp < 0x800) || (more == 3 && cp < 0x10000) || cp > 0x10ffff || (cp >= 0xd800 && cp <= 0xdfff)) return false;
        i += more + 1;
    }
    return true;
}

int pack_hdr_len(const sw_ctx* c) { return (int)(c->pack.mod.size() + c->pack.qual.size() + 8); }

void pack_bound(const sw_ctx* c, int64_t K, int64_t data_bytes, int64_t* msg, int64_t* whole) {
    *msg = K * pck::MSG_MAX + data_bytes;
    *whole = K * (pck::WHOLE_MAX + pack_hdr_len(c)) + data_bytes;
}

// the class header of the whole stream in device memory (after sw_create and after sw_set_event_class: one small copy)
int pack_header(sw_ctx* c) {
    if (!c->pack.hdr_stale) return SW_OK;
    CHK(dgrow(c, c->pack.d_hdr, (size_t)pck::HDR_MAX + 248, 0));
    std::vector<uint8_t>& h = c->pack.hdr;
    h.clear();
    for (const std::string* s : {&c->pack.mod, &c->pack.qual}) {
        h.push_back(0x8c);
        h.push_back((uint8_t)s->size());
        h.insert(h.end(), s->begin(), s->end());
        h.push_back(0x94);
    }
    h.push_back(0x93);
    h.push_back(0x94);
    HIPCHK(c, hipMemcpyAsync(c->pack.d_hdr.p, h.data(), h.size(), hipMemcpyHostToDevice, c->stream));
    c->pack.hdr_stale = false;
    return SW_OK;
}

// the six launches behind the argument checks, on the context's stream.  bound_*: sw_pack_bound's values (the host does
// not know the totals: the writers' grids come from the bounds).
int pack_launch(sw_ctx* c, int64_t K, const PackArrays& a, int64_t bound_msg, int64_t bound_whole) {
    const bool prof = c->profiling;
    auto t0 = std::chrono::steady_clock::now();
    CHK(pack_header(c));
    const int64_t tiles = (K + pck::TILE - 1) / pck::TILE;
    CHK(dgrow(c, c->pack.d, (size_t)(2 * tiles) * sizeof(int64_t) + 256, 0));
    pck::i64* tsum = (pck::i64*)c->pack.d.p;
    const pck::PackIn in{a.sp_id, a.op_id, a.arity, a.creator, (const pck::u64*)a.t, a.sig, a.data, (const pck::i64*)a.data_off,
                         (pck::i64)a.data_bytes, a.data_none, (const unsigned char*)c->val.d_keys.p, (const unsigned char*)c->pack.d_hdr.p,
                         pack_hdr_len(c), c->n};
    pck::i64* moff = (pck::i64*)a.msg_off;
    pck::i64* woff = (pck::i64*)a.whole_off;
    hipLaunchKernelGGL(pck::k_pack_lengths, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream, in, (pck::i64)K, moff, woff, a.enc);
    hipLaunchKernelGGL(pck::k_pack_tile_sums, dim3((unsigned)tiles, 2), dim3(pck::SCAN_THREADS), 0, c->stream, (pck::i64)K, (pck::i64)tiles,
                       (const pck::i64*)moff, (const pck::i64*)woff, tsum);
    hipLaunchKernelGGL(pck::k_pack_scan_sums, dim3(2), dim3(pck::SCAN_THREADS), 0, c->stream, (pck::i64)K, (pck::i64)tiles, moff, woff, tsum);
    hipLaunchKernelGGL(pck::k_pack_offsets, dim3((unsigned)tiles, 2), dim3(pck::SCAN_THREADS), 0, c->stream, (pck::i64)K, (pck::i64)tiles, moff, woff,
                       (const pck::i64*)tsum);
    c->ctr.kernel_launches += 4;
    HIPCHK(c, hipGetLastError());
    if (prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->pack.ms[0] = ms_since(t0); t0 = std::chrono::steady_clock::now(); }
    for (int w = 0; w < 2; ++w) {
        const int64_t chunks = ((w ? bound_whole : bound_msg) + 15) / 16;
        const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(4096, (chunks + pck::WRITE_THREADS - 1) / pck::WRITE_THREADS));
        const int64_t trips = (chunks + blocks * pck::WRITE_THREADS - 1) / (blocks * pck::WRITE_THREADS);
        if (w) hipLaunchKernelGGL(pck::k_pack_write<true>, dim3((unsigned)blocks), dim3(pck::WRITE_THREADS), 0, c->stream, in, (pck::i64)K,
                                  (const pck::i64*)woff, a.whole, (pck::i64)trips);
        else hipLaunchKernelGGL(pck::k_pack_write<false>, dim3((unsigned)blocks), dim3(pck::WRITE_THREADS), 0, c->stream, in, (pck::i64)K,
                                (const pck::i64*)moff, a.msgs, (pck::i64)trips);
    }
    c->ctr.kernel_launches += 2;
    HIPCHK(c, hipGetLastError());
    c->pack.ms[0] = prof ? c->pack.ms[0] : 0;
    c->pack.ms[1] = 0;
    if (prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->pack.ms[1] = ms_since(t0); }
    c->pack.calls++;
    c->pack.events += K;
    return SW_OK;
}

// what both forms check before anything else; the bounds come back
int pack_pre(sw_ctx* c, int64_t K, const void* sp, const void* op, const void* arity, const void* creator, const void* t, const void* sig,
             const void* data, const void* data_off, int64_t data_bytes, const void* data_none, const void* msgs, const void* msg_off,
             int64_t msg_cap, const void* whole, const void* whole_off, int64_t whole_cap, int64_t* bm, int64_t* bw, const char* what) {
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (c->val.keys.empty()) return fail(c, SW_ENOTSUP, "%s: no member keys (sw_set_member_keys first)", what);
    if (K < 0 || data_bytes < 0 || msg_cap < 0 || whole_cap < 0) return fail(c, SW_EINVAL, "%s: negative count, length or capacity", what);
    if (K > 0x7fffffff) return fail(c, SW_ERANGE, "%s: more than 2^31 events", what);
    if (!msg_off || !whole_off) return fail(c, SW_EINVAL, "%s: NULL offset arrays", what);
    if (K > 0 && (!sp || !op || !arity || !creator || !t || !sig || !msgs || !whole)) return fail(c, SW_EINVAL, "%s: NULL arrays", what);
    if (!data_off && (data || data_bytes || data_none)) return fail(c, SW_EINVAL, "%s: data needs its offsets (or none of data, offsets, length, flags)", what);
    if (data_off && data_bytes > 0 && !data) return fail(c, SW_EINVAL, "%s: %lld data bytes and a NULL buffer", what, (long long)data_bytes);
    pack_bound(c, K, data_bytes, bm, bw);
    if (msg_cap < *bm || whole_cap < *bw)
        return fail(c, SW_ERANGE, "%s: capacities %lld / %lld below sw_pack_bound's %lld / %lld (nothing written)", what, (long long)msg_cap,
                    (long long)whole_cap, (long long)*bm, (long long)*bw);
    return SW_OK;
}

}  // namespace

extern "C" {

int sw_set_event_class(sw_ctx* c, const char* module, const char* qualname) {
    if (!c) return SW_EINVAL;
    if (!utf8_name(module) || !utf8_name(qualname)) return fail(c, SW_EINVAL, "sw_set_event_class: module and qualified name must be 1 .. 255 bytes of UTF-8");
    if (c->pack.mod == module && c->pack.qual == qualname) return SW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // a pack call may still be reading the old header
    c->pack.mod = module;
    c->pack.qual = qualname;
    c->pack.hdr_stale = true;
    return SW_OK;
}

int sw_get_event_class(sw_ctx* c, char* module_out, char* qualname_out) {
    if (!c) return SW_EINVAL;
    if (module_out) memcpy(module_out, c->pack.mod.c_str(), c->pack.mod.size() + 1);
    if (qualname_out) memcpy(qualname_out, c->pack.qual.c_str(), c->pack.qual.size() + 1);
    return SW_OK;
}

int sw_pack_bound(sw_ctx* c, int64_t K, int64_t data_bytes, int64_t* msg_bytes, int64_t* whole_bytes) {
    if (!c) return SW_EINVAL;
    if (K < 0 || data_bytes < 0) return fail(c, SW_EINVAL, "sw_pack_bound: negative count or length");
    if (K > 0x7fffffff) return fail(c, SW_ERANGE, "sw_pack_bound: more than 2^31 events");
    int64_t m = 0, w = 0;
    pack_bound(c, K, data_bytes, &m, &w);
    if (msg_bytes) *msg_bytes = m;
    if (whole_bytes) *whole_bytes = w;
    return SW_OK;
}

int sw_pack_events_device(sw_ctx* c, int64_t K, const uint8_t* d_sp_id32, const uint8_t* d_op_id32, const uint8_t* d_arity, const int32_t* d_creator,
                          const double* d_t, const uint8_t* d_sig64, const uint8_t* d_data, const int64_t* d_data_off, int64_t data_bytes,
                          const uint8_t* d_data_none, uint8_t* d_msgs, int64_t* d_msg_off, int64_t msg_cap, uint8_t* d_whole, int64_t* d_whole_off,
                          int64_t whole_cap, uint8_t* d_encodable, void* user_stream) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_pack_events_device";
    int64_t bm = 0, bw = 0;
    CHK(pack_pre(c, K, d_sp_id32, d_op_id32, d_arity, d_creator, d_t, d_sig64, d_data, d_data_off, data_bytes, d_data_none, d_msgs, d_msg_off, msg_cap,
                 d_whole, d_whole_off, whole_cap, &bm, &bw, what));
    const size_t k = (size_t)K;
    if (K == 0) {   // (no event: only the two offset arrays are touched; the alignment of whatever else was passed is asked for all the same)
        if (((uintptr_t)d_msgs | (uintptr_t)d_whole | (uintptr_t)d_sig64 | (uintptr_t)d_sp_id32 | (uintptr_t)d_op_id32) & 15) return misaligned(c, what, 16);
        if (((uintptr_t)d_data_off | (uintptr_t)d_t) & 7) return misaligned(c, what, 8);
        if ((uintptr_t)d_creator & 3) return misaligned(c, what, 4);
    }
    // (the two streams are empty rows when no event is packed, whatever their capacity)
    CHK(device_args(c, what, {{d_msgs, K ? (size_t)msg_cap : 0, 16}, {d_whole, K ? (size_t)whole_cap : 0, 16}, {d_sig64, k * 64, 16}, {d_sp_id32, k * 32, 16},
                              {d_op_id32, k * 32, 16}, {d_msg_off, (k + 1) * 8, 8}, {d_whole_off, (k + 1) * 8, 8}, {d_data_off, K ? (k + 1) * 8 : 0, 8},
                              {d_t, k * 8, 8}, {d_creator, k * 4, 4}, {d_arity, k, 1}, {d_encodable, k, 1}, {d_data, K ? (size_t)data_bytes : 0, 1},
                              {d_data_none, k, 1}}));
    UserStream bracket;   // the producers of the arrays; earlier readers of the outputs
    CHK(bracket.join(c, (hipStream_t)user_stream));
    if (K == 0) {
        HIPCHK(c, hipMemsetAsync(d_msg_off, 0, 8, c->stream));
        HIPCHK(c, hipMemsetAsync(d_whole_off, 0, 8, c->stream));
    } else {
        CHK(pack_launch(c, K, PackArrays{d_sp_id32, d_op_id32, d_arity, d_creator, d_t, d_sig64, d_data, d_data_off, data_bytes, d_data_none, d_msgs,
                                         d_msg_off, d_whole, d_whole_off, d_encodable}, bm, bw));
    }
    return bracket.leave();   // whatever the caller enqueues next reads complete streams
}

int sw_pack_events(sw_ctx* c, int64_t K, const uint8_t* sp_id32, const uint8_t* op_id32, const uint8_t* arity, const int32_t* creator, const double* t,
                   const uint8_t* sig64, const uint8_t* data, const int64_t* data_off, int64_t data_bytes, const uint8_t* data_none, uint8_t* msgs,
                   int64_t* msg_off, int64_t msg_cap, uint8_t* whole, int64_t* whole_off, int64_t whole_cap, uint8_t* encodable, int64_t* msg_bytes,
                   int64_t* whole_bytes) {
    if (!c) return SW_EINVAL;
    if (msg_bytes) *msg_bytes = 0;
    if (whole_bytes) *whole_bytes = 0;
    int64_t bm = 0, bw = 0;
    CHK(pack_pre(c, K, sp_id32, op_id32, arity, creator, t, sig64, data, data_off, data_bytes, data_none, msgs, msg_off, msg_cap, whole, whole_off,
                 whole_cap, &bm, &bw, "sw_pack_events"));
    msg_off[0] = whole_off[0] = 0;
    if (K == 0) return SW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t k = (size_t)K, db = (size_t)data_bytes;
    Stage st;   // (the two streams come back behind the offsets, by the totals those report)
    const size_t o_sp = st.in(sp_id32, k * 32), o_op = st.in(op_id32, k * 32), o_ar = st.in(arity, k), o_cr = st.in(creator, k * 4), o_t = st.in(t, k * 8);
    const size_t o_sig = st.in(sig64, k * 64), o_doff = st.in(data_off, (k + 1) * 8), o_d = st.in(data, db), o_dn = st.in(data_none, k);
    const size_t o_moff = st.out(msg_off, (k + 1) * 8), o_woff = st.out(whole_off, (k + 1) * 8), o_m = st.out(msgs, (size_t)bm, 0), o_w = st.out(whole, (size_t)bw, 0);
    const size_t o_enc = st.out(encodable, k);
    unsigned char* B = nullptr;
    CHK(stage_up(c, c->pack.d_in, st, &B));
    CHK(pack_launch(c, K, PackArrays{B + o_sp, B + o_op, B + o_ar, (const int32_t*)(B + o_cr), (const double*)(B + o_t), B + o_sig,
                                     data_off ? B + o_d : nullptr, data_off ? (const int64_t*)(B + o_doff) : nullptr, data_bytes,
                                     data_none ? B + o_dn : nullptr, B + o_m, (int64_t*)(B + o_moff), B + o_w, (int64_t*)(B + o_woff), B + o_enc}, bm, bw));
    CHK(stage_down(c, st, B));
    const int64_t tm = msg_off[K], tw = whole_off[K];
    if (tm < 0 || tm > bm || tw < 0 || tw > bw) return fail(c, SW_EIO, "sw_pack_events: totals %lld / %lld outside the bounds (internal error)", (long long)tm, (long long)tw);
    st.out_bytes(msgs, (size_t)tm);
    st.out_bytes(whole, (size_t)tw);
    CHK(stage_down(c, st, B));
    c->pack.bytes += tm + tw;
    if (msg_bytes) *msg_bytes = tm;
    if (whole_bytes) *whole_bytes = tw;
    return SW_OK;
}

int sw_get_pack_stats(sw_ctx* c, int64_t* calls, int64_t* events, int64_t* bytes, double* phase_ms) {
    if (!c) return SW_EINVAL;
    if (calls) *calls = c->pack.calls;
    if (events) *events = c->pack.events;
    if (bytes) *bytes = c->pack.bytes;
    if (phase_ms) for (int i = 0; i < 2; ++i) phase_ms[i] = c->pack.ms[i];
    return SW_OK;
}

// ---- the data of events kept on the device (data.hip.h) -------------------------------------------------
}  // extern "C"

namespace {

struct DataPlan {   // the scratch of one call inside data.d
    dat::i64* off;            // [K + 1] lengths, then scanned offsets; [K + 1]: the bad-slot count (low 32 bits)
    unsigned char* none;      // [K]
    dat::i64* tsum;           // tile sums of the scan
    int* slot;                // [slots] dense rank -> payload position (ingest append)
    unsigned char* ok;        // [oks] the folded verdicts (ingest)
};

int data_scratch(sw_ctx* c, int64_t K, int64_t slots, int64_t oks, DataPlan* p) {
    const size_t k = (size_t)K, tiles = (k + pck::TILE - 1) / pck::TILE;
    Carve cv;
    const size_t o_off = cv.take((k + 2) * 8), o_none = cv.take(k), o_ts = cv.take((tiles + 1) * 8), o_slot = cv.take((size_t)slots * 4), o_ok = cv.take((size_t)oks);
    CHK(dgrow(c, c->data.d, cv.off + 256, 0));
    unsigned char* B = c->data.d.p;
    *p = DataPlan{(dat::i64*)(B + o_off), B + o_none, (dat::i64*)(B + o_ts), (int*)(B + o_slot), B + o_ok};
    return SW_OK;
}

// room for the data of `events` events in `bytes` bytes (contents kept): arena with its slack, offsets, flags
int data_reserve(sw_ctx* c, int64_t events, int64_t bytes) {
    CHK(dgrow(c, c->data.d_arena, (size_t)bytes + dat::SLACK + 256, (size_t)c->data.used));
    CHK(dgrow(c, c->data.d_off, (size_t)events + 1, c->data.d_off.p ? (size_t)c->data.n_data + 1 : 0));
    CHK(dgrow(c, c->data.d_none, (size_t)events + 256, (size_t)c->data.n_data));
    return SW_OK;
}

// lengths, scan, and the read-back of the byte total and the bad-slot count: ONE synchronisation
int data_plan(sw_ctx* c, int64_t K, const dat::SegIn& in, const DataPlan& p, int64_t* total, int64_t* bad) {
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(c, hipMemsetAsync(p.off + K, 0, 16, c->stream));   // off[K] (K = 0: the total) and the count
    if (K > 0) {
        const int64_t tiles = (K + pck::TILE - 1) / pck::TILE;
        hipLaunchKernelGGL(dat::k_data_lengths, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream, in, (dat::i64)K, p.off, p.none, (int*)(p.off + K + 1));
        hipLaunchKernelGGL(pck::k_pack_tile_sums, dim3((unsigned)tiles, 1), dim3(pck::SCAN_THREADS), 0, c->stream, (pck::i64)K, (pck::i64)tiles,
                           (const pck::i64*)p.off, (const pck::i64*)p.off, p.tsum);
        hipLaunchKernelGGL(pck::k_pack_scan_sums, dim3(1), dim3(pck::SCAN_THREADS), 0, c->stream, (pck::i64)K, (pck::i64)tiles, p.off, p.off, p.tsum);
        hipLaunchKernelGGL(pck::k_pack_offsets, dim3((unsigned)tiles, 1), dim3(pck::SCAN_THREADS), 0, c->stream, (pck::i64)K, (pck::i64)tiles, p.off, p.off,
                           (const pck::i64*)p.tsum);
        c->ctr.kernel_launches += 4;
        HIPCHK(c, hipGetLastError());
    }
    long long rb[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(rb, p.off + K, sizeof rb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *total = rb[0];
    *bad = rb[1] & 0xffffffffll;
    c->data.ms[0] = c->profiling ? ms_since(t0) : 0;
    c->data.ms[1] = 0;
    return SW_OK;
}

// the copy of `total` bytes to dst + dst_base (the destination holds dst_base + total bytes at least), and the offsets
// (plus `base`) and flags to where they stay; asynchronous
int data_copy(sw_ctx* c, int64_t K, const dat::SegIn& in, const DataPlan& p, int64_t total, unsigned char* dst, int64_t dst_base, int64_t base,
              int64_t* off_out, unsigned char* none_out) {
    const auto t0 = std::chrono::steady_clock::now();
    if (total > 0) {
        const int64_t chunks = ((dst_base & 15) + total + 15) / 16;
        const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(4096, (chunks + dat::WRITE_THREADS - 1) / dat::WRITE_THREADS));
        const int64_t trips = (chunks + blocks * dat::WRITE_THREADS - 1) / (blocks * dat::WRITE_THREADS);
        hipLaunchKernelGGL(dat::k_data_copy, dim3((unsigned)blocks), dim3(dat::WRITE_THREADS), 0, c->stream, in, (dat::i64)K, (const dat::i64*)p.off, dst,
                           (dat::i64)dst_base, (dat::i64)trips);
        c->ctr.kernel_launches++;
    }
    hipLaunchKernelGGL(dat::k_data_store_off, dim3((unsigned)((K + 256) / 256)), dim3(256), 0, c->stream, (dat::i64)K, (const dat::i64*)p.off, (dat::i64)base,
                       (dat::i64*)off_out, (const unsigned char*)p.none, none_out);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    if (c->profiling) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->data.ms[1] = ms_since(t0); }
    return SW_OK;
}

// what both forms of sw_set_event_data check first
int data_set_args(sw_ctx* c, int64_t first, int64_t K, const void* data, const void* data_off, int64_t data_bytes, const void* data_none, const char* what) {
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (K < 0 || data_bytes < 0) return fail(c, SW_EINVAL, "%s: negative count or length", what);
    if (first != c->data.n_data) return fail(c, SW_EINVAL, "%s must continue at event %lld (got %lld): data is contiguous from 0", what, (long long)c->data.n_data, (long long)first);
    if (first + K > c->N) return fail(c, SW_ERANGE, "%s: events [%lld, %lld) outside the stored hashgraph", what, (long long)first, (long long)(first + K));
    if (!data_off && (data || data_bytes || data_none)) return fail(c, SW_EINVAL, "%s: data needs its offsets (or none of data, offsets, length, flags)", what);
    if (data_off && data_bytes > 0 && !data) return fail(c, SW_EINVAL, "%s: %lld data bytes and a NULL buffer", what, (long long)data_bytes);
    return SW_OK;
}

// the store call behind the argument checks: every array in device memory and visible to the context's stream
int data_set_body(sw_ctx* c, int64_t K, const uint8_t* d_data, const int64_t* d_off, int64_t data_bytes, const uint8_t* d_none, const char* what) {
    DataPlan p{};
    CHK(data_scratch(c, K, 0, 0, &p));
    const dat::SegIn in{d_data, (const dat::i64*)d_off, d_none, nullptr, (dat::i64)K, (dat::i64)data_bytes, 0};
    int64_t total = 0, bad = 0;
    CHK(data_plan(c, K, in, p, &total, &bad));
    if (bad) return fail(c, SW_EINVAL, "%s: %lld events with offsets that are negative, decreasing, beyond the %lld data bytes, or a length above %d (nothing stored)",
                         what, (long long)bad, (long long)data_bytes, dat::MAX_DATA);
    if (total < 0 || total > data_bytes) return fail(c, SW_EIO, "%s: %lld bytes from a buffer of %lld (internal error)", what, (long long)total, (long long)data_bytes);
    CHK(data_reserve(c, c->data.n_data + K, c->data.used + total));
    CHK(data_copy(c, K, in, p, total, c->data.d_arena.p, c->data.used, c->data.used, (int64_t*)c->data.d_off.p + c->data.n_data, c->data.d_none.p + c->data.n_data));
    c->data.n_data += K;
    c->data.used += total;
    c->data.store_calls++;
    return SW_OK;
}

int data_gather_args(sw_ctx* c, int64_t K, const void* event, int64_t cap, const void* data, const void* off, const void* none, int64_t* n_bytes, bool* query, const char* what) {
    if (!n_bytes) return fail(c, SW_EINVAL, "%s: n_bytes is NULL", what);
    *n_bytes = 0;
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (K < 0 || cap < 0) return fail(c, SW_EINVAL, "%s: negative count or capacity", what);
    if (K > 0x7fffffff) return fail(c, SW_ERANGE, "%s: more than 2^31 events", what);
    if (K > 0 && !event) return fail(c, SW_EINVAL, "%s: NULL event indices", what);
    *query = cap == 0 && !data && !off && !none;
    if (!*query && (!off || (K > 0 && !none) || (cap > 0 && !data))) return fail(c, SW_EINVAL, "%s: NULL output arrays (capacity %lld)", what, (long long)cap);
    if (K > 0 && c->data.n_data == 0) return fail(c, SW_ERANGE, "%s: no event has data (nothing written)", what);
    return SW_OK;
}

// the gather behind the argument checks, in two steps: lengths, scan and the refusals (one synchronisation) ...
int data_gather_plan(sw_ctx* c, int64_t K, const int32_t* d_event, int64_t cap, int64_t* n_bytes, DataPlan* p, dat::SegIn* in, const char* what) {
    CHK(data_scratch(c, K, 0, 0, p));
    *in = dat::SegIn{c->data.d_arena.p, (const dat::i64*)c->data.d_off.p, c->data.d_none.p, d_event, (dat::i64)c->data.n_data, (dat::i64)c->data.used, 1};
    int64_t total = 0, bad = 0;
    CHK(data_plan(c, K, *in, *p, &total, &bad));
    if (bad) return fail(c, SW_ERANGE, "%s: %lld indices outside the %lld events that have data (nothing written)", what, (long long)bad, (long long)c->data.n_data);
    *n_bytes = total;
    if (total > cap) return fail(c, SW_ERANGE, "%s: %lld bytes to gather, capacity %lld (nothing written)", what, (long long)total, (long long)cap);
    return SW_OK;
}
// ... and the copy into device arrays that hold *n_bytes bytes, K + 1 offsets and K flags
int data_gather_copy(sw_ctx* c, int64_t K, const DataPlan& p, const dat::SegIn& in, int64_t total, uint8_t* d_data, int64_t* d_off, uint8_t* d_none) {
    CHK(data_copy(c, K, in, p, total, d_data, 0, 0, d_off, d_none));
    c->data.gather_calls++;
    c->data.gather_bytes += total;
    return SW_OK;
}

int data_payload_args(sw_ctx* c, const void* data, const void* data_off, int64_t data_bytes, const void* data_none, const char* what) {
    if (c->data.n_data != c->N)
        return fail(c, SW_ENOTSUP, "%s: %lld of the %lld stored events have no data entry (sw_set_event_data first)", what, (long long)(c->N - c->data.n_data), (long long)c->N);
    if (data_bytes < 0) return fail(c, SW_EINVAL, "%s: negative data length", what);
    if (!data_off && (data || data_bytes || data_none)) return fail(c, SW_EINVAL, "%s: data needs its offsets (or none of data, offsets, length, flags)", what);
    if (data_off && data_bytes > 0 && !data) return fail(c, SW_EINVAL, "%s: %lld data bytes and a NULL buffer", what, (long long)data_bytes);
    return SW_OK;
}

// payload_core whose accepted events bring their data.  Everything that can be refused or can run out of memory in the
// ordinary case comes first; behind payload_core's commit a failure poisons the context.
int ingest_data_core(sw_ctx* c, int64_t K, const uint8_t* d_id32, const uint8_t* d_sp_id32, const uint8_t* d_op_id32, const uint8_t* d_arity,
                     const int32_t* d_creator, const uint8_t* d_ok, const double* d_t, const uint8_t* d_sig64, const uint8_t* d_data, const int64_t* d_off,
                     int64_t data_bytes, const uint8_t* d_none, hipStream_t us, int32_t* d_out, int64_t* n_stored) {
    const int64_t N0 = c->N;
    DataPlan p{};
    CHK(data_scratch(c, K, K, K, &p));
    CHK(data_reserve(c, N0 + K, c->data.used + data_bytes));
    UserStream bracket;   // (left by the destructor on a failure; a success has drained the stream)
    CHK(bracket.join(c, us));
    // an event whose data range cannot be used is not valid (-3): pack's d_encodable rule, folded into a copy of d_ok
    // The lengths of the ranges that stay ok are summed: ranges of a peer may overlap (offsets that jump back across a
    // rejected event), and the append could then outgrow the reservation behind the commit.  Such a payload is refused whole.
    dat::u64* d_sum = (dat::u64*)(p.off + K + 1);
    HIPCHK(c, hipMemsetAsync(d_sum, 0, sizeof(dat::u64), c->stream));
    hipLaunchKernelGGL(dat::k_data_fold_ok, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream, (dat::i64)K, d_ok, (const dat::i64*)d_off,
                       (dat::i64)data_bytes, p.ok, d_sum);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    unsigned long long usable = 0;
    HIPCHK(c, hipMemcpyAsync(&usable, d_sum, sizeof usable, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (usable > (unsigned long long)data_bytes)
        return fail(c, SW_EINVAL, "the usable data ranges of the payload hold %llu bytes, its buffer %lld: ranges overlap (nothing stored)", usable,
                    (long long)data_bytes);
    CHK(payload_core(c, K, d_id32, d_sp_id32, d_op_id32, d_arity, d_creator, p.ok, d_t, d_sig64, c->stream, d_out, n_stored));
    bracket.drained();   // (by payload_core, and again by after() below)
    const int64_t A = *n_stored;
    if (A == 0) return SW_OK;
    // ---- committed: the data of the new events, in dense order (slot r = the payload position of the event with index N0 + r)
    const auto after = [&]() -> int {
        HIPCHK(c, hipMemsetAsync(p.slot, 0x7f, (size_t)A * sizeof(int32_t), c->stream));
        hipLaunchKernelGGL(dat::k_data_slots, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream, (dat::i64)K, (const int*)d_out, (int)N0, (dat::i64)A, p.slot);
        c->ctr.kernel_launches++;
        const dat::SegIn in{d_data, (const dat::i64*)d_off, d_none, p.slot, (dat::i64)K, (dat::i64)data_bytes, 0};
        int64_t total = 0, bad = 0;
        CHK(data_plan(c, A, in, p, &total, &bad));
        if (bad || total < 0 || total > data_bytes)   // (the stored events' ranges are among the usable ones, summed above)
            return fail(c, SW_EIO, "data of the accepted events: %lld bad slots, %lld bytes of %lld (internal error)", (long long)bad, (long long)total, (long long)data_bytes);
        CHK(data_copy(c, A, in, p, total, c->data.d_arena.p, c->data.used, c->data.used, (int64_t*)c->data.d_off.p + N0, c->data.d_none.p + N0));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // the copy has read the caller's arrays: on return they may be reused or freed
        c->data.n_data = N0 + A;
        c->data.used += total;
        c->data.store_calls++;
        return SW_OK;
    };
    const int rc = after();
    if (rc != SW_OK) c->poisoned = true;
    return rc;
}

}  // namespace

extern "C" {

int sw_set_event_data_device(sw_ctx* c, int64_t first, int64_t K, const uint8_t* d_data, const int64_t* d_data_off, int64_t data_bytes,
                             const uint8_t* d_data_none, void* user_stream) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_set_event_data_device";
    CHK(data_set_args(c, first, K, d_data, d_data_off, data_bytes, d_data_none, what));
    if (K == 0) return ((uintptr_t)d_data_off & 7) ? misaligned(c, what, 8) : SW_OK;   // (asked for K = 0 too)
    const size_t k = (size_t)K;
    CHK(device_args(c, what, {{d_data_off, (k + 1) * 8, 8}, {d_data, (size_t)data_bytes, 1}, {d_data_none, k, 1}}));
    UserStream bracket;
    CHK(bracket.join(c, (hipStream_t)user_stream));
    CHK(data_set_body(c, K, d_data, d_data_off, data_bytes, d_data_none, what));
    return bracket.leave();   // the caller may reuse its arrays behind this
}

int sw_set_event_data(sw_ctx* c, int64_t first, int64_t K, const uint8_t* data, const int64_t* data_off, int64_t data_bytes, const uint8_t* data_none) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_set_event_data";
    CHK(data_set_args(c, first, K, data, data_off, data_bytes, data_none, what));
    if (K == 0) return SW_OK;
    if (data_off)
        for (int64_t i = 0; i < K; ++i) {
            const int64_t a = data_off[i], b = data_off[i + 1];
            if (a < 0 || b < a || b > data_bytes || b - a > dat::MAX_DATA)
                return fail(c, SW_EINVAL, "%s: event %lld has the data range [%lld, %lld) of %lld bytes (at most %d each; nothing stored)", what,
                            (long long)(first + i), (long long)a, (long long)b, (long long)data_bytes, dat::MAX_DATA);
        }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t k = (size_t)K;
    Stage st;
    const size_t o_off = st.in(data_off, (k + 1) * 8), o_d = st.in(data, (size_t)data_bytes), o_n = st.in(data_none, k);
    unsigned char* B = nullptr;
    CHK(stage_up(c, c->data.d_in, st, &B));
    return data_set_body(c, K, data_off ? B + o_d : nullptr, data_off ? (const int64_t*)(B + o_off) : nullptr, data_bytes, data_none ? B + o_n : nullptr, what);
}

int sw_get_event_data(sw_ctx* c, int64_t first, int64_t K, int64_t cap, uint8_t* data, int64_t* data_off, uint8_t* data_none, int64_t* n_bytes) {
    if (!c) return SW_EINVAL;
    if (!n_bytes) return fail(c, SW_EINVAL, "sw_get_event_data: n_bytes is NULL");
    *n_bytes = 0;
    if (first < 0 || K < 0 || first + K > c->data.n_data)
        return fail(c, SW_ERANGE, "events [%lld, %lld) beyond the %lld events that have data", (long long)first, (long long)(first + K), (long long)c->data.n_data);
    if (cap < 0) return fail(c, SW_EINVAL, "sw_get_event_data: negative capacity");
    if (K == 0) { if (data_off) data_off[0] = 0; return SW_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int64_t> off((size_t)K + 1);
    HIPCHK(c, hipMemcpyAsync(off.data(), c->data.d_off.p + first, ((size_t)K + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t a = off[0], bytes = off[(size_t)K] - a;
    if (a < 0 || bytes < 0 || off[(size_t)K] > c->data.used) return fail(c, SW_EIO, "sw_get_event_data: stored offsets [%lld, %lld) (internal error)", (long long)a, (long long)off[(size_t)K]);
    *n_bytes = bytes;
    if (bytes > cap) return fail(c, SW_ERANGE, "sw_get_event_data: %lld bytes, capacity %lld (nothing written)", (long long)bytes, (long long)cap);
    if (!data_off || !data_none || (bytes > 0 && !data)) return fail(c, SW_EINVAL, "sw_get_event_data: NULL output arrays");
    if (bytes) HIPCHK(c, hipMemcpyAsync(data, c->data.d_arena.p + a, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(data_none, c->data.d_none.p + first, (size_t)K, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i <= K; ++i) data_off[i] = off[(size_t)i] - a;
    return SW_OK;
}

int sw_gather_event_data_device(sw_ctx* c, int64_t K, const int32_t* d_event, int64_t cap, uint8_t* d_data, int64_t* d_data_off, uint8_t* d_data_none,
                                void* user_stream, int64_t* n_bytes) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_gather_event_data_device";
    bool query = false;
    CHK(data_gather_args(c, K, d_event, cap, d_data, d_data_off, d_data_none, n_bytes, &query, what));
    // (empty rows are skipped: the alignment of a data buffer of capacity 0 and of the indices of no event is asked for all the same)
    if (cap == 0 && ((uintptr_t)d_data & 15)) return misaligned(c, what, 16);
    if (K == 0 && ((uintptr_t)d_event & 3)) return misaligned(c, what, 4);
    const size_t k = (size_t)K;
    CHK(device_args(c, what, {{d_data, (size_t)cap, 16}, {d_data_off, (k + 1) * 8, 8}, {d_event, k * 4, 4}, {d_data_none, k, 1}}));
    UserStream bracket;   // the producer of d_event; earlier readers of the outputs
    CHK(bracket.join(c, (hipStream_t)user_stream));
    DataPlan p{};
    dat::SegIn in{};
    CHK(data_gather_plan(c, K, d_event, cap, n_bytes, &p, &in, what));
    if (!query) CHK(data_gather_copy(c, K, p, in, *n_bytes, d_data, d_data_off, d_data_none));
    return bracket.leave();   // whatever the caller enqueues next reads complete arrays
}

int sw_gather_event_data(sw_ctx* c, int64_t K, const int32_t* event, int64_t cap, uint8_t* data, int64_t* data_off, uint8_t* data_none, int64_t* n_bytes) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_gather_event_data";
    bool query = false;
    CHK(data_gather_args(c, K, event, cap, data, data_off, data_none, n_bytes, &query, what));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t k = (size_t)K;
    Stage si;
    si.in(event, k * 4);
    unsigned char* E = nullptr;
    CHK(stage_up(c, c->data.d_in, si, &E));
    DataPlan p{};
    dat::SegIn in{};
    CHK(data_gather_plan(c, K, (const int32_t*)E, cap, n_bytes, &p, &in, what));
    if (query) return SW_OK;
    Stage st;   // the outputs, sized from the total (not from the caller's capacity)
    const size_t o_off = st.out(data_off, (k + 1) * 8), o_n = st.out(data_none, k), o_d = st.out(data, (size_t)*n_bytes + 16, (size_t)*n_bytes);
    unsigned char* B = nullptr;
    CHK(stage_up(c, c->data.d_out, st, &B));
    CHK(data_gather_copy(c, K, p, in, *n_bytes, B + o_d, (int64_t*)(B + o_off), B + o_n));
    return stage_down(c, st, B);
}

int sw_ingest_payload_data_device(sw_ctx* c, int64_t K, const uint8_t* d_id32, const uint8_t* d_sp_id32, const uint8_t* d_op_id32, const uint8_t* d_arity,
                                  const int32_t* d_creator, const uint8_t* d_ok, const double* d_t, const uint8_t* d_sig64, void* user_stream,
                                  int32_t* d_index_out, int64_t* n_stored, const uint8_t* d_data, const int64_t* d_data_off, int64_t data_bytes,
                                  const uint8_t* d_data_none) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_ingest_payload_data_device";
    CHK(payload_args(c, K, d_id32, d_sp_id32, d_op_id32, d_arity, d_creator, d_index_out, n_stored, what));
    CHK(data_payload_args(c, d_data, d_data_off, data_bytes, d_data_none, what));
    if (K == 0) return SW_OK;
    const size_t k = (size_t)K;
    CHK(device_args(c, what, {{d_id32, k * 32, 8}, {d_sp_id32, k * 32, 8}, {d_op_id32, k * 32, 8}, {d_data_off, (k + 1) * 8, 8}, {d_arity, k, 1}, {d_creator, k * 4, 1},
                              {d_index_out, k * 4, 1}, {d_ok, k, 1}, {d_t, k * 8, 1}, {d_sig64, k * 64, 1}, {d_data, (size_t)data_bytes, 1}, {d_data_none, k, 1}}));
    return ingest_data_core(c, K, d_id32, d_sp_id32, d_op_id32, d_arity, d_creator, d_ok, d_t, d_sig64, d_data, d_data_off, data_bytes, d_data_none,
                            (hipStream_t)user_stream, d_index_out, n_stored);
}

int sw_ingest_payload_data(sw_ctx* c, int64_t K, const uint8_t* id32, const uint8_t* sp_id32, const uint8_t* op_id32, const uint8_t* arity,
                           const int32_t* creator, const uint8_t* ok, const double* t, const uint8_t* sig64, int32_t* index_out, int64_t* n_stored,
                           const uint8_t* data, const int64_t* data_off, int64_t data_bytes, const uint8_t* data_none) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_ingest_payload_data";
    CHK(payload_args(c, K, id32, sp_id32, op_id32, arity, creator, index_out, n_stored, what));
    CHK(data_payload_args(c, data, data_off, data_bytes, data_none, what));
    if (K == 0) return SW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t k = (size_t)K;
    Stage st;
    const size_t o_id = st.in(id32, k * 32), o_sp = st.in(sp_id32, k * 32), o_op = st.in(op_id32, k * 32), o_ar = st.in(arity, k), o_cr = st.in(creator, k * 4);
    const size_t o_ok = st.in(ok, k), o_t = st.in(t, k * 8), o_sig = st.in(sig64, k * 64), o_out = st.out(index_out, k * 4);
    const size_t o_doff = st.in(data_off, (k + 1) * 8), o_d = st.in(data, (size_t)data_bytes), o_dn = st.in(data_none, k);
    unsigned char* B = nullptr;
    CHK(stage_up(c, c->data.d_in, st, &B));
    CHK(ingest_data_core(c, K, B + o_id, B + o_sp, B + o_op, B + o_ar, (const int32_t*)(B + o_cr), ok ? B + o_ok : nullptr,
                         t ? (const double*)(B + o_t) : nullptr, sig64 ? B + o_sig : nullptr, data_off ? B + o_d : nullptr,
                         data_off ? (const int64_t*)(B + o_doff) : nullptr, data_bytes, data_none ? B + o_dn : nullptr, c->stream,
                         (int32_t*)(B + o_out), n_stored));
    return stage_down(c, st, B);
}

}  // extern "C"
namespace {

// ---- the parts sw_sync_pull, sw_sync_pull_validated, sw_sync_pull_data and sw_sync_pull_walk share --------------------------
// what they ask of the pulling context, and of the pair
int pull_pre(sw_ctx* dst, int64_t dst_head, sw_ctx* src, bool validate, bool data, const char* what) {
    if (dst == src) return fail(dst, SW_EINVAL, "%s: a context cannot pull from itself", what);
    if (dst->device != src->device) return fail(dst, SW_ENOTSUP, "%s: the contexts live on devices %d and %d (same device only)", what, dst->device, src->device);
    if (dst->n != src->n) return fail(dst, SW_EINVAL, "%s: %d members here, %d at the peer", what, dst->n, src->n);
    if (dst->poisoned) return fail(dst, SW_EIO, "context unusable after an earlier device failure");
    if (validate && dst->val.keys.empty()) return fail(dst, SW_ENOTSUP, "%s: no member keys (sw_set_member_keys first)", what);
    if (dst->ids.n_ids != dst->N)
        return fail(dst, SW_ENOTSUP, "%s: %lld of the %lld stored events have no id (sw_set_event_ids first)", what, (long long)(dst->N - dst->ids.n_ids), (long long)dst->N);
    if (data && dst->data.n_data != dst->N)
        return fail(dst, SW_ENOTSUP, "%s: %lld of the %lld stored events have no data entry (sw_set_event_data first)", what, (long long)(dst->N - dst->data.n_data), (long long)dst->N);
    if (dst_head < dst->first_resident || dst_head >= dst->divided) return fail(dst, SW_ERANGE, "%s: head %lld is not a divided, resident event", what, (long long)dst_head);
    return SW_OK;
}

// behind the checks of the answering context: what dst knows at its head (swirld.py:125-126), left in its own scratch
// (dst->d_q); src's stream waits for it
int pull_begin(sw_ctx* dst, int64_t dst_head, sw_ctx* src, bool validate, bool data, const char* what) {
    if (data && src->data.n_data != src->N)
        return fail(dst, SW_ENOTSUP, "%s: %lld of the peer's %lld stored events have no data entry (sw_set_event_data first)", what, (long long)(src->N - src->data.n_data), (long long)src->N);
    HIPCHK(dst, hipSetDevice(dst->device));
    if (validate && !dst->pack.h_cnt.reserve(1)) return fail(dst, SW_ENOMEM, "hipHostMalloc for the count of valid events failed");
    CHK(heights_on_device(dst));
    const int np = dst->npad;
    CHK(dgrow(dst, dst->d_q, (size_t)3 * np, 0));
    CHK(ensure_event(dst, dst->ev_user));
    hipLaunchKernelGGL(k_known_heights, dim3(1), dim3(np), 0, dst->stream, (const int*)dst->d_L.p, (const int*)dst->d_ht.p, (int)dst_head, np, dst->d_q.p);
    dst->ctr.kernel_launches++;
    HIPCHK(dst, hipGetLastError());
    // (not a UserStream: no caller's stream here.  The PEER's stream is put behind ours, one way, and the answer comes back
    // through ingest_arrays, which puts ours behind the peer's and drains it)
    HIPCHK(dst, hipEventRecord(dst->ev_user, dst->stream));
    HIPCHK(dst, hipStreamWaitEvent(src->stream, dst->ev_user, 0));
    return SW_OK;
}

// src answers with the chain ranges of k_sync_diff: ranges, count (its one synchronisation: dst's heights have been consumed
// by then), gather into its own scratch
int pull_ranges(sw_ctx* dst, sw_ctx* src, int64_t src_head, bool with_event, const char* what, int64_t* total_out, ExportArrays* d) {
    const bool prof = src->profiling;
    auto t0 = std::chrono::steady_clock::now();
    int64_t total = 0;
    if (const int rc = export_ranges(src, src_head, dst->d_q.p, hipMemcpyDeviceToDevice, &total); rc != SW_OK) { dst->err = src->err; return rc; }
    src->xp.ms[0] = prof ? ms_since(t0) : 0;
    src->xp.ms[1] = 0;
    if (total > 0x3fffffffll || dst->N + total > 0x7ffffff0ll) return fail(dst, SW_ERANGE, "%s: more than 2^31 events", what);
    t0 = std::chrono::steady_clock::now();
    int rc = export_scratch(src, total, true, true, with_event, d);
    if (rc == SW_OK) rc = export_gather(src, total, *d);
    if (rc != SW_OK) { dst->err = src->err; return rc; }
    if (prof) { HIPCHK(src, hipStreamSynchronize(src->stream)); src->xp.ms[1] = ms_since(t0); }
    src->xp.calls++;
    src->xp.events += total;
    *total_out = total;
    return SW_OK;
}

// `total` events in device arrays written on stream `from` (the peer's, or dst's own), with or without data arrays:
//   validate  dst, its stream ordered behind `from`, builds the signed bytes (with the data, or with data None), judges them by
//             its OWN keys and event class, ANDs the verdicts with the encodable flags and counts them
//   then      dst ingests what is valid (Node.sync's loop, swirld.py:130-136), keeping the data when `store_data`; the dense
//             indices are left in dst->ids.d_pl_in.  dst's stream is drained before the call returns.
int ingest_arrays(sw_ctx* dst, hipStream_t from, int64_t total, const ExportArrays& d, const uint8_t* x_data, const int64_t* x_off, int64_t dbytes,
                  const uint8_t* x_none, bool validate, bool store_data, int64_t* n_valid, int64_t* n_stored) {
    const size_t k = (size_t)total;
    int rc = SW_OK;
    CHK(dgrow(dst, dst->ids.d_pl_in, k * sizeof(int32_t), 0));
    const uint8_t* ok = nullptr;
    if (validate) {
        int64_t bm = 0, bw = 0;
        pack_bound(dst, total, dbytes, &bm, &bw);
        Carve cv;
        const size_t o_moff = cv.take((k + 1) * 8), o_woff = cv.take((k + 1) * 8), o_m = cv.take((size_t)bm), o_w = cv.take((size_t)bw);
        const size_t o_enc = cv.take(k), o_ok = cv.take(k), o_cnt = cv.take(sizeof(int32_t));
        CHK(dgrow(dst, dst->pack.d_out, cv.off + 256, 0));
        unsigned char* B = dst->pack.d_out.p;
        // (not a UserStream: `from` is the peer's stream or our own, and nothing is handed back to it: our stream is drained
        // before the call returns, which is what frees the peer's scratch)
        HIPCHK(dst, hipEventRecord(dst->ev_user, from));
        HIPCHK(dst, hipStreamWaitEvent(dst->stream, dst->ev_user, 0));
        HIPCHK(dst, hipMemsetAsync(B + o_cnt, 0, sizeof(int32_t), dst->stream));
        rc = pack_launch(dst, total, PackArrays{d.sp_id, d.op_id, d.arity, d.creator, d.t, d.sig, x_data, x_off, dbytes, x_none, B + o_m, (int64_t*)(B + o_moff),
                                                B + o_w, (int64_t*)(B + o_woff), B + o_enc}, bm, bw);
        if (rc == SW_OK) {
            const swv::Payload p{B + o_m, (const long long*)(B + o_moff), (long long)bm, B + o_w, (const long long*)(B + o_woff), (long long)bw, d.sig, d.creator, d.id};
            rc = validate_launch(dst, total, p, B + o_ok);
        }
        if (rc != SW_OK) { (void)hipStreamSynchronize(dst->stream); return rc; }   // (src's scratch is free again only once dst has read it)
        dst->val.calls++;
        dst->val.events += total;
        hipLaunchKernelGGL(pck::k_pack_and_count, dim3((unsigned)std::min<int64_t>(1024, (total + 255) / 256)), dim3(256), 0, dst->stream, (pck::i64)total,
                           B + o_ok, (const unsigned char*)(B + o_enc), (int*)(B + o_cnt));
        dst->ctr.kernel_launches++;
        HIPCHK(dst, hipGetLastError());
        HIPCHK(dst, hipMemcpyAsync(dst->pack.h_cnt.p, B + o_cnt, sizeof(int32_t), hipMemcpyDeviceToHost, dst->stream));
        ok = B + o_ok;
    }
    int64_t stored = 0;
    if (store_data)
        rc = ingest_data_core(dst, total, d.id, d.sp_id, d.op_id, d.arity, d.creator, ok, d.t, d.sig, x_data, x_off, dbytes, x_none, from,
                              (int32_t*)dst->ids.d_pl_in.p, &stored);
    else
        rc = payload_core(dst, total, d.id, d.sp_id, d.op_id, d.arity, d.creator, ok, d.t, d.sig, from, (int32_t*)dst->ids.d_pl_in.p, &stored);
    const hipError_t drained = hipStreamSynchronize(dst->stream);   // src's scratch is free again only once dst has read it
    if (rc != SW_OK) return rc;
    HIPCHK(dst, drained);
    if (validate && n_valid) *n_valid = *dst->pack.h_cnt.p;
    if (n_stored) *n_stored = stored;
    return SW_OK;
}

// behind src's export of `total` events into `d` (its scratch, written on its stream):
//   data      src gathers the data of those events beside the other arrays (its second synchronisation: the byte total)
//   validate  dst, its stream ordered behind src's, builds the signed bytes (with the data, or with data None), judges them by
//             its OWN keys and event class, ANDs the verdicts with the encodable flags and counts them
//   then      dst ingests what is valid (Node.sync's loop, swirld.py:130-136), on the exact path through the host append
int pull_finish(sw_ctx* dst, sw_ctx* src, int64_t total, const ExportArrays& d, bool validate, bool data, const char* what, int64_t* n_valid,
                int64_t* n_stored) {
    const size_t k = (size_t)total;
    int rc = SW_OK;
    int64_t dbytes = 0;
    const uint8_t* x_data = nullptr;
    const int64_t* x_off = nullptr;
    const uint8_t* x_none = nullptr;
    if (data) {
        DataPlan sp{};
        int64_t bad = 0;
        const dat::SegIn sin{src->data.d_arena.p, (const dat::i64*)src->data.d_off.p, src->data.d_none.p, d.event, (dat::i64)src->data.n_data, (dat::i64)src->data.used, 1};
        rc = data_scratch(src, total, 0, 0, &sp);
        if (rc == SW_OK) rc = data_plan(src, total, sin, sp, &dbytes, &bad);
        if (rc == SW_OK && bad) rc = fail(src, SW_EIO, "%s: %lld exported events without data (internal error)", what, (long long)bad);
        Carve sv;
        const size_t s_d = sv.take((size_t)dbytes + 16), s_off = sv.take((k + 1) * 8), s_n = sv.take(k);
        if (rc == SW_OK) rc = dgrow(src, src->data.d_out, sv.off + 256, 0);
        unsigned char* S = src->data.d_out.p;
        if (rc == SW_OK) rc = data_copy(src, total, sin, sp, dbytes, S + s_d, 0, 0, (int64_t*)(S + s_off), S + s_n);
        if (rc != SW_OK) { dst->err = src->err; return rc; }
        src->data.gather_calls++;
        src->data.gather_bytes += dbytes;
        x_data = S + s_d;
        x_off = (const int64_t*)(S + s_off);
        x_none = S + s_n;
    }
    return ingest_arrays(dst, src->stream, total, d, x_data, x_off, dbytes, x_none, validate, data, n_valid, n_stored);
}

// ---- answering a sync by the pruned walk (walk.hip.h) ------------------------------------------------------
// what every walk call asks of the answering context: either path, but every can_see row resident
int walk_pre(sw_ctx* c, int64_t head, bool need_ids, const char* what) {
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (c->vm.active) return fail(c, SW_ENOTSUP, "%s is not available with the windowed table", what);
    if (need_ids && c->ids.n_ids != c->N)
        return fail(c, SW_ENOTSUP, "%s: %lld of the %lld stored events have no id (sw_set_event_ids first)", what, (long long)(c->N - c->ids.n_ids), (long long)c->N);
    if (head < c->first_resident || head >= c->divided || head >= c->N)
        return fail(c, SW_ERANGE, "%s: head %lld is not a divided, resident event", what, (long long)head);
    return SW_OK;
}

// trunk[c] of every member as of the stored events, in walk.d_trunk, on the context's stream (asynchronous).  Recomputed only
// when events have arrived since.
int fork_trunks(sw_ctx* c) {
    const int np = c->npad;
    CHK(dgrow(c, c->walk.d_trunk, (size_t)2 * np, 0));
    if (c->walk.trunk_N == c->N) return SW_OK;
    CHK(heights_on_device(c));
    const int64_t N = c->N;
    if (N > 0) {
        CHK(dgrow(c, c->walk.d_children, (size_t)N, 0));
        HIPCHK(c, hipMemsetAsync(c->walk.d_children.p, 0, (size_t)N * sizeof(int32_t), c->stream));
    }
    HIPCHK(c, hipMemsetAsync(c->walk.d_trunk.p + np, 0, (size_t)np * sizeof(int32_t), c->stream));
    CHK(fill_i32(c, c->walk.d_trunk.p, (size_t)np, wlk::NO_CAP));
    if (N > 0) {
        const unsigned blocks = (unsigned)std::min<int64_t>(2048, (N + wlk::TRUNK_THREADS - 1) / wlk::TRUNK_THREADS);
        hipLaunchKernelGGL(wlk::k_fork_trunks, dim3(blocks), dim3(wlk::TRUNK_THREADS), 0, c->stream, (const int*)c->d_sp.p, (const int*)c->d_cr.p,
                           (const int*)c->d_ht.p, c->n, (long long)N, c->walk.d_children.p, c->walk.d_trunk.p + np, c->walk.d_trunk.p);
        c->ctr.kernel_launches++;
        HIPCHK(c, hipGetLastError());
    }
    c->walk.trunk_N = N;
    return SW_OK;
}

// k_walk_bfs, k_walk_list when the caller can take the events, and the header, on the context's stream; ONE synchronisation,
// for the count.  `known` and `cap` (n int32 each, either may be NULL) are copied with `kind`; they are compared with heights
// and never used as an index.  An error word from the walk poisons the context: its tables are not what they must be.
int walk_run(sw_ctx* c, int64_t head, const int32_t* known, const int32_t* cap, hipMemcpyKind kind, bool with_list, int64_t* total) {
    CHK(heights_on_device(c));
    const int np = c->npad, n = c->n;
    const size_t ev = (size_t)head + 1, words = (ev + 31) / 32;
    CHK(dgrow(c, c->walk.d, (size_t)wlk::H_WORDS + 2 * (size_t)np, 0));
    CHK(dgrow(c, c->walk.d_bits, words, 0));
    CHK(dgrow(c, c->walk.d_q, ev, 0));
    CHK(dgrow(c, c->walk.d_list, ev, 0));
    if (c->payload_pending) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_payload, 0));   // timestamps / signatures of a bulk host append
    int32_t* d_hdr = c->walk.d.p;
    int32_t* d_known = d_hdr + wlk::H_WORDS;
    int32_t* d_cap = d_known + np;
    HIPCHK(c, hipMemsetAsync(d_hdr, 0, wlk::H_WORDS * sizeof(int32_t), c->stream));
    if (known) HIPCHK(c, hipMemcpyAsync(d_known, known, (size_t)n * sizeof(int32_t), kind, c->stream));
    if (cap) HIPCHK(c, hipMemcpyAsync(d_cap, cap, (size_t)n * sizeof(int32_t), kind, c->stream));
    HIPCHK(c, hipMemsetAsync(c->walk.d_bits.p, 0, words * sizeof(unsigned), c->stream));
    const bool prof = c->profiling;
    auto t0 = std::chrono::steady_clock::now();
    const wlk::WalkIn in{c->d_sp.p, c->d_op.p, c->d_cr.p, c->d_ht.p, n, (int)head};
    const size_t lds = (size_t)(n + wlk::C_WORDS) * sizeof(int);
    hipLaunchKernelGGL(wlk::k_walk_bfs, dim3(1), dim3(c->walk.threads), lds, c->stream, in, known ? (const int*)d_known : nullptr,
                       cap ? (const int*)d_cap : nullptr, c->walk.d_bits.p, c->walk.d_q.p, d_hdr);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    c->walk.ms[0] = c->walk.ms[1] = c->walk.ms[2] = 0;
    if (prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->walk.ms[0] = ms_since(t0); t0 = std::chrono::steady_clock::now(); }
    if (with_list) {
        hipLaunchKernelGGL(wlk::k_walk_list, dim3(1), dim3(wlk::LIST_THREADS), 0, c->stream, (const unsigned*)c->walk.d_bits.p, (int)head, d_hdr, c->walk.d_list.p);
        c->ctr.kernel_launches++;
        HIPCHK(c, hipGetLastError());
    }
    int32_t hdr[wlk::H_WORDS] = {0};
    HIPCHK(c, hipMemcpyAsync(hdr, d_hdr, sizeof hdr, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (prof) c->walk.ms[with_list ? 1 : 0] += ms_since(t0);
    if (hdr[wlk::H_ERR] || hdr[wlk::H_COUNT] < 1 || hdr[wlk::H_COUNT] > head + 1) {
        c->poisoned = true;
        return fail(c, SW_EIO, "walk from head %lld: error %d after %d levels, %d events (a parent or creator table entry out of range, or the queue overran)",
                    (long long)head, hdr[wlk::H_ERR], hdr[wlk::H_LEVELS], hdr[wlk::H_COUNT]);
    }
    c->walk.levels = hdr[wlk::H_LEVELS];
    *total = hdr[wlk::H_COUNT];
    return SW_OK;
}

// the gather of `total` slots behind walk_run's list, on the context's stream (asynchronous)
int walk_gather(sw_ctx* c, int64_t total, const ExportArrays& o) {
    const gsp::ExportIn in{nullptr, nullptr, nullptr, c->d_sp.p, c->d_op.p, c->ids.d_id.p, c->d_sig.p, (const unsigned long long*)c->d_t.p};
    const gsp::ExportOut out{o.id, o.sp_id, o.op_id, o.arity, o.creator, (unsigned long long*)o.t, o.sig, o.event};
    const int G = c->xp.lanes;
    const dim3 grid((unsigned)std::min<int64_t>(2048, (total * G + wlk::GATHER_THREADS - 1) / wlk::GATHER_THREADS)), block(wlk::GATHER_THREADS);
    const int* list = c->walk.d_list.p;
    const int* cr = c->d_cr.p;
    if (G == 4) hipLaunchKernelGGL(wlk::k_walk_gather<4>, grid, block, 0, c->stream, in, out, list, cr, (int)total);
    else if (G == 8) hipLaunchKernelGGL(wlk::k_walk_gather<8>, grid, block, 0, c->stream, in, out, list, cr, (int)total);
    else hipLaunchKernelGGL(wlk::k_walk_gather<16>, grid, block, 0, c->stream, in, out, list, cr, (int)total);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    return SW_OK;
}

}  // namespace
extern "C" {

int sw_get_fork_trunks(sw_ctx* c, int32_t* trunk_out) {
    if (!c || !trunk_out) return SW_EINVAL;
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (c->vm.active) return fail(c, SW_ENOTSUP, "sw_get_fork_trunks is not available with the windowed table");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(fork_trunks(c));
    std::vector<int32_t> tmp(c->npad);
    HIPCHK(c, hipMemcpyAsync(tmp.data(), c->walk.d_trunk.p, (size_t)c->npad * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::copy(tmp.begin(), tmp.begin() + c->n, trunk_out);
    return SW_OK;
}

int sw_sync_walk(sw_ctx* c, int64_t head, const int32_t* known, const int32_t* cap, int64_t cap_events, int32_t* events_out, int64_t* n_out) {
    if (!c) return SW_EINVAL;
    if (!n_out) return fail(c, SW_EINVAL, "sw_sync_walk: n_out is NULL");
    *n_out = 0;
    CHK(walk_pre(c, head, false, "sw_sync_walk"));
    if (cap_events < 0 || (cap_events > 0 && !events_out)) return fail(c, SW_EINVAL, "sw_sync_walk: NULL output array (capacity %lld)", (long long)cap_events);
    HIPCHK(c, hipSetDevice(c->device));
    int64_t total = 0;
    CHK(walk_run(c, head, known, cap, hipMemcpyHostToDevice, cap_events > 0, &total));
    *n_out = total;
    if (total > cap_events) return fail(c, SW_ERANGE, "sw_sync_walk: %lld events, capacity %lld (nothing written)", (long long)total, (long long)cap_events);
    HIPCHK(c, hipMemcpyAsync(events_out, c->walk.d_list.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->walk.calls++;
    c->walk.events += total;
    return SW_OK;
}

int sw_export_walk_device(sw_ctx* c, int64_t head, const int32_t* d_known, const int32_t* d_cap, int64_t cap_events, uint8_t* d_id32, uint8_t* d_sp_id32,
                          uint8_t* d_op_id32, uint8_t* d_arity, int32_t* d_creator, double* d_t, uint8_t* d_sig64, int32_t* d_event, void* user_stream,
                          int64_t* n_out) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_export_walk_device";
    if (!n_out) return fail(c, SW_EINVAL, "%s: n_out is NULL", what);
    *n_out = 0;
    CHK(walk_pre(c, head, true, what));
    if (cap_events < 0 || (cap_events > 0 && (!d_id32 || !d_sp_id32 || !d_op_id32 || !d_arity || !d_creator)))
        return fail(c, SW_EINVAL, "%s: NULL output arrays (capacity %lld)", what, (long long)cap_events);
    // (with capacity 0 the rows are empty and skipped: the alignment of whatever was passed is asked for all the same)
    if (cap_events == 0 && (((uintptr_t)d_id32 | (uintptr_t)d_sp_id32 | (uintptr_t)d_op_id32 | (uintptr_t)d_sig64) & 15)) return misaligned(c, what, 16);
    const size_t k = (size_t)cap_events, nb = (size_t)c->n * sizeof(int32_t);
    CHK(device_args(c, what, {{d_id32, k * 32, 16}, {d_sp_id32, k * 32, 16}, {d_op_id32, k * 32, 16}, {d_sig64, k * 64, 16}, {d_known, nb, 1}, {d_cap, nb, 1},
                              {d_arity, k, 1}, {d_creator, k * 4, 1}, {d_t, k * 8, 1}, {d_event, k * 4, 1}}));
    UserStream bracket;   // the producers of d_known and d_cap; earlier readers of the output arrays
    CHK(bracket.join(c, (hipStream_t)user_stream));
    int64_t total = 0;
    CHK(walk_run(c, head, d_known, d_cap, hipMemcpyDeviceToDevice, cap_events > 0, &total));
    *n_out = total;
    if (total > cap_events) return fail(c, SW_ERANGE, "%s: %lld events to export, capacity %lld (nothing written)", what, (long long)total, (long long)cap_events);
    const auto t0 = std::chrono::steady_clock::now();
    CHK(walk_gather(c, total, ExportArrays{d_id32, d_sp_id32, d_op_id32, d_arity, d_creator, d_t, d_sig64, d_event}));
    CHK(bracket.leave());   // whatever the caller enqueues next reads complete arrays
    if (c->profiling) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->walk.ms[2] = ms_since(t0); }
    c->walk.calls++;
    c->walk.events += total;
    return SW_OK;
}

int sw_export_walk(sw_ctx* c, int64_t head, const int32_t* known, const int32_t* cap, int64_t cap_events, uint8_t* id32, uint8_t* sp_id32, uint8_t* op_id32,
                   uint8_t* arity, int32_t* creator, double* t, uint8_t* sig64, int32_t* event, int64_t* n_out) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_export_walk";
    if (!n_out) return fail(c, SW_EINVAL, "%s: n_out is NULL", what);
    *n_out = 0;
    CHK(walk_pre(c, head, true, what));
    if (cap_events < 0 || (cap_events > 0 && (!id32 || !sp_id32 || !op_id32 || !arity || !creator)))
        return fail(c, SW_EINVAL, "%s: NULL output arrays (capacity %lld)", what, (long long)cap_events);
    HIPCHK(c, hipSetDevice(c->device));
    int64_t total = 0;
    CHK(walk_run(c, head, known, cap, hipMemcpyHostToDevice, cap_events > 0, &total));
    *n_out = total;
    if (total > cap_events) return fail(c, SW_ERANGE, "%s: %lld events to export, capacity %lld (nothing written)", what, (long long)total, (long long)cap_events);
    const auto t0 = std::chrono::steady_clock::now();
    ExportArrays d{};
    Stage st;
    CHK(export_scratch(c, total, t != nullptr, sig64 != nullptr, event != nullptr, &d, &st, ExportArrays{id32, sp_id32, op_id32, arity, creator, t, sig64, event}));
    CHK(walk_gather(c, total, d));
    CHK(stage_down(c, st, c->xp.d_out.p));
    if (c->profiling) c->walk.ms[2] = ms_since(t0);
    c->walk.calls++;
    c->walk.events += total;
    return SW_OK;
}

int sw_sync_pull_walk(sw_ctx* dst, int64_t dst_head, sw_ctx* src, int64_t src_head, int use_trunks, int validate, int data, int64_t* n_sent,
                      int64_t* n_valid, int64_t* n_stored) {
    if (!dst || !src) return SW_EINVAL;
    const char* what = "sw_sync_pull_walk";
    if (n_sent) *n_sent = 0;
    if (n_valid) *n_valid = 0;
    if (n_stored) *n_stored = 0;
    CHK(pull_pre(dst, dst_head, src, validate != 0, data != 0, what));
    if (const int rc = walk_pre(src, src_head, true, "sw_sync_pull_walk (peer)"); rc != SW_OK) { dst->err = src->err; return rc; }
    // ---- 1. what dst knows at its head, as in sw_sync_pull
    CHK(pull_begin(dst, dst_head, src, validate != 0, data != 0, what));
    // ---- 2. src: the trunk heights of its forked members (the answerer applies the rule, as Node.ask_sync does), the walk
    // pruned at min(dst's heights, trunks), the count (its one synchronisation), list and gather into its own scratch
    int64_t total = 0;
    ExportArrays d{};
    int rc = use_trunks ? fork_trunks(src) : SW_OK;
    if (rc == SW_OK) rc = walk_run(src, src_head, dst->d_q.p, use_trunks ? src->walk.d_trunk.p : nullptr, hipMemcpyDeviceToDevice, true, &total);
    if (rc != SW_OK) { dst->err = src->err; return rc; }
    if (total > 0x3fffffffll || dst->N + total > 0x7ffffff0ll) return fail(dst, SW_ERANGE, "%s: more than 2^31 events", what);
    const auto t0 = std::chrono::steady_clock::now();
    rc = export_scratch(src, total, true, true, data != 0, &d);
    if (rc == SW_OK) rc = walk_gather(src, total, d);
    if (rc != SW_OK) { dst->err = src->err; return rc; }
    if (src->profiling) { HIPCHK(src, hipStreamSynchronize(src->stream)); src->walk.ms[2] = ms_since(t0); }
    src->walk.calls++;
    src->walk.events += total;
    if (n_sent) *n_sent = total;
    // ---- 3. the rest as in sw_sync_pull_data / sw_sync_pull_validated / sw_sync_pull
    return pull_finish(dst, src, total, d, validate != 0, data != 0, what, n_valid, n_stored);
}

int sw_get_walk_stats(sw_ctx* c, int64_t* calls, int64_t* events, int64_t* levels, double* phase_ms) {
    if (!c) return SW_EINVAL;
    if (calls) *calls = c->walk.calls;
    if (events) *events = c->walk.events;
    if (levels) *levels = c->walk.levels;
    if (phase_ms) for (int i = 0; i < 3; ++i) phase_ms[i] = c->walk.ms[i];
    return SW_OK;
}

int sw_sync_pull(sw_ctx* dst, int64_t dst_head, sw_ctx* src, int64_t src_head, int64_t* n_sent, int64_t* n_stored) {
    if (!dst || !src) return SW_EINVAL;
    if (n_sent) *n_sent = 0;
    if (n_stored) *n_stored = 0;
    const char* what = "sw_sync_pull";
    CHK(pull_pre(dst, dst_head, src, false, false, what));
    if (const int rc = export_pre(src, src_head, "sw_sync_pull (peer)"); rc != SW_OK) { dst->err = src->err; return rc; }
    // ---- 1. what dst knows at its head (swirld.py:125-126), left in its own scratch; src's stream waits for it
    CHK(pull_begin(dst, dst_head, src, false, false, what));
    // ---- 2. src: ranges, count (its one synchronisation: dst's heights have been consumed by then), gather into its own scratch
    int64_t total = 0;
    ExportArrays d{};
    CHK(pull_ranges(dst, src, src_head, false, what, &total, &d));
    if (n_sent) *n_sent = total;
    // ---- 3. dst ingests (Node.sync's loop, swirld.py:130-136), its stream ordered behind src's
    return pull_finish(dst, src, total, d, false, false, what, nullptr, n_stored);
}

int sw_sync_pull_validated(sw_ctx* dst, int64_t dst_head, sw_ctx* src, int64_t src_head, int64_t* n_sent, int64_t* n_valid, int64_t* n_stored) {
    if (!dst || !src) return SW_EINVAL;
    const char* what = "sw_sync_pull_validated";
    if (n_sent) *n_sent = 0;
    if (n_valid) *n_valid = 0;
    if (n_stored) *n_stored = 0;
    CHK(pull_pre(dst, dst_head, src, true, false, what));
    if (const int rc = export_pre(src, src_head, "sw_sync_pull_validated (peer)"); rc != SW_OK) { dst->err = src->err; return rc; }
    // ---- 1. and 2. as in sw_sync_pull: dst's known heights, src's ranges, count and gather
    CHK(pull_begin(dst, dst_head, src, true, false, what));
    int64_t total = 0;
    ExportArrays d{};
    CHK(pull_ranges(dst, src, src_head, false, what, &total, &d));
    if (n_sent) *n_sent = total;
    // ---- 3. and 4. dst, its stream ordered behind src's: the signed bytes (data None: the context stores no event data), the
    // verdicts by dst's OWN keys and event class, and the ingest of what is valid (Node.sync's loop, swirld.py:130-136)
    return pull_finish(dst, src, total, d, true, false, what, n_valid, n_stored);
}

int sw_sync_pull_data(sw_ctx* dst, int64_t dst_head, sw_ctx* src, int64_t src_head, int validate, int64_t* n_sent, int64_t* n_valid, int64_t* n_stored) {
    if (!dst || !src) return SW_EINVAL;
    const char* what = "sw_sync_pull_data";
    if (n_sent) *n_sent = 0;
    if (n_valid) *n_valid = 0;
    if (n_stored) *n_stored = 0;
    CHK(pull_pre(dst, dst_head, src, validate != 0, true, what));
    if (const int rc = export_pre(src, src_head, "sw_sync_pull_data (peer)"); rc != SW_OK) { dst->err = src->err; return rc; }
    // ---- 1. and 2. as in sw_sync_pull: dst's known heights, src's ranges, count and gather (with the dense indices)
    CHK(pull_begin(dst, dst_head, src, validate != 0, true, what));
    int64_t total = 0;
    ExportArrays d{};
    CHK(pull_ranges(dst, src, src_head, true, what, &total, &d));
    if (n_sent) *n_sent = total;
    // ---- 3. to 5.: src's data of those events, dst's verdicts on the signed bytes WITH the data, dst's ingest
    return pull_finish(dst, src, total, d, validate != 0, true, what, n_valid, n_stored);
}

int sw_get_data_stats(sw_ctx* c, int64_t* events, int64_t* bytes, int64_t* store_calls, int64_t* gather_calls, int64_t* gather_bytes, double* phase_ms) {
    if (!c) return SW_EINVAL;
    if (events) *events = c->data.n_data;
    if (bytes) *bytes = c->data.used;
    if (store_calls) *store_calls = c->data.store_calls;
    if (gather_calls) *gather_calls = c->data.gather_calls;
    if (gather_bytes) *gather_bytes = c->data.gather_bytes;
    if (phase_ms) for (int i = 0; i < 2; ++i) phase_ms[i] = c->data.ms[i];
    return SW_OK;
}

// ---- the wire bytes of a sync answer (wire.hip.h) -------------------------------------------------------
}  // extern "C"
namespace {

struct WireArrays {   // what the message writer reads, every array in device memory
    const uint8_t *head, *id, *sp_id, *op_id, *arity;
    const int32_t* creator;
    const double* t;
    const uint8_t *sig, *data;
    const int64_t* data_off;
    int64_t data_bytes;
    const uint8_t* data_none;
};

int wire_pre_len(const sw_ctx* c) { return (int)(c->pack.mod.size() + c->pack.qual.size() + 10); }
int64_t wire_base(const sw_ctx* c, int64_t K) { return (int64_t)wire_pre_len(c) + 8 + 8 * (K + 1) + wir::HEAD_PART; }
int64_t wire_bound(const sw_ctx* c, int64_t K, int64_t data_bytes) { return wire_base(c, K) + K * wir::REC_MAX + data_bytes + 3; }

struct WireSet { unsigned char* pre; unsigned char* skeys; int32_t* sperm; wir::i64* res; };
WireSet wire_set(const sw_ctx* c) {
    Carve cv;
    const size_t o_pre = cv.take(wir::PRE_MAX), o_keys = cv.take((size_t)c->n * 32), o_perm = cv.take((size_t)c->n * 4), o_res = cv.take(64);
    unsigned char* B = c->wire.d_set.p;
    return WireSet{B + o_pre, B + o_keys, (int32_t*)(B + o_perm), (wir::i64*)(B + o_res)};
}

// the prefix under the context's event class and the sorted key table, in device memory: rebuilt when either has changed
int wire_settings(sw_ctx* c) {
    CHK(dgrow(c, c->wire.d_set, (size_t)wir::PRE_MAX + (size_t)c->n * 36 + 4 * 256 + 64, 0));
    const WireSet ws = wire_set(c);
    const bool pre_stale = c->wire.mod != c->pack.mod || c->wire.qual != c->pack.qual, keys_stale = c->wire.keys != c->val.keys;
    if (!pre_stale && !keys_stale) return SW_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // an earlier call may still be reading the old settings, or copying them
    if (pre_stale) {
        std::vector<uint8_t>& h = c->wire.pre;
        h.assign({0x80, 0x04});
        for (const std::string* s : {&c->pack.mod, &c->pack.qual}) {
            h.push_back(0x8c);
            h.push_back((uint8_t)s->size());
            h.insert(h.end(), s->begin(), s->end());
        }
        for (const uint8_t b : {0x93, 0x94, 0x30, 0x8e}) h.push_back(b);
        HIPCHK(c, hipMemcpyAsync(ws.pre, h.data(), h.size(), hipMemcpyHostToDevice, c->stream));
        c->wire.mod = c->pack.mod;
        c->wire.qual = c->pack.qual;
    }
    if (keys_stale) {
        const int n = c->val.keys.empty() ? 0 : c->n;
        c->wire.skeys.assign((size_t)c->n * 32, 0);
        c->wire.sperm.assign((size_t)c->n, -1);
        if (n) {
            wir::sort_keys(c->val.keys.data(), n, c->wire.skeys.data(), c->wire.sperm.data());
            HIPCHK(c, hipMemcpyAsync(ws.skeys, c->wire.skeys.data(), (size_t)n * 32, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(ws.sperm, c->wire.sperm.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        }
        c->wire.keys = c->val.keys;
    }
    return SW_OK;
}

// pack.hip.h's scan of one stream of K lengths in place (off[K] = the total), on the context's stream
void wire_scan(sw_ctx* c, int64_t K, pck::i64* off, pck::i64* tsum) {
    const int64_t tiles = (K + pck::TILE - 1) / pck::TILE;
    if (tiles) hipLaunchKernelGGL(pck::k_pack_tile_sums, dim3((unsigned)tiles, 1), dim3(pck::SCAN_THREADS), 0, c->stream, (pck::i64)K, (pck::i64)tiles,
                                  (const pck::i64*)off, (const pck::i64*)off, tsum);
    hipLaunchKernelGGL(pck::k_pack_scan_sums, dim3(1), dim3(pck::SCAN_THREADS), 0, c->stream, (pck::i64)K, (pck::i64)tiles, off, off, tsum);
    if (tiles) hipLaunchKernelGGL(pck::k_pack_offsets, dim3((unsigned)tiles, 1), dim3(pck::SCAN_THREADS), 0, c->stream, (pck::i64)K, (pck::i64)tiles, off, off,
                                  (const pck::i64*)tsum);
    c->ctr.kernel_launches += tiles ? 3 : 1;
}

// the launches of the writer on the context's stream (asynchronous): d_msg holds `bound` = wire_bound(...) bytes at least,
// *d_msg_len receives the length or -1, *d_bad_out (may be NULL) the first unencodable event
int wire_pack_launch(sw_ctx* c, int64_t K, const WireArrays& a, uint8_t* d_msg, int64_t bound, int64_t* d_msg_len, unsigned long long** d_bad_out) {
    CHK(wire_settings(c));
    const int64_t tiles = (K + pck::TILE - 1) / pck::TILE;
    Carve cv;
    const size_t o_off = cv.take((size_t)(K + 1) * 8), o_ts = cv.take((size_t)(tiles + 1) * 8), o_bad = cv.take(8);
    CHK(dgrow(c, c->wire.d, cv.off + 256, 0));
    unsigned char* B = c->wire.d.p;
    pck::i64* off = (pck::i64*)(B + o_off);
    pck::u64* bad = (pck::u64*)(B + o_bad);
    const WireSet ws = wire_set(c);
    const wir::WireIn w{pck::PackIn{a.sp_id, a.op_id, a.arity, a.creator, (const pck::u64*)a.t, a.sig, a.data, (const pck::i64*)a.data_off, (pck::i64)a.data_bytes,
                                    a.data_none, (const unsigned char*)c->val.d_keys.p, ws.pre, wire_pre_len(c), c->n},
                        a.id, a.head};
    HIPCHK(c, hipMemsetAsync(bad, 0xff, 8, c->stream));
    if (K > 0) {
        hipLaunchKernelGGL(wir::k_wire_lengths, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream, w, (pck::i64)K, off, bad);
        c->ctr.kernel_launches++;
    }
    wire_scan(c, K, off, (pck::i64*)(B + o_ts));
    const int64_t chunks = (bound + 15) / 16;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(c->wire.blocks, (chunks + wir::WRITE_THREADS - 1) / wir::WRITE_THREADS));
    const int64_t trips = (chunks + blocks * wir::WRITE_THREADS - 1) / (blocks * wir::WRITE_THREADS);
    hipLaunchKernelGGL(wir::k_wire_write, dim3((unsigned)blocks), dim3(wir::WRITE_THREADS), 0, c->stream, w, (pck::i64)K, (const pck::i64*)off,
                       (pck::i64)wire_base(c, K), (const pck::u64*)bad, d_msg, (pck::i64*)d_msg_len, (pck::i64)trips);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    if (d_bad_out) *d_bad_out = bad;
    c->wire.pack_calls++;
    c->wire.pack_events += K;
    return SW_OK;
}

// what both forms of sw_pack_message check before anything else
int wire_pack_pre(sw_ctx* c, int64_t K, const WireArrays& a, const void* msg, const char* what) {
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (c->val.keys.empty()) return fail(c, SW_ENOTSUP, "%s: no member keys (sw_set_member_keys first)", what);
    if (K < 0 || a.data_bytes < 0) return fail(c, SW_EINVAL, "%s: negative count or length", what);
    if (K > 0x7fffffff) return fail(c, SW_ERANGE, "%s: more than 2^31 events", what);
    if (!a.head || !msg) return fail(c, SW_EINVAL, "%s: NULL head or message buffer", what);
    if (K > 0 && (!a.id || !a.sp_id || !a.op_id || !a.arity || !a.creator || !a.t || !a.sig)) return fail(c, SW_EINVAL, "%s: NULL arrays", what);
    if (!a.data_off && (a.data || a.data_bytes || a.data_none)) return fail(c, SW_EINVAL, "%s: data needs its offsets (or none of data, offsets, length, flags)", what);
    if (a.data_off && a.data_bytes > 0 && !a.data) return fail(c, SW_EINVAL, "%s: %lld data bytes and a NULL buffer", what, (long long)a.data_bytes);
    return SW_OK;
}

struct WireOut {      // what the reader writes, every array in device memory
    uint8_t *head, *id, *sp_id, *op_id, *arity;
    int32_t* creator;
    double* t;
    uint8_t *sig, *data;
    int64_t* data_off;
    uint8_t* data_none;
};

// the reader on the context's stream: TWO synchronisations, for K behind the header and for the verdict with the data bytes.
// *n_events: K, or -1 for a message that is not canonical; SW_ERANGE with the sizes that suffice when a capacity is too small.
int wire_unpack_run(sw_ctx* c, const uint8_t* d_msg, int64_t msg_bytes, int64_t cap_events, int64_t cap_data, const WireOut& o, int64_t* n_events,
                    int64_t* n_data, const char* what) {
    *n_events = -1;
    *n_data = 0;
    CHK(wire_settings(c));
    c->wire.unpack_calls++;
    const int pre_len = wire_pre_len(c);
    if (msg_bytes < pre_len + 8) { c->wire.refused++; return SW_OK; }
    const WireSet ws = wire_set(c);
    const wir::ReadIn in{d_msg, (wir::i64)msg_bytes, ws.pre, pre_len, ws.skeys, ws.sperm, c->val.keys.empty() ? 0 : c->n};
    hipLaunchKernelGGL(wir::k_wire_header, dim3(1), dim3(256), 0, c->stream, in, ws.res);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    long long K = -1;
    HIPCHK(c, hipMemcpyAsync(&K, ws.res, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (K < 0) { c->wire.refused++; return SW_OK; }
    if (K > cap_events) {
        *n_events = K;
        *n_data = msg_bytes - wire_base(c, K) - 3 - K * wir::REC_MIN;
        return fail(c, SW_ERANGE, "%s: %lld events in the message, capacity %lld (at most %lld data bytes; nothing written)", what, K, (long long)cap_events,
                    (long long)*n_data);
    }
    const int64_t tiles = (K + pck::TILE - 1) / pck::TILE;
    Carve cv;
    const size_t o_ts = cv.take((size_t)(tiles + 1) * 8), o_src = cv.take((size_t)K * 8);
    CHK(dgrow(c, c->wire.d, cv.off + 256, 0));
    unsigned char* B = c->wire.d.p;
    const wir::ReadOut ro{o.head, o.id, o.sp_id, o.op_id, o.arity, o.creator, (wir::u64*)o.t, o.sig, (wir::i64*)o.data_off, o.data_none, (wir::i64*)(B + o_src)};
    wir::i64* flag = ws.res + 1;
    hipLaunchKernelGGL(wir::k_wire_table, dim3((unsigned)((K + 256) / 256)), dim3(256), 0, c->stream, in, (wir::i64)K, o.head, flag);
    c->ctr.kernel_launches++;
    if (K > 0) {
        hipLaunchKernelGGL(wir::k_wire_records, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream, in, (wir::i64)K, ro, flag);
        c->ctr.kernel_launches++;
    }
    wire_scan(c, K, (pck::i64*)o.data_off, (pck::i64*)(B + o_ts));
    const int64_t chunks = (cap_data + 15) / 16;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(4096, (chunks + 255) / 256));
    hipLaunchKernelGGL(wir::k_wire_data, dim3((unsigned)blocks), dim3(256), 0, c->stream, d_msg, (wir::i64)K, ro, (wir::i64)cap_data, (const wir::i64*)flag, o.data,
                       ws.res + 2);
    c->ctr.kernel_launches++;
    HIPCHK(c, hipGetLastError());
    long long v[2] = {-1, 0};
    HIPCHK(c, hipMemcpyAsync(v, ws.res + 2, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (v[0] < 0) { c->wire.refused++; return SW_OK; }
    *n_events = K;
    *n_data = v[1];
    if (v[1] > cap_data) return fail(c, SW_ERANGE, "%s: %lld data bytes in the message, capacity %lld (no data written)", what, v[1], (long long)cap_data);
    c->wire.unpack_events += K;
    return SW_OK;
}

int wire_unpack_pre(sw_ctx* c, const void* msg, int64_t msg_bytes, int64_t cap_events, int64_t cap_data, const WireOut& o, const void* n_events,
                    const void* n_data, const char* what) {
    if (!n_events || !n_data) return fail(c, SW_EINVAL, "%s: n_events or n_data_bytes is NULL", what);
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (msg_bytes < 0 || cap_events < 0 || cap_data < 0) return fail(c, SW_EINVAL, "%s: negative length or capacity", what);
    if (cap_events > 0x7fffffff) return fail(c, SW_ERANGE, "%s: more than 2^31 events", what);
    if ((msg_bytes > 0 && !msg) || !o.head || !o.data_off) return fail(c, SW_EINVAL, "%s: NULL message, head or offsets", what);
    if (cap_events > 0 && (!o.id || !o.sp_id || !o.op_id || !o.arity || !o.creator || !o.t || !o.sig || !o.data_none)) return fail(c, SW_EINVAL, "%s: NULL output arrays", what);
    if (cap_data > 0 && !o.data) return fail(c, SW_EINVAL, "%s: NULL data buffer (capacity %lld)", what, (long long)cap_data);
    return SW_OK;
}

// walk, export, data gather and the message of sw_export_message, left in wire.d_out (*d_msg, *len bytes; *K events)
int wire_export_run(sw_ctx* c, int64_t head, const int32_t* known, const int32_t* cap, hipMemcpyKind kind, bool with_data, const char* what, uint8_t** d_msg,
                    int64_t* len, int64_t* n_events) {
    CHK(walk_pre(c, head, true, what));
    if (c->val.keys.empty()) return fail(c, SW_ENOTSUP, "%s: no member keys (sw_set_member_keys first)", what);
    if (with_data && c->data.n_data != c->N)
        return fail(c, SW_ENOTSUP, "%s: %lld of the %lld stored events have no data entry (sw_set_event_data first)", what, (long long)(c->N - c->data.n_data), (long long)c->N);
    int64_t total = 0;
    CHK(walk_run(c, head, known, cap, kind, true, &total));
    ExportArrays d{};
    CHK(export_scratch(c, total, true, true, true, &d));
    CHK(walk_gather(c, total, d));
    c->walk.calls++;
    c->walk.events += total;
    const size_t k = (size_t)total;
    int64_t dbytes = 0;
    const uint8_t* x_data = nullptr;
    const int64_t* x_off = nullptr;
    const uint8_t* x_none = nullptr;
    if (with_data) {
        DataPlan sp{};
        int64_t bad = 0;
        const dat::SegIn sin{c->data.d_arena.p, (const dat::i64*)c->data.d_off.p, c->data.d_none.p, d.event, (dat::i64)c->data.n_data, (dat::i64)c->data.used, 1};
        CHK(data_scratch(c, total, 0, 0, &sp));
        CHK(data_plan(c, total, sin, sp, &dbytes, &bad));
        if (bad) return fail(c, SW_EIO, "%s: %lld exported events without data (internal error)", what, (long long)bad);
        Carve sv;
        const size_t s_d = sv.take((size_t)dbytes + 16), s_off = sv.take((k + 1) * 8), s_n = sv.take(k);
        CHK(dgrow(c, c->data.d_out, sv.off + 256, 0));
        unsigned char* S = c->data.d_out.p;
        CHK(data_copy(c, total, sin, sp, dbytes, S + s_d, 0, 0, (int64_t*)(S + s_off), S + s_n));
        c->data.gather_calls++;
        c->data.gather_bytes += dbytes;
        x_data = S + s_d;
        x_off = (const int64_t*)(S + s_off);
        x_none = S + s_n;
    }
    const int64_t bound = wire_bound(c, total, dbytes);
    CHK(dgrow(c, c->wire.d_out, (size_t)bound + 256, 0));
    CHK(wire_settings(c));
    int64_t* d_len = (int64_t*)(wire_set(c).res + 4);
    CHK(wire_pack_launch(c, total, WireArrays{c->ids.d_id.p + (size_t)head * 32, d.id, d.sp_id, d.op_id, d.arity, d.creator, d.t, d.sig, x_data, x_off, dbytes, x_none},
                         c->wire.d_out.p, bound, d_len, nullptr));
    long long l = -1;
    HIPCHK(c, hipMemcpyAsync(&l, d_len, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (l < 0 || l > bound) return fail(c, SW_EIO, "%s: a stored event cannot be encoded (length %lld, bound %lld: internal error)", what, l, (long long)bound);
    c->wire.pack_bytes += l;
    *d_msg = c->wire.d_out.p;
    *len = l;
    *n_events = total;
    return SW_OK;
}

// unpack, validate and ingest of sw_ingest_message: d_msg in device memory, visible to the context's stream.  The head is left
// at *d_head, the dense indices in d_pl_in.
int wire_ingest_run(sw_ctx* c, const uint8_t* d_msg, int64_t msg_bytes, bool validate, bool with_data, const char* what, uint8_t** d_head, int64_t* n_events,
                    int64_t* n_valid, int64_t* n_stored) {
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (validate && c->val.keys.empty()) return fail(c, SW_ENOTSUP, "%s: no member keys (sw_set_member_keys first)", what);
    if (c->ids.n_ids != c->N)
        return fail(c, SW_ENOTSUP, "%s: %lld of the %lld stored events have no id (sw_set_event_ids first)", what, (long long)(c->N - c->ids.n_ids), (long long)c->N);
    if (with_data && c->data.n_data != c->N)
        return fail(c, SW_ENOTSUP, "%s: %lld of the %lld stored events have no data entry (sw_set_event_data first)", what, (long long)(c->N - c->data.n_data), (long long)c->N);
    if (validate && !c->pack.h_cnt.reserve(1)) return fail(c, SW_ENOMEM, "hipHostMalloc for the count of valid events failed");
    CHK(ensure_event(c, c->ev_user));
    const int64_t kcap = std::min<int64_t>(msg_bytes / wir::REC_MIN, 0x3fffffff), dcap = msg_bytes;
    const size_t k = (size_t)kcap;
    Carve cv;
    const size_t o_head = cv.take(32), o_id = cv.take(k * 32), o_sp = cv.take(k * 32), o_op = cv.take(k * 32), o_ar = cv.take(k), o_cr = cv.take(k * 4);
    const size_t o_t = cv.take(k * 8), o_sig = cv.take(k * 64), o_doff = cv.take((k + 1) * 8), o_dn = cv.take(k), o_d = cv.take((size_t)dcap + 16);
    CHK(dgrow(c, c->wire.d_out, cv.off + 256, 0));
    unsigned char* B = c->wire.d_out.p;
    const WireOut o{B + o_head, B + o_id, B + o_sp, B + o_op, B + o_ar, (int32_t*)(B + o_cr), (double*)(B + o_t), B + o_sig, B + o_d, (int64_t*)(B + o_doff), B + o_dn};
    int64_t K = -1, dbytes = 0;
    CHK(wire_unpack_run(c, d_msg, msg_bytes, kcap, dcap, o, &K, &dbytes, what));
    *n_events = K;
    *d_head = o.head;
    if (K < 0) return SW_OK;
    if (c->N + K > 0x7ffffff0ll) return fail(c, SW_ERANGE, "%s: more than 2^31 events", what);
    if (K == 0) return SW_OK;
    const ExportArrays d{o.id, o.sp_id, o.op_id, o.arity, o.creator, o.t, o.sig, nullptr};
    return ingest_arrays(c, c->stream, K, d, o.data, o.data_off, dbytes, o.data_none, validate, with_data, n_valid, n_stored);
}

}  // namespace
extern "C" {

int sw_pack_message_bound(sw_ctx* c, int64_t K, int64_t data_bytes, int64_t* msg_bytes) {
    if (!c) return SW_EINVAL;
    if (K < 0 || data_bytes < 0) return fail(c, SW_EINVAL, "sw_pack_message_bound: negative count or length");
    if (K > 0x7fffffff) return fail(c, SW_ERANGE, "sw_pack_message_bound: more than 2^31 events");
    if (msg_bytes) *msg_bytes = wire_bound(c, K, data_bytes);
    return SW_OK;
}

int sw_pack_message_device(sw_ctx* c, int64_t K, const uint8_t* d_head32, const uint8_t* d_id32, const uint8_t* d_sp_id32, const uint8_t* d_op_id32,
                           const uint8_t* d_arity, const int32_t* d_creator, const double* d_t, const uint8_t* d_sig64, const uint8_t* d_data,
                           const int64_t* d_data_off, int64_t data_bytes, const uint8_t* d_data_none, uint8_t* d_msg, int64_t msg_cap, int64_t* d_msg_len,
                           void* user_stream) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_pack_message_device";
    const WireArrays a{d_head32, d_id32, d_sp_id32, d_op_id32, d_arity, d_creator, d_t, d_sig64, d_data, d_data_off, data_bytes, d_data_none};
    CHK(wire_pack_pre(c, K, a, d_msg, what));
    if (!d_msg_len) return fail(c, SW_EINVAL, "%s: d_msg_len is NULL", what);
    const int64_t bound = wire_bound(c, K, data_bytes);
    if (msg_cap < bound) return fail(c, SW_ERANGE, "%s: capacity %lld below sw_pack_message_bound's %lld (nothing written)", what, (long long)msg_cap, (long long)bound);
    const size_t k = (size_t)K;
    if (K == 0) {   // (an empty message: the event arrays are empty rows; the alignment of whatever was passed is asked for all the same)
        if (((uintptr_t)d_sig64 | (uintptr_t)d_id32 | (uintptr_t)d_sp_id32 | (uintptr_t)d_op_id32) & 15) return misaligned(c, what, 16);
        if (((uintptr_t)d_data_off | (uintptr_t)d_t) & 7) return misaligned(c, what, 8);
        if ((uintptr_t)d_creator & 3) return misaligned(c, what, 4);
    }
    // (the message buffer holds the bound at least, which is never 0)
    CHK(device_args(c, what, {{d_msg, (size_t)msg_cap, 16}, {d_sig64, k * 64, 16}, {d_id32, k * 32, 16}, {d_sp_id32, k * 32, 16}, {d_op_id32, k * 32, 16},
                              {d_msg_len, 8, 8}, {d_data_off, K ? (k + 1) * 8 : 0, 8}, {d_t, k * 8, 8}, {d_creator, k * 4, 4}, {d_head32, 32, 1}, {d_arity, k, 1},
                              {d_data, K ? (size_t)data_bytes : 0, 1}, {d_data_none, k, 1}}));
    UserStream bracket;
    CHK(bracket.join(c, (hipStream_t)user_stream));
    CHK(wire_pack_launch(c, K, a, d_msg, bound, d_msg_len, nullptr));
    return bracket.leave();
}

int sw_pack_message(sw_ctx* c, int64_t K, const uint8_t* head32, const uint8_t* id32, const uint8_t* sp_id32, const uint8_t* op_id32, const uint8_t* arity,
                    const int32_t* creator, const double* t, const uint8_t* sig64, const uint8_t* data, const int64_t* data_off, int64_t data_bytes,
                    const uint8_t* data_none, uint8_t* msg, int64_t msg_cap, int64_t* msg_bytes) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_pack_message";
    if (!msg_bytes) return fail(c, SW_EINVAL, "%s: msg_bytes is NULL", what);
    *msg_bytes = 0;
    CHK(wire_pack_pre(c, K, WireArrays{head32, id32, sp_id32, op_id32, arity, creator, t, sig64, data, data_off, data_bytes, data_none}, msg, what));
    if (msg_cap < 0) return fail(c, SW_EINVAL, "%s: negative capacity", what);
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t bound = wire_bound(c, K, data_bytes);
    const size_t k = (size_t)K;
    Stage st;   // (the message comes back by the length the writer reports)
    const size_t o_head = st.in(head32, 32), o_id = st.in(id32, k * 32), o_sp = st.in(sp_id32, k * 32), o_op = st.in(op_id32, k * 32), o_ar = st.in(arity, k);
    const size_t o_cr = st.in(creator, k * 4), o_t = st.in(t, k * 8), o_sig = st.in(sig64, k * 64), o_doff = st.in(data_off, (k + 1) * 8);
    const size_t o_d = st.in(data, (size_t)data_bytes), o_dn = st.in(data_none, k), o_len = st.scratch(8), o_m = st.out(msg, (size_t)bound, 0);
    unsigned char* B = nullptr;
    CHK(stage_up(c, c->wire.d_in, st, &B));
    unsigned long long* d_bad = nullptr;
    CHK(wire_pack_launch(c, K, WireArrays{B + o_head, B + o_id, B + o_sp, B + o_op, B + o_ar, (const int32_t*)(B + o_cr), (const double*)(B + o_t), B + o_sig,
                                          data_off ? B + o_d : nullptr, data_off ? (const int64_t*)(B + o_doff) : nullptr, data_bytes,
                                          data_none ? B + o_dn : nullptr}, B + o_m, bound, (int64_t*)(B + o_len), &d_bad));
    long long len = -1;
    unsigned long long bad = 0;
    HIPCHK(c, hipMemcpyAsync(&len, B + o_len, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (len < 0)
        return fail(c, SW_EINVAL, "%s: event %llu cannot be encoded (arity not 0 or 2, creator outside the %d members, or a data range that is unusable or longer than %d): no message",
                    what, bad, c->n, wir::MAX_DATA);
    if (len > bound) return fail(c, SW_EIO, "%s: length %lld beyond the bound %lld (internal error)", what, len, (long long)bound);
    *msg_bytes = len;
    if (len > msg_cap) return fail(c, SW_ERANGE, "%s: the message has %lld bytes, capacity %lld (nothing written)", what, len, (long long)msg_cap);
    st.out_bytes(msg, (size_t)len);
    CHK(stage_down(c, st, B));
    c->wire.pack_bytes += len;
    return SW_OK;
}

int sw_unpack_message_device(sw_ctx* c, const uint8_t* d_msg, int64_t msg_bytes, int64_t cap_events, int64_t cap_data, uint8_t* d_head32, uint8_t* d_id32,
                             uint8_t* d_sp_id32, uint8_t* d_op_id32, uint8_t* d_arity, int32_t* d_creator, double* d_t, uint8_t* d_sig64, uint8_t* d_data,
                             int64_t* d_data_off, uint8_t* d_data_none, void* user_stream, int64_t* n_events, int64_t* n_data_bytes) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_unpack_message_device";
    const WireOut o{d_head32, d_id32, d_sp_id32, d_op_id32, d_arity, d_creator, d_t, d_sig64, d_data, d_data_off, d_data_none};
    CHK(wire_unpack_pre(c, d_msg, msg_bytes, cap_events, cap_data, o, n_events, n_data_bytes, what));
    *n_events = -1;
    *n_data_bytes = 0;
    // (empty rows are skipped: the alignment of a data buffer of capacity 0, and of the arrays of no event, is asked for all the same)
    if (cap_data == 0 && ((uintptr_t)d_data & 15)) return misaligned(c, what, 16);
    if (cap_events == 0 && ((uintptr_t)d_t & 7)) return misaligned(c, what, 8);
    if (cap_events == 0 && ((uintptr_t)d_creator & 3)) return misaligned(c, what, 4);
    const size_t k = (size_t)cap_events;
    CHK(device_args(c, what, {{d_data, (size_t)cap_data, 16}, {d_data_off, (k + 1) * 8, 8}, {d_t, k * 8, 8}, {d_creator, k * 4, 4}, {d_msg, (size_t)msg_bytes, 1},
                              {d_head32, 32, 1}, {d_id32, k * 32, 1}, {d_sp_id32, k * 32, 1}, {d_op_id32, k * 32, 1}, {d_arity, k, 1}, {d_sig64, k * 64, 1},
                              {d_data_none, k, 1}}));
    UserStream bracket;
    CHK(bracket.join(c, (hipStream_t)user_stream));
    CHK(wire_unpack_run(c, d_msg, msg_bytes, cap_events, cap_data, o, n_events, n_data_bytes, what));
    return bracket.leave();
}

int sw_unpack_message(sw_ctx* c, const uint8_t* msg, int64_t msg_bytes, int64_t cap_events, int64_t cap_data, uint8_t* head32, uint8_t* id32, uint8_t* sp_id32,
                      uint8_t* op_id32, uint8_t* arity, int32_t* creator, double* t, uint8_t* sig64, uint8_t* data, int64_t* data_off, uint8_t* data_none,
                      int64_t* n_events, int64_t* n_data_bytes) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_unpack_message";
    CHK(wire_unpack_pre(c, msg, msg_bytes, cap_events, cap_data, WireOut{head32, id32, sp_id32, op_id32, arity, creator, t, sig64, data, data_off, data_none},
                        n_events, n_data_bytes, what));
    *n_events = -1;
    *n_data_bytes = 0;
    HIPCHK(c, hipSetDevice(c->device));
    // no more events or data bytes than the message can hold need room on the device
    const int64_t ke = std::min<int64_t>(cap_events, msg_bytes / wir::REC_MIN), kd = std::min<int64_t>(cap_data, msg_bytes);
    const size_t k = (size_t)ke;
    Stage st;   // (every array comes back by the counts the reader reports)
    const size_t o_msg = st.in(msg, (size_t)msg_bytes), o_head = st.out(head32, 32, 0), o_id = st.out(id32, k * 32, 0), o_sp = st.out(sp_id32, k * 32, 0);
    const size_t o_op = st.out(op_id32, k * 32, 0), o_ar = st.out(arity, k, 0), o_cr = st.out(creator, k * 4, 0), o_t = st.out(t, k * 8, 0), o_sig = st.out(sig64, k * 64, 0);
    const size_t o_doff = st.out(data_off, (k + 1) * 8, 0), o_dn = st.out(data_none, k, 0), o_d = st.out(data, (size_t)kd + 16, 0);
    unsigned char* B = nullptr;
    CHK(stage_up(c, c->wire.d_in, st, &B));
    const WireOut o{B + o_head, B + o_id, B + o_sp, B + o_op, B + o_ar, (int32_t*)(B + o_cr), (double*)(B + o_t), B + o_sig, B + o_d, (int64_t*)(B + o_doff), B + o_dn};
    int64_t K = -1, nd = 0;
    const int rc = wire_unpack_run(c, B + o_msg, msg_bytes, ke, kd, o, &K, &nd, what);
    *n_events = K;
    *n_data_bytes = nd;
    if (rc != SW_OK || K < 0) return rc;
    const size_t kk = (size_t)K;
    st.out_bytes(head32, 32); st.out_bytes(id32, kk * 32); st.out_bytes(sp_id32, kk * 32); st.out_bytes(op_id32, kk * 32); st.out_bytes(arity, kk);
    st.out_bytes(creator, kk * 4); st.out_bytes(t, kk * 8); st.out_bytes(sig64, kk * 64); st.out_bytes(data_off, (kk + 1) * 8); st.out_bytes(data_none, kk);
    st.out_bytes(data, (size_t)nd);
    return stage_down(c, st, B);
}

int sw_export_message_device(sw_ctx* c, int64_t head_event, const int32_t* d_known, const int32_t* d_cap, int with_data, uint8_t* d_msg, int64_t msg_cap,
                             void* user_stream, int64_t* msg_bytes, int64_t* n_events) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_export_message_device";
    if (!msg_bytes || !n_events) return fail(c, SW_EINVAL, "%s: msg_bytes or n_events is NULL", what);
    *msg_bytes = *n_events = 0;
    if (msg_cap < 0 || (msg_cap > 0 && !d_msg)) return fail(c, SW_EINVAL, "%s: NULL message buffer (capacity %lld)", what, (long long)msg_cap);
    CHK(device_args(c, what, {{d_known, (size_t)c->n * 4, 1}, {d_cap, (size_t)c->n * 4, 1}, {d_msg, (size_t)msg_cap, 1}}));
    UserStream bracket;
    CHK(bracket.join(c, (hipStream_t)user_stream));
    uint8_t* m = nullptr;
    CHK(wire_export_run(c, head_event, d_known, d_cap, hipMemcpyDeviceToDevice, with_data != 0, what, &m, msg_bytes, n_events));
    if (*msg_bytes > msg_cap) return fail(c, SW_ERANGE, "%s: the message has %lld bytes, capacity %lld (nothing written)", what, (long long)*msg_bytes, (long long)msg_cap);
    HIPCHK(c, hipMemcpyAsync(d_msg, m, (size_t)*msg_bytes, hipMemcpyDeviceToDevice, c->stream));
    return bracket.leave();
}

int sw_export_message(sw_ctx* c, int64_t head_event, const int32_t* known, const int32_t* cap, int with_data, uint8_t* msg, int64_t msg_cap, int64_t* msg_bytes,
                      int64_t* n_events) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_export_message";
    if (!msg_bytes || !n_events) return fail(c, SW_EINVAL, "%s: msg_bytes or n_events is NULL", what);
    *msg_bytes = *n_events = 0;
    if (msg_cap < 0 || (msg_cap > 0 && !msg)) return fail(c, SW_EINVAL, "%s: NULL message buffer (capacity %lld)", what, (long long)msg_cap);
    HIPCHK(c, hipSetDevice(c->device));
    uint8_t* m = nullptr;
    CHK(wire_export_run(c, head_event, known, cap, hipMemcpyHostToDevice, with_data != 0, what, &m, msg_bytes, n_events));
    if (*msg_bytes > msg_cap) return fail(c, SW_ERANGE, "%s: the message has %lld bytes, capacity %lld (nothing written)", what, (long long)*msg_bytes, (long long)msg_cap);
    HIPCHK(c, hipMemcpyAsync(msg, m, (size_t)*msg_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

int sw_ingest_message_device(sw_ctx* c, const uint8_t* d_msg, int64_t msg_bytes, int validate, int with_data, uint8_t* d_head32_out, int32_t* d_index_out,
                             void* user_stream, int64_t* n_events, int64_t* n_valid, int64_t* n_stored) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_ingest_message_device";
    if (!n_events) return fail(c, SW_EINVAL, "%s: n_events is NULL", what);
    *n_events = -1;
    if (n_valid) *n_valid = 0;
    if (n_stored) *n_stored = 0;
    if (msg_bytes < 0 || (msg_bytes > 0 && !d_msg)) return fail(c, SW_EINVAL, "%s: NULL message (%lld bytes)", what, (long long)msg_bytes);
    const size_t kcap = (size_t)(msg_bytes / wir::REC_MIN);
    CHK(device_args(c, what, {{d_msg, (size_t)msg_bytes, 1}, {d_head32_out, 32, 1}, {d_index_out, kcap * 4, 1}}));
    UserStream bracket;
    CHK(bracket.join(c, (hipStream_t)user_stream));
    uint8_t* d_head = nullptr;
    CHK(wire_ingest_run(c, d_msg, msg_bytes, validate != 0, with_data != 0, what, &d_head, n_events, n_valid, n_stored));
    if (*n_events < 0) return bracket.leave();   // (a refused message: nothing is written, and the caller's stream is handed back)
    if (d_head32_out) HIPCHK(c, hipMemcpyAsync(d_head32_out, d_head, 32, hipMemcpyDeviceToDevice, c->stream));
    if (d_index_out && *n_events > 0) HIPCHK(c, hipMemcpyAsync(d_index_out, c->ids.d_pl_in.p, (size_t)*n_events * 4, hipMemcpyDeviceToDevice, c->stream));
    return bracket.leave();
}

int sw_ingest_message(sw_ctx* c, const uint8_t* msg, int64_t msg_bytes, int validate, int with_data, uint8_t* head32_out, int32_t* index_out, int64_t* n_events,
                      int64_t* n_valid, int64_t* n_stored) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_ingest_message";
    if (!n_events) return fail(c, SW_EINVAL, "%s: n_events is NULL", what);
    *n_events = -1;
    if (n_valid) *n_valid = 0;
    if (n_stored) *n_stored = 0;
    if (msg_bytes < 0 || (msg_bytes > 0 && !msg)) return fail(c, SW_EINVAL, "%s: NULL message (%lld bytes)", what, (long long)msg_bytes);
    HIPCHK(c, hipSetDevice(c->device));
    CHK(dgrow(c, c->wire.d_in, (size_t)msg_bytes + 256, 0));
    if (msg_bytes) HIPCHK(c, hipMemcpyAsync(c->wire.d_in.p, msg, (size_t)msg_bytes, hipMemcpyHostToDevice, c->stream));
    uint8_t* d_head = nullptr;
    CHK(wire_ingest_run(c, c->wire.d_in.p, msg_bytes, validate != 0, with_data != 0, what, &d_head, n_events, n_valid, n_stored));
    if (*n_events < 0) return SW_OK;
    if (head32_out) HIPCHK(c, hipMemcpyAsync(head32_out, d_head, 32, hipMemcpyDeviceToHost, c->stream));
    if (index_out && *n_events > 0) HIPCHK(c, hipMemcpyAsync(index_out, c->ids.d_pl_in.p, (size_t)*n_events * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

int sw_get_wire_stats(sw_ctx* c, int64_t* pack_calls, int64_t* pack_events, int64_t* pack_bytes, int64_t* unpack_calls, int64_t* unpack_events, int64_t* refused) {
    if (!c) return SW_EINVAL;
    if (pack_calls) *pack_calls = c->wire.pack_calls;
    if (pack_events) *pack_events = c->wire.pack_events;
    if (pack_bytes) *pack_bytes = c->wire.pack_bytes;
    if (unpack_calls) *unpack_calls = c->wire.unpack_calls;
    if (unpack_events) *unpack_events = c->wire.unpack_events;
    if (refused) *refused = c->wire.refused;
    return SW_OK;
}

// ---- creating signed events on the device (sign.hip.h) -------------------------------------------------
}  // extern "C"

namespace {

struct SignArrays {   // what a sign call reads and writes, every array in device memory
    const int32_t *creator, *sp, *op;
    const double* t;
    const uint8_t* data;
    const int64_t* data_off;
    int64_t data_bytes;
    const uint8_t* data_none;
    uint8_t *id, *sp_id, *op_id, *arity, *sig;
};

// what every form checks before anything else
int sign_pre(sw_ctx* c, int64_t K, const void* creator, const void* sp, const void* op, const void* t, const void* data, const void* data_off,
             int64_t data_bytes, const void* data_none, const char* what) {
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (c->val.keys.empty()) return fail(c, SW_ENOTSUP, "%s: no member keys (sw_set_member_keys first)", what);
    if (c->sign.has.empty()) return fail(c, SW_ENOTSUP, "%s: no signing keys (sw_set_signing_keys first)", what);
    if (c->ids.n_ids != c->N)
        return fail(c, SW_ENOTSUP, "%s: %lld of the %lld stored events have no id (sw_set_event_ids first)", what, (long long)(c->N - c->ids.n_ids), (long long)c->N);
    if (K < 0 || data_bytes < 0) return fail(c, SW_EINVAL, "%s: negative count or length", what);
    if (K > 0x3fffffffll || c->N + K > 0x7ffffff0ll) return fail(c, SW_ERANGE, "%s: more than 2^31 events", what);
    if (K > 0 && (!creator || !sp || !op || !t)) return fail(c, SW_EINVAL, "%s: NULL event arrays", what);
    if (!data_off && (data || data_bytes || data_none)) return fail(c, SW_EINVAL, "%s: data needs its offsets (or none of data, offsets, length, flags)", what);
    if (data_off && data_bytes > 0 && !data) return fail(c, SW_EINVAL, "%s: %lld data bytes and a NULL buffer", what, (long long)data_bytes);
    return SW_OK;
}

// The call behind the argument checks, on the context's stream: checks and levels (ONE synchronisation: the verdict, the
// level count and the widest level come back together), the sort by level, one launch per level.  Returns with the level
// launches enqueued.  *usable: the data bytes of all ranges together (they may overlap).
int sign_core(sw_ctx* c, int64_t K, const SignArrays& a, const char* what, int64_t* usable) {
    const bool prof = c->profiling;
    auto t0 = std::chrono::steady_clock::now();
    c->sign.ms[0] = c->sign.ms[1] = c->sign.ms[2] = 0;
    CHK(pack_header(c));
    const size_t k = (size_t)K;
    Carve cv;
    const size_t o_blk = cv.take(256), o_lvl = cv.take(k * 4), o_cnt = cv.take((k + 2) * 8), o_cur = cv.take(k * 4), o_ev = cv.take(k * 4);
    const size_t o_ts = cv.take(((k + pck::TILE - 1) / pck::TILE + 1) * 8);
    CHK(dgrow(c, c->sign.d, cv.off + 256, 0));
    unsigned char* B = c->sign.d.p;
    unsigned long long* d_v = (unsigned long long*)(B + o_blk);   // [0] verdict, [1] data bytes, then stat[4] as ints
    int* d_stat = (int*)(B + o_blk + 16);
    int* lvl = (int*)(B + o_lvl);
    pck::i64* cnt = (pck::i64*)(B + o_cnt);
    int* cursor = (int*)(B + o_cur);
    int* level_events = (int*)(B + o_ev);
    pck::i64* tsum = (pck::i64*)(B + o_ts);
    const int n = c->n;
    const sws::SignIn in{a.creator, a.sp, a.op, (const sws::u64*)a.t, a.data, (const sws::i64*)a.data_off, (sws::i64)a.data_bytes, a.data_none,
                         (const int*)c->d_cr.p, (const uint8_t*)c->ids.d_id.p, (int)c->N, n, (const uint8_t*)c->val.d_keys.p,
                         (const uint8_t*)c->sign.d_keys.p + (size_t)n * sizeof(sws::Secret), (const sws::Secret*)c->sign.d_keys.p,
                         (const swv::niels*)c->val.d_tab.p + (size_t)n * swv::ROW, (const uint8_t*)c->pack.d_hdr.p, pack_hdr_len(c)};
    const sws::SignOut out{a.id, a.sp_id, a.op_id, a.arity, a.sig};
    HIPCHK(c, hipMemsetAsync(B + o_blk, 0, 256, c->stream));
    HIPCHK(c, hipMemsetAsync(B + o_blk, 0xff, 8, c->stream));   // ing::V_NONE
    HIPCHK(c, hipMemsetAsync(cnt, 0, (k + 2) * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(cursor, 0, k * 4, c->stream));
    const dim3 ev_grid((unsigned)((K + 255) / 256));
    hipLaunchKernelGGL(sws::k_sign_check, ev_grid, dim3(256), 0, c->stream, in, (int)K, d_v, d_v + 1);
    hipLaunchKernelGGL(sws::k_sign_levels, dim3(1), dim3(sws::LV_TILE), 0, c->stream, a.sp, a.op, (int)c->N, (int)K, lvl, (unsigned long long*)cnt, d_stat);
    c->ctr.kernel_launches += 2;
    HIPCHK(c, hipGetLastError());
    unsigned long long rb[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(rb, B + o_blk, sizeof rb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (rb[0] != ing::V_NONE) {
        const long long e = (long long)(rb[0] >> 8);
        switch ((int)(rb[0] & 0xff)) {
            case ing::V_CREATOR: return fail(c, SW_EINVAL, "event %lld: creator out of range", e);
            case ing::V_ARITY: return fail(c, SW_EINVAL, "event %lld: must have 0 or 2 parents", e);
            case ing::V_ORDER: return fail(c, SW_EINVAL, "event %lld: parent index not earlier (not a topological order)", e);
            case ing::V_SELF: return fail(c, SW_EINVAL, "event %lld: self-parent is by another member", e);
            case ing::V_OTHER: return fail(c, SW_EINVAL, "event %lld: other-parent is by the same member", e);
            case sws::V_NOKEY: return fail(c, SW_EINVAL, "event %lld: no signing key for its creator", e);
            default: return fail(c, SW_EINVAL, "event %lld: data range negative, decreasing, beyond the %lld data bytes, or longer than %d", e,
                                 (long long)a.data_bytes, tpl::MAX_DATA);
        }
    }
    int stat[4];
    memcpy(stat, rb + 2, sizeof stat);
    const int nlev = stat[0], widest = stat[1];
    if (stat[2] || nlev < 1 || nlev > K || widest < 1 || widest > K)
        return fail(c, SW_EIO, "%s: %d levels, widest %d, flag %d for %lld events (internal error)", what, nlev, widest, stat[2], (long long)K);
    *usable = (int64_t)rb[1];
    // ---- the batch sorted by level: counts -> offsets (the scan of pack.hip.h), scatter
    const int64_t tiles = (nlev + pck::TILE - 1) / pck::TILE;
    hipLaunchKernelGGL(pck::k_pack_tile_sums, dim3((unsigned)tiles, 1), dim3(pck::SCAN_THREADS), 0, c->stream, (pck::i64)nlev, (pck::i64)tiles,
                       (const pck::i64*)cnt, (const pck::i64*)cnt, tsum);
    hipLaunchKernelGGL(pck::k_pack_scan_sums, dim3(1), dim3(pck::SCAN_THREADS), 0, c->stream, (pck::i64)nlev, (pck::i64)tiles, cnt, cnt, tsum);
    hipLaunchKernelGGL(pck::k_pack_offsets, dim3((unsigned)tiles, 1), dim3(pck::SCAN_THREADS), 0, c->stream, (pck::i64)nlev, (pck::i64)tiles, cnt, cnt,
                       (const pck::i64*)tsum);
    hipLaunchKernelGGL(sws::k_sign_scatter, ev_grid, dim3(256), 0, c->stream, (int)K, (const int*)lvl, (const sws::i64*)cnt, cursor, level_events);
    c->ctr.kernel_launches += 4;
    HIPCHK(c, hipGetLastError());
    if (prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->sign.ms[0] = ms_since(t0); t0 = std::chrono::steady_clock::now(); }
    // ---- one launch per level, back to back
    const dim3 lv_grid((unsigned)((widest + 63) / 64));
    for (int l = 0; l < nlev; ++l)
        hipLaunchKernelGGL(sws::k_sign_level, lv_grid, dim3(64), 0, c->stream, in, out, (const sws::i64*)cnt, (const int*)level_events, l);
    c->ctr.kernel_launches += nlev;
    HIPCHK(c, hipGetLastError());
    if (prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->sign.ms[1] = ms_since(t0); }
    c->sign.calls++;
    c->sign.events += K;
    c->sign.levels = nlev;
    return SW_OK;
}

// the alignment and residency rules of the device forms (those of sw_pack_events_device); out arrays may be NULL (create)
int sign_device_args(sw_ctx* c, int64_t K, const int32_t* cr, const int32_t* sp, const int32_t* op, const double* t, const uint8_t* data,
                     const int64_t* data_off, int64_t data_bytes, const uint8_t* data_none, const uint8_t* id, const uint8_t* sp_id, const uint8_t* op_id,
                     const uint8_t* arity, const uint8_t* sig, const char* what) {
    const size_t k = (size_t)K;   // (K > 0: no row of an array that was passed is empty)
    return device_args(c, what, {{id, k * 32, 16}, {sp_id, k * 32, 16}, {op_id, k * 32, 16}, {sig, k * 64, 16}, {data_off, (k + 1) * 8, 8}, {t, k * 8, 8},
                                 {cr, k * 4, 4}, {sp, k * 4, 4}, {op, k * 4, 4}, {data, (size_t)data_bytes, 1}, {data_none, k, 1}, {arity, k, 1}});
}

// the signed arrays of a create call at the front of sign.d_in (the host form stages its inputs behind `end`)
struct CreateScratch { size_t id, sp, op, ar, sig, end; };
CreateScratch create_scratch(size_t k) {
    Carve cv;
    CreateScratch s{};
    s.id = cv.take(k * 32); s.sp = cv.take(k * 32); s.op = cv.take(k * 32); s.ar = cv.take(k); s.sig = cv.take(k * 64);
    s.end = cv.off;
    return s;
}

// ONE event signed by one wavefront (turn.hip.h) in place of sign_core's levels.
struct OneSign {
    const uint8_t* d_head_id = nullptr;   // in: the other parent is the stored event with THIS id (device memory), looked up on the device
    bool absent = false;                  // out: ... and no stored event has it (nothing signed, nothing stored)
};

// The checks of sign_core for K = 1 and the signer behind them, on the context's stream; ONE synchronisation, which brings back
// the verdict, the data bytes, the looked-up parent and (profiling) the signer's stamps together.  *d_op: where the other
// parent's index lies in device memory (the caller's array, or the slot the lookup wrote).
int sign_one_core(sw_ctx* c, SignArrays a, const char* what, int64_t* usable, OneSign* one, const int32_t** d_op) {
    const bool prof = c->profiling;
    const auto t0 = std::chrono::steady_clock::now();
    c->sign.ms[0] = c->sign.ms[1] = c->sign.ms[2] = 0;
    CHK(pack_header(c));
    CHK(dgrow(c, c->sign.d, 512, 0));
    unsigned char* B = c->sign.d.p;   // [0] verdict, [1] data bytes, [4] the looked-up parent (int), [8 .. 8 + ST_COUNT) stamps
    unsigned long long* d_v = (unsigned long long*)B;
    int32_t* d_slot = (int32_t*)(B + 32);
    unsigned long long* d_stamps = d_v + 8;
    HIPCHK(c, hipMemsetAsync(B, 0, 256, c->stream));
    HIPCHK(c, hipMemsetAsync(B, 0xff, 8, c->stream));   // ing::V_NONE
    if (one->d_head_id) {
        hipLaunchKernelGGL(rsv::k_tab_lookup, dim3(1), dim3(64), 0, c->stream, (const int*)c->ids.d_idtab.p, c->ids.n_ids ? c->ids.idtab_log : 0,
                           (const unsigned char*)c->ids.d_id.p, (const unsigned char*)one->d_head_id, 1, (int*)d_slot);
        c->ctr.kernel_launches++;
        a.op = d_slot;
    }
    *d_op = a.op;
    const int n = c->n;
    const sws::SignIn in{a.creator, a.sp, a.op, (const sws::u64*)a.t, a.data, (const sws::i64*)a.data_off, (sws::i64)a.data_bytes, a.data_none,
                         (const int*)c->d_cr.p, (const uint8_t*)c->ids.d_id.p, (int)c->N, n, (const uint8_t*)c->val.d_keys.p,
                         (const uint8_t*)c->sign.d_keys.p + (size_t)n * sizeof(sws::Secret), (const sws::Secret*)c->sign.d_keys.p,
                         (const swv::niels*)c->val.d_tab.p + (size_t)n * swv::ROW, (const uint8_t*)c->pack.d_hdr.p, pack_hdr_len(c)};
    const sws::SignOut out{a.id, a.sp_id, a.op_id, a.arity, a.sig};
    hipLaunchKernelGGL(sws::k_sign_check, dim3(1), dim3(256), 0, c->stream, in, 1, d_v, d_v + 1);
    if (prof) hipLaunchKernelGGL(swt::k_sign_one<true>, dim3(1), dim3(swt::LANES), 0, c->stream, in, out, (const unsigned long long*)d_v, d_stamps);
    else hipLaunchKernelGGL(swt::k_sign_one<false>, dim3(1), dim3(swt::LANES), 0, c->stream, in, out, (const unsigned long long*)d_v, d_stamps);
    c->ctr.kernel_launches += 2;
    HIPCHK(c, hipGetLastError());
    unsigned long long rb[8 + swt::ST_COUNT] = {0};
    HIPCHK(c, hipMemcpyAsync(rb, B, sizeof rb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int32_t slot = 0;
    memcpy(&slot, rb + 4, sizeof slot);
    if (one->d_head_id && slot < 0) { one->absent = true; return SW_OK; }
    if (rb[0] != ing::V_NONE) {
        switch ((int)(rb[0] & 0xff)) {
            case ing::V_CREATOR: return fail(c, SW_EINVAL, "%s: creator out of range", what);
            case ing::V_ARITY: return fail(c, SW_EINVAL, "%s: an event must have 0 or 2 parents", what);
            case ing::V_ORDER: return fail(c, SW_EINVAL, "%s: a parent is not a stored event", what);
            case ing::V_SELF: return fail(c, SW_EINVAL, "%s: self-parent is by another member", what);
            case ing::V_OTHER: return fail(c, SW_EINVAL, "%s: other-parent is by the same member", what);
            case sws::V_NOKEY: return fail(c, SW_EINVAL, "%s: no signing key for its creator", what);
            default: return fail(c, SW_EINVAL, "%s: data longer than %d bytes", what, tpl::MAX_DATA);
        }
    }
    *usable = (int64_t)rb[1];
    if (prof) {
        c->sign.ms[1] = ms_since(t0);
        memcpy(c->turn.stamps, rb + 8, sizeof c->turn.stamps);
        c->turn.profiled++;
    }
    c->turn.events++;
    return SW_OK;
}

// sw_create_events behind the argument checks: every array in device memory and visible to the context's stream.
// Everything that can be refused or can run out of memory comes first; behind the append a failure poisons the context.
int create_core(sw_ctx* c, int64_t K, const int32_t* d_cr, const int32_t* d_sp, const int32_t* d_op, const double* d_t, const uint8_t* d_data,
                const int64_t* d_off, int64_t data_bytes, const uint8_t* d_none, uint8_t* d_id_out, uint8_t* d_sig_out, const char* what,
                OneSign* one = nullptr) {
    const int64_t N0 = c->N;
    const bool with_data = c->data.n_data == N0;
    const size_t k = (size_t)K;
    // ---- reservations: ids and table, the data store, the signed arrays
    CHK(idindex_reserve(c, N0 + K));
    DataPlan p{};
    if (with_data) {
        CHK(data_scratch(c, K, 0, 0, &p));
        CHK(data_reserve(c, N0 + K, c->data.used + data_bytes));
    }
    const CreateScratch L = create_scratch(k);
    const size_t o_id = L.id, o_sp = L.sp, o_op = L.op, o_ar = L.ar, o_sig = L.sig;
    CHK(dgrow(c, c->sign.d_in, L.end + 256, 0));
    unsigned char* B = c->sign.d_in.p;
    int64_t usable = 0;
    const SignArrays sa{d_cr, d_sp, d_op, d_t, d_data, d_off, data_bytes, d_none, B + o_id, B + o_sp, B + o_op, B + o_ar, B + o_sig};
    if (one) {   // K == 1: the one-wave signer (turn.hip.h); the other parent may come from the id index, and be absent
        CHK(sign_one_core(c, sa, what, &usable, one, &d_op));
        if (one->absent) return SW_OK;
    } else {
        CHK(sign_core(c, K, sa, what, &usable));
    }
    if (with_data && usable > data_bytes)
        return fail(c, SW_EINVAL, "%s: the data ranges hold %lld bytes, the buffer %lld: ranges overlap (nothing stored)", what, (long long)usable, (long long)data_bytes);
    const auto t0 = std::chrono::steady_clock::now();
    // ---- the ids into the (uncommitted) tail and the table: two equal events, or one that is stored already, show here
    HIPCHK(c, hipMemcpyAsync(c->ids.d_id.p + (size_t)N0 * 32, B + o_id, k * 32, hipMemcpyDeviceToDevice, c->stream));
    int flag = 0;
    CHK(idtab_insert(c, N0, K, &flag));
    if (flag != 0) {
        CHK(idtab_rebuild(c));   // (the table as it was)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (flag == 1) return fail(c, SW_EINVAL, "%s: an event of the batch equals a stored event or another one of the batch (nothing stored)", what);
        return fail(c, SW_EIO, "%s: id table full (internal error)", what);
    }
    // ---- append (bulk device path or its fallbacks; atomic)
    const int rc = append_device_body(c, K, d_cr, d_sp, d_op, d_t, B + o_sig, c->stream);
    if (rc != SW_OK) {
        if (!c->poisoned) {
            const std::string msg = c->err;
            if (idtab_rebuild(c) != SW_OK || hipStreamSynchronize(c->stream) != hipSuccess) c->poisoned = true;
            c->err = msg;
        }
        return rc;
    }
    c->ids.n_ids = N0 + K;
    // ---- committed
    const auto after = [&]() -> int {
        if (with_data) CHK(data_set_body(c, K, d_data, d_off, data_bytes, d_none, what));
        if (d_id_out) HIPCHK(c, hipMemcpyAsync(d_id_out, B + o_id, k * 32, hipMemcpyDeviceToDevice, c->stream));
        if (d_sig_out) HIPCHK(c, hipMemcpyAsync(d_sig_out, B + o_sig, k * 64, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // on return the caller's arrays may be reused or freed
        return SW_OK;
    };
    const int rc2 = after();
    if (rc2 != SW_OK) c->poisoned = true;
    if (c->profiling) c->sign.ms[2] = ms_since(t0);
    return rc2;
}

}  // namespace

extern "C" {

int sw_set_signing_keys(sw_ctx* c, int64_t K, const int32_t* member, const uint8_t* seed32) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_set_signing_keys";
    if (c->poisoned) return fail(c, SW_EIO, "context unusable after an earlier device failure");
    if (c->val.keys.empty()) return fail(c, SW_ENOTSUP, "%s: no member keys (sw_set_member_keys first)", what);
    if (K < 0 || K > c->n || (K > 0 && (!member || !seed32))) return fail(c, SW_EINVAL, "%s: bad count or NULL arrays", what);
    if (K == 0) return SW_OK;
    const size_t n = (size_t)c->n, k = (size_t)K;
    std::vector<char> seen(n, 0);
    for (int64_t j = 0; j < K; ++j) {
        const int m = member[j];
        if (m < 0 || m >= c->n) return fail(c, SW_EINVAL, "%s: member %d out of range", what, m);
        if (!c->val.usable[(size_t)m]) return fail(c, SW_EINVAL, "%s: member %d has an unusable key", what, m);
        if (seen[(size_t)m]) return fail(c, SW_EINVAL, "%s: member %d given twice", what, m);
        seen[(size_t)m] = 1;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->sign.d_keys.p) {
        CHK(dgrow(c, c->sign.d_keys, n * (sizeof(sws::Secret) + 1), 0));
        HIPCHK(c, hipMemsetAsync(c->sign.d_keys.p, 0, c->sign.d_keys.cap, c->stream));
    }
    Carve cv;
    const size_t o_m = cv.take(k * 4), o_seed = cv.take(k * 32), o_ok = cv.take(k);
    CHK(dgrow(c, c->sign.d, cv.off + 256, 0));
    unsigned char* B = c->sign.d.p;
    sws::Secret* secret = (sws::Secret*)c->sign.d_keys.p;
    uint8_t* has = c->sign.d_keys.p + n * sizeof(sws::Secret);
    const swv::niels* rowB = (const swv::niels*)c->val.d_tab.p + n * swv::ROW;
    std::vector<uint8_t> ok(k);
    // the seeds pass through scratch for the length of this call, and are overwritten before it returns whatever happens
    const auto run = [&]() -> int {
        HIPCHK(c, hipMemcpyAsync(B + o_m, member, k * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(B + o_seed, seed32, k * 32, hipMemcpyHostToDevice, c->stream));
        const dim3 grid((unsigned)((K + 63) / 64));
        hipLaunchKernelGGL(sws::k_sign_keys, grid, dim3(64), 0, c->stream, (int)K, (const int*)(B + o_m), (const uint8_t*)(B + o_seed),
                           (const uint8_t*)c->val.d_keys.p, rowB, 0, secret, has, B + o_ok);
        c->ctr.kernel_launches++;
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(ok.data(), B + o_ok, k, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int64_t j = 0; j < K; ++j)
            if (!ok[(size_t)j]) return fail(c, SW_EINVAL, "%s: the seed given for member %d does not derive that member's key (nothing changed)", what, member[j]);
        hipLaunchKernelGGL(sws::k_sign_keys, grid, dim3(64), 0, c->stream, (int)K, (const int*)(B + o_m), (const uint8_t*)(B + o_seed),
                           (const uint8_t*)c->val.d_keys.p, rowB, 1, secret, has, B + o_ok);
        c->ctr.kernel_launches++;
        HIPCHK(c, hipGetLastError());
        return SW_OK;
    };
    const int rc = run();
    (void)hipMemsetAsync(B + o_seed, 0, k * 32, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (rc != SW_OK) return rc;
    if (c->sign.has.empty()) c->sign.has.assign(n, 0);
    for (int64_t j = 0; j < K; ++j) c->sign.has[(size_t)member[j]] = 1;
    c->sign.keysets++;
    return SW_OK;
}

int sw_clear_signing_keys(sw_ctx* c) {
    if (!c) return SW_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    return sign_keys_clear(c);
}

int sw_get_signing_members(sw_ctx* c, uint8_t* has_key) {
    if (!c) return SW_EINVAL;
    if (!has_key) return fail(c, SW_EINVAL, "sw_get_signing_members: NULL output");
    for (int m = 0; m < c->n; ++m) has_key[m] = c->sign.has.empty() ? 0 : c->sign.has[(size_t)m];
    return SW_OK;
}

int sw_sign_events_device(sw_ctx* c, int64_t K, const int32_t* d_creator, const int32_t* d_self_parent, const int32_t* d_other_parent, const double* d_t,
                          const uint8_t* d_data, const int64_t* d_data_off, int64_t data_bytes, const uint8_t* d_data_none, uint8_t* d_id32,
                          uint8_t* d_sp_id32, uint8_t* d_op_id32, uint8_t* d_arity, uint8_t* d_sig64, void* user_stream) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_sign_events_device";
    CHK(sign_pre(c, K, d_creator, d_self_parent, d_other_parent, d_t, d_data, d_data_off, data_bytes, d_data_none, what));
    if (K == 0) return SW_OK;
    if (!d_id32 || !d_sp_id32 || !d_op_id32 || !d_arity || !d_sig64) return fail(c, SW_EINVAL, "%s: NULL output arrays", what);
    CHK(sign_device_args(c, K, d_creator, d_self_parent, d_other_parent, d_t, d_data, d_data_off, data_bytes, d_data_none, d_id32, d_sp_id32, d_op_id32,
                         d_arity, d_sig64, what));
    UserStream bracket;   // the producers of the arrays; earlier readers of the outputs
    CHK(bracket.join(c, (hipStream_t)user_stream));
    int64_t usable = 0;
    CHK(sign_core(c, K, SignArrays{d_creator, d_self_parent, d_other_parent, d_t, d_data, d_data_off, data_bytes, d_data_none, d_id32, d_sp_id32,
                                   d_op_id32, d_arity, d_sig64}, what, &usable));
    return bracket.leave();   // whatever the caller enqueues next reads complete arrays
}

}  // extern "C"

namespace {

// the inputs of the host-array forms staged in sign.d_in behind what `st` holds already (the signed arrays); pointers into the
// staging come back
struct SignStaged { const int32_t *cr, *sp, *op; const double* t; const uint8_t* data; const int64_t* off; const uint8_t* none; };
int sign_stage(sw_ctx* c, int64_t K, Stage& st, const int32_t* creator, const int32_t* sp, const int32_t* op, const double* t, const uint8_t* data,
               const int64_t* data_off, int64_t data_bytes, const uint8_t* data_none, SignStaged* s) {
    const size_t k = (size_t)K;
    const size_t o_cr = st.in(creator, k * 4), o_sp = st.in(sp, k * 4), o_op = st.in(op, k * 4), o_t = st.in(t, k * 8);
    const size_t o_doff = st.in(data_off, (k + 1) * 8), o_d = st.in(data, (size_t)data_bytes), o_dn = st.in(data_none, k);
    unsigned char* B = nullptr;
    CHK(stage_up(c, c->sign.d_in, st, &B));
    *s = SignStaged{(const int32_t*)(B + o_cr), (const int32_t*)(B + o_sp), (const int32_t*)(B + o_op), (const double*)(B + o_t),
                    data_off ? B + o_d : nullptr, data_off ? (const int64_t*)(B + o_doff) : nullptr, data_none ? B + o_dn : nullptr};
    return SW_OK;
}

}  // namespace

extern "C" {

int sw_sign_events(sw_ctx* c, int64_t K, const int32_t* creator, const int32_t* self_parent, const int32_t* other_parent, const double* t,
                   const uint8_t* data, const int64_t* data_off, int64_t data_bytes, const uint8_t* data_none, uint8_t* id32, uint8_t* sp_id32,
                   uint8_t* op_id32, uint8_t* arity, uint8_t* sig64) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_sign_events";
    CHK(sign_pre(c, K, creator, self_parent, other_parent, t, data, data_off, data_bytes, data_none, what));
    if (K == 0) return SW_OK;
    if (!id32 || !sp_id32 || !op_id32 || !arity || !sig64) return fail(c, SW_EINVAL, "%s: NULL output arrays", what);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t k = (size_t)K;
    Stage st;
    const size_t o_id = st.out(id32, k * 32), o_spid = st.out(sp_id32, k * 32), o_opid = st.out(op_id32, k * 32), o_ar = st.out(arity, k), o_sig = st.out(sig64, k * 64);
    SignStaged s{};
    CHK(sign_stage(c, K, st, creator, self_parent, other_parent, t, data, data_off, data_bytes, data_none, &s));
    unsigned char* B = c->sign.d_in.p;
    int64_t usable = 0;
    CHK(sign_core(c, K, SignArrays{s.cr, s.sp, s.op, s.t, s.data, s.off, data_bytes, s.none, B + o_id, B + o_spid, B + o_opid, B + o_ar, B + o_sig}, what, &usable));
    return stage_down(c, st, B);
}

int sw_create_events_device(sw_ctx* c, int64_t K, const int32_t* d_creator, const int32_t* d_self_parent, const int32_t* d_other_parent, const double* d_t,
                            const uint8_t* d_data, const int64_t* d_data_off, int64_t data_bytes, const uint8_t* d_data_none, void* user_stream,
                            int64_t* first_out, uint8_t* d_id32, uint8_t* d_sig64) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_create_events_device";
    CHK(sign_pre(c, K, d_creator, d_self_parent, d_other_parent, d_t, d_data, d_data_off, data_bytes, d_data_none, what));
    if (first_out) *first_out = c->N;
    if (K == 0) return SW_OK;
    CHK(sign_device_args(c, K, d_creator, d_self_parent, d_other_parent, d_t, d_data, d_data_off, data_bytes, d_data_none, d_id32, nullptr, nullptr, nullptr,
                         d_sig64, what));
    UserStream bracket;
    CHK(bracket.join(c, (hipStream_t)user_stream));
    CHK(create_core(c, K, d_creator, d_self_parent, d_other_parent, d_t, d_data, d_data_off, data_bytes, d_data_none, d_id32, d_sig64, what));
    bracket.drained();   // (create_core synchronises the stream before a successful return: the join half is all this form needs)
    return SW_OK;
}

int sw_create_events(sw_ctx* c, int64_t K, const int32_t* creator, const int32_t* self_parent, const int32_t* other_parent, const double* t,
                     const uint8_t* data, const int64_t* data_off, int64_t data_bytes, const uint8_t* data_none, int64_t* first_out, uint8_t* id32,
                     uint8_t* sig64) {
    if (!c) return SW_EINVAL;
    const char* what = "sw_create_events";
    CHK(sign_pre(c, K, creator, self_parent, other_parent, t, data, data_off, data_bytes, data_none, what));
    if (first_out) *first_out = c->N;
    if (K == 0) return SW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t k = (size_t)K;
    const CreateScratch L = create_scratch(k);
    Stage st;
    st.scratch(L.end);   // (the signed arrays, where create_core puts them)
    SignStaged s{};
    CHK(sign_stage(c, K, st, creator, self_parent, other_parent, t, data, data_off, data_bytes, data_none, &s));
    CHK(create_core(c, K, s.cr, s.sp, s.op, s.t, s.data, s.off, data_bytes, s.none, nullptr, nullptr, what));
    const unsigned char* B = c->sign.d_in.p;   // (create_core found the buffer large enough: it has not moved)
    if (id32) HIPCHK(c, hipMemcpyAsync(id32, B + L.id, k * 32, hipMemcpyDeviceToHost, c->stream));
    if (sig64) HIPCHK(c, hipMemcpyAsync(sig64, B + L.sig, k * 64, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

int sw_get_sign_stats(sw_ctx* c, int64_t* calls, int64_t* events, int64_t* levels, int64_t* key_sets, double* phase_ms) {
    if (!c) return SW_EINVAL;
    if (calls) *calls = c->sign.calls;
    if (events) *events = c->sign.events;
    if (levels) *levels = c->sign.levels;
    if (key_sets) *key_sets = c->sign.keysets;
    if (phase_ms) for (int i = 0; i < 3; ++i) phase_ms[i] = c->sign.ms[i];
    return SW_OK;
}

// ---- one event signed by one wavefront, and the gossip turn around it (turn.hip.h) -----------------------
}  // extern "C"

namespace {

// One event as host values -> the K = 1 arrays sw_create_events would stage -> create_core with the one-wave signer.  The
// staged values live on this frame: the stream is drained before it is left, whatever happens.  (sw_create_event and
// sw_gossip_turn take no stream of the caller's: the only UserStream under them is the one inside the append, which joins the
// context's stream with itself and drains it.)
int create_one(sw_ctx* c, int member, int64_t sp, int64_t op, double t, const uint8_t* data, int64_t data_len, OneSign* one, uint8_t* id32_out,
               uint8_t* sig64_out, const char* what) {
    const auto narrow = [](int64_t v) { return v < 0 ? (int32_t)-1 : v > 0x7fffffff ? (int32_t)0x7fffffff : (int32_t)v; };
    const int32_t cr = member, s = narrow(sp), o = narrow(op);
    const int64_t nbytes = data_len > 0 ? data_len : 0;
    const int64_t off[2] = {0, nbytes};
    const uint8_t none = data_len < 0 ? 1 : 0;
    if (data_len > 0 && !data) return fail(c, SW_EINVAL, "%s: %lld data bytes and a NULL buffer", what, (long long)data_len);
    CHK(sign_pre(c, 1, &cr, &s, &o, &t, nbytes ? data : nullptr, off, nbytes, &none, what));
    if (data_len > tpl::MAX_DATA) return fail(c, SW_EINVAL, "%s: data longer than %d bytes", what, tpl::MAX_DATA);
    HIPCHK(c, hipSetDevice(c->device));
    const CreateScratch L = create_scratch(1);
    const auto run = [&]() -> int {
        Stage plan;
        plan.scratch(L.end);
        SignStaged st{};
        CHK(sign_stage(c, 1, plan, &cr, &s, &o, &t, nbytes ? data : nullptr, off, nbytes, &none, &st));
        CHK(create_core(c, 1, st.cr, st.sp, st.op, st.t, st.data, st.off, nbytes, st.none, nullptr, nullptr, what, one));
        if (one->absent) return SW_OK;
        const unsigned char* B = c->sign.d_in.p;   // (create_core found the buffer large enough: it has not moved)
        if (id32_out) HIPCHK(c, hipMemcpyAsync(id32_out, B + L.id, 32, hipMemcpyDeviceToHost, c->stream));
        if (sig64_out) HIPCHK(c, hipMemcpyAsync(sig64_out, B + L.sig, 64, hipMemcpyDeviceToHost, c->stream));
        if (id32_out || sig64_out) HIPCHK(c, hipStreamSynchronize(c->stream));
        return SW_OK;
    };
    const int rc = run();
    if (rc != SW_OK) (void)hipStreamSynchronize(c->stream);
    return rc;
}

}  // namespace

extern "C" {

int sw_create_event(sw_ctx* c, int member, int64_t self_parent, int64_t other_parent, double t, const uint8_t* data, int64_t data_len,
                    int64_t* index_out, uint8_t* id32_out, uint8_t* sig64_out) {
    if (!c) return SW_EINVAL;
    const int64_t N0 = c->N;
    OneSign one;
    CHK(create_one(c, member, self_parent, other_parent, t, data, data_len, &one, id32_out, sig64_out, "sw_create_event"));
    if (index_out) *index_out = N0;
    c->turn.calls++;
    return SW_OK;
}

int sw_gossip_turn(sw_ctx* dst, int member, int64_t dst_head, sw_ctx* src, int64_t src_head, double t, const uint8_t* data, int64_t data_len,
                   int flags, int32_t* new_rounds, int cap_rounds, void* result, size_t result_bytes) {
    if (!dst || !src) return SW_EINVAL;
    const char* what = "sw_gossip_turn";
    if (!result || result_bytes < 8) return fail(dst, SW_EINVAL, "%s: NULL or short result", what);
    sw_turn_result res{};
    res.new_head = -1;
    const auto put = [&]() { memcpy(result, &res, std::min(result_bytes, sizeof res)); };
    put();
    const bool validate = flags & SW_TURN_VALIDATE, with_data = flags & SW_TURN_DATA, trunks = flags & SW_TURN_TRUNKS;
    const bool consensus = !(flags & SW_TURN_NO_CONSENSUS);
    // ---- refusals: before anything is launched or stored
    if (flags & ~(SW_TURN_VALIDATE | SW_TURN_DATA | SW_TURN_TRUNKS | SW_TURN_NO_CONSENSUS)) return fail(dst, SW_EINVAL, "%s: unknown flag bits in %d", what, flags);
    if (dst == src) return fail(dst, SW_EINVAL, "%s: a context cannot gossip with itself", what);
    if (dst->n != src->n) return fail(dst, SW_EINVAL, "%s: %d members here, %d at the peer", what, dst->n, src->n);
    if (dst->poisoned || src->poisoned) return fail(dst, SW_EIO, "context unusable after an earlier device failure");
    if (dst->vm.active || src->vm.active) return fail(dst, SW_ENOTSUP, "%s is not available with the windowed table", what);
    if (dst->val.keys.empty()) return fail(dst, SW_ENOTSUP, "%s: no member keys (sw_set_member_keys first)", what);
    if (member < 0 || member >= dst->n) return fail(dst, SW_EINVAL, "%s: member %d out of range", what, member);
    if (dst->sign.has.empty() || !dst->sign.has[(size_t)member]) return fail(dst, SW_ENOTSUP, "%s: no signing key for member %d (sw_set_signing_keys first)", what, member);
    if (dst->ids.n_ids != dst->N || src->ids.n_ids != src->N) return fail(dst, SW_ENOTSUP, "%s: the id index of %s is incomplete (sw_set_event_ids first)", what, dst->ids.n_ids != dst->N ? "this context" : "the peer");
    if (with_data && (dst->data.n_data != dst->N || src->data.n_data != src->N))
        return fail(dst, SW_ENOTSUP, "%s: the data store of %s is incomplete (sw_set_event_data first)", what, dst->data.n_data != dst->N ? "this context" : "the peer");
    if (dst->divided != dst->N) return fail(dst, SW_EINVAL, "%s: %lld undivided events (sw_divide_rounds first)", what, (long long)(dst->N - dst->divided));
    if (dst_head < 0 || dst_head >= dst->N || dst->cr[(size_t)dst_head] != member)
        return fail(dst, SW_EINVAL, "%s: head %lld is not an event of member %d (swirld.py:86)", what, (long long)dst_head, member);
    if (src_head >= 0 && src_head < src->N && src->cr[(size_t)src_head] == member)
        return fail(dst, SW_EINVAL, "%s: the peer's head %lld is an event of member %d itself (swirld.py:87)", what, (long long)src_head, member);
    if (data_len > tpl::MAX_DATA) return fail(dst, SW_EINVAL, "%s: data longer than %d bytes", what, tpl::MAX_DATA);
    if (data_len > 0 && !data) return fail(dst, SW_EINVAL, "%s: %lld data bytes and a NULL buffer", what, (long long)data_len);
    if (consensus && (cap_rounds < 0 || (cap_rounds > 0 && !new_rounds))) return fail(dst, SW_EINVAL, "%s: NULL new_rounds (capacity %d)", what, cap_rounds);
    CHK(pull_pre(dst, dst_head, src, validate, with_data, what));
    if (const int rc = walk_pre(src, src_head, true, "sw_gossip_turn (peer)"); rc != SW_OK) { dst->err = src->err; return rc; }
    // ---- 1. the pull (swirld.py:125-136)
    const int64_t N_before = dst->N;
    CHK(sw_sync_pull_walk(dst, dst_head, src, src_head, trunks, validate, with_data, &res.n_sent, &res.n_valid, &res.n_stored));
    res.stage = SW_TURN_STAGE_PULLED;
    put();
    dst->turn.turns++;
    // ---- 2. and 3. the new event on my head and the peer's, whose index comes from the id index on the device
    OneSign one;
    one.d_head_id = (const uint8_t*)src->ids.d_id.p + (size_t)src_head * 32;
    const int64_t N_pulled = dst->N;
    CHK(create_one(dst, member, dst_head, -1, t, data, data_len, &one, nullptr, nullptr, what));
    if (!one.absent) res.new_head = N_pulled;
    res.stage = SW_TURN_STAGE_CREATED;
    put();
    if (!consensus) return SW_OK;
    // ---- 4. divide_rounds, decide_fame, find_order (swirld.py:326-328)
    CHK(sw_divide_rounds(dst, N_before, dst->N - N_before));
    res.stage = SW_TURN_STAGE_DIVIDED;
    put();
    int n_new = 0;
    CHK(sw_decide_fame(dst, new_rounds, cap_rounds, &n_new));
    res.n_new_rounds = n_new;
    res.stage = SW_TURN_STAGE_FAME;
    put();
    std::vector<int32_t> ordered((size_t)std::max<int64_t>(dst->N, 1));
    CHK(sw_find_order(dst, new_rounds, n_new, ordered.data(), dst->N, &res.n_ordered));
    res.stage = SW_TURN_STAGE_ORDERED;
    put();
    return SW_OK;
}

int sw_get_turn_stats(sw_ctx* c, int64_t* create_calls, int64_t* events, int64_t* turns, int64_t* stamped, uint64_t* stamps, double* tick_ns) {
    if (!c) return SW_EINVAL;
    if (create_calls) *create_calls = c->turn.calls;
    if (events) *events = c->turn.events;
    if (turns) *turns = c->turn.turns;
    if (stamped) *stamped = c->turn.profiled;
    if (stamps) for (int i = 0; i < swt::ST_COUNT; ++i) stamps[i] = c->turn.stamps[i];
    if (tick_ns) {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || khz <= 0) { (void)hipGetLastError(); khz = 100000; }
        *tick_ns = 1e6 / khz;
    }
    return SW_OK;
}


// ---- ingest-side crypto batches: stateless, one thread per message ------------
}  // extern "C"

namespace {
__global__ void __launch_bounds__(64)
k_verify_batch(const uint8_t* __restrict__ msgs, const long long* __restrict__ off, const uint8_t* __restrict__ sig,
               const uint8_t* __restrict__ pk, int K, uint8_t* ok) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    ok[i] = swc::ed25519_verify(sig + (size_t)i * 64, msgs + off[i], (uint64_t)(off[i + 1] - off[i]), pk + (size_t)i * 32) ? 1 : 0;
}
__global__ void __launch_bounds__(64)
k_blake2b_batch(const uint8_t* __restrict__ msgs, const long long* __restrict__ off, int K, uint8_t* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    swc::blake2b_256(msgs + off[i], (uint64_t)(off[i + 1] - off[i]), out + (size_t)i * 32);
}
int crypto_batch(int device, int64_t K, const uint8_t* msgs, const int64_t* off, const uint8_t* sig, const uint8_t* pk, uint8_t* out, bool verify) {
    if (K < 0 || (K > 0 && (!msgs || !off || !out || (verify && (!sig || !pk))))) return fail(nullptr, SW_EINVAL, "NULL batch arrays");
    if (K == 0) return SW_OK;
    if (K > 0x7fffffff) return fail(nullptr, SW_ERANGE, "batch too large");
    for (int64_t i = 0; i < K; ++i) if (off[i + 1] < off[i] || off[i] < 0) return fail(nullptr, SW_EINVAL, "message offsets must be non-decreasing");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(nullptr, SW_ENODEV, "no such HIP device (there is no CPU fallback)");
    HIPCHK(nullptr, hipSetDevice(device));
    const size_t nbytes = (size_t)off[K];
    const size_t out_per = verify ? 1 : 32;
    DBuf<unsigned char> d_m, d_off, d_sig, d_pk, d_out;
    CHK(dgrow(nullptr, d_m, std::max<size_t>(nbytes, 1), 0));
    CHK(dgrow(nullptr, d_off, (size_t)(K + 1) * 8, 0));
    CHK(dgrow(nullptr, d_out, (size_t)K * out_per, 0));
    HIPCHK(nullptr, hipMemcpy(d_m.p, msgs, nbytes, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(d_off.p, off, (size_t)(K + 1) * 8, hipMemcpyHostToDevice));
    const unsigned blocks = (unsigned)((K + 63) / 64);
    if (verify) {
        CHK(dgrow(nullptr, d_sig, (size_t)K * 64, 0));
        CHK(dgrow(nullptr, d_pk, (size_t)K * 32, 0));
        HIPCHK(nullptr, hipMemcpy(d_sig.p, sig, (size_t)K * 64, hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(d_pk.p, pk, (size_t)K * 32, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_verify_batch, dim3(blocks), dim3(64), 0, nullptr, (const uint8_t*)d_m.p, (const long long*)d_off.p,
                           (const uint8_t*)d_sig.p, (const uint8_t*)d_pk.p, (int)K, (uint8_t*)d_out.p);
    } else {
        hipLaunchKernelGGL(k_blake2b_batch, dim3(blocks), dim3(64), 0, nullptr, (const uint8_t*)d_m.p, (const long long*)d_off.p, (int)K, (uint8_t*)d_out.p);
    }
    HIPCHK(nullptr, hipGetLastError());
    HIPCHK(nullptr, hipMemcpy(out, d_out.p, (size_t)K * out_per, hipMemcpyDeviceToHost));
    return SW_OK;
}
}  // namespace

extern "C" {
int sw_crypto_verify_batch(int device, int64_t K, const uint8_t* msgs, const int64_t* msg_off, const uint8_t* sig64,
                           const uint8_t* pk32, uint8_t* ok) {
    return crypto_batch(device, K, msgs, msg_off, sig64, pk32, ok, true);
}
int sw_crypto_hash_batch(int device, int64_t K, const uint8_t* msgs, const int64_t* msg_off, uint8_t* out32) {
    return crypto_batch(device, K, msgs, msg_off, nullptr, nullptr, out32, false);
}
}  // extern "C"

// ---- batches of small hashgraphs: one wavefront each, one launch (batch.hip.h) ----
#include "batch_synth.hip.h"
#include "batch_network.hip.h"
#include "batch_api.hip.h"
#include "batch_synth_api.hip.h"
// ... and their results read in one call: a ragged gather over the whole batch (sw_export_batch_*)
#include "batch_export.hip.h"
#include "batch_export_api.hip.h"
// ... and gossip networks of consecutive hashgraphs: one wavefront runs a network's turns (sw_network_batch_*)
#include "batch_network_api.hip.h"
