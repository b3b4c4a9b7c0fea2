/*
 * swirld_hip.h — C-ABI of the MI355X-native virtual-voting hot path of py-swirld.
 *
 * The reference (Lapin0t/py-swirld) has no FFI or plugin interface: its hot path
 * is three methods of one Python class, `Node` (swirld.py:36-328).  This header is
 * therefore the boundary a maintainer would bind with ctypes from inside `Node`
 * (see INTEGRATION.md); each entry point names the reference code it replaces.
 *
 * Conventions
 *  - plain C types only; the caller owns every buffer (typically numpy arrays);
 *  - every function returns SW_OK (0) or a negative errno-style code and never
 *    throws; sw_last_error() gives a human-readable message for the last failure;
 *  - one context per Node view; a context is NOT thread-safe (the reference is
 *    single-threaded by design, README.md:27-28, swirld.py:152); independent
 *    contexts may live on different devices/streams;
 *  - events are addressed by DENSE INDEX = the order in which they were appended,
 *    which must be a topological order (parents before children), exactly the
 *    order `Node.add_event` is called in (swirld.py:114-120, 133-144); members are
 *    addressed by dense index 0..n-1 (the host glue keeps pk -> index);
 *  - "absent" event / parent / witness is -1.
 */
#ifndef SWIRLD_HIP_H
#define SWIRLD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SW_OK          0
#define SW_EIO        (-5)   /* HIP runtime error (message in sw_last_error)            */
#define SW_ENOMEM     (-12)
#define SW_ENODEV     (-19)  /* no usable GPU / device index out of range               */
#define SW_EINVAL     (-22)
#define SW_ERANGE     (-34)  /* index / round range outside the stored hashgraph        */
#define SW_EOVERFLOW  (-75)  /* total stake too large for the 32-bit tally              */
#define SW_ENOTSUP    (-95)  /* outside the supported domain (forks refused, exact path) */

#define SW_MAX_MEMBERS 1024

typedef struct sw_ctx sw_ctx;

/* ABI version of this header (bumped on any signature change). */
int sw_version(void);

/*
 * Context = the voting state of one Node (swirld.py:38-72): `stake`, `tot_stake`,
 * `min_s` (handled as the exact integer tests 3x > 2T and 2x > T, Appendix A Q1),
 * module constant C = coin_period (swirld.py:17).
 * device = HIP device ordinal.  Fails with SW_ENODEV when no GPU is present: there
 * is no CPU fallback in this library.
 */
int sw_create(int n_members, const uint64_t* stake, int coin_period, int device, sw_ctx** out);
int sw_destroy(sw_ctx* ctx);
const char* sw_last_error(const sw_ctx* ctx);   /* ctx may be NULL: last create() error */

/* Pre-size device storage for n_events events (optional; append grows on demand). */
int sw_reserve(sw_ctx* ctx, int64_t n_events);

/*
 * Mirror of Node.add_event (swirld.py:114-120) for K events in topological order:
 * stores creator / parents, computes `height` (0 for roots, 1+max(parent heights)).
 * self_parent/other_parent are dense indices (both -1 for a root, swirld.py:85-87).
 * t = Event.t (float64 timestamp), sig64 = Event.s (64-byte signature; its first
 * byte's top bit is the coin bit of swirld.py:272, all 64 bytes feed the whitening
 * of swirld.py:281-285).  t and sig64 may be NULL (zeros are stored).
 * Validation mirrors is_valid_event's structural half (swirld.py:104-108): parents
 * must exist, self-parent must be by the same creator, other-parent by another.
 * A fork (an event whose self-parent is not its creator's latest event, or a second
 * root of one member) is stored, as the reference stores it (no fork detection,
 * README.md:84), and moves the context to the EXACT path (sw_set_forks below): from
 * then on every call runs the reference's own statements on the device, one wavefront,
 * results identical to the reference's on forked input — and far slower than the
 * round-synchronous path, which needs one self-parent chain per member.
 */
int sw_append_events(sw_ctx* ctx, int64_t K, const int32_t* creator, const int32_t* self_parent,
                     const int32_t* other_parent, const double* t, const uint8_t* sig64);
int64_t sw_num_events(const sw_ctx* ctx);

/*
 * sw_append_events for K events that are ALREADY IN DEVICE MEMORY (batched signature checks, a torch pipeline, a
 * generator kernel, a peer's events arriving by RCCL): same meaning, same state afterwards — every getter and every
 * later call behaves as if the same arrays had gone through sw_append_events.  All arrays lie in memory of the
 * context's device (`d_t`, `d_sig64` may be NULL: zeros are stored); a host pointer, or memory of another device, is
 * SW_EINVAL before anything is launched.  `user_stream` is a hipStream_t or NULL (the null stream), as for
 * sw_import_rows: the context's stream waits, on the device, for what has been enqueued there so far.  On return the
 * caller may reuse or free the arrays.
 *
 * The device path (ingest.hip.h) validates the batch, ranks every event in its creator's chain, builds the per-member
 * tables and the chain pool and computes the heights (swirld.py:117-120) on the device; it reads back one verdict
 * word, the per-member tables and 8 B per event (creator, chain position).  The heights kernel runs behind the call;
 * whoever needs heights waits for it, and the full host mirror of parents and heights is downloaded only for
 * sw_get_height, the gossip getters, a later small append or the exact path.
 *
 * Atomic on rejection like sw_append_events (nothing stored, context usable), with the same code for the same
 * defect: SW_EINVAL for creator out of range, one parent only, a parent index not earlier than the event (indices at
 * or beyond the end of the batch included), self-parent by another member, other-parent by the same member;
 * sw_last_error names the event.  With several defects in one batch the device path reports the LOWEST offending
 * event, and for it the first failing check in the order just given.  (The bulk host path differs there: its host
 * loop runs before its other-parent kernel, so any defect of the loop — or a fork — wins over an other-parent defect
 * whatever the index.)
 *
 * What falls back: the batch is copied to the host and handed to sw_append_events when the context is on the exact
 * path, the table is windowed (sw_set_window), the batch is not bulk-sized (bulk: K >= 8192, or the first append, or
 * 8 K >= events stored — small appends keep the host mirrors incremental), or the device validation finds a FORK
 * (self-parent by the same creator but not its latest event, or a second root).  In the fork case nothing has been
 * committed, so the host path decides as ever: exact path with sw_set_forks(ctx, 1), SW_ENOTSUP and nothing stored
 * with sw_set_forks(ctx, 0).
 *
 * sw_get_ingest_stats: batches / events the device path committed, batches that fell back (rejected pointer checks do
 * not count), and the events whose height the sequential host loop computed (0 for device-appended events) — since
 * sw_create.  Any pointer may be NULL.
 */
int sw_append_events_device(sw_ctx* ctx, int64_t K, const int32_t* d_creator, const int32_t* d_self_parent,
                            const int32_t* d_other_parent, const double* d_t, const uint8_t* d_sig64, void* user_stream);
int sw_get_ingest_stats(sw_ctx* ctx, int64_t* device_batches, int64_t* device_events, int64_t* fallback_batches,
                        int64_t* host_height_events);

/*
 * Events by ID (Node.sync swirld.py:130-136, node.py).  A peer's sync payload names events by their 32-byte
 * ids (BLAKE2b-256 of the pickled event) and their parents by id, in no particular order, events the receiver already has
 * included.  The context can learn the ids of its events — an ID INDEX, allocated on first use: 32 bytes per event in dense
 * order, and a device hash table id -> dense index (open addressing, power-of-two capacity, load <= 1/2, rebuilt when it
 * grows; keyed by the first 64-bit word of the id, a hit confirmed on all 32 bytes; every probe loop is bounded by the
 * capacity, ids being attacker-chosen) — and then takes a whole payload addressed by id.
 * sw_rewind keeps the ids (the events stay), sw_reset forgets them.  The index is COMPLETE when every stored event has an
 * id (an empty context counts as complete).
 *
 * sw_set_event_ids     ids of the stored events [first, first + K) (how events appended by index get theirs).  `first` must
 *                      equal the number of events that have ids already.  SW_EINVAL, nothing stored, when an id is already
 *                      present or occurs twice in the call.
 * sw_get_event_ids     the ids of [first, first + K); SW_ERANGE beyond the events that have ids.
 * sw_lookup_event_ids  index_out[i] = dense index of id i, or -1 (looked up on the device).
 *
 * sw_ingest_payload_device   Node.sync's loop over K events in ANY order, on the device: known ids are recognised, the rest
 *   is validated, ordered topologically and appended; invalid events are DROPPED and the rest is stored (the reference's
 *   behaviour, swirld.py:135 — unlike sw_append_events_device the call is not atomic per batch).  Needs a complete index
 *   (SW_ENOTSUP and nothing stored otherwise).  All d_* arrays lie in memory of the context's device (checked like
 *   sw_append_events_device's; a host pointer is SW_EINVAL before any launch); the three id arrays must be 8-byte aligned
 *   (SW_EINVAL).  Per event: d_id32 its id; d_sp_id32 / d_op_id32 the parents' ids (ignored when the arity is 0); d_arity
 *   (uint8) the number of parents claimed, len(ev.p); d_creator a dense member index; d_ok (uint8, NULL = all 1) 1 when
 *   signature and hash were verified (what sw_validate_payload_device left, or what sw_crypto_verify_batch wrote ANDed
 *   with the caller's hash comparison); d_t,
 *   d_sig64 nullable as for sw_append_events_device; user_stream as there.  d_index_out: K int32 in device memory;
 *   *n_stored (host): the events stored.  index_out[i] is
 *     an index <  the event count before the call   the id is stored already (nothing is stored again)
 *     an index >= the event count before the call   stored by this call at that dense index
 *     -2  a later copy of an id that occurs earlier in this payload (the lowest position counts)
 *     -3  d_ok is 0                       -4  creator outside [0, n)          -5  arity neither 0 nor 2
 *     -6  a parent that is neither stored nor accepted in this call (children of dropped events, unknown ids, cycles)
 *     -7  self-parent by another member   -8  other-parent by the same member
 *   (several defects: the first in this order).  Acceptance runs in WAVES: wave 0 accepts the locally valid events whose
 *   parents are both stored, and the locally valid roots; wave w those whose parents are all stored or accepted in waves
 *   < w, at least one in wave w - 1; the call ends with the first wave that accepts nothing (at most accepted + 1 waves,
 *   driven from the host in batches of launches with one read-back of per-wave counts; no kernel waits for another
 *   workgroup).  The accepted set is what Node.sync's loop stores under any topological order of the payload.  Accepted
 *   events get the dense indices (count before) + rank, rank sorting by (wave, payload position): a topological order that
 *   keeps every member's chain in chain order.  They then go through the body of sw_append_events_device — same bulk
 *   predicate, fallbacks and fork handling (exact path under sw_set_forks(1); SW_ENOTSUP under sw_set_forks(0)); the ids
 *   are committed only after the append has succeeded.  If it fails, context and index are unchanged, *n_stored is 0 and
 *   index_out is unspecified.
 * sw_ingest_payload    the same with every array (and index_out) in HOST memory: staged into context scratch on the
 *   context's stream, same device code.
 * sw_get_payload_stats payload calls so far, waves and accepted events of the most recent one, rebuilds of the id table
 *   since sw_create, and — under sw_set_profiling — the host time in ms of the most recent call's phases: phase_ms[4] =
 *   resolve, waves, sort + gather, append + id commit.  Any pointer may be NULL.
 */
int sw_set_event_ids(sw_ctx* ctx, int64_t first, int64_t K, const uint8_t* id32);
int sw_get_event_ids(sw_ctx* ctx, int64_t first, int64_t K, uint8_t* out);
int sw_lookup_event_ids(sw_ctx* ctx, int64_t K, const uint8_t* id32, int32_t* index_out);
int sw_ingest_payload_device(sw_ctx* ctx, int64_t K, const uint8_t* d_id32, const uint8_t* d_sp_id32, const uint8_t* d_op_id32,
                             const uint8_t* d_arity, const int32_t* d_creator, const uint8_t* d_ok, const double* d_t,
                             const uint8_t* d_sig64, void* user_stream, int32_t* d_index_out, int64_t* n_stored);
int sw_ingest_payload(sw_ctx* ctx, int64_t K, const uint8_t* id32, const uint8_t* sp_id32, const uint8_t* op_id32,
                      const uint8_t* arity, const int32_t* creator, const uint8_t* ok, const double* t, const uint8_t* sig64,
                      int32_t* index_out, int64_t* n_stored);
int sw_get_payload_stats(sw_ctx* ctx, int64_t* calls, int64_t* waves, int64_t* accepted, int64_t* table_rebuilds, double* phase_ms);

/*
 * Node.divide_rounds(events) (swirld.py:187-222) for the K events [first, first+K):
 * fills can_see rows, round numbers and the witness table.  `first` must equal the
 * number of events already divided (the reference processes every new event exactly
 * once, in order: swirld.py:325).
 */
int sw_divide_rounds(sw_ctx* ctx, int64_t first, int64_t K);

/*
 * Node.decide_fame() (swirld.py:224-277).  Writes the newly decided rounds (`new_c`,
 * swirld.py:274-277) in ascending order to new_rounds[0..*n_new) and adds them to
 * the consensus set.  cap = capacity of new_rounds; SW_ERANGE if too small (state is
 * still updated, *n_new holds the required size).
 */
int sw_decide_fame(sw_ctx* ctx, int32_t* new_rounds, int cap, int* n_new);

/*
 * Multi-GPU building block (no reference counterpart: the reference is one thread): the
 * elections of decide_fame are independent per candidate witness (swirld.py:256-272 given
 * `witnesses` and the voters' strongly-seen sets), so `nparts` contexts holding the same divided
 * hashgraph can each run the candidate rounds max_c + part, max_c + part + nparts, ... .
 * sw_decide_fame_partial writes this part's view — famous[R][n_members] (-1 undecided or not
 * owned) and decided[R] (1: every witness of the round is decided, swirld.py:274-275) — and commits
 * nothing.  The element-wise MAX of all parts' tables (one all-reduce; py-swirld_amd/partition.py)
 * given to sw_commit_fame on every part leaves each context exactly as sw_decide_fame() would:
 * same famous table, consensus set and new_c — and nothing else: the deciding call / voter of a
 * witness (what Node.votes' existence rule needs) is recorded only on the part that ran its
 * election, so after a sw_commit_fame sw_get_vote returns SW_ENOTSUP until sw_reset / sw_rewind.
 */
int sw_decide_fame_partial(sw_ctx* ctx, int part, int nparts, int8_t* famous, uint8_t* decided,
                           int r_cap, int* r_out);
int sw_commit_fame(sw_ctx* ctx, const int8_t* famous, const uint8_t* decided, int R,
                   int32_t* new_rounds, int cap, int* n_new);

/*
 * Multi-GPU building block, part 2 (no reference counterpart — its `network` is a dict,
 * swirld.py:40, 337): the can_see table split by EVENT RANGES.  Every part holds the whole hashgraph
 * (sw_append_events: 16 B per event) and computes the can_see rows of its own range only; the rows
 * are exchanged (RCCL broadcast / all-gather of int32 rows, py-swirld_amd/partition.py StrongSplit),
 * after which sw_divide_rounds finds them in place and runs the round loop without sweeping.
 *   sw_cansee_range   sweeps the rows of [first, first + K) from a halo in front of the range
 *                     (the chunk-parallel sweep, k_cansee_chunks: a parent below the halo is a leaf,
 *                     entries the window cannot know are PROVISIONAL and counted).  Asynchronous.
 *   sw_cansee_repair  repairs those entries from the final rows below the range — which must have
 *                     been imported (or computed) before; device-gated: costs nothing when the sweep
 *                     counted none, sweeps the range again from final rows when they are too many.
 *                     Ranges are repaired in ascending order.
 *   sw_export_rows    copies the rows of [first, first + K) to caller-provided DEVICE memory
 *                     (K * row_stride int32, row_stride = members padded to a multiple of 64:
 *                     sw_row_stride), ordered after the sweep / repair; `user_stream` (a hipStream_t,
 *                     may be NULL = the null stream) is made to wait for the copy, so a collective
 *                     enqueued on it afterwards sends complete rows.
 *   sw_import_rows    the opposite direction: waits (on the device) for what `user_stream` has
 *                     enqueued so far, copies the rows into the table and marks them present.
 * Rows present (swept by sw_cansee_range, imported) are not swept again by sw_divide_rounds; a
 * sw_divide_rounds call must lie entirely inside or entirely outside the present ranges.
 * Fast path with at most 256 members and the plain (non-windowed) table only: SW_ENOTSUP otherwise.
 * sw_get_range_stats synchronises and returns the provisional entries counted, the entries the repair
 * changed and the ranges swept a second time, since the last sw_rewind.
 */
int sw_row_stride(const sw_ctx* ctx);
int sw_cansee_range(sw_ctx* ctx, int64_t first, int64_t K);
int sw_cansee_repair(sw_ctx* ctx, int64_t first, int64_t K);
int sw_export_rows(sw_ctx* ctx, int64_t first, int64_t K, void* dst_device, void* user_stream);
int sw_import_rows(sw_ctx* ctx, int64_t first, int64_t K, const void* src_device, void* user_stream);
int sw_get_range_stats(sw_ctx* ctx, int64_t* provisional, int64_t* repaired, int64_t* resweeps);

/*
 * Multi-GPU building block, part 3 (last bullet; no reference counterpart): ONE hashgraph's ROUND LOOP over
 * `parts` linked contexts — one per GPU of this process, or several on one GPU — split INSIDE an iteration (swirld.py:208-216
 * once per candidate event): the band events whose threshold masks an iteration builds, and the members whose candidate
 * windows it tallies, are dealt to the parts; every part stores what it produces (mask rows and popcounts, round numbers and
 * sees-masks of the band events, its members' verdict words) into the tables of EVERY part through peer-mapped device memory
 * (plain stores and atomics over xGMI: no collective inside an iteration), and the parts' streams meet at the iteration's two
 * kernel boundaries through events.  Everything else of sw_divide_rounds stays replicated: each part holds the whole hashgraph
 * and sweeps the whole can_see table.
 *   sw_split_link    links `parts` (2 .. 8) contexts that hold the SAME events (same sw_append_events calls) and are divided up
 *                    to the same point; peer access between their devices is enabled.  Unit stake only (SW_ENOTSUP otherwise);
 *                    not on the exact (forked) path, not with the windowed table.
 *   afterwards       EVERY part calls sw_divide_rounds with the same arguments, each from its own host thread (the calls meet
 *                    iteration by iteration; a part that never arrives makes the others fail with SW_EIO after 30 s);
 *                    sw_decide_fame / sw_find_order / getters per context as usual — each part ends with the complete state.
 *   sw_rewind        of linked contexts: EVERY part rewinds and is synchronised (sw_synchronize) before ANY part divides again — a
 *                    part's first band kernel stores into the others' tables, which their rewind would wipe afterwards.
 *   sw_split_unlink  dissolves the group (also done by sw_destroy of any of its contexts).
 * Results are those of an unlinked context (tests/test_gpu_split_loop.py: parts on one GPU against the oracle).
 */
int sw_split_link(sw_ctx* const* ctxs, int parts);
int sw_split_unlink(sw_ctx* ctx);

/*
 * Node.find_order(new_c) (swirld.py:280-311) for the given rounds (processed in
 * ascending order like sorted(new_c)).  Appends to the internal `transactions` list
 * and writes the newly ordered event indices, in final order, to out_events.
 */
int sw_find_order(sw_ctx* ctx, const int32_t* rounds, int n_rounds, int32_t* out_events,
                  int64_t cap, int64_t* n_out);

/* ---- getters (lazy dict views of the Node state; all copy device -> caller) ---- */
int sw_get_height(sw_ctx* ctx, int64_t first, int64_t K, int32_t* out);          /* Node.height   */
int sw_get_round(sw_ctx* ctx, int64_t first, int64_t K, int32_t* out);           /* Node.round    */
/* Node.can_see rows: out[K][n_members], entry = latest event of that member seen, -1 absent */
int sw_get_can_see(sw_ctx* ctx, int64_t first, int64_t K, int32_t* out);
int sw_max_round(sw_ctx* ctx, int* out);                                          /* max(witnesses) */
/* Node.witnesses[r][member] for r in [r0, r1): out[(r1-r0)][n_members]; dict order inside
 * a round = ascending event index (registration order, swirld.py:197, 222). */
int sw_get_witnesses(sw_ctx* ctx, int r0, int r1, int32_t* out);
/* Node.famous for the same table: -1 undecided, 0 False, 1 True (swirld.py:263). */
int sw_get_famous(sw_ctx* ctx, int r0, int r1, int8_t* out);
/* Node.famous keyed by event (swirld.py:64) for the events [first, first+K): -1 = undecided or not a
 * witness, else 0 / 1.  Differs from the slot view only with forks (a replaced witness keeps its entry). */
int sw_get_famous_events(sw_ctx* ctx, int64_t first, int64_t K, int8_t* out);
/* Node.consensus membership for r in [r0, r1): 1 if r in consensus (swirld.py:276). */
int sw_get_consensus(sw_ctx* ctx, int r0, int r1, uint8_t* out);
/* Diagnostic: per event the member bitmask {c_ : round[can_see[e][c_]] == round[e]}
 * (the inner test of swirld.py:211-214 / 250-252); out[K][ceil(n/64)] little-endian words. */
int sw_get_sees_mask(sw_ctx* ctx, int64_t first, int64_t K, uint64_t* out);
/* Diagnostic: Node.votes[voter][candidate] for voter = witness (rv, mv), candidate =
 * witness (rc, mc): -1 = no entry, 0/1 = vote (swirld.py:258-272).  Recomputed from the voter
 * masks with the semantics of one batch decide_fame() call; valid after sw_decide_fame. */
int sw_get_vote(sw_ctx* ctx, int rv, int mv, int rc, int mc, int8_t* out);

/*
 * Node.votes IN BULK (swirld.py:60-61, 256-272; kernels in csrc/votes.hip.h): every entry of the voter
 * rounds rv0 <= round(y) < rv1 as one table, computed on the device from the voter masks, the witness table, the coin bits,
 * the stakes and the deciding call / voter of every witness.
 *
 * THE TABLE: one row per pair (voter witness y, candidate round rc) for which votes[y] holds at least one entry for a
 * witness of round rc.  row_voter[row] = the dense index of y, row_cand_round[row] = rc; exists[row][j] and value[row][j],
 * j < ceil(n_members / 64) little-endian words (the stride of sw_get_sees_mask), are member bitmasks: bit mc of exists is set
 * iff votes[y][witnesses[rc][mc]] exists, bit mc of value is that entry's value (value is a subset of exists).  Rows are
 * sorted by (round(y), y, rc) ascending.  Existence and value of every bit are what sw_get_vote(round(y), creator(y), rc,
 * mc) answers on the same context; the comment above that function is the specification (tests/model_votes.py states the
 * table in numpy).
 * PRECONDITIONS as for sw_get_vote: SW_ENOTSUP on the exact path and after sw_commit_fame; SW_ERANGE for rv0 < 0 or rv1
 * beyond the round table; SW_EINVAL when rv1 reaches rounds sw_decide_fame has not seen yet.  rv0 >= rv1: an empty table,
 * SW_OK.  A windowed context is served (no can_see row is read).
 * CAPACITY: *n_rows and *n_entries (host; the set bits of exists) are always written.  cap_rows < *n_rows returns
 * SW_ERANGE and writes no array: cap_rows = 0 (arrays may be NULL) asks for the size.
 * sw_export_votes_device   the four arrays in memory of the context's device (SW_EINVAL otherwise, before anything is
 *   launched; d_exists and d_value 16-byte aligned).  STREAMS as for sw_export_payload_device: the context's stream first
 *   waits for what `user_stream` has enqueued, `user_stream` is made to wait for the table.  The one host synchronisation
 *   is the read-back of the two counts.
 * sw_export_votes   the same with the arrays in HOST memory (written into context scratch by the same kernels, copied out).
 * sw_get_votes_stats   calls, rows and entries exported since sw_create, election levels replayed for them, and — under
 *   sw_set_profiling — the host time in ms of the most recent call's phases: phase_ms[2] = plan + existence + counts,
 *   rows + values.  Any pointer may be NULL.
 */
int sw_export_votes_device(sw_ctx* ctx, int rv0, int rv1, int64_t cap_rows,
                           int32_t* d_row_voter, int32_t* d_row_cand_round, uint64_t* d_exists, uint64_t* d_value,
                           int64_t* n_rows, int64_t* n_entries, void* user_stream);
int sw_export_votes(sw_ctx* ctx, int rv0, int rv1, int64_t cap_rows,
                    int32_t* row_voter, int32_t* row_cand_round, uint64_t* exists, uint64_t* value,
                    int64_t* n_rows, int64_t* n_entries);
int sw_get_votes_stats(sw_ctx* ctx, int64_t* calls, int64_t* rows, int64_t* entries, int64_t* levels, double* phase_ms);
/* Node.transactions / Node.idx: total ordered so far, and a slice of the order. */
int sw_num_ordered(sw_ctx* ctx, int64_t* out);
int sw_get_transactions(sw_ctx* ctx, int64_t first, int64_t K, int32_t* out);

/*
 * Gossip side, from the device-resident state.
 * sw_get_known_heights: what Node.sync puts into its request (swirld.py:125-126):
 *   out[member] = height of the newest event of that member the (divided) event `head_event`
 *   can see, -1 if none.
 * sw_sync_diff: what Node.ask_sync answers (swirld.py:154-161): the events a peer that reported
 *   known_height[member] (-1: member unknown to it) is missing, as chain position ranges
 *   [pos_first[m], pos_end[m]) of every member's self-parent chain — the ancestors-or-self of
 *   `head_event` above the peer's heights, the head always included.  Equals the reference's
 *   height-pruned BFS as a SET whenever the heights come from a real can_see row; for arbitrary
 *   heights it is a superset (a receiver drops what it cannot validate).
 * sw_get_chain_events: the event indices at chain positions [p0, p1) of one member.
 */
int sw_get_known_heights(sw_ctx* ctx, int64_t head_event, int32_t* out);
int sw_sync_diff(sw_ctx* ctx, int64_t head_event, const int32_t* known_height, int32_t* pos_first,
                 int32_t* pos_end, int64_t* n_events);
int sw_get_chain_events(sw_ctx* ctx, int member, int32_t p0, int32_t p1, int32_t* out);

/*
 * Answering a sync ON THE DEVICE (Node.ask_sync swirld.py:148-161 and the asking half of Node.sync,
 * swirld.py:125-136; kernels in csrc/gossip.hip.h).  The events sw_sync_diff names leave the answering context as the arrays
 * sw_ingest_payload_device takes, so that a payload goes from one context's device memory into another's — or into a send
 * buffer — without a host copy of any event.
 *
 * sw_get_known_heights_device   sw_get_known_heights with the answer left in device memory: d_out holds n_members int32 (not
 *   the padded row: nothing is written behind them) in memory of the context's device (SW_EINVAL otherwise); `user_stream`
 *   (a hipStream_t or NULL, the null stream) is made to wait for the result.
 *
 * sw_export_payload_device   exports exactly the events sw_sync_diff(head_event, known_height) names; *n_out (host) is that
 *   call's n_events.  ORDER: member-major — member 0's range first — and chain order inside a member: with off[m] the
 *   exclusive prefix sum of the range lengths, slot s of member m is the event at chain position pos_first[m] + (s - off[m]).
 *   This order is NOT topological: ordering is the ingest's job.  PER SLOT: d_id32 the event's id; d_sp_id32 / d_op_id32 its
 *   parents' ids (32 zero bytes each for a root); d_arity (uint8) 2, or 0 for a root; d_creator the dense member index; d_t,
 *   d_sig64 (either may be NULL: not exported) bit-exact copies of what was appended; d_event (may be NULL) the dense index
 *   of the event in THIS context.  d_known_height: n_members int32 in device memory, negative = member unknown to the
 *   asker; NULL = the asker knows nobody.  The heights are the asker's claim: they are compared with stored heights and
 *   never used as an index.  Every array must lie in memory of the context's device, the three id arrays and d_sig64
 *   16-byte aligned: SW_EINVAL before anything is launched.
 *   CAPACITY: `cap` is the number of events the arrays can take.  If the diff is larger the call returns SW_ERANGE with
 *   *n_out = the number required and writes nothing; cap = 0 with all arrays NULL is how to ask for the size.
 *   STREAMS: as for sw_export_rows — the context's stream first waits, on the device, for what `user_stream` has enqueued so
 *   far (the producer of d_known_height), and `user_stream` is then made to wait for the gather: an ingest enqueued on it, or
 *   given it as its user_stream, reads complete arrays.  The call synchronises once, to read the count.
 *   NEEDS a complete id index (SW_ENOTSUP otherwise; sw_set_event_ids), the fast path (SW_ENOTSUP on the exact, forked
 *   path), a divided, resident head (SW_ERANGE); SW_EIO on a poisoned context.  Works with the windowed table wherever
 *   sw_sync_diff does.  READ-ONLY: no getter and no later call answers differently afterwards (counters.kernel_launches
 *   moves).
 * sw_export_payload    the same with every array in HOST memory: gathered into context scratch by the same device code,
 *   then copied out.
 *
 * sw_sync_pull   the reference's sync without the new event (swirld.py:125-136) between two contexts on ONE device: dst
 *   computes its known heights at dst_head, src computes ranges, count and the gather (into scratch src owns) at src_head,
 *   dst ingests through the body of sw_ingest_payload_device, its stream ordered behind src's; nothing but the count
 *   crosses to the host.  *n_sent = the events exported, *n_stored = the events dst stored: its events [count before, count
 *   before + n_stored), whose ids sw_get_event_ids gives.  Preconditions of both halves; contexts on different devices:
 *   SW_ENOTSUP; dst == src, or differing member counts: SW_EINVAL (same members and stake are the caller's business).  The
 *   error message is left in dst.
 *
 * sw_get_export_stats   export calls (sw_sync_pull counts for its src) and events exported since sw_create, and — under
 *   sw_set_profiling — the host time in ms of the most recent call's phases: phase_ms[2] = ranges + count, gather.  Any
 *   pointer may be NULL.
 */
int sw_get_known_heights_device(sw_ctx* ctx, int64_t head_event, int32_t* d_out, void* user_stream);
int sw_export_payload_device(sw_ctx* ctx, int64_t head_event, const int32_t* d_known_height, int64_t cap,
                             uint8_t* d_id32, uint8_t* d_sp_id32, uint8_t* d_op_id32, uint8_t* d_arity, int32_t* d_creator,
                             double* d_t, uint8_t* d_sig64, int32_t* d_event, void* user_stream, int64_t* n_out);
int sw_export_payload(sw_ctx* ctx, int64_t head_event, const int32_t* known_height, int64_t cap,
                      uint8_t* id32, uint8_t* sp_id32, uint8_t* op_id32, uint8_t* arity, int32_t* creator,
                      double* t, uint8_t* sig64, int32_t* event, int64_t* n_out);
int sw_sync_pull(sw_ctx* dst, int64_t dst_head, sw_ctx* src, int64_t src_head, int64_t* n_sent, int64_t* n_stored);
int sw_get_export_stats(sw_ctx* ctx, int64_t* calls, int64_t* events, double* phase_ms);

/*
 * What find_order decides per event, kept (Node.find_order swirld.py:283-309; kernels in csrc/consensus.hip.h).  The
 * reference computes, for every event x it orders, the ROUND RECEIVED r (swirld.py:283: the first decided round whose famous
 * witnesses all see x) and the CONSENSUS TIMESTAMP ts[x] (swirld.py:305: .5 * (first + second) of the middle of the sorted
 * times at which the creators of those witnesses first saw x), sorts by them (swirld.py:306) and drops them: its Node keeps
 * neither.  Here every sw_find_order call on the fast path leaves both in per-event tables on the device, and its part of
 * the order in a device copy of `transactions`; sw_rewind / sw_reset empty them with the order.
 *
 * sw_get_round_received   swirld.py:283-309: out[i] = round received of event first + i, -1 = not ordered yet.
 * sw_get_consensus_time   swirld.py:283-309: out[i] = consensus timestamp of event first + i, bit for bit the double
 *   swirld.py:305 computes; a quiet NaN = not ordered yet.  Both: [first, first + K) inside [0, sw_num_events), SW_ERANGE
 *   otherwise; out NULL or K = 0: nothing to do.  One small kernel into context scratch and one copy back.
 *
 * sw_export_ordered_device   swirld.py:283-309 as a stream: positions [first, first + K) of the order (the indices of
 *   sw_get_transactions), per position p the dense index of the event (d_event), its id (d_id32, 32 B), its creator's member
 *   index (d_creator), its round received (d_round_received) and its consensus timestamp (d_time) — non-decreasing in
 *   (round received, timestamp) along p, as swirld.py:306-309 appends them.  Every array may be NULL: not wanted.
 *   [first, first + K) inside [0, sw_num_ordered): SW_ERANGE otherwise, nothing written.  d_id32 non-NULL NEEDS a complete
 *   id index (SW_ENOTSUP otherwise; sw_set_event_ids) and 16-byte alignment (SW_EINVAL); every array must lie in memory of
 *   the context's device (SW_EINVAL before anything is launched).
 *   STREAMS: as for sw_export_payload_device — the context's stream first waits, on the device, for what `user_stream` (a
 *   hipStream_t or NULL, the null stream) has enqueued so far, and `user_stream` is then made to wait for the gather: what
 *   the caller enqueues on it next reads complete arrays.  No host synchronisation.
 * sw_export_ordered   swirld.py:283-309, the same with every array in HOST memory: gathered into context scratch by the same
 *   device code, then copied out.
 *   All four: the fast path only (SW_ENOTSUP on the exact, forked path); SW_EIO on a poisoned context; SW_EINVAL for a NULL
 *   context.  READ-ONLY: no getter and no later call answers differently afterwards (counters.kernel_launches and the
 *   statistics below move).
 *
 * sw_get_consensus_stats   swirld.py:283-309 has no counterpart: sw_find_order calls that recorded events and the events
 *   they recorded, export calls (both forms) and the positions they exported, since sw_create.  Any pointer may be NULL.
 */
int sw_get_round_received(sw_ctx* ctx, int64_t first, int64_t K, int32_t* out);
int sw_get_consensus_time(sw_ctx* ctx, int64_t first, int64_t K, double* out);
int sw_export_ordered_device(sw_ctx* ctx, int64_t first, int64_t K, int32_t* d_event, uint8_t* d_id32, int32_t* d_creator,
                             int32_t* d_round_received, double* d_time, void* user_stream);
int sw_export_ordered(sw_ctx* ctx, int64_t first, int64_t K, int32_t* event, uint8_t* id32, int32_t* creator,
                      int32_t* round_received, double* time);
int sw_get_consensus_stats(sw_ctx* ctx, int64_t* record_calls, int64_t* recorded_events, int64_t* export_calls,
                           int64_t* exported_events);

/*
 * Ingest-side crypto in batches — what Node.is_valid_event spends its time in
 * (swirld.py:99-103), stateless, one GPU thread per message; message i = msgs[msg_off[i] .. msg_off[i+1]).
 * sw_crypto_verify_batch: ok[i] = 1 iff libsodium's crypto_sign_verify_detached(sig_i, msg_i, pk_i)
 *   would return 0 (swirld.py:99-100 via pysodium): Ed25519 with libsodium 1.0.18's rejections
 *   (non-canonical S, small-order R or key, non-canonical key).
 * sw_crypto_hash_batch: out32[i] = BLAKE2b-256(msg_i) = crypto_generichash(msg_i), the event id
 *   (swirld.py:95, 103).
 * One signature costs a GPU thread ~1-2 ms of latency (a CPU core: ~60 us): batches of thousands
 * (a bulk sync payload) are where the device wins; Node.sync uses it above a batch-size threshold.
 */
int sw_crypto_verify_batch(int device, int64_t K, const uint8_t* msgs, const int64_t* msg_off,
                           const uint8_t* sig64, const uint8_t* pk32, uint8_t* ok);
int sw_crypto_hash_batch(int device, int64_t K, const uint8_t* msgs, const int64_t* msg_off, uint8_t* out32);

/*
 * Validating a payload ON THE DEVICE against the member keys (the crypto of Node.is_valid_event, swirld.py:97-103; kernels
 * in csrc/validate.hip.h).  A hashgraph's members are fixed, so the context keeps a table of fixed-base
 * multiples of every member's key (48 KB per member) and a verification is 128 table additions and one inversion.  The
 * verdicts are left in device memory: they are the d_ok sw_ingest_payload_device takes.
 *
 * sw_set_member_keys   pk32: n_members * 32 bytes in HOST memory, key m the Ed25519 public key of member m.  Builds the
 *   table on the device (one kernel, one synchronisation).  A key libsodium 1.0.18 refuses (non-canonical, small order, not
 *   on the curve) makes its member UNUSABLE: every event of that member is invalid; *n_unusable (may be NULL) counts them.
 *   Keys survive sw_rewind and sw_reset; setting keys again rebuilds the table.
 * sw_get_member_keys   the keys as set and one byte per member, 1 = usable (either pointer may be NULL).  SW_ENOTSUP when no
 *   keys are set.
 *
 * sw_validate_payload_device   K events, every array in memory of the context's device (a host pointer: SW_EINVAL before
 *   anything is launched).  Event i was signed over d_msgs[d_msg_off[i] .. d_msg_off[i+1]) (dumps(ev[:-1]), swirld.py:99) with
 *   signature d_sig64 + 64 i by member d_creator[i]; its id d_id32 + 32 i is the hash of d_whole[d_whole_off[i] ..
 *   d_whole_off[i+1]) (dumps(ev), swirld.py:103).  d_whole, d_whole_off, whole_bytes all NULL / 0: no id check (d_id32 is
 *   then ignored).  msg_bytes / whole_bytes are the lengths of the two byte buffers; the offset arrays hold K + 1 entries.
 *   d_ok[i] = 1 iff  creator i is in [0, n_members) and its key is usable,  [off[i], off[i+1]) of both buffers is
 *   non-negative, non-decreasing and inside the buffer (the offsets derive from a peer's bytes: nothing outside the buffers
 *   is ever read),  libsodium 1.0.18's crypto_sign_verify_detached(sig_i, msg_i, pk[creator_i]) would return 0,  and — with
 *   the id check — BLAKE2b-256(whole_i) equals id_i.  Otherwise 0.  d_id32 and the offsets must be 8-byte aligned.
 *   STREAMS: as for sw_export_payload_device — the context's stream first waits, on the device, for what `user_stream` (a
 *   hipStream_t or NULL, the null stream) has enqueued so far, and `user_stream` is then made to wait for the verdicts: an
 *   ingest enqueued on it, or given it as its user_stream, reads a complete d_ok.  No allocation, no copy and no host
 *   synchronisation.  K = 0 is a no-op.
 *   SW_ENOTSUP when no keys are set; SW_EIO on a poisoned context.  Works on the exact (forked) path and with the windowed
 *   table: it touches no hashgraph state.  READ-ONLY: no getter and no later call answers differently afterwards
 *   (counters.kernel_launches and the statistics below move).
 * sw_validate_payload   the same with every array, and ok, in HOST memory: staged into context scratch, judged by the same
 *   kernel, copied back.
 *
 * sw_get_validate_stats   validation calls and the events they judged since sw_create, the events accepted (counted by the
 *   host-array form only: the device form never reads its verdicts), table builds, and — under sw_set_profiling — the host
 *   time in ms of the last table build and of the last validation: phase_ms[2].  Any pointer may be NULL.
 */
int sw_set_member_keys(sw_ctx* ctx, const uint8_t* pk32, int32_t* n_unusable);
int sw_get_member_keys(sw_ctx* ctx, uint8_t* pk32_out, uint8_t* usable_out);
int sw_validate_payload_device(sw_ctx* ctx, int64_t K, const uint8_t* d_msgs, const int64_t* d_msg_off, int64_t msg_bytes,
                               const uint8_t* d_whole, const int64_t* d_whole_off, int64_t whole_bytes,
                               const uint8_t* d_sig64, const int32_t* d_creator, const uint8_t* d_id32, uint8_t* d_ok,
                               void* user_stream);
int sw_validate_payload(sw_ctx* ctx, int64_t K, const uint8_t* msgs, const int64_t* msg_off, int64_t msg_bytes,
                        const uint8_t* whole, const int64_t* whole_off, int64_t whole_bytes,
                        const uint8_t* sig64, const int32_t* creator, const uint8_t* id32, uint8_t* ok);
int sw_get_validate_stats(sw_ctx* ctx, int64_t* calls, int64_t* events, int64_t* accepted, int64_t* table_builds,
                          double* phase_ms);

/*
 * The signed bytes of events, built ON THE DEVICE (kernels in csrc/pack.hip.h): the two byte streams
 * sw_validate_payload_device reads — dumps(ev[:-1]), what the signature covers (swirld.py:99), and dumps(ev), what the id
 * is the hash of (swirld.py:95, :103) — from the arrays sw_export_payload_device writes.  For parents () or two 32-byte
 * ids, a float timestamp, a 32-byte creator key, a 64-byte signature and data None or a bytes object of at most 60 000
 * bytes, pickle protocol 4 writes a fixed template of one frame without memo reads (tests/model_pack.py); these calls
 * write exactly those bytes.
 *
 * sw_set_event_class / sw_get_event_class   module and qualified name of the Event class (Event.__module__,
 *   Event.__qualname__): they are part of dumps(ev) and so of every id.  NUL-terminated UTF-8 of 1 .. 255 bytes each, else
 *   SW_EINVAL; default "swirld", "Event".  The getter's buffers hold 256 bytes each (either may be NULL).  The setting
 *   survives sw_rewind and sw_reset.
 * sw_pack_bound   upper bounds of the two streams for ANY K events with data_bytes bytes of data between them (host
 *   arithmetic: 137 K + data_bytes, and (214 + len(module) + len(qualname)) K + data_bytes).
 *
 * sw_pack_events_device   K events, every array in memory of the context's device (a host pointer: SW_EINVAL before
 *   anything is launched).  In: d_sp_id32, d_op_id32, d_arity, d_creator, d_t, d_sig64 as sw_export_payload_device writes
 *   them (the parents' ids are read only where the arity is 2); the creator's key bytes come from the context
 *   (sw_set_member_keys; SW_ENOTSUP without).  Data: d_data, d_data_off, data_bytes and d_data_none all NULL / 0 means
 *   every event's data is None; otherwise event i's data is d_data[d_data_off[i] .. d_data_off[i+1]) (K + 1 int64 offsets,
 *   an empty range is b''), and d_data_none (uint8 per event, may be NULL) nonzero marks None.
 *   Out: d_msgs / d_msg_off and d_whole / d_whole_off — bytes and K + 1 int64 offsets each, in the form
 *   sw_validate_payload_device takes; the totals are off[K].  Bytes at and beyond off[K] are not written.  d_encodable
 *   (uint8 per event, may be NULL): 0 for an event that has no such bytes — an arity that is neither 0 nor 2, a creator
 *   outside [0, n_members), a data range that is negative, decreasing, beyond data_bytes or longer than 60 000.  Such an
 *   event has length 0 in both streams and nothing is read for it (the offsets may derive from a peer's bytes: nothing
 *   outside [0, data_bytes) is ever read).  Its verdict from sw_validate_payload_device is 0.
 *   msg_cap / whole_cap: the capacities of d_msgs / d_whole; below sw_pack_bound's values: SW_ERANGE, before any launch.
 *   The two byte streams, d_sig64 and the id arrays must be 16-byte aligned, offsets and timestamps 8-byte aligned
 *   (SW_EINVAL).  STREAMS: as for sw_validate_payload_device — the context's stream first waits for what `user_stream` has
 *   enqueued so far, and `user_stream` is then made to wait for the result.  No allocation beyond growing context
 *   scratch, no copy of an array (the first call after sw_create or sw_set_event_class uploads the class header, at most
 *   518 bytes) and no host synchronisation.  K = 0 is a no-op that writes off[0] = 0.  SW_EIO on a poisoned context.
 *   READ-ONLY with respect to the hashgraph: it works on the exact path and with the windowed table, and no getter and
 *   no later call answers differently afterwards (counters.kernel_launches and the statistics below move).
 * sw_pack_events   the same with every array in HOST memory, staged through context scratch; *msg_bytes / *whole_bytes
 *   (may be NULL) receive the totals.
 *
 * sw_sync_pull_validated   sw_sync_pull with is_valid_event's crypto in the middle (swirld.py:97-103): after src's gather,
 *   dst — on its stream, behind src's — packs the exported arrays into scratch of its own, validates them with ITS OWN
 *   member keys and event class (id check on), ANDs the verdicts with the encodable flags and ingests with that as d_ok.
 *   *n_valid: the events that passed, counted on the device and read at the call's final drain.  Preconditions: those of
 *   sw_sync_pull, and keys set in dst (SW_ENOTSUP, nothing stored).  The context does NOT store event data: the bytes are
 *   built with data None, so events that src's members signed with other data fail the id check and are rejected one by
 *   one, with their descendants.  sw_sync_pull_data (below) is the pull for hashgraphs whose events carry data.
 *
 * sw_get_pack_stats   pack calls (sw_sync_pull_validated's included) and the events they encoded since sw_create, the
 *   bytes written (counted by the host-array form only: the device form never reads its totals), and — under
 *   sw_set_profiling — the host time in ms of the last call's lengths-and-scan and of its two writers: phase_ms[2].
 */
int sw_set_event_class(sw_ctx* ctx, const char* module, const char* qualname);
int sw_get_event_class(sw_ctx* ctx, char* module_out, char* qualname_out);
int sw_pack_bound(sw_ctx* ctx, int64_t K, int64_t data_bytes, int64_t* msg_bytes, int64_t* whole_bytes);
int sw_pack_events_device(sw_ctx* ctx, int64_t K, const uint8_t* d_sp_id32, const uint8_t* d_op_id32, const uint8_t* d_arity,
                          const int32_t* d_creator, const double* d_t, const uint8_t* d_sig64, const uint8_t* d_data,
                          const int64_t* d_data_off, int64_t data_bytes, const uint8_t* d_data_none, uint8_t* d_msgs,
                          int64_t* d_msg_off, int64_t msg_cap, uint8_t* d_whole, int64_t* d_whole_off, int64_t whole_cap,
                          uint8_t* d_encodable, void* user_stream);
int sw_pack_events(sw_ctx* ctx, int64_t K, const uint8_t* sp_id32, const uint8_t* op_id32, const uint8_t* arity,
                   const int32_t* creator, const double* t, const uint8_t* sig64, const uint8_t* data, const int64_t* data_off,
                   int64_t data_bytes, const uint8_t* data_none, uint8_t* msgs, int64_t* msg_off, int64_t msg_cap, uint8_t* whole,
                   int64_t* whole_off, int64_t whole_cap, uint8_t* encodable, int64_t* msg_bytes, int64_t* whole_bytes);
int sw_sync_pull_validated(sw_ctx* dst, int64_t dst_head, sw_ctx* src, int64_t src_head, int64_t* n_sent, int64_t* n_valid,
                           int64_t* n_stored);
int sw_get_pack_stats(sw_ctx* ctx, int64_t* calls, int64_t* events, int64_t* bytes, double* phase_ms);

/*
 * The DATA of events kept on the device (kernels in csrc/data.hip.h): Event.d, the transaction an event
 * carries (swirld.py:30, :82-95) — a bytes object of 0 .. 60 000 bytes, or None, per event.  It is part of what is signed
 * and of what the id is the hash of.  A context keeps it in one byte arena with int64 offsets and one None flag per event,
 * allocated on first use and grown geometrically; the layout is that of sw_pack_events_device's data arguments.  The store
 * is COMPLETE when every stored event has an entry (an empty context counts), the semantics of the id index: events
 * appended by index (sw_append_events[_device], sw_ingest_payload[_device], sw_sync_pull[_validated]) get NO entry, and the
 * store stays incomplete until sw_set_event_data has caught up.  sw_rewind keeps the data (the events stay), sw_reset
 * forgets it.  The store is independent of the voting state: it works on the exact path and with the windowed table.
 * OUT OF SCOPE: the data of rows the window has evicted is NOT evicted, and data that is neither None nor bytes cannot
 * be stored (a caller stores None for it and keeps the object itself).
 *
 * sw_set_event_data   the data of the stored events [first, first + K), host arrays: event first + i has
 *   data[data_off[i] .. data_off[i+1]) (K + 1 int64 offsets; an empty range is b''), data_none (uint8 per event, may be
 *   NULL) nonzero marks None whatever the range.  data, data_off, data_none all NULL (data_bytes 0): every event is None.
 *   `first` must equal the number of events that have data (SW_EINVAL); first + K beyond the stored events: SW_ERANGE.  An
 *   offset that is negative, decreasing, beyond data_bytes, or a length above 60 000: SW_EINVAL, nothing stored.
 * sw_set_event_data_device   the same from memory of the context's device (a host pointer: SW_EINVAL before anything is
 *   launched; d_data_off 8-byte aligned), with the stream contract of sw_pack_events_device.  The offsets are checked on
 *   the device; the call synchronises once, to read the byte total and the verdict.
 * sw_get_event_data   the entries of [first, first + K) (beyond the events that have data: SW_ERANGE): K + 1 offsets
 *   rebased to 0, the bytes, the None flags (a None entry has an empty range).  *n_bytes receives the bytes required;
 *   cap below that: SW_ERANGE, nothing written.
 * sw_gather_event_data_device   the data of K events named by DENSE INDEX in d_event (int32, device memory), in the order
 *   given, repeats allowed: d_data_off receives K + 1 int64 offsets from 0, d_data the bytes back to back, d_data_none the
 *   flags.  This turns the d_event array of sw_export_payload_device, or of sw_export_ordered_device, into the payloads of
 *   a sync answer or of the consensus stream.  An index outside [0, events that have data): SW_ERANGE, nothing written.
 *   The call synchronises once, to read the byte total and the bad-index count; *n_bytes receives the total; cap (the
 *   capacity of d_data) below it: SW_ERANGE, nothing written; cap = 0 with the three arrays NULL asks for the size
 *   (SW_OK when it is 0).  d_data 16-byte aligned, d_data_off 8-byte aligned, every array in memory of the context's
 *   device: SW_EINVAL before any launch.  Streams as above.  READ-ONLY with respect to every getter (kernel_launches and
 *   the statistics below move).
 * sw_gather_event_data   the same with host arrays, staged through context scratch.
 * sw_ingest_payload_data_device   sw_ingest_payload_device whose accepted events bring their data: the four data
 *   arguments as for sw_pack_events_device, one range per payload event.  Needs a complete id index AND a complete data
 *   store (SW_ENOTSUP, nothing stored).  An event whose range is negative, decreasing, beyond data_bytes or longer than
 *   60 000 is not valid: its d_index_out is -3 (its descendants' -6), the rule sw_pack_events_device's d_encodable states.
 *   The data of the events stored by the call is appended in dense-index order.  Memory for the whole payload is reserved
 *   before anything is committed; behind the commit a failure leaves the context poisoned (SW_EIO from then on), as a
 *   failed id-table insert does.  The buffers may derive from a peer's bytes: no byte outside [0, data_bytes) is read and
 *   no offset is followed before it is checked.  The ranges of a peer may OVERLAP (offsets that jump back across a rejected
 *   event): when the usable ranges together hold more than data_bytes bytes the whole payload is refused, SW_EINVAL,
 *   nothing stored — so what is appended never exceeds what was reserved.  A usable range is required of EVERY event,
 *   also of one whose d_data_none flag is set (the flag decides between None and the range's bytes, it does not excuse an
 *   unusable range; sw_set_event_data and sw_pack_events_device's d_encodable judge the same way).
 *   STREAMS: as for sw_ingest_payload_device — the context's stream first waits for what `user_stream` has enqueued so
 *   far; the call synchronises with the host before it returns (after the fold, inside the ingest, and after the copy of
 *   the data), so on return every array, the data arrays included, may be reused or freed, and d_index_out is complete.
 * sw_ingest_payload_data   the same with host arrays.
 * sw_sync_pull_data   sw_sync_pull (validate = 0) or sw_sync_pull_validated (validate != 0) for events WITH data: src
 *   gathers the data of the exported events into its scratch, beside the other arrays (one more synchronisation of src's
 *   stream, for the byte total); with `validate`, dst packs the signed bytes with that data, validates with its own keys,
 *   ANDs the encodable flags, and ingests through the data ingest.  Needs complete data stores on both sides
 *   (SW_ENOTSUP).  Only the event count and the byte total cross to the host.  *n_valid is written only with `validate`.
 * sw_get_data_stats   events that have data, arena bytes in use, store calls (set and ingest), gather calls (sw_sync_pull_data's
 *   included), bytes gathered, and — under sw_set_profiling — the host time in ms of the last call's lengths + scan and of
 *   its copy: phase_ms[2].  Any pointer may be NULL.
 */
int sw_set_event_data(sw_ctx* ctx, int64_t first, int64_t K, const uint8_t* data, const int64_t* data_off, int64_t data_bytes,
                      const uint8_t* data_none);
int sw_set_event_data_device(sw_ctx* ctx, int64_t first, int64_t K, const uint8_t* d_data, const int64_t* d_data_off,
                             int64_t data_bytes, const uint8_t* d_data_none, void* user_stream);
int sw_get_event_data(sw_ctx* ctx, int64_t first, int64_t K, int64_t cap, uint8_t* data, int64_t* data_off, uint8_t* data_none,
                      int64_t* n_bytes);
int sw_gather_event_data_device(sw_ctx* ctx, int64_t K, const int32_t* d_event, int64_t cap, uint8_t* d_data, int64_t* d_data_off,
                                uint8_t* d_data_none, void* user_stream, int64_t* n_bytes);
int sw_gather_event_data(sw_ctx* ctx, int64_t K, const int32_t* event, int64_t cap, uint8_t* data, int64_t* data_off,
                         uint8_t* data_none, int64_t* n_bytes);
int sw_ingest_payload_data_device(sw_ctx* ctx, int64_t K, const uint8_t* d_id32, const uint8_t* d_sp_id32, const uint8_t* d_op_id32,
                                  const uint8_t* d_arity, const int32_t* d_creator, const uint8_t* d_ok, const double* d_t,
                                  const uint8_t* d_sig64, void* user_stream, int32_t* d_index_out, int64_t* n_stored,
                                  const uint8_t* d_data, const int64_t* d_data_off, int64_t data_bytes, const uint8_t* d_data_none);
int sw_ingest_payload_data(sw_ctx* ctx, int64_t K, const uint8_t* id32, const uint8_t* sp_id32, const uint8_t* op_id32,
                           const uint8_t* arity, const int32_t* creator, const uint8_t* ok, const double* t, const uint8_t* sig64,
                           int32_t* index_out, int64_t* n_stored, const uint8_t* data, const int64_t* data_off, int64_t data_bytes,
                           const uint8_t* data_none);
int sw_sync_pull_data(sw_ctx* dst, int64_t dst_head, sw_ctx* src, int64_t src_head, int validate, int64_t* n_sent, int64_t* n_valid,
                      int64_t* n_stored);
int sw_get_data_stats(sw_ctx* ctx, int64_t* events, int64_t* bytes, int64_t* store_calls, int64_t* gather_calls,
                      int64_t* gather_bytes, double* phase_ms);

/*
 * Answering a sync BY THE PRUNED WALK, forked hashgraphs included (Node.ask_sync swirld.py:148-161; kernels in
 * csrc/walk.hip.h).  sw_sync_diff describes the answer as one chain range per member and so stops at the
 * first forked event; these calls run the reference's walk itself — a BFS from the head over the parents that does not
 * descend below what the asker reported per member (swirld.py:154-161) — and work on the fast AND the exact path.  None of
 * them changes what an existing call answers; in windowed mode (sw_set_window) all of them return SW_ENOTSUP.
 *
 * THE SET (swirld.py:154-161), for ANY heights: head_event is in; a parent p of an included event is in iff
 * known[creator(p)] < 0 or height(p) > known[creator(p)]; nothing is reached through an excluded event.  `known`: n_members
 * int32, negative = member unknown to the asker, NULL = the asker knows nobody.  `cap` (may be NULL): n_members int32, every
 * entry >= -1, INT32_MAX = no cap; the walk prunes at min(known[c], cap[c]), so a cap of -1 sends everything of that member.
 * Both are the asker's / caller's claim: compared with stored heights, never used as an index.  With real can_see heights
 * on a fork-free hashgraph the set is sw_sync_diff's; with other heights it is a subset of it (sw_sync_diff's header).
 * THE ORDER: ascending dense index — deterministic, and topological (parents have lower indices).
 *
 * sw_get_fork_trunks   the trunk rule of a forked member (one reported height cannot say which branch the asker holds):
 *   trunk_out[c] (host, n_members) = the smallest height among the stored events of member c that are the self-parent of
 *   at least two stored events; -1 if c has at least two roots; INT32_MAX if c has not forked (all INT32_MAX on a fork-free
 *   context).  Passed as `cap`, it prunes a forked member's events at its earliest fork point.  Either path.
 *
 * sw_sync_walk   swirld.py:154-161: the set as dense indices, ascending, in events_out (host).  known, cap in host memory.
 *   CAPACITY: cap_events is the number of entries events_out can take; a larger set returns SW_ERANGE with *n_out = the
 *   number required and writes nothing; cap_events = 0 with events_out NULL asks for the size.  Needs NO id index.
 *
 * sw_export_walk_device   swirld.py:154-161, 76-95: the set as the arrays sw_ingest_payload_device takes, PER SLOT as
 *   sw_export_payload_device writes them (id, parents' ids or 32 zero bytes each for a root, arity 2 or 0, creator, d_t,
 *   d_sig64, d_event; the last three may be NULL), slot s holding the s-th event in ascending dense index.  d_known, d_cap
 *   and every array in memory of the context's device, the three id arrays and d_sig64 16-byte aligned (SW_EINVAL before
 *   anything is launched).  CAPACITY as above (cap_events = 0 with all arrays NULL asks for the size).  STREAMS as for
 *   sw_export_payload_device: the context's stream first waits for what `user_stream` has enqueued, `user_stream` is made to
 *   wait for the gather; the call synchronises once, to read the count.  NEEDS a complete id index (SW_ENOTSUP), a divided,
 *   resident head (SW_ERANGE); SW_EIO on a poisoned context, and if the walk meets a table entry out of range (the context
 *   is poisoned then).  READ-ONLY otherwise (counters.kernel_launches moves).
 * sw_export_walk   the same with every array in HOST memory.
 *
 * sw_sync_pull_walk   swirld.py:125-136 between two contexts on ONE device, as sw_sync_pull_data, with src answering by the
 *   walk: dst's known heights at dst_head, src's walk at src_head, then — validate != 0 — the signed bytes judged by dst's
 *   keys (sw_sync_pull_validated), — data != 0 — the events' data from src's store into dst's (sw_sync_pull_data), and dst's
 *   ingest.  use_trunks != 0: the walk is capped by SRC's fork trunks, which stay on the device — the answerer applies the
 *   rule.  Either context may be on either path (an exact dst ingests through the host append).  *n_sent, *n_valid (written
 *   only when validate != 0), *n_stored and the error codes as for sw_sync_pull_data.
 *
 * sw_get_walk_stats   walk calls and events named since sw_create, the levels of the most recent walk, and — under
 *   sw_set_profiling — the host time in ms of the most recent call's phases: phase_ms[3] = walk + count, list, gather.  Any
 *   pointer may be NULL.
 */
int sw_get_fork_trunks(sw_ctx* ctx, int32_t* trunk_out);
int sw_sync_walk(sw_ctx* ctx, int64_t head_event, const int32_t* known, const int32_t* cap, int64_t cap_events,
                 int32_t* events_out, int64_t* n_out);
int sw_export_walk_device(sw_ctx* ctx, int64_t head_event, const int32_t* d_known, const int32_t* d_cap, int64_t cap_events,
                          uint8_t* d_id32, uint8_t* d_sp_id32, uint8_t* d_op_id32, uint8_t* d_arity, int32_t* d_creator,
                          double* d_t, uint8_t* d_sig64, int32_t* d_event, void* user_stream, int64_t* n_out);
int sw_export_walk(sw_ctx* ctx, int64_t head_event, const int32_t* known, const int32_t* cap, int64_t cap_events,
                   uint8_t* id32, uint8_t* sp_id32, uint8_t* op_id32, uint8_t* arity, int32_t* creator,
                   double* t, uint8_t* sig64, int32_t* event, int64_t* n_out);
int sw_sync_pull_walk(sw_ctx* dst, int64_t dst_head, sw_ctx* src, int64_t src_head, int use_trunks, int validate, int data,
                      int64_t* n_sent, int64_t* n_valid, int64_t* n_stored);
int sw_get_walk_stats(sw_ctx* ctx, int64_t* calls, int64_t* events, int64_t* levels, double* phase_ms);

/*
 * The WIRE BYTES of a sync answer, built and parsed on the device (kernels in csrc/wire.hip.h).  The canonical
 * form is a protocol-4 pickle without frames that any pickle.loads turns into (head, {id: Event(d, p, t, c, s)}), i.e. what
 * Node.ask_sync pickles (swirld.py:166) and Node.sync unpickles (swirld.py:129); it carries a table of record offsets in a
 * bytes object that is pushed and popped, so that one lane owns one record.  tests/model_wire.py states the layout.
 *
 * sw_pack_message_bound    upper bound of the message of any K events with data_bytes bytes of data.
 * sw_pack_message_device   the message of K events from DEVICE arrays: those sw_export_walk_device and
 *   sw_gather_event_data_device leave, plus the head's id (32 bytes).  d_msg (16-byte aligned, msg_cap >= the bound, else
 *   SW_ERANGE) receives the bytes, *d_msg_len (device memory, 8-byte aligned) the length.  ONE event that cannot be encoded
 *   (sw_pack_events_device's d_encodable rule) makes the message unbuildable: *d_msg_len is -1 and d_msg is not written.
 *   Nothing at or beyond the message's end is written.  No host synchronisation; stream contract of sw_pack_events_device.
 * sw_pack_message   the same with HOST arrays; *msg_bytes receives the length; an unencodable event is SW_EINVAL and named
 *   in the message of sw_last_error; a message longer than msg_cap is SW_ERANGE with *msg_bytes set, nothing written.
 * sw_unpack_message_device   the strict reader: the message (device memory, no alignment asked) is accepted only if it is
 *   byte for byte what the writer produces for SOME arrays under this context's event class.  Every offset and length is
 *   judged before it is followed.  SW_OK with *n_events = K and the arrays written (head, K events in the layout
 *   sw_ingest_payload_data_device takes; creator -1 for a key of no member, the lowest index among equal keys; a root's
 *   parent ids zero; d_data_off holds cap_events + 1 entries, d_data cap_data bytes, 16-byte aligned), or SW_OK with
 *   *n_events = -1 for anything else (a framed pickle.dumps, another class, a flipped byte, truncation) and nothing promised
 *   about the arrays.  SW_ERANGE when K exceeds cap_events (*n_events = K, *n_data_bytes = an upper bound of the data; nothing
 *   written) or the data exceed cap_data (*n_data_bytes exact; no data written).  Synchronises twice: K, the verdict.
 * sw_unpack_message   the same with HOST arrays.
 * sw_export_message[_device]   walk, export, data gather (with_data; else every d is None) and message in one call, on the
 *   fast or the exact path, `known` / `cap` as for sw_export_walk[_device].  The refusals of sw_export_walk; SW_ENOTSUP
 *   without member keys, or with_data and an incomplete data store; SW_ERANGE with *msg_bytes set when msg_cap is too small.
 * sw_ingest_message[_device]   unpack, then (validate) the signed bytes built and judged with THIS context's keys and event
 *   class, ANDed with the encodable flags as in sw_sync_pull_validated, then sw_ingest_payload[_data]_device's ingest
 *   (with_data keeps the data; the signed bytes are built with the data either way).  *n_events = -1 and nothing stored for a
 *   message that is not canonical.  head32_out (32 bytes) and index_out (msg_bytes / 150 entries suffice; sw_ingest_payload's
 *   codes) may be NULL.  Needs a complete id index, with_data a complete data store, validate member keys (SW_ENOTSUP).
 * sw_get_wire_stats   writer calls, events and bytes (forms that know the length), reader calls, events, refused messages.
 */
int sw_pack_message_bound(sw_ctx* ctx, int64_t K, int64_t data_bytes, int64_t* msg_bytes);
int sw_pack_message_device(sw_ctx* ctx, int64_t K, const uint8_t* d_head32, const uint8_t* d_id32, const uint8_t* d_sp_id32,
                           const uint8_t* d_op_id32, const uint8_t* d_arity, const int32_t* d_creator, const double* d_t,
                           const uint8_t* d_sig64, const uint8_t* d_data, const int64_t* d_data_off, int64_t data_bytes,
                           const uint8_t* d_data_none, uint8_t* d_msg, int64_t msg_cap, int64_t* d_msg_len, void* user_stream);
int sw_pack_message(sw_ctx* ctx, int64_t K, const uint8_t* head32, const uint8_t* id32, const uint8_t* sp_id32,
                    const uint8_t* op_id32, const uint8_t* arity, const int32_t* creator, const double* t, const uint8_t* sig64,
                    const uint8_t* data, const int64_t* data_off, int64_t data_bytes, const uint8_t* data_none, uint8_t* msg,
                    int64_t msg_cap, int64_t* msg_bytes);
int sw_unpack_message_device(sw_ctx* ctx, const uint8_t* d_msg, int64_t msg_bytes, int64_t cap_events, int64_t cap_data,
                             uint8_t* d_head32, uint8_t* d_id32, uint8_t* d_sp_id32, uint8_t* d_op_id32, uint8_t* d_arity,
                             int32_t* d_creator, double* d_t, uint8_t* d_sig64, uint8_t* d_data, int64_t* d_data_off,
                             uint8_t* d_data_none, void* user_stream, int64_t* n_events, int64_t* n_data_bytes);
int sw_unpack_message(sw_ctx* ctx, const uint8_t* msg, int64_t msg_bytes, int64_t cap_events, int64_t cap_data, uint8_t* head32,
                      uint8_t* id32, uint8_t* sp_id32, uint8_t* op_id32, uint8_t* arity, int32_t* creator, double* t,
                      uint8_t* sig64, uint8_t* data, int64_t* data_off, uint8_t* data_none, int64_t* n_events,
                      int64_t* n_data_bytes);
int sw_export_message_device(sw_ctx* ctx, int64_t head_event, const int32_t* d_known, const int32_t* d_cap, int with_data,
                             uint8_t* d_msg, int64_t msg_cap, void* user_stream, int64_t* msg_bytes, int64_t* n_events);
int sw_export_message(sw_ctx* ctx, int64_t head_event, const int32_t* known, const int32_t* cap, int with_data, uint8_t* msg,
                      int64_t msg_cap, int64_t* msg_bytes, int64_t* n_events);
int sw_ingest_message_device(sw_ctx* ctx, const uint8_t* d_msg, int64_t msg_bytes, int validate, int with_data,
                             uint8_t* d_head32_out, int32_t* d_index_out, void* user_stream, int64_t* n_events, int64_t* n_valid,
                             int64_t* n_stored);
int sw_ingest_message(sw_ctx* ctx, const uint8_t* msg, int64_t msg_bytes, int validate, int with_data, uint8_t* head32_out,
                      int32_t* index_out, int64_t* n_events, int64_t* n_valid, int64_t* n_stored);
int sw_get_wire_stats(sw_ctx* ctx, int64_t* pack_calls, int64_t* pack_events, int64_t* pack_bytes, int64_t* unpack_calls,
                      int64_t* unpack_events, int64_t* refused);

/*
 * CREATING signed events on the device (kernels in csrc/sign.hip.h): the producing half of Node.new_event
 * (swirld.py:82-95) for K events at once — the Ed25519 signature over dumps((d, p, t, pk)) and the id
 * crypto_generichash(dumps(ev)), bit for bit what libsodium, pickle and hashlib give, from the same index arrays
 * sw_append_events takes.  An event's signed bytes hold its parents' ids and an id is the hash of bytes that hold the
 * signature, so a batch is signed LEVEL by level: one launch per level, enqueued back to back.  Neither byte stream is
 * materialised.  The signing keys are a setting of the context like the member keys: sw_rewind and sw_reset keep them,
 * sw_set_member_keys called again drops them.  The secrets (clamped scalar and hash prefix per member) live in ONE device
 * array and leave it through no getter.
 *
 * sw_set_signing_keys   the 32-byte Ed25519 seeds of K members (any subset; member[j] is a dense member index, its seed
 *   the bytes seed32[32 j .. 32 j + 32)).  Needs sw_set_member_keys (SW_ENOTSUP).  The key pair is derived on the device as
 *   crypto_sign_seed_keypair derives it; a seed whose public key differs from that member's key: SW_EINVAL, nothing
 *   changed — as for a member out of range, with an unusable key, or given twice.  Members set by earlier calls keep
 *   their keys.  The seeds pass through context scratch for the length of the call and are overwritten before it returns.
 * sw_clear_signing_keys   overwrites the device copy with zeros; sw_destroy does the same.
 * sw_get_signing_members   has_key[m] = 1 when the context holds member m's signing key: n bytes.
 * sw_sign_events_device   READ-ONLY with respect to the hashgraph (kernel_launches and the statistics below move).  K
 *   events in topological order as sw_append_events_device takes them: d_creator, d_self_parent, d_other_parent (int32), d_t
 *   (float64).  Parent indices are DENSE indices in the numbering the append would give: an index below sw_num_events
 *   names a stored event, an index at or above it the batch position index - sw_num_events; negative: none.  The four data
 *   arguments are those of sw_pack_events_device.  Output: d_id32, d_sp_id32, d_op_id32 (32 bytes per event; the parents'
 *   ids of a root are zeros), d_arity (0 or 2), d_sig64 — exactly the arrays sw_ingest_payload[_data]_device and
 *   sw_pack_events_device take.  Needs member keys, signing keys and a complete id index (SW_ENOTSUP).  Structural defects
 *   get the codes, and the lowest-offender rule, of sw_append_events_device, and are found before anything is signed; the
 *   lowest offending event is named in sw_last_error.  A creator without a signing key, an unusable data range, or data
 *   longer than 60 000 bytes: SW_EINVAL.  FORKS are not a defect here: signing is a pure function of the arrays.
 *   Alignment: the id arrays and the signatures 16 bytes, d_t and d_data_off 8, the index arrays 4; every array in memory
 *   of the context's device (a host pointer: SW_EINVAL before anything is launched).  STREAMS: as for
 *   sw_pack_events_device; the call synchronises with the host ONCE, to read the verdict together with the number of
 *   levels and the widest level (which size the launches).  K = 0 is a no-op.
 * sw_sign_events   the same with host arrays, staged through context scratch.
 * sw_create_events_device   the same inputs; signs into context scratch, then commits through the bodies of the ingest:
 *   the append (sw_append_events_device's: its bulk predicate, fork handling and fallbacks), the id index, and — when the
 *   data store is complete — the data append.  ATOMIC on rejection as sw_append_events_device is: memory for the ids
 *   and the data is reserved first; two equal events in the batch, or one equal to a stored event, are refused
 *   (SW_EINVAL: equal events have equal ids), as are data ranges that together hold more than data_bytes bytes.  Behind the
 *   append a failure leaves the context poisoned, as in sw_ingest_payload_data.  *first_out receives the dense index of
 *   the first created event (the K events get consecutive indices in the order given); d_id32 / d_sig64 (optional,
 *   16-byte aligned) receive the batch's ids and signatures.  Afterwards the context is in the state
 *   sw_ingest_payload_data would leave for the same, host-signed events.  Synchronises before it returns.
 * sw_create_events   the same with host arrays.
 * sw_get_sign_stats   sign calls (create calls included) and events signed so far, the levels of the last call, calls of
 *   sw_set_signing_keys that changed the keys, and — under sw_set_profiling — the host time in ms of the last call's
 *   levels + sort, signing, and commit: phase_ms[3].  Any pointer may be NULL.
 */
int sw_set_signing_keys(sw_ctx* ctx, int64_t K, const int32_t* member, const uint8_t* seed32);
int sw_clear_signing_keys(sw_ctx* ctx);
int sw_get_signing_members(sw_ctx* ctx, uint8_t* has_key);
int sw_sign_events_device(sw_ctx* ctx, int64_t K, const int32_t* d_creator, const int32_t* d_self_parent, const int32_t* d_other_parent,
                          const double* d_t, const uint8_t* d_data, const int64_t* d_data_off, int64_t data_bytes,
                          const uint8_t* d_data_none, uint8_t* d_id32, uint8_t* d_sp_id32, uint8_t* d_op_id32, uint8_t* d_arity,
                          uint8_t* d_sig64, void* user_stream);
int sw_sign_events(sw_ctx* ctx, int64_t K, const int32_t* creator, const int32_t* self_parent, const int32_t* other_parent, const double* t,
                   const uint8_t* data, const int64_t* data_off, int64_t data_bytes, const uint8_t* data_none, uint8_t* id32,
                   uint8_t* sp_id32, uint8_t* op_id32, uint8_t* arity, uint8_t* sig64);
int sw_create_events_device(sw_ctx* ctx, int64_t K, const int32_t* d_creator, const int32_t* d_self_parent, const int32_t* d_other_parent,
                            const double* d_t, const uint8_t* d_data, const int64_t* d_data_off, int64_t data_bytes,
                            const uint8_t* d_data_none, void* user_stream, int64_t* first_out, uint8_t* d_id32, uint8_t* d_sig64);
int sw_create_events(sw_ctx* ctx, int64_t K, const int32_t* creator, const int32_t* self_parent, const int32_t* other_parent,
                     const double* t, const uint8_t* data, const int64_t* data_off, int64_t data_bytes, const uint8_t* data_none,
                     int64_t* first_out, uint8_t* id32, uint8_t* sig64);
int sw_get_sign_stats(sw_ctx* ctx, int64_t* calls, int64_t* events, int64_t* levels, int64_t* key_sets, double* phase_ms);

/*
 * ONE event signed by one wavefront, and the GOSSIP TURN around it (kernels in csrc/turn.hip.h): what a
 * node does per step (swirld.py:322-328, 125-146) — sync with a peer, create one event on its own head and the peer's,
 * divide_rounds, decide_fame, find_order — as one call between two contexts of one GPU.  sw_create_events gives an event
 * one lane; here the 64 lanes of a wave share the base-point multiplication of its signature (one radix-16 digit each, a
 * butterfly of six complete additions).  Signature and id are bit for bit those of sw_sign_events.
 *
 * sw_create_event   one event of `member` at time t: both parents -1 a root, otherwise both stored events (dense indices).
 *   data_len < 0: data None; otherwise data_len bytes at `data` (host memory; 0 .. 60 000).  Preconditions, verdicts,
 *   refusal codes, commit order (ids, append, data when the store is complete) and atomicity are those of
 *   sw_create_events with K = 1 for the same event, and the context is left in the state that call would leave.
 *   *index_out, id32_out[32], sig64_out[64] (host memory, any may be NULL) receive the dense index, the id and the
 *   signature.  Synchronises once for the verdict, then as the commit does.
 * sw_gossip_turn   `dst` (the node of `member`, at its head dst_head) syncs with `src` (at its head src_head) and creates
 *   the event (data, (dst_head, src_head's event), t, member).  DEFINED BY EQUIVALENCE: dst is left in the state of
 *     1. sw_sync_pull_walk(dst, dst_head, src, src_head, SW_TURN_TRUNKS, SW_TURN_VALIDATE, SW_TURN_DATA, ..);
 *     2. the index of src_head's id in dst's id index — looked up on the device; the created event's other parent reaches
 *        the signer from device memory;
 *     3. when that id is present: sw_create_event(dst, member, dst_head, that index, t, data, data_len, ..); when it is
 *        absent (under SW_TURN_VALIDATE: dst rejected it, the reference's is_valid_event(remote_head) false) no event is
 *        created, new_head = -1 and the call returns SW_OK;
 *     4. unless SW_TURN_NO_CONSENSUS: sw_divide_rounds(dst, N_before, n_stored + created), sw_decide_fame into
 *        new_rounds[cap_rounds], sw_find_order of those rounds;
 *   and src is left untouched as those calls leave it.  REFUSALS are judged before anything is launched or stored:
 *   SW_EINVAL for dst == src, differing member counts, dst_head not an event of `member` (swirld.py:86), src_head an event
 *   of `member` (swirld.py:87), undivided events in dst, data_len above 60 000, unknown flag bits, a NULL or short result;
 *   SW_ENOTSUP for no signing key of `member`, no member keys, an incomplete id index on either side, SW_TURN_DATA with
 *   an incomplete data store on either side, a windowed context on either side, contexts on different devices.  Every
 *   other refusal is that of the call it comes from.  A failure behind the pull keeps what the pull stored (as the
 *   reference's sync does); result.stage says how far the turn got.  The head lookup and the event's verdict share one
 *   read-back: the turn adds no synchronisation to those of the composed calls and saves the lookup's.
 *   `result` receives min(result_bytes, sizeof(sw_turn_result)) bytes (fields are only ever appended; at least the
 *   first 8 bytes must fit: SW_EINVAL).
 * sw_get_turn_stats   sw_create_event calls, events the wave signed, sw_gossip_turn calls, launches that were stamped;
 *   stamps[8]: under sw_set_profiling the signer's lane 0 stores wall_clock64() at its phase boundaries — entry, key and
 *   prefix loaded, first SHA-512 + reduce, base multiplication, inversion + encode, second SHA-512 + reduce, sc_muladd,
 *   BLAKE2b id — and these are the last stamped launch's; *tick_ns the length of a tick in ns.  Any pointer may be NULL.
 */
#define SW_TURN_VALIDATE      1   /* the pull validates against dst's member keys (sw_sync_pull_walk's `validate`)      */
#define SW_TURN_DATA          2   /* events travel with their data into dst's data store (`data`)                       */
#define SW_TURN_TRUNKS        4   /* src caps its walk by its fork trunks (`use_trunks`)                                */
#define SW_TURN_NO_CONSENSUS  8   /* stop behind the created event: no divide_rounds, decide_fame, find_order           */
/* sw_turn_result.stage: the last step that completed */
#define SW_TURN_STAGE_NONE     0  /* refused, or the pull failed: nothing stored                                        */
#define SW_TURN_STAGE_PULLED   1  /* the pull stored n_stored events                                                    */
#define SW_TURN_STAGE_CREATED  2  /* ... and the event exists (or src_head is absent: new_head = -1)                    */
#define SW_TURN_STAGE_DIVIDED  3
#define SW_TURN_STAGE_FAME     4
#define SW_TURN_STAGE_ORDERED  5  /* the whole turn                                                                     */
typedef struct sw_turn_result {
    int64_t n_sent, n_valid, n_stored;   /* of the pull (n_valid only under SW_TURN_VALIDATE)                           */
    int64_t new_head;                    /* dense index of the created event in dst, or -1                              */
    int64_t n_new_rounds;                /* rounds sw_decide_fame added to the consensus (written to new_rounds)        */
    int64_t n_ordered;                   /* events ordered by this turn                                                 */
    int64_t stage;
} sw_turn_result;
int sw_create_event(sw_ctx* ctx, int member, int64_t self_parent, int64_t other_parent, double t, const uint8_t* data,
                    int64_t data_len, int64_t* index_out, uint8_t* id32_out, uint8_t* sig64_out);
int sw_gossip_turn(sw_ctx* dst, int member, int64_t dst_head, sw_ctx* src, int64_t src_head, double t, const uint8_t* data,
                   int64_t data_len, int flags, int32_t* new_rounds, int cap_rounds, void* result, size_t result_bytes);
int sw_get_turn_stats(sw_ctx* ctx, int64_t* create_calls, int64_t* events, int64_t* turns, int64_t* stamped, uint64_t* stamps,
                      double* tick_ns);

/* Exact work counters of the calls so far: used by bench.py's roofline. */
typedef struct sw_counters {
    int64_t events_divided;      /* events through divide_rounds                          */
    int64_t rounds;              /* max round + 1                                          */
    int64_t tally_evals;         /* strongly-sees tallies evaluated by the bulk round loop */
    int64_t round_iterations;    /* bulk round-loop iterations (>= rounds)                 */
    int64_t voter_evals;         /* V: voter tallies in decide_fame (swirld.py:247-254)    */
    int64_t majority_evals;      /* P2: majority() evaluations, d >= 2 (swirld.py:260)     */
    int64_t levels;              /* DAG height levels swept by the can_see kernel          */
    int64_t kernel_launches;
    int64_t far_hops;            /* hop masks rebuilt from rows because the hop lay outside the band */
    int64_t band_events;         /* band events whose threshold mask was built by the round loop      */
    int64_t coin_votes;          /* votes cast in coin rounds, d % C == 0 (swirld.py:267-272)          */
    int64_t coin_flips;          /* ... of which taken from the voter's signature bit (swirld.py:272)  */
    int64_t chunk_sweeps;        /* chunks of the can_see table swept concurrently (k_cansee_chunks)     */
    int64_t chunk_provisional;   /* entries a chunk could not know (ancestor older than its halo)        */
    int64_t chunk_repaired;      /* ... of which changed by the repair kernel                            */
    int64_t chunk_resweeps;      /* chunks swept a second time from final rows (too many to repair)      */
    /* ABI v5 */
    int64_t finalize_from_rows;  /* events whose round / sees-mask no band pass of their own round wrote: recomputed from their rows */
    int64_t order_rounds_host_sorted; /* find_order: rounds the host sorted (a tie on timestamp and the first 8 key bytes)   */
    int64_t gated_calls;         /* divide_rounds calls that ran ONE round loop gated on the device by the sweep (SW_GATED)           */
    int64_t gated_idle_iterations; /* ... iterations of those loops (inside round_iterations) in which every searching member waited for the sweep */
} sw_counters;
int sw_get_counters(sw_ctx* ctx, sw_counters* out);
/* The same for a caller built against another version of this header: copies min(out_bytes, sizeof(sw_counters))
 * bytes (fields are only ever appended), so a shorter struct is never overrun and a longer one keeps its tail. */
int sw_get_counters_sized(sw_ctx* ctx, void* out, size_t out_bytes);
/* Which step-3 kernel of the round loop the most recent sw_divide_rounds used: 0 = k_tally (column lanes, stake-weighted
 * or SW_TALLY_IMPL=0), 1 = k_tally_bits (one wave per candidate slot), 2 = k_tally_tree (one workgroup per member, two-level
 * search).  Without SW_TALLY_IMPL the library chooses per call (DESIGN.md §4 "Which tally"); measurement tools name the
 * kernel they price by this.  No reference counterpart. */
int sw_get_tally_impl(const sw_ctx* ctx);

/* Per-phase GPU time of the most recent divide_rounds / decide_fame call, measured with
 * hipEvents on the context's own stream (ms).  Enabled by sw_set_profiling(ctx, 1). */
typedef struct sw_timings {
    float can_see_ms;        /* span of the can_see stream (overlaps the round loop)     */
    float rounds_ms;         /* round-synchronous strongly-sees loop (all iterations)    */
    float tally_ms;          /* ... of which: the tally kernel (dominant kernel)         */
    int32_t tally_launches;
    float finalize_ms;       /* span of the aux stream: round numbers, sees-masks, witness   */
                             /* rows, voter masks per sub-batch (overlaps the round loop)    */
    float fame_ms;           /* decide_fame: voter tallies + elections                   */
    float total_ms;
    /* per kernel family (hipEvent pairs around each launch, so dispatch gaps are included) */
    float cansee_kernel_ms;  /* sum over the can_see sweep launches                       */
    int32_t cansee_launches;
    float resolve_ms;        /* sum over the k_resolve_band launches that did work         */
    int32_t resolve_launches;
    float elections_ms;      /* the elections kernel of the most recent decide_fame        */
} sw_timings;
int sw_set_profiling(sw_ctx* ctx, int enable);
int sw_get_timings(sw_ctx* ctx, sw_timings* out);
/* Diagnostics: with SW_DEBUG_CLOCKS=1 in the environment at sw_create, the two round-loop kernels
 * stamp their phases (100 MHz clock) per iteration; copies up to cap_words of the
 * [4096 iterations][32] table of the most recent run.  profiles/loop_phases.py reads it. */
int sw_debug_clocks(sw_ctx* ctx, unsigned long long* out, int64_t cap_words);
/* Diagnostics: with SW_DEBUG_CLOCKS=3 every workgroup of the two round-loop kernels stamps the time it was done: copies up
 * to cap_words of the [4096 iterations][2 kernels][2048 workgroups] table.  profiles/block_ends.py reads it. */
int sw_debug_block_clocks(sw_ctx* ctx, unsigned long long* out, int64_t cap_words);
/* Diagnostics (no context: the counts are the process's): what the library's contexts and calls hold right now — bytes of
 * device memory, bytes of pinned host memory, events, streams.  Any pointer may be NULL.  After the last sw_destroy every
 * count is back at what it was before the first sw_create: a test sees a leak without asking the device how much memory
 * other processes have left.  Not counted: the physical chunks of the windowed can_see table (sw_set_window), which are
 * mapped and released apart from everything else. */
int sw_debug_live_resources(int64_t* device_bytes, int64_t* pinned_bytes, int64_t* events, int64_t* streams);

/* Measurement utility (no reference counterpart): forget all voting state (rounds,
 * witnesses, fame, consensus, order) as if divide_rounds had never been called; the
 * appended events stay resident.  Lets bench.py time repeated passes over one DAG. */
int sw_rewind(sw_ctx* ctx);
/* Measurement utility: sw_rewind + forget the appended events as well; device storage stays
 * allocated.  Lets bench.py time repeated end-to-end passes (ingest included) on one context. */
int sw_reset(sw_ctx* ctx);

/*
 * Windowed can_see table (the reference keeps every row forever, swirld.py:69-72,
 * README.md:66-68).  sw_set_window(ctx, 1, chunk_mb) — before the first append — puts the table
 * under HIP virtual memory management: one reserved address range, physical chunks (chunk_mb MB, 0 =
 * 64) mapped as events arrive.  After every sw_find_order the rows no later call can read are
 * evicted (chunks unmapped and recycled): rows older than every member's latest event, than every
 * member's first unordered event, and than the thresholds of the oldest round still in play.
 * Afterwards: sw_get_can_see / the gossip getters on an evicted row, and an appended event whose
 * parent row was evicted, fail with SW_ERANGE; everything else behaves as without a window.
 * sw_get_window: first resident event, bytes of the table currently mapped, number of evictions.
 */
int sw_set_window(sw_ctx* ctx, int enable, int chunk_mb);
int sw_get_window(sw_ctx* ctx, int64_t* first_resident_event, int64_t* resident_bytes, int64_t* evictions);
/* A silent member pins the window at its last event: its latest row is the self-parent of its next event, and
 * its front round keeps that round's thresholds in play (the reference keeps every row: swirld.py:69-72).
 * sw_set_window_lapse(ctx, events > 0) — windowed mode only, default 0 = never — lets a member LAPSE once it
 * has been silent for more than `events` events: it stops holding the window back, and in exchange its further
 * events are refused with SW_ERANGE (so are, as before, events whose other-parent row was evicted) until
 * sw_rewind / sw_reset.  Results for every accepted event stay those of the reference. */
int sw_set_window_lapse(sw_ctx* ctx, int64_t events);

/*
 * Forked hashgraphs (swirld.py:170-184 height-based maxi, :221-222 witness overwrite, README.md:84).
 * sw_set_forks(ctx, 1) [default]: a forked event is accepted and the context switches, once and for
 * good (until sw_reset), to the exact path — csrc/exact.hip.h, the reference's divide_rounds /
 * decide_fame / find_order statement by statement on the device-resident state, the fast path's
 * state handed over as it is.  sw_set_forks(ctx, 0): forked events are refused with SW_ENOTSUP and
 * nothing of the call is stored (what a Node that drops forked events wants).  Not available on the
 * exact path (SW_ENOTSUP): sw_decide_fame_partial / sw_commit_fame, sw_get_vote, sw_get_sees_mask,
 * sw_sync_diff, sw_get_chain_events, the windowed table.
 * sw_get_exact: 1 once the context runs on the exact path.
 * sw_get_witness_order: the members of witnesses[r] in dict insertion order (swirld.py:234, 240) —
 * on the fast path the ascending event index of the table entries; with forks the position of a
 * member's FIRST witness of the round (a fork sibling replaces the value, not the position).
 */
int sw_set_forks(sw_ctx* ctx, int accept);
int sw_get_exact(sw_ctx* ctx, int* out);
int sw_get_witness_order(sw_ctx* ctx, int r, int32_t* members, int* n_out);

/*
 * THE HISTORY OF THE EXACT PATH (csrc/exact_history.hip.h): what the reference keeps on a forked hashgraph
 * beyond the bare order (swirld.py:256-272, 283, 305).  A context switch, OFF by default: without it an exact context
 * answers as described above (SW_ENOTSUP for everything below and for the consensus getters), call for call and launch for
 * launch.  The vote history is the reference's unbounded dict: a caller opts in to its memory.
 *
 * sw_set_exact_history(ctx, 0 | 1)   only before the first event is appended (SW_EINVAL afterwards); sw_reset keeps it.
 * sw_get_exact_history   the switch, and whether the votes are available right now (either pointer may be NULL).
 *
 * WITH THE SWITCH ON, on the exact path:
 *   sw_get_round_received, sw_get_consensus_time, sw_export_ordered[_device], sw_get_consensus_stats answer with every
 *   contract they have on the fast path (ids need the complete id index, stream contract, read-only); what the fast path
 *   recorded before the fork stays.  A find_order call that returns an error records nothing.
 *   sw_get_vote and sw_export_votes[_device] stay refused: their (round, member) form cannot name a voter that a later fork
 *   sibling replaced in the witness table.
 *
 * THE VOTES KEYED BY EVENT, on either path (SW_ENOTSUP with the switch off):
 *   sw_get_votes_by_event     out[i] = votes[voter[i]][cand[i]] for K pairs of dense event indices in HOST arrays; -1 = no
 *                             entry (also for an index outside the stored events).
 *   sw_export_vote_entries[_device]   the entries from position `first` on as three arrays (voter event, candidate event,
 *                             value 0 / 1).  *n_total (host) = all entries, always written once the checks passed.  CAPACITY
 *                             as for the other exports: cap_entries = 0 with NULL arrays asks for the size; fewer than
 *                             n_total - first gives SW_ERANGE and writes nothing.  The device form takes arrays in memory of
 *                             the context's device (SW_EINVAL otherwise, before anything is launched) and follows the STREAMS
 *                             contract of sw_export_payload_device; it synchronises at most once, for the count.
 *   sw_get_vote_store_stats   entries, capacity (entries), bytes of device memory, growths, entries taken over from the fast
 *                             path's table, pairs looked up, entries exported.  Any pointer may be NULL.
 *   ENTRY ORDER: the store's — first the entries taken over from the fast path (the rows of sw_export_votes: by round of
 *   the voter, voter, candidate round, candidate member), then first insertion by the exact path.  It is NOT the
 *   reference's dict order; a consumer that needs an order sorts.
 *   On a context that is still fork-free the same entries are computed from the table of sw_export_votes, with that call's
 *   preconditions (SW_EINVAL while rounds are divided that sw_decide_fame has not seen, SW_ENOTSUP after sw_commit_fame); the
 *   store is refilled only when sw_divide_rounds or sw_decide_fame ran since the last read.  A table with more entries than
 *   the ceiling is refused as "unavailable" on every read, like a store that overflowed.
 *   UNAVAILABLE (SW_ENOTSUP, the message says "unavailable" and why) until sw_rewind / sw_reset: the store reached its
 *   ceiling; a decide_fame call ended in the reference's KeyError; the context forked after sw_commit_fame, or with rounds
 *   divided that sw_decide_fame had not seen.  Consensus results are the same either way.
 *   Environment (read at sw_create, and again by sw_rewind / sw_reset on the exact path, where the store is empty):
 *   SW_VOTE_STORE_INIT, the first capacity in entries (default 4096; the store doubles); SW_VOTE_STORE_MAX, the ceiling in
 *   entries (default 2^24).  9 bytes of log and at least 8 bytes of index per entry.  MEMORY: before every sw_decide_fame the
 *   store is grown to what the call could write at most, n^2 * w (w - 1) / 2 more entries for w undecided rounds, capped at the
 *   ceiling — so a call over many undecided rounds (a batch pass, many members) reserves up to the ceiling, about 25 bytes per
 *   entry of it (0.4 GB at the default), however few votes are cast; lower the ceiling where that is too much.
 */
int sw_set_exact_history(sw_ctx* ctx, int enable);
int sw_get_exact_history(sw_ctx* ctx, int* enabled, int* votes_available);
int sw_get_votes_by_event(sw_ctx* ctx, int64_t K, const int32_t* voter, const int32_t* cand, int8_t* out);
int sw_export_vote_entries_device(sw_ctx* ctx, int64_t first, int64_t cap_entries, int32_t* d_voter, int32_t* d_cand, int8_t* d_value,
                                  int64_t* n_total, void* user_stream);
int sw_export_vote_entries(sw_ctx* ctx, int64_t first, int64_t cap_entries, int32_t* voter, int32_t* cand, int8_t* value, int64_t* n_total);
int sw_get_vote_store_stats(sw_ctx* ctx, int64_t* entries, int64_t* capacity, int64_t* bytes, int64_t* grows, int64_t* imported,
                            int64_t* lookups, int64_t* exported);

/*
 * BATCHES OF SMALL HASHGRAPHS (csrc/batch.hip.h, csrc/batch_layout.h).  A batch holds B independent
 * hashgraphs of ONE member count in one device allocation; a step runs, for every hashgraph that takes part, the
 * reference's main-loop step (swirld.py:325-328: divide_rounds(new events), decide_fame(), find_order(new_c)) by one
 * wavefront per hashgraph in ONE launch — the statements of the exact path (csrc/exact.hip.h), so results are the
 * reference's with or without forks.  What a batch does not have: growth (all capacity is fixed at create), mixed member
 * counts, the event-keyed vote log, an id index, gossip between nodes, crypto — those remain features of a sw_ctx.  (What it
 * does have is a generator of whole gossip histories, sw_synth_batch below: one hashgraph's DAG as sw_synth_hashgraph
 * draws it, not a network of nodes.)
 *
 * sw_batch_bytes     the device bytes sw_batch_create will allocate (-1 for a shape it refuses: an argument out of range, or
 *                    a total of 2^62 bytes or more — sw_batch_create answers SW_EINVAL to the same shapes): a head of 576 B per
 *                    hashgraph and, per hashgraph, with np = n_members rounded up to a multiple of 16, E = cap_events,
 *                    R = cap_rounds, every term rounded up to 64 B:
 *                      4 E np (can_see) + 131 E + 21 (events, queue, items, log) + R (9 np + 10) (round tables)
 *                      + 2 n^2 R (vote layers) + 26 np + 192.
 * sw_batch_create    stake = NULL (unit stake) or uint64 [B][n_members], per hashgraph within the limits of sw_create
 *                    (SW_EOVERFLOW otherwise).  cap_events >= 1 events per hashgraph; cap_rounds = 0 means cap_events + 3,
 *                    which always suffices (round <= height) — lower it to save memory (the vote layers take 2 n^2 bytes
 *                    per round): an append whose greatest height + 3 exceeds it is refused.  An allocation failure is
 *                    SW_ENOMEM with the byte count in sw_batch_last_error(NULL).
 * sw_batch_append    the new events of all hashgraphs, concatenated: hashgraph b gets [off[b], off[b + 1]) (off[0] = 0),
 *                    parents are indices LOCAL to the hashgraph.  t and sig64 may be NULL (zeros).  Validated per
 *                    hashgraph like sw_append_events on the exact path (creator range, 0 or 2 parents, parents earlier,
 *                    self-parent by the creator, other-parent by another member); forks are stored.  ATOMIC over the
 *                    batch: one bad event anywhere is SW_EINVAL, the message names hashgraph and event, nothing is
 *                    stored anywhere.  SW_ERANGE, nothing stored, beyond cap_events or cap_rounds.
 * sw_batch_step      hashgraph b divides its next K[b] undivided events, then decides fame and orders; K[b] = 0: it sits
 *                    the step out (no decide_fame call is made for it — the call schedule is part of the reference's
 *                    semantics); K = NULL: every hashgraph takes all its undivided events (none: it sits out).  SW_ERANGE,
 *                    nothing run, if a K[b] exceeds the undivided events.  A hashgraph whose step ends in one of the
 *                    reference's exceptions (KeyError, the IndexError of swirld.py:305) is FROZEN: its status is
 *                    (stage, code, event) and it is left as the reference's Node is at the exception — divided rounds, settled fame,
 *                    and the ordered events of the rounds of new_c that completed before the one that raised (swirld.py:307-309
 *                    append per round; the summary's n_ordered counts them) —, all readable; later steps skip it whatever K says.  The
 *                    call returns SW_OK with *n_failed (nullable) = hashgraphs frozen by THIS step.
 * sw_batch_get_summary   out[B][SW_BATCH_SUMMARY_WORDS]: events, divided, rounds, ordered (total), then the last step's
 *                    n_new_rounds and n_ordered, then the status: stage (SW_BATCH_STAGE_*), code (-2 KeyError, -3 IndexError,
 *                    -22), event (meaningful with a stage: the event the IndexError or a missing round was met at, -1 if none).  No device access: the values of the last step's read-back.
 * sw_batch_get_*     per hashgraph b, a copy out of its slab, with the meaning of the sw_get_* of the same name;
 *                    sw_batch_get_new_rounds: sorted(new_c) of b's last step; sw_batch_get_transactions: the ordered events
 *                    [first, first + K) with their round received and consensus timestamp (each array nullable).
 *                    One blocking copy per call and array: for every hashgraph at once see sw_export_batch_* below.
 */
typedef struct sw_batch sw_batch;
#define SW_BATCH_SUMMARY_WORDS 9
#define SW_BATCH_STAGE_NONE   0
#define SW_BATCH_STAGE_DIVIDE 1
#define SW_BATCH_STAGE_FAME   2
#define SW_BATCH_STAGE_ORDER  3
int64_t sw_batch_bytes(int64_t B, int n_members, int64_t cap_events, int64_t cap_rounds);
int sw_batch_create(int64_t B, int n_members, const uint64_t* stake, int coin_period, int64_t cap_events, int64_t cap_rounds, int device,
                    sw_batch** out);
int sw_batch_destroy(sw_batch* batch);
const char* sw_batch_last_error(const sw_batch* batch);   /* batch may be NULL: last create() error */
int sw_batch_shape(sw_batch* batch, int64_t* B, int* n_members, int* npad, int64_t* cap_events, int64_t* cap_rounds, int64_t* bytes);
int sw_batch_append(sw_batch* batch, const int64_t* off, const int32_t* creator, const int32_t* self_parent, const int32_t* other_parent,
                    const double* t, const uint8_t* sig64);
int sw_batch_step(sw_batch* batch, const int64_t* K, int64_t* n_failed);
int sw_batch_get_summary(sw_batch* batch, int64_t* out);
int sw_batch_get_height(sw_batch* batch, int64_t b, int64_t first, int64_t K, int32_t* out);
int sw_batch_get_round(sw_batch* batch, int64_t b, int64_t first, int64_t K, int32_t* out);
int sw_batch_get_can_see(sw_batch* batch, int64_t b, int64_t first, int64_t K, int32_t* out);
int sw_batch_get_witnesses(sw_batch* batch, int64_t b, int r0, int r1, int32_t* out);
int sw_batch_get_witness_order(sw_batch* batch, int64_t b, int r, int32_t* members, int* n_out);
int sw_batch_get_famous(sw_batch* batch, int64_t b, int r0, int r1, int8_t* out);
int sw_batch_get_famous_events(sw_batch* batch, int64_t b, int64_t first, int64_t K, int8_t* out);
int sw_batch_get_consensus(sw_batch* batch, int64_t b, int r0, int r1, uint8_t* out);
int sw_batch_get_new_rounds(sw_batch* batch, int64_t b, int32_t* out, int cap, int* n_out);
int sw_batch_get_transactions(sw_batch* batch, int64_t b, int64_t first, int64_t K, int32_t* events, int32_t* round_received,
                              double* consensus_time);

/*
 * GOSSIP HISTORIES GENERATED ON THE DEVICE (csrc/batch_synth.hip.h).  Instead of generating every hashgraph
 * on the host (sw_synth_hashgraph), validating and uploading it (sw_batch_append, 88 bytes per event), give a seed and
 * parameters per hashgraph and let the batch generate its own events, in instalments: one wavefront per participating
 * hashgraph, one launch and one read-back of 8 bytes per participating hashgraph per call.
 *   THE INVARIANT: after sw_synth_batch_begin with (seed_b, mode_b, p0_b, p1_b) and any sequence of sw_synth_batch calls
 * that stored N_b events in total, hashgraph b holds exactly what sw_synth_hashgraph(n_members, N_b, seed_b, mode_b, p0_b,
 * p1_b, ...) writes — creator, parents, t[i] = (double)i and the 64 signature bytes, bit for bit — with the heights of
 * swirld.py:117-120 and the per-event defaults of an appended event.  Steps, getters and exports cannot tell the two apart.
 *
 * sw_synth_batch_begin      which: NULL = every hashgraph, else which[b] != 0 selects b.  seed: [B] (read where selected).
 *                           mode / p0 / p1: [B], each nullable (0 / 0.0 / 0.0); meaning and ranges: sw_synth_hashgraph's.
 *                           SW_EINVAL, nothing changed: NULL seed, a batch of fewer than 2 members, a selected hashgraph
 *                           that already holds events, a mode outside 0..3.  Again on a hashgraph that is still empty:
 *                           replaces its parameters.  The first call allocates the generator state, outside
 *                           sw_batch_bytes: 16 n_members + 160 bytes per hashgraph, its three parts rounded up to 64 B.
 * sw_synth_batch            hashgraph b generates and stores its next K[b] events (0: none); *total (nullable) = events
 *                           stored.  SW_EINVAL, nothing stored: NULL K, a negative K[b], K[b] > 0 for a hashgraph without
 *                           parameters, a first instalment with 0 < K[b] < n_members (the roots come first and together),
 *                           K[b] > 0 for a hashgraph that has taken a sw_batch_append since begin (the generator's heads no
 *                           longer describe it).  A frozen hashgraph may still be fed, as by sw_batch_append.  ATOMIC over
 *                           the batch: a hashgraph that would exceed cap_events, or whose greatest height + 3 would exceed
 *                           cap_rounds, is SW_ERANGE, the message names it, nothing observable is stored anywhere and no
 *                           generator advances — the same call repeated with an admissible K gives what it would have
 *                           given had the refused call never been made.  Every call ends synchronised.
 * sw_synth_batch_stats      out[4]: sw_synth_batch calls that stored events, events generated, kernel launches (begin's
 *                           included), refreshes of the append mirror: sw_synth_batch does not copy creators and heights
 *                           back to the host, so the first sw_batch_append that feeds a hashgraph with generated events
 *                           reads that hashgraph's two columns from its slab first (counted once per hashgraph and
 *                           append), then validates and stores exactly as on a host-fed batch.
 * sw_get_batch_events       the stored events [first, first + K) of hashgraph b as sw_batch_append takes them; every array
 *                           nullable.  One blocking copy per requested array; SW_ERANGE for a hashgraph or a range outside
 *                           what is stored.  Any batch, generated or host-fed.
 */
int sw_synth_batch_begin(sw_batch* batch, const uint8_t* which, const uint64_t* seed, const int32_t* mode, const double* p0,
                         const double* p1);
int sw_synth_batch(sw_batch* batch, const int64_t* K, int64_t* total);
int sw_synth_batch_stats(sw_batch* batch, int64_t out[4]);
int sw_get_batch_events(sw_batch* batch, int64_t b, int64_t first, int64_t K, int32_t* creator, int32_t* self_parent,
                        int32_t* other_parent, double* t, uint8_t* sig64);

/*
 * THE RESULTS OF A WHOLE BATCH IN ONE CALL (csrc/batch_export.hip.h).  The sw_batch_get_* above cost one
 * blocking copy per hashgraph and array; these return, for every hashgraph at once, RAGGED arrays: the segments of the
 * hashgraphs concatenated, hashgraph b at entries [off[b], off[b + 1]) of every data array, off of B + 1 entries, off[B] =
 * *total.  One kernel launch per call; the host form ends in ONE synchronisation (one copy back per requested array), the
 * _device form in none.
 *   CONTROL arrays (first, count, which, r0, r1, and off, which is written) are HOST memory in both forms: the ranges are
 * checked against what the host already holds from the last step's read-back, and off is its prefix sum — *total is known
 * before anything is enqueued.  DATA arrays are host memory in the plain form and memory of the batch's device, 16-byte
 * aligned, in the _device form, whose user_stream (the caller's hipStream_t) has the earlier users of the arrays enqueued
 * and is made to wait for the gather.  Every data array is nullable (not wanted).  With ALL of them NULL the call is a
 * SIZING call: it fills off and *total (nullable), ignores cap, launches nothing.  cap: entries the data arrays can take.
 *   Defaults: first / r0 NULL = 0; count / r1 NULL = up to the end (the ordered events, the stored events, the rounds of
 * the hashgraph); which NULL = every hashgraph, which[b] = 0: an empty segment.
 *   Refused before any device work, nothing written to a data array: NULL batch or off (SW_EINVAL); a negative range or one
 * beyond the end (SW_ERANGE); *total > cap (SW_ERANGE, off and *total filled: size and retry); a device data array that is
 * not 16-byte aligned or not memory of the batch's device (SW_EINVAL).  *total = 0: SW_OK, no launch.  FROZEN hashgraphs
 * are exported like any other, with what their slab holds (the log of the rounds a failing call completed included).
 *
 * sw_export_batch_ordered      log positions [first[b], first[b] + count[b]): event, round received, consensus timestamp —
 *                              sw_batch_get_transactions for every hashgraph, bit for bit.
 * sw_export_batch_new_rounds   sorted(new_c) of each hashgraph's own last step (sw_batch_get_new_rounds); empty for a
 *                              frozen hashgraph: the step that froze it returned no new_c.
 * sw_export_batch_events       creator, height, round (-1: not divided yet) and famous_events of the stored events
 *                              [first[b], first[b] + count[b]).
 * sw_export_batch_rounds       rounds [r0[b], r1[b]): witnesses and famous as rows of n_members columns (off, cap and *total
 *                              count ROUNDS: the arrays hold *total x n_members elements), consensus one byte per round.
 * sw_export_batch_stats        out[4]: calls, kernel launches, entries written (*total of every call that launched),
 *                              device-to-host copies, since the batch was created.
 */
int sw_export_batch_ordered(sw_batch* batch, const int64_t* first, const int64_t* count, int64_t cap, int64_t* off, int32_t* event,
                            int32_t* round_received, double* time, int64_t* total);
int sw_export_batch_ordered_device(sw_batch* batch, const int64_t* first, const int64_t* count, int64_t cap, int64_t* off, int32_t* d_event,
                                   int32_t* d_round_received, double* d_time, int64_t* total, void* user_stream);
int sw_export_batch_new_rounds(sw_batch* batch, const uint8_t* which, int64_t cap, int64_t* off, int32_t* rounds, int64_t* total);
int sw_export_batch_new_rounds_device(sw_batch* batch, const uint8_t* which, int64_t cap, int64_t* off, int32_t* d_rounds, int64_t* total,
                                      void* user_stream);
int sw_export_batch_events(sw_batch* batch, const int64_t* first, const int64_t* count, int64_t cap, int64_t* off, int32_t* creator,
                           int32_t* height, int32_t* round, int8_t* famous, int64_t* total);
int sw_export_batch_events_device(sw_batch* batch, const int64_t* first, const int64_t* count, int64_t cap, int64_t* off, int32_t* d_creator,
                                  int32_t* d_height, int32_t* d_round, int8_t* d_famous, int64_t* total, void* user_stream);
int sw_export_batch_rounds(sw_batch* batch, const int32_t* r0, const int32_t* r1, int64_t cap, int64_t* off, int32_t* witnesses,
                           int8_t* famous, uint8_t* consensus, int64_t* total);
int sw_export_batch_rounds_device(sw_batch* batch, const int32_t* r0, const int32_t* r1, int64_t cap, int64_t* off, int32_t* d_witnesses,
                                  int8_t* d_famous, uint8_t* d_consensus, int64_t* total, void* user_stream);
int sw_export_batch_stats(sw_batch* batch, int64_t out[4]);

/*
 * GOSSIP NETWORKS IN A BATCH (csrc/batch_network.hip.h).  Consecutive hashgraphs of a batch form a network:
 * with n = n_members and G = B / n, hashgraph g n + i is node i's VIEW of network g, and one wavefront runs the turns of
 * one network, one after the other, in one launch — the reference's test(n_nodes, n_turns) (swirld.py:331-345) without a
 * host between the turns.  Turn (i, j): node i pulls from node j != i what the reference's ask_sync answers (the BFS of
 * swirld.py:154-159 in view j, pruned by the heights of can_see[head_i]), stores what it does not hold behind its events in
 * ascending local index of j, creates its event on (head_i, head_j) and runs the main-loop step over all of it (the step of
 * sw_batch_step, unchanged).  Stored events carry their NETWORK EVENT NUMBER, the creation order inside the network: root
 * i is number i, turn k creates number n + k, the same in every view.  There is no crypto and there are no ids.
 *   LIMITS: no forks (every node is honest), no crypto, one turn at a time per network, cap_events bounds the events a
 * NETWORK creates (n + its turns), not only what a view holds.
 *   STOPPED networks: a turn whose step freezes the puller's view — where the reference raises and test() dies — stops the
 * network with status (stage, code, view): SW_BATCH_STAGE_* of the frozen step.  The one deliberate deviation: an imported
 * event with a parent that resolves neither in the puller's view nor earlier in the import stops the network with
 * SW_NETWORK_STAGE_BROKEN before the turn stores anything, where the reference skips the invalid event (swirld.py:135);
 * between honest nodes it does not happen.  A stopped network runs no further turn, in this call or a later one, whatever
 * the schedule says; the other networks go on.
 *   THE NETWORK STATE is an allocation of its own, made by the first begin, outside sw_batch_bytes:
 * align64(128 G) + align64(16 B) + 2 B align64(4 cap_events) bytes (per view the number column and the number -> index
 * table, per network both generators and the counts).
 *
 * sw_network_batch_begin   which: NULL = every network, else which[g] != 0 selects g.  seed: [G] (read where selected).
 *                          View i stores root i (t = root_t[g][i], NULL: (double)i; signature root_sig64[g][i], NULL: the
 *                          generated one) and divides it.  SW_EINVAL, nothing changed: B not a multiple of n_members,
 *                          n_members < 2, a selected network with a non-empty view or a view with generator parameters,
 *                          views of one network with different stake rows.
 * sw_network_batch_turns   the explicit schedule, ragged like sw_batch_append: network g runs the turns [off[g], off[g + 1])
 *                          of puller / peer, with t and sig64 (each nullable) per turn for the created event.
 * sw_network_batch_run     network g runs its next T[g] turns of the schedule it draws itself: bit for bit what
 *                          sw_network_batch_turns does with sw_synth_schedule's turns and NULL t / sig64, and prefix-stable:
 *                          run(T1) then run(T2) equals run(T1 + T2).
 *                          GENERATED: t = (double)number; the signature of event number e is the words [8 e, 8 e + 8) of
 *                          sw_synth_hashgraph's signature stream for seed[g] (it advances by 8 words per created event
 *                          whether or not an explicit signature replaced it).
 *                          Both forms check everything before anything is enqueued, ATOMIC over the batch.  SW_EINVAL: a
 *                          network with turns that was never begun, puller == peer, a node outside 0..n_members-1.
 *                          SW_ERANGE: n_members + turns so far + turns of this call > cap_events, or that + 3 > cap_rounds
 *                          (conservative: a view never holds more than the network has created).  SW_OK with *n_stopped
 *                          (nullable) = networks stopped by THIS call.  One launch per 64 turns of the longest network,
 *                          one read-back per call; the counts, summaries and getters of the views end up exactly as after
 *                          the equivalent sw_batch_append + sw_batch_step calls.
 * sw_network_batch_get     out[G][SW_NETWORK_BATCH_WORDS]: begun, turns run, events created, status: stage, code, view (-1).
 * sw_network_batch_heads   out[B]: the local index of each view's head (-1: not a view of a begun network).
 * sw_get_network_event_numbers   the network event numbers of the stored events [first, first + K) of view b.
 * sw_export_network_event_numbers[_device]   the same for every hashgraph at once, ragged, with the control arrays and the
 *                          refusals of sw_export_batch_events (a hashgraph that is no view has no entries).
 * sw_network_batch_stats   out[4]: calls that ran turns, turns run, events imported, kernel launches (begin's included).
 * AFTERWARDS sw_batch_append and sw_synth_batch on a view are SW_EINVAL, sw_batch_step finds nothing undivided there;
 * hashgraphs of networks that were not begun behave exactly as before.
 */
#define SW_NETWORK_BATCH_WORDS 6
#define SW_NETWORK_STAGE_BROKEN 4
int sw_network_batch_begin(sw_batch* batch, const uint8_t* which, const uint64_t* seed, const double* root_t, const uint8_t* root_sig64);
int sw_network_batch_turns(sw_batch* batch, const int64_t* off, const int32_t* puller, const int32_t* peer, const double* t,
                           const uint8_t* sig64, int64_t* n_stopped);
int sw_network_batch_run(sw_batch* batch, const int64_t* T, int64_t* n_stopped);
int sw_network_batch_get(sw_batch* batch, int64_t* out);
int sw_network_batch_heads(sw_batch* batch, int32_t* out);
int sw_network_batch_stats(sw_batch* batch, int64_t out[4]);
int sw_get_network_event_numbers(sw_batch* batch, int64_t b, int64_t first, int64_t K, int32_t* out);
int sw_export_network_event_numbers(sw_batch* batch, const int64_t* first, const int64_t* count, int64_t cap, int64_t* off, int32_t* numbers,
                                  int64_t* total);
int sw_export_network_event_numbers_device(sw_batch* batch, const int64_t* first, const int64_t* count, int64_t cap, int64_t* off,
                                         int32_t* d_numbers, int64_t* total, void* user_stream);

/* Block until all work queued on the context's stream is complete. */
int sw_synchronize(sw_ctx* ctx);

/*
 * Host utility (no GPU): synthetic gossip hashgraph with the DAG shape swirld.test()
 * produces (swirld.py:323, 342-344).  Events 0..n-1 are the roots.
 * mode 0: uniform gossip.  mode 1: two cliques, cross-clique probability p0.
 * mode 2: a fraction p0 of members has relative activity p1.  mode 3: stale
 * other-parents (walk back the peer's self-parent chain with probability p0 per step).
 * t (nullable) = float(index); sig64 (nullable) = N*64 seeded random bytes.
 */
int sw_synth_hashgraph(int n, int64_t N, uint64_t seed, int mode, double p0, double p1,
                       int32_t* creator, int32_t* self_parent, int32_t* other_parent,
                       double* t, uint8_t* sig64);
/*
 * Host utility (no GPU): the turns [first_turn, first_turn + T) of the schedule a network of n nodes draws for itself
 * under `seed` (sw_network_batch_run): per turn the puller, uniform in 0..n-1, and its peer, uniform among the others
 * (swirld.py:342, 323).  SW_EINVAL for n < 2, a negative range, NULL arrays with T > 0.
 */
int sw_synth_schedule(int n, uint64_t seed, int64_t first_turn, int64_t T, int32_t* puller, int32_t* peer);

#ifdef __cplusplus
}
#endif
#endif /* SWIRLD_HIP_H */
