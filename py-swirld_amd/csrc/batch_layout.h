// Where everything of a batch of hashgraphs lies (batch.hip.h, DESIGN.md "Batches of small hashgraphs"): ONE device
// allocation, a head (one record and one summary per hashgraph) followed by B equal slabs.  A slab holds everything the
// swx::State, swx::FameScratch and swx::OrderScratch of its hashgraph point to, at capacities fixed at create; every
// segment starts on a 64-byte boundary; every offset is 64-bit (a batch may exceed 4 GiB, and so may the distance
// between two of its hashgraphs).
// Host-only: the standard library alone, so a plain C++ compiler builds it (tests/batch_layout_main.cpp).
#pragma once

#include <cstdint>

namespace swb_layout {

typedef uint64_t u64;

constexpr u64 ALIGN = 64;
constexpr u64 REC_BYTES = 512;      // room for one swb::Rec (batch.hip.h asserts that it fits)
constexpr int SUMMARY_WORDS = 8;    // int64 words the device keeps per hashgraph (one read-back per step)
constexpr int HDR_WORDS = 16;       // swx::H_WORDS

// the segments of a slab, in address order
enum Seg {
    SEG_L,          // can_see rows           int32 [cap_events][npad]
    SEG_CR, SEG_SP, SEG_OP, SEG_HT, SEG_ROUND,   // per event, int32
    SEG_T,          // float64 per event
    SEG_SIG,        // 64 B per event
    SEG_TBD, SEG_FAM_EV,                         // 1 B per event
    SEG_WIT, SEG_WORDER,                         // int32 [cap_rounds][npad]
    SEG_WCNT,       // int32 [cap_rounds]
    SEG_CONS,       // uint8 [cap_rounds]
    SEG_FAM_SLOT,   // int8  [cap_rounds][npad]
    SEG_DONE,       // uint8 [cap_rounds]
    SEG_NEW_ROUNDS, // int32 [cap_rounds]
    SEG_VOTES,      // int8  2 layers x n x n x cap_rounds
    SEG_QUEUE,      // int32 [cap_events + 1]
    SEG_VISITED,    // uint8 [cap_events + 1], all zero between calls
    SEG_ITEMS_EV, SEG_ITEMS_TS, SEG_ITEMS_RR,    // [cap_events + 1]: int32, float64, int32
    SEG_LOG_EV, SEG_LOG_RR, SEG_LOG_TS,          // the transaction log [cap_events]: int32, int32, float64
    SEG_STAKE,      // uint32 [npad]
    SEG_SM, SEG_FW, SEG_SFLAG, SEG_TIMES, SEG_TSORT,   // [npad]: uint8, int32, uint8, float64, float64
    SEG_WHITE,      // 64 B
    SEG_HDR,        // int64 [HDR_WORDS]
    SEG_COUNT
};

constexpr u64 align_up(u64 v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }

// The batch's row stride: the smallest multiple of 16 that holds n members (rows of int32 on 64-byte boundaries).
// The functions of exact.hip.h take the stride as a parameter; sw_create uses 64 x words.
constexpr int npad_of(int n) { return (n + 15) / 16 * 16; }

// cap_rounds = 0: cap_events + 3, which always suffices (round <= height < cap_events)
constexpr u64 rounds_of(u64 cap_events, u64 cap_rounds) { return cap_rounds ? cap_rounds : cap_events + 3; }

struct Layout {
    u64 B = 0, n = 0, npad = 0, cap_events = 0, cap_rounds = 0;
    u64 off[SEG_COUNT] = {};    // byte offset of a segment inside its slab
    u64 size[SEG_COUNT] = {};   // bytes of the segment (a multiple of 64)
    u64 slab = 0;               // bytes of one hashgraph
    u64 recs = 0, summaries = 0, slabs = 0;   // byte offsets inside the allocation
    u64 total = 0;              // bytes of the allocation

    u64 slab_at(u64 b) const { return slabs + b * slab; }
    u64 at(u64 b, int seg) const { return slab_at(b) + off[seg]; }
    u64 rec_at(u64 b) const { return recs + b * REC_BYTES; }
    u64 summary_at(u64 b) const { return summaries + b * SUMMARY_WORDS * 8; }
};

inline Layout make(u64 B, u64 n, u64 npad, u64 cap_events, u64 cap_rounds) {
    Layout l;
    l.B = B; l.n = n; l.npad = npad; l.cap_events = cap_events; l.cap_rounds = rounds_of(cap_events, cap_rounds);
    const u64 E = l.cap_events, R = l.cap_rounds, np = npad;
    u64* s = l.size;
    s[SEG_L] = E * np * 4;
    s[SEG_CR] = s[SEG_SP] = s[SEG_OP] = s[SEG_HT] = s[SEG_ROUND] = E * 4;
    s[SEG_T] = E * 8;
    s[SEG_SIG] = E * 64;
    s[SEG_TBD] = s[SEG_FAM_EV] = E;
    s[SEG_WIT] = s[SEG_WORDER] = R * np * 4;
    s[SEG_WCNT] = R * 4;
    s[SEG_CONS] = R;
    s[SEG_FAM_SLOT] = R * np;
    s[SEG_DONE] = R;
    s[SEG_NEW_ROUNDS] = R * 4;
    s[SEG_VOTES] = 2 * n * n * R;
    s[SEG_QUEUE] = (E + 1) * 4;
    s[SEG_VISITED] = E + 1;
    s[SEG_ITEMS_EV] = (E + 1) * 4;
    s[SEG_ITEMS_TS] = (E + 1) * 8;
    s[SEG_ITEMS_RR] = (E + 1) * 4;
    s[SEG_LOG_EV] = s[SEG_LOG_RR] = E * 4;
    s[SEG_LOG_TS] = E * 8;
    s[SEG_STAKE] = np * 4;
    s[SEG_SM] = np;
    s[SEG_FW] = np * 4;
    s[SEG_SFLAG] = np;
    s[SEG_TIMES] = s[SEG_TSORT] = np * 8;
    s[SEG_WHITE] = 64;
    s[SEG_HDR] = HDR_WORDS * 8;
    u64 at = 0;
    for (int i = 0; i < SEG_COUNT; ++i) {
        s[i] = align_up(s[i]);
        l.off[i] = at;
        at += s[i];
    }
    l.slab = at;
    l.recs = 0;
    l.summaries = align_up(B * REC_BYTES);
    l.slabs = l.summaries + align_up(B * SUMMARY_WORDS * 8);
    l.total = l.slabs + B * l.slab;
    return l;
}

// Whether a shape's total fits 64-bit arithmetic with room to spare (below 2^62 bytes): make() multiplies its arguments
// without a check, so the entry points ask this first.  An upper bound of the total in 128 bits: every segment rounded
// up by at most 64 bytes.  (Arguments within the entry points' own limits: B <= 2^24, n, npad <= 1024, capacities <= 2^30.)
inline bool fits(u64 B, u64 n, u64 npad, u64 cap_events, u64 cap_rounds) {
    typedef unsigned __int128 u128;
    const u128 E = cap_events, R = rounds_of(cap_events, cap_rounds), np = npad;
    const u128 slab = 4 * E * np + 131 * E + 21 + R * (9 * np + 10) + 2 * (u128)n * n * R + 26 * np + 192 + (u128)SEG_COUNT * ALIGN;
    const u128 total = (u128)B * (slab + REC_BYTES + SUMMARY_WORDS * 8) + 2 * ALIGN;
    return total < ((u128)1 << 62);
}

// what sw_batch_bytes returns
inline u64 batch_bytes(u64 B, u64 n, u64 cap_events, u64 cap_rounds) { return make(B, n, (u64)npad_of((int)n), cap_events, cap_rounds).total; }

}  // namespace swb_layout
