// Stand-alone program over py-swirld_amd/csrc/batch_layout.h (built with AddressSanitizer and UBSan by
// tests/test_batch_layout_host.py) — TEST INFRASTRUCTURE.  For a shape given on the command line
//   batch_layout_main B n npad cap_events cap_rounds
// it checks what the device code relies on and prints the figures the Python side compares with its own model:
//   every segment of a slab starts on a 64-byte boundary, the segments are disjoint and in order and fill the slab;
//   records, summaries and slabs are disjoint, 64-byte aligned and monotone in b, in 64-bit arithmetic;
//   the end of the last slab is the total, and — at the batch's own npad — what sw_batch_bytes returns.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "../py-swirld_amd/csrc/batch_layout.h"

using namespace swb_layout;

static int bad(const char* what, u64 a, u64 b) {
    fprintf(stderr, "FAILED: %s (%" PRIu64 ", %" PRIu64 ")\n", what, a, b);
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: %s B n npad cap_events cap_rounds\n", argv[0]); return 2; }
    const u64 B = strtoull(argv[1], nullptr, 10), n = strtoull(argv[2], nullptr, 10), npad = strtoull(argv[3], nullptr, 10),
              E = strtoull(argv[4], nullptr, 10), R = strtoull(argv[5], nullptr, 10);
    if (!fits(B, n, npad, E, R)) { printf("fits 0\n"); return 0; }   // (make() would wrap: the entry points refuse such a shape)
    const Layout l = make(B, n, npad, E, R);
    if (l.cap_rounds != (R ? R : E + 3)) return bad("cap_rounds = 0 means cap_events + 3", l.cap_rounds, E + 3);
    // segments of one slab
    u64 end = 0;
    for (int i = 0; i < SEG_COUNT; ++i) {
        if (l.off[i] % ALIGN) return bad("segment not 64-byte aligned", (u64)i, l.off[i]);
        if (l.size[i] % ALIGN || l.size[i] == 0) return bad("segment size", (u64)i, l.size[i]);
        if (l.off[i] != end) return bad("segments are not back to back", (u64)i, l.off[i]);
        end = l.off[i] + l.size[i];
    }
    if (end != l.slab) return bad("the segments do not fill the slab", end, l.slab);
    // the sizes hold what the device code indexes
    const u64 Rr = l.cap_rounds;
    const u64 need[SEG_COUNT] = {E * npad * 4, E * 4, E * 4, E * 4, E * 4, E * 4, E * 8, E * 64, E, E, Rr * npad * 4, Rr * npad * 4, Rr * 4, Rr, Rr * npad,
                                 Rr, Rr * 4, 2 * n * n * Rr, (E + 1) * 4, E + 1, (E + 1) * 4, (E + 1) * 8, (E + 1) * 4, E * 4, E * 4, E * 8,
                                 npad * 4, npad, npad * 4, npad, npad * 8, npad * 8, 64, 128};
    for (int i = 0; i < SEG_COUNT; ++i)
        if (l.size[i] < need[i] || l.size[i] >= need[i] + ALIGN) return bad("segment size against the arrays it holds", (u64)i, l.size[i]);
    // head and slabs
    if (l.recs != 0 || l.summaries < B * REC_BYTES || l.slabs < l.summaries + B * SUMMARY_WORDS * 8) return bad("head regions overlap", l.summaries, l.slabs);
    if (l.summaries % ALIGN || l.slabs % ALIGN || l.slab % ALIGN) return bad("head alignment", l.summaries, l.slabs);
    // monotone in b, disjoint, aligned: every hashgraph up to 4096, then a stride, always the last one
    const u64 stride = B > 4096 ? B / 1024 : 1;
    u64 prev_end = l.slabs, prev_rec_end = 0, prev_sum_end = l.summaries;
    for (u64 b = 0; b < B; b = (b < 4096 || b + stride >= B) ? b + 1 : b + stride) {
        const u64 a = l.slab_at(b);
        if (a % ALIGN) return bad("slab not aligned", b, a);
        if (a < prev_end) return bad("slabs overlap or go backwards", b, a);
        if (a != l.slabs + b * l.slab) return bad("slab address", b, a);
        for (int i = 0; i < SEG_COUNT; ++i)
            if (l.at(b, i) != a + l.off[i] || l.at(b, i) + l.size[i] > a + l.slab) return bad("segment address", b, (u64)i);
        prev_end = a + l.slab;
        if (l.rec_at(b) < prev_rec_end || l.rec_at(b) + REC_BYTES > l.summaries) return bad("record address", b, l.rec_at(b));
        prev_rec_end = l.rec_at(b) + REC_BYTES;
        if (l.summary_at(b) < prev_sum_end || l.summary_at(b) + SUMMARY_WORDS * 8 > l.slabs) return bad("summary address", b, l.summary_at(b));
        prev_sum_end = l.summary_at(b) + SUMMARY_WORDS * 8;
    }
    if (l.slab_at(B - 1) + l.slab != l.total) return bad("the last slab ends at the total", l.slab_at(B - 1) + l.slab, l.total);
    if (npad == (u64)npad_of((int)n) && l.total != batch_bytes(B, n, E, R)) return bad("total against sw_batch_bytes", l.total, batch_bytes(B, n, E, R));
    printf("slab %" PRIu64 "\n", l.slab);
    printf("total %" PRIu64 "\n", l.total);
    printf("last_slab %" PRIu64 "\n", l.slab_at(B - 1));
    printf("last_hdr %" PRIu64 "\n", l.at(B - 1, SEG_HDR));
    printf("npad_of %d\n", npad_of((int)n));
    printf("batch_bytes %" PRIu64 "\n", batch_bytes(B, n, E, R));
    printf("fits %d\n", (int)fits(B, n, npad, E, R));
    return 0;
}
