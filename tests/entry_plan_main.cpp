// Stand-alone driver of csrc/entry_plan.h (tests/test_entry_plan_host.py builds it with AddressSanitizer and UBSan).
//   entry_plan_main align                          first_misaligned over the row sets below, one result a line
//   entry_plan_main stage <form> <K> <optional>    the offsets, total and copies of the staging plan of <form> (pack_events,
//                                                  pack_message, unpack_message) beside the literal Carve::take sequence it replaced
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../py-swirld_amd/csrc/entry_plan.h"

using entry::Arg;
using entry::Carve;
using entry::Stage;

static void print(const char* tag, const std::vector<size_t>& v) {
    printf("%s", tag);
    for (size_t x : v) printf(" %zu", x);
    printf("\n");
}

static void print_copies(const Stage& st) {
    std::vector<size_t> up, down;
    for (int i = 0; i < st.n_up; ++i) { up.push_back(st.up[i].off); up.push_back(st.up[i].bytes); }
    for (int i = 0; i < st.n_down; ++i) { down.push_back(st.down[i].off); down.push_back(st.down[i].bytes); }
    print("up", up);
    print("down", down);
    printf("full %d\n", st.full ? 1 : 0);
}

static int align_cases() {
    alignas(64) static unsigned char buf[256];
    const unsigned char* a = buf;
    const struct { const char* name; std::vector<Arg> rows; } sets[] = {
        {"aligned", {{a, 64, 16}, {a + 8, 8, 8}, {a + 4, 4, 4}, {a + 3, 5, 1}}},
        {"off_by_one_16", {{a, 64, 16}, {a + 17, 32, 16}}},
        {"off_by_one_8", {{a + 1, 8, 8}}},
        {"off_by_one_4", {{a, 4, 4}, {a + 8, 8, 8}, {a + 5, 4, 4}}},
        {"half_16", {{a + 8, 64, 16}}},
        {"half_8", {{a + 4, 64, 8}}},
        {"half_4", {{a + 2, 64, 4}}},
        {"null_rows", {{nullptr, 64, 16}, {nullptr, 0, 8}}},
        {"zero_byte_rows", {{a + 1, 0, 16}, {a + 1, 0, 8}, {a + 1, 0, 4}}},
        {"skipped_then_bad", {{nullptr, 8, 8}, {a + 1, 0, 8}, {a + 2, 8, 8}}},
        {"first_of_two", {{a + 1, 4, 4}, {a + 1, 16, 16}}},
        {"empty", {}},
    };
    for (const auto& s : sets) printf("%s %d\n", s.name, entry::first_misaligned(s.rows.data(), (int)s.rows.size()));
    return 0;
}

// Host arrays of a call: distinct non-NULL addresses (never read), or NULL for the optional ones that are left out.
static unsigned char g_host[32];
static void* arr(int i, bool present = true) { return present ? g_host + i : nullptr; }

static int stage_case(const char* form, size_t k, bool opt) {
    const size_t db = opt ? 5 * k + 3 : 0, bm = 200 * k + db, bw = 300 * k + db;   // data bytes and the two stream bounds
    Carve cv;
    Stage st;
    std::vector<size_t> lit, got;
    if (!strcmp(form, "pack_events")) {
        lit = {cv.take(k * 32), cv.take(k * 32), cv.take(k), cv.take(k * 4), cv.take(k * 8), cv.take(k * 64), cv.take(opt ? (k + 1) * 8 : 0), cv.take(db),
               cv.take(opt ? k : 0), cv.take((k + 1) * 8), cv.take((k + 1) * 8), cv.take(bm), cv.take(bw), cv.take(k)};
        got = {st.in(arr(0), k * 32), st.in(arr(1), k * 32), st.in(arr(2), k), st.in(arr(3), k * 4), st.in(arr(4), k * 8), st.in(arr(5), k * 64),
               st.in(arr(6, opt), (k + 1) * 8), st.in(arr(7, opt), db), st.in(arr(8, opt), k), st.out(arr(9), (k + 1) * 8), st.out(arr(10), (k + 1) * 8),
               st.out(arr(11), bm, 0), st.out(arr(12), bw, 0), st.out(arr(13, opt), k)};
        print_copies(st);               // before the totals are known: the two streams download nothing
        st.out_bytes(arr(11), 7 * k);   // ... and what the device reports afterwards
        st.out_bytes(arr(12), 9 * k);
    } else if (!strcmp(form, "pack_message")) {
        const size_t bound = 100 + 250 * k + db;
        lit = {cv.take(32), cv.take(k * 32), cv.take(k * 32), cv.take(k * 32), cv.take(k), cv.take(k * 4), cv.take(k * 8), cv.take(k * 64),
               cv.take(opt ? (k + 1) * 8 : 0), cv.take(db), cv.take(opt ? k : 0), cv.take(8), cv.take(bound)};
        got = {st.in(arr(0), 32), st.in(arr(1), k * 32), st.in(arr(2), k * 32), st.in(arr(3), k * 32), st.in(arr(4), k), st.in(arr(5), k * 4), st.in(arr(6), k * 8),
               st.in(arr(7), k * 64), st.in(arr(8, opt), (k + 1) * 8), st.in(arr(9, opt), db), st.in(arr(10, opt), k), st.scratch(8), st.out(arr(11), bound, 0)};
        print_copies(st);
        st.out_bytes(arr(11), 90 + 11 * k);
    } else if (!strcmp(form, "unpack_message")) {
        const size_t msg_bytes = 64 + 150 * k + db, kd = db;
        lit = {cv.take(msg_bytes), cv.take(32), cv.take(k * 32), cv.take(k * 32), cv.take(k * 32), cv.take(k), cv.take(k * 4), cv.take(k * 8), cv.take(k * 64),
               cv.take((k + 1) * 8), cv.take(k), cv.take(kd + 16)};
        got = {st.in(arr(0), msg_bytes), st.out(arr(1), 32, 0), st.out(arr(2), k * 32, 0), st.out(arr(3), k * 32, 0), st.out(arr(4), k * 32, 0), st.out(arr(5), k, 0),
               st.out(arr(6), k * 4, 0), st.out(arr(7), k * 8, 0), st.out(arr(8), k * 64, 0), st.out(arr(9), (k + 1) * 8, 0), st.out(arr(10), k, 0),
               st.out(arr(11, opt), kd + 16, 0)};
        print_copies(st);
        const size_t kk = k / 2;   // the message held fewer events than the arrays can take
        st.out_bytes(arr(1), 32);
        for (int i = 2; i <= 4; ++i) st.out_bytes(arr(i), kk * 32);
        st.out_bytes(arr(5), kk); st.out_bytes(arr(6), kk * 4); st.out_bytes(arr(7), kk * 8); st.out_bytes(arr(8), kk * 64);
        st.out_bytes(arr(9), (kk + 1) * 8); st.out_bytes(arr(10), kk);
        if (opt) st.out_bytes(arr(11), kd / 2);
    } else {
        fprintf(stderr, "unknown form %s\n", form);
        return 2;
    }
    lit.push_back(cv.off);
    got.push_back(st.total());
    print("carve", lit);
    print("stage", got);
    print_copies(st);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "align")) return align_cases();
    if (argc == 5 && !strcmp(argv[1], "stage")) return stage_case(argv[2], (size_t)strtoull(argv[3], nullptr, 10), atoi(argv[4]) != 0);
    fprintf(stderr, "usage: %s align | stage <form> <K> <0|1>\n", argv[0]);
    return 2;
}
