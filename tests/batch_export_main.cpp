// Stand-alone check of the whole-batch export's per-chunk function (py-swirld_amd/csrc/batch_export.hip.h,
// swbx::export_chunk), built by tests/test_batch_export_host.py with AddressSanitizer and UBSan.  Random plans: 1 to 3000
// hashgraphs of 0 to 5 entries with runs of empty segments at the front, in the middle and at the end; elements of 1, 4 and
// 8 bytes; plain arrays and rows of n columns at a stride of npad.  Every source segment is an allocation of its own of
// exactly the bytes the export may read (the last row ends at column n), the offsets are exactly B + 1 entries, the output
// exactly total x columns x width bytes: one byte read or written beyond any of them is a sanitizer error.  Every chunk is
// run, in a shuffled order (chunks are independent), and the output compared with a naive loop.
// Usage: batch_export_main <seed> <trials>; prints "ok <plans> <entries>".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "../py-swirld_amd/csrc/batch_export.hip.h"

namespace {

std::mt19937_64 rng;
int64_t rnd(int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); }

std::vector<long long> counts(int64_t B) {
    std::vector<long long> c((size_t)B);
    for (auto& v : c) v = rnd(0, 5);
    auto clear = [&](int64_t a, int64_t len) { for (int64_t b = a; b < a + len && b < B; ++b) c[(size_t)b] = 0; };
    const int shape = (int)rnd(0, 5);
    if (shape & 1) clear(0, rnd(1, 40));                          // empty at the front
    if (shape & 2) clear(rnd(0, B - 1), rnd(1, 70));              // ... in the middle
    if (shape & 4) clear(B - std::min<int64_t>(B, rnd(1, 40)), 40);   // ... at the end
    if (rnd(0, 9) == 0) clear(0, B);                              // nothing at all
    if (rnd(0, 9) == 0) { clear(0, B); c[(size_t)rnd(0, B - 1)] = rnd(1, 5); }   // one hashgraph alone
    return c;
}

template <class T>
long long run_plan(int64_t B, int cols, long long stride) {
    const std::vector<long long> cnt = counts(B);
    long long* off = (long long*)malloc((size_t)(B + 1) * sizeof(long long));
    off[0] = 0;
    for (int64_t b = 0; b < B; ++b) off[b + 1] = off[b] + cnt[(size_t)b];
    const long long total = off[B];
    unsigned long long* src = (unsigned long long*)malloc((size_t)B * sizeof(unsigned long long));
    std::vector<T*> seg((size_t)B, nullptr);
    std::vector<T> want;
    for (int64_t b = 0; b < B; ++b) {
        const long long k = cnt[(size_t)b];
        src[b] = 0;   // an empty segment has no source: its address is never used
        if (!k) continue;
        const size_t len = (size_t)((k - 1) * stride + cols);
        T* s = (T*)malloc(len * sizeof(T));
        for (size_t i = 0; i < len; ++i) s[i] = (T)rng();
        for (long long e = 0; e < k; ++e)
            for (int j = 0; j < cols; ++j) want.push_back(s[e * stride + j]);
        seg[(size_t)b] = s;
        src[b] = (unsigned long long)(uintptr_t)s;
    }
    const size_t out_elems = (size_t)total * cols;
    T* out = (T*)malloc(out_elems ? out_elems * sizeof(T) : 1);
    memset(out, 0xa5, out_elems * sizeof(T));
    swbx::Plan p{};
    p.off = off; p.B = B; p.total = total; p.n_arrays = 2;
    p.a[1] = swbx::Array{src, (unsigned char*)out, (int)sizeof(T), cols, stride};   // (array 0 stays empty: k is honoured)
    const long long chunks = swbx::chunks_of(total, cols, (int)sizeof(T));
    std::vector<long long> order((size_t)chunks + 4);
    std::iota(order.begin(), order.end(), -1ll);   // one chunk before the first and three behind the last: they do nothing
    std::shuffle(order.begin(), order.end(), rng);
    for (long long ch : order) swbx::export_chunk(p, 1, ch);
    if (want.size() != out_elems || (out_elems && memcmp(out, want.data(), out_elems * sizeof(T)) != 0)) {
        fprintf(stderr, "mismatch: B %lld, width %d, cols %d, stride %lld, total %lld\n", (long long)B, (int)sizeof(T), cols, stride, total);
        exit(1);
    }
    for (T* s : seg) free(s);
    free(out); free(src); free(off);
    return total;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int trials = argc > 2 ? atoi(argv[2]) : 60;
    rng.seed(seed);
    static const int rows[4][2] = {{4, 16}, {5, 16}, {33, 48}, {64, 64}};
    long long plans = 0, entries = 0;
    for (int t = 0; t < trials; ++t) {
        const int64_t B = t == 0 ? 1 : t == 1 ? 3000 : t == 2 ? 2 : t % 3 == 0 ? rnd(1, 40) : rnd(1, 3000);
        for (int mode = 0; mode < 5; ++mode) {
            const int cols = mode ? rows[mode - 1][0] : 1;
            const long long stride = mode ? rows[mode - 1][1] : 1;
            entries += run_plan<uint8_t>(B, cols, stride);
            entries += run_plan<uint32_t>(B, cols, stride);
            entries += run_plan<uint64_t>(B, cols, stride);
            plans += 3;
        }
    }
    printf("ok %lld %lld\n", plans, entries);
    return 0;
}
