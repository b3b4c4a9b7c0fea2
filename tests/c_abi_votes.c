/* A plain-C user of sw_export_votes (include/swirld_hip.h): the size query, then the table.  Prints the rows, the entries
 * and an FNV-1a digest over the four arrays.  Built and run by tests/test_gpu_votes.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "swirld_hip.h"

#define CK(x) do { int rc_ = (x); if (rc_ != SW_OK) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, sw_last_error(ctx)); return 1; } } while (0)

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 32;
    const long long N = argc > 2 ? atoll(argv[2]) : 20000;
    const int nwo = (n + 63) / 64;
    sw_ctx* ctx = NULL;
    uint64_t* stake = malloc(sizeof(uint64_t) * n);
    for (int i = 0; i < n; ++i) stake[i] = 1;
    int32_t *cr = malloc(4 * N), *sp = malloc(4 * N), *op = malloc(4 * N);
    double* t = malloc(8 * N);
    uint8_t* sig = malloc(64 * N);
    if (sw_synth_hashgraph(n, N, 11, 0, 0.0, 0.0, cr, sp, op, t, sig) != SW_OK) return 2;
    if (sw_create(n, stake, 6, 0, &ctx) != SW_OK) { fprintf(stderr, "sw_create: %s\n", sw_last_error(NULL)); return 3; }
    CK(sw_append_events(ctx, N, cr, sp, op, t, sig));
    CK(sw_divide_rounds(ctx, 0, N));
    int maxr = -1, n_new = 0;
    CK(sw_max_round(ctx, &maxr));
    int32_t* newc = malloc(4 * (maxr + 2));
    CK(sw_decide_fame(ctx, newc, maxr + 2, &n_new));
    int64_t rows = 0, entries = 0;
    int rc = sw_export_votes(ctx, 1, maxr + 1, 0, NULL, NULL, NULL, NULL, &rows, &entries);
    if (rc != SW_ERANGE || rows <= 0) { fprintf(stderr, "size query -> %d, %lld rows\n", rc, (long long)rows); return 4; }
    int32_t *voter = malloc(4 * rows), *cand = malloc(4 * rows);
    uint64_t *exists = malloc(8 * rows * nwo), *value = malloc(8 * rows * nwo);
    int64_t rows2 = 0, entries2 = 0;
    CK(sw_export_votes(ctx, 1, maxr + 1, rows, voter, cand, exists, value, &rows2, &entries2));
    if (rows2 != rows || entries2 != entries) return 5;
    unsigned long long h = 1469598103934665603ull;
    for (long long i = 0; i < rows; ++i) { h ^= (unsigned long long)(long long)voter[i]; h *= 1099511628211ull; }
    for (long long i = 0; i < rows; ++i) { h ^= (unsigned long long)(long long)cand[i]; h *= 1099511628211ull; }
    for (long long i = 0; i < rows * nwo; ++i) { h ^= exists[i]; h *= 1099511628211ull; }
    for (long long i = 0; i < rows * nwo; ++i) { h ^= value[i]; h *= 1099511628211ull; }
    printf("%lld %lld %llu\n", (long long)rows, (long long)entries, h);
    sw_destroy(ctx);
    return 0;
}
