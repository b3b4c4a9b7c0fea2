// Host side of the generated histories (include/swirld_hip.h: sw_synth_batch*, sw_get_batch_events), included behind
// batch_api.hip.h.  A call of sw_synth_batch: the host checks arguments and cap_events against its own counts, uploads the
// compact list of participating hashgraphs (who, current state copy, first, K) in ONE copy, launches k_batch_synth
// (batch_synth.hip.h) once, reads 8 bytes per participating hashgraph back (greatest height generated, error word) in the
// one synchronisation the call ends in, and only then decides: every hashgraph within cap_rounds — the counts advance and
// the state copies flip; one beyond it — SW_ERANGE and nothing moves.  What the kernel wrote lies behind events[b] and in
// the copy nobody reads, so a refused call is not observable.
#pragma once

namespace {

int synth_state(sw_batch* c) {
    if (c->sy_state.p) return SW_OK;
    c->sy_lay = swbs::state_layout(c->n);
    const size_t bytes = (size_t)c->B * c->sy_lay.stride;
    unsigned char* q = nullptr;
    if (hipMalloc((void**)&q, bytes) != hipSuccess) { (void)hipGetLastError(); return bfail(c, SW_ENOMEM, "hipMalloc(%zu bytes) for the generator state failed", bytes); }
    c->sy_state.adopt(q, bytes);
    return SW_OK;
}

// room for `bytes` of lists in the pinned buffer and in staging
int synth_lists(sw_batch* c, size_t bytes) {
    if (bytes > c->up_h.cap) {
        BHIPCHK(c, hipStreamSynchronize(c->stream));
        if (!c->up_h.reserve(std::max(bytes, 2 * c->up_h.cap))) return bfail(c, SW_ENOMEM, "pinned host memory for a call's lists (%zu bytes)", bytes);
    }
    return batch_staging(c, bytes);
}

// sw_batch_append validates against the host mirrors of creator and height, which sw_synth_batch does not keep: the
// hashgraphs this append feeds that are behind get theirs from the slab first (two copies each, one synchronisation).
int batch_synth_refresh(sw_batch* c, const int64_t* off) {
    bool any = false;
    for (int64_t b = 0; b < c->B; ++b) {
        if (off[b + 1] == off[b] || !c->sy_behind[b]) continue;
        if (!any) BHIPCHK(c, hipSetDevice(c->device));
        any = true;
        const size_t have = c->cr[b].size(), want = (size_t)c->events[b];
        c->cr[b].resize(want); c->ht[b].resize(want);
        BHIPCHK(c, hipMemcpyAsync(c->cr[b].data() + have, (const int32_t*)c->seg(b, swb_layout::SEG_CR) + have, (want - have) * 4, hipMemcpyDeviceToHost, c->stream));
        BHIPCHK(c, hipMemcpyAsync(c->ht[b].data() + have, (const int32_t*)c->seg(b, swb_layout::SEG_HT) + have, (want - have) * 4, hipMemcpyDeviceToHost, c->stream));
        c->sy_behind[b] = 0;
        c->sy_refreshes++;
    }
    if (any) BHIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

}  // namespace

extern "C" {

int sw_synth_batch_begin(sw_batch* c, const uint8_t* which, const uint64_t* seed, const int32_t* mode, const double* p0, const double* p1) {
    if (!c) return SW_EINVAL;
    if (!seed) return bfail(c, SW_EINVAL, "seed is NULL");
    if (c->n < 2) return bfail(c, SW_EINVAL, "a generated history needs 2 members or more (the batch has %d)", c->n);
    const int64_t B = c->B;
    int64_t m = 0;
    for (int64_t b = 0; b < B; ++b) {
        if (which && !which[b]) continue;
        if (c->events[b]) return bfail(c, SW_EINVAL, "hashgraph %lld already holds %lld events: a generated history starts empty", (long long)b, (long long)c->events[b]);
        if (mode && (mode[b] < 0 || mode[b] > 3)) return bfail(c, SW_EINVAL, "hashgraph %lld: mode %d outside 0..3", (long long)b, mode[b]);
        ++m;
    }
    if (!m) return SW_OK;
    BHIPCHK(c, hipSetDevice(c->device));
    CHK(synth_state(c));
    // the lists: seed, p0, p1 (8 bytes each), who, mode (4 bytes each)
    const size_t o_seed = 0, o_p0 = (size_t)m * 8, o_p1 = (size_t)m * 16, o_who = (size_t)m * 24, o_mode = (size_t)m * 28, bytes = (size_t)m * 32;
    CHK(synth_lists(c, bytes));
    unsigned char* h = c->up_h.p;
    int64_t at = 0;
    for (int64_t b = 0; b < B; ++b) {
        if (which && !which[b]) continue;
        ((uint64_t*)(h + o_seed))[at] = seed[b];
        ((double*)(h + o_p0))[at] = p0 ? p0[b] : 0.0;
        ((double*)(h + o_p1))[at] = p1 ? p1[b] : 0.0;
        ((int*)(h + o_who))[at] = (int)b;
        ((int*)(h + o_mode))[at] = mode ? mode[b] : 0;
        ++at;
    }
    unsigned char* d = c->staging.p;
    BHIPCHK(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_batch_synth_begin, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, c->stream, c->sy_state.p, c->sy_lay, c->n, (long long)m,
                       (const int*)(d + o_who), (const int*)(d + o_mode), (const unsigned long long*)(d + o_seed), (const double*)(d + o_p0),
                       (const double*)(d + o_p1));
    BHIPCHK(c, hipGetLastError());
    BHIPCHK(c, hipStreamSynchronize(c->stream));
    c->sy_launches++;
    for (int64_t b = 0; b < B; ++b)
        if (!which || which[b]) { c->sy_has[b] = 1; c->sy_cur[b] = 0; }
    return SW_OK;
}

int sw_synth_batch(sw_batch* c, const int64_t* K, int64_t* total) {
    if (!c) return SW_EINVAL;
    if (total) *total = 0;
    if (!K) return bfail(c, SW_EINVAL, "K is NULL");
    const int64_t B = c->B;
    const int n = c->n;
    int64_t m = 0, sum = 0;
    for (int64_t b = 0; b < B; ++b) {
        if (K[b] < 0) return bfail(c, SW_EINVAL, "K[%lld] = %lld is negative", (long long)b, (long long)K[b]);
        if (!K[b]) continue;
        if (c->nw_view[b]) return bfail(c, SW_EINVAL, "hashgraph %lld is a view of a gossip network: its events come from the network's turns", (long long)b);
        if (!c->sy_has[b]) return bfail(c, SW_EINVAL, "hashgraph %lld has no generator parameters (sw_synth_batch_begin)", (long long)b);
        if (c->sy_fed[b])
            return bfail(c, SW_EINVAL, "hashgraph %lld has taken a host append since sw_synth_batch_begin: the generator's heads no longer describe it", (long long)b);
        if (c->events[b] == 0 && K[b] < n)
            return bfail(c, SW_EINVAL, "hashgraph %lld: the first instalment is %lld events, the %d roots come first and together", (long long)b, (long long)K[b], n);
        ++m;
    }
    for (int64_t b = 0; b < B; ++b) {
        if (K[b] > c->cap_events - c->events[b])
            return bfail(c, SW_ERANGE, "hashgraph %lld: %lld events stored + %lld generated exceed cap_events = %lld", (long long)b, (long long)c->events[b], (long long)K[b], (long long)c->cap_events);
        sum += K[b];
    }
    if (!m) return SW_OK;
    BHIPCHK(c, hipSetDevice(c->device));
    // the lists: first, K (8 bytes each), who, cur (4 bytes each), and behind them what comes back: 2 ints per entry
    const size_t o_first = 0, o_K = (size_t)m * 8, o_who = (size_t)m * 16, o_cur = (size_t)m * 20, o_res = (size_t)m * 24, bytes = (size_t)m * 32;
    CHK(synth_lists(c, bytes));
    unsigned char* h = c->up_h.p;
    int64_t at = 0;
    for (int64_t b = 0; b < B; ++b) {
        if (!K[b]) continue;
        ((long long*)(h + o_first))[at] = c->events[b];
        ((long long*)(h + o_K))[at] = K[b];
        ((int*)(h + o_who))[at] = (int)b;
        ((int*)(h + o_cur))[at] = c->sy_cur[b];
        ++at;
    }
    unsigned char* d = c->staging.p;
    BHIPCHK(c, hipMemcpyAsync(d, h, o_res, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_batch_synth, dim3((unsigned)m), dim3(64), 0, c->stream, c->recs(), c->sy_state.p, c->sy_lay, (const int*)(d + o_who),
                       (const int*)(d + o_cur), (const long long*)(d + o_first), (const long long*)(d + o_K), (int*)(d + o_res));
    BHIPCHK(c, hipGetLastError());
    c->sy_launches++;
    BHIPCHK(c, hipMemcpyAsync(h + o_res, d + o_res, (size_t)m * 8, hipMemcpyDeviceToHost, c->stream));
    BHIPCHK(c, hipStreamSynchronize(c->stream));
    // the verdict, before anything moves
    const int* res = (const int*)(h + o_res);
    const int* who = (const int*)(h + o_who);
    for (int64_t i = 0; i < m; ++i) {
        const int64_t b = who[i];
        if (res[2 * i + swbs::R_ERROR]) return bfail(c, SW_EIO, "hashgraph %lld: the generator refused what the host had checked (nothing stored)", (long long)b);
        const int hmax = std::max(c->hmax[b], res[2 * i + swbs::R_HEIGHT]);
        if ((int64_t)hmax + 3 > c->cap_rounds)
            return bfail(c, SW_ERANGE, "hashgraph %lld: height %d needs %d rounds of capacity, cap_rounds = %lld (nothing stored)", (long long)b, hmax, hmax + 3, (long long)c->cap_rounds);
    }
    for (int64_t i = 0; i < m; ++i) {
        const int64_t b = who[i];
        c->hmax[b] = std::max(c->hmax[b], res[2 * i + swbs::R_HEIGHT]);
        c->events[b] += K[b];
        c->sy_cur[b] ^= 1;
        c->sy_behind[b] = 1;
    }
    c->sy_calls++;
    c->sy_events += sum;
    if (total) *total = sum;
    return SW_OK;
}

int sw_synth_batch_stats(sw_batch* c, int64_t out[4]) {
    if (!c || !out) return SW_EINVAL;
    out[0] = c->sy_calls; out[1] = c->sy_events; out[2] = c->sy_launches; out[3] = c->sy_refreshes;
    return SW_OK;
}

int sw_get_batch_events(sw_batch* c, int64_t b, int64_t first, int64_t K, int32_t* creator, int32_t* self_parent, int32_t* other_parent, double* t,
                        uint8_t* sig64) {
    if (!c) return SW_EINVAL;
    CHK(batch_index(c, b, "sw_get_batch_events"));
    CHK(batch_event_range(c, b, first, K, c->events[b], "sw_get_batch_events"));
    if (creator) CHK(batch_copy(c, creator, (const int32_t*)c->seg(b, swb_layout::SEG_CR) + first, (size_t)K * 4));
    if (self_parent) CHK(batch_copy(c, self_parent, (const int32_t*)c->seg(b, swb_layout::SEG_SP) + first, (size_t)K * 4));
    if (other_parent) CHK(batch_copy(c, other_parent, (const int32_t*)c->seg(b, swb_layout::SEG_OP) + first, (size_t)K * 4));
    if (t) CHK(batch_copy(c, t, (const double*)c->seg(b, swb_layout::SEG_T) + first, (size_t)K * 8));
    if (sig64) CHK(batch_copy(c, sig64, c->seg(b, swb_layout::SEG_SIG) + (size_t)first * 64, (size_t)K * 64));
    return SW_OK;
}

}  // extern "C"
