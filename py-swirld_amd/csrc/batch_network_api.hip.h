// Host side of the gossip networks of a batch (include/swirld_hip.h: sw_network_batch_*), included behind the other batch
// files.  Every call checks everything on the host before anything is enqueued — the schedule, that every network was
// begun, and the capacities against the conservative bound n + turns so far + turns of this call (a view never holds more
// than its network has created, and a height is below that count) — so nothing is ever refused after the launch and no
// state needs two copies.  One upload of the lists, one launch of k_batch_network_turns (batch_network.hip.h) per
// MAX_TURNS_PER_LAUNCH turns of the longest network, one read-back: the summaries, the view words and the network words.
#pragma once

namespace {

constexpr size_t nw_up64(size_t v) { return (v + 63) & ~(size_t)63; }

const swbn::Net* nw_net(const sw_batch* c, int64_t g) { return (const swbn::Net*)(c->nw_h.p + (size_t)g * sizeof(swbn::Net)); }
const swbn::View* nw_view_words(const sw_batch* c, int64_t b) { return (const swbn::View*)(c->nw_h.p + c->nw_lay.views + (size_t)b * sizeof(swbn::View)); }

int network_shape(sw_batch* c, const char* what) {
    if (c->n < 2) return bfail(c, SW_EINVAL, "%s: a network needs 2 members or more (the batch has %d)", what, c->n);
    if (c->B % c->n) return bfail(c, SW_EINVAL, "%s: %lld hashgraphs are not a multiple of %d members: consecutive hashgraphs form a network", what, (long long)c->B, c->n);
    return SW_OK;
}

int network_state(sw_batch* c) {
    if (c->nw_state.p) return SW_OK;
    c->nw_lay = swbn::layout((uint64_t)c->B, (uint64_t)c->n, (uint64_t)c->cap_events);
    const size_t bytes = (size_t)c->nw_lay.total;
    if (!c->nw_h.reserve((size_t)c->nw_lay.cols)) return bfail(c, SW_ENOMEM, "pinned host memory for the network words (%zu bytes)", (size_t)c->nw_lay.cols);
    memset(c->nw_h.p, 0, (size_t)c->nw_lay.cols);
    unsigned char* q = nullptr;
    if (hipMalloc((void**)&q, bytes) != hipSuccess) { (void)hipGetLastError(); return bfail(c, SW_ENOMEM, "hipMalloc(%zu bytes) for the network state failed", bytes); }
    c->nw_state.adopt(q, bytes);
    BHIPCHK(c, hipMemsetAsync(q, 0, (size_t)c->nw_lay.cols, c->stream));   // no network begun, none stopped
    c->nw_begun.assign((size_t)(c->B / c->n), 0); c->nw_stopped.assign((size_t)(c->B / c->n), 0);
    return SW_OK;
}

// the one read-back of a call, and what the host's counts become: exactly what append + step would have left
int network_read_back(sw_batch* c, const std::vector<int>& who, int64_t* n_stopped) {
    const int n = c->n;
    // what took part: per network the summaries and the words of its n views (each contiguous) and its own words; a call
    // that runs most of a large batch takes the three arrays whole instead of thousands of small copies
    const size_t sum_row = swb_layout::SUMMARY_WORDS * sizeof(long long);
    if (who.size() > 16) {
        BHIPCHK(c, hipMemcpyAsync(c->sum_h.p, c->mem.p + c->lay.summaries, (size_t)c->B * sum_row, hipMemcpyDeviceToHost, c->stream));
        BHIPCHK(c, hipMemcpyAsync(c->nw_h.p, c->nw_state.p, (size_t)c->nw_lay.cols, hipMemcpyDeviceToHost, c->stream));
    } else {
        for (int g : who) {
            const size_t b0 = (size_t)g * n, o_net = (size_t)g * sizeof(swbn::Net), o_view = (size_t)c->nw_lay.views + b0 * sizeof(swbn::View);
            BHIPCHK(c, hipMemcpyAsync(c->sum_h.p + b0 * swb_layout::SUMMARY_WORDS, c->mem.p + c->lay.summaries + b0 * sum_row, (size_t)n * sum_row,
                                      hipMemcpyDeviceToHost, c->stream));
            BHIPCHK(c, hipMemcpyAsync(c->nw_h.p + o_net, c->nw_state.p + o_net, sizeof(swbn::Net), hipMemcpyDeviceToHost, c->stream));
            BHIPCHK(c, hipMemcpyAsync(c->nw_h.p + o_view, c->nw_state.p + o_view, (size_t)n * sizeof(swbn::View), hipMemcpyDeviceToHost, c->stream));
        }
    }
    BHIPCHK(c, hipStreamSynchronize(c->stream));
    int64_t stopped = 0;
    for (int g : who) {
        for (int i = 0; i < n; ++i) {
            const int64_t b = (int64_t)g * n + i;
            const swbn::View* v = nw_view_words(c, b);
            const long long* s = c->sum_h.p + b * swb_layout::SUMMARY_WORDS;
            c->events[b] = v->events;
            c->hmax[b] = v->hmax;
            c->divided[b] = s[swb::S_DIVIDED];
            c->sy_behind[b] = 1;   // (the creator / height mirrors of sw_batch_append: a view takes no append, they stay empty)
            if (s[swb::S_STAGE] != swb::STAGE_NONE) c->frozen[b] = 1;
        }
        if (nw_net(c, g)->stage != 0 && !c->nw_stopped[(size_t)g]) { c->nw_stopped[(size_t)g] = 1; ++stopped; }
    }
    if (n_stopped) *n_stopped = stopped;
    return SW_OK;
}

// cnt[g] turns per network; explicit form: off / puller / peer (t, sig nullable); drawn form: puller == NULL
int network_go(sw_batch* c, const char* what, const std::vector<int64_t>& cnt, const int64_t* off, const int32_t* puller, const int32_t* peer,
               const double* t, const uint8_t* sig64, int64_t* n_stopped) {
    const int n = c->n;
    const int64_t G = c->B / n;
    std::vector<int> who;
    int64_t most = 0;
    for (int64_t g = 0; g < G; ++g) {
        if (!cnt[(size_t)g]) continue;
        if (!c->nw_state.p || !c->nw_begun[(size_t)g]) return bfail(c, SW_EINVAL, "%s: network %lld was never begun (sw_network_batch_begin)", what, (long long)g);
        if (c->nw_stopped[(size_t)g]) continue;   // skipped, whatever the schedule says
        if (puller)
            for (int64_t k = off[g]; k < off[g + 1]; ++k) {
                if (puller[k] < 0 || puller[k] >= n || peer[k] < 0 || peer[k] >= n)
                    return bfail(c, SW_EINVAL, "%s: network %lld, turn %lld: node %d pulls from node %d, outside 0..%d", what, (long long)g, (long long)(k - off[g]), puller[k], peer[k], n - 1);
                if (puller[k] == peer[k])
                    return bfail(c, SW_EINVAL, "%s: network %lld, turn %lld: node %d pulls from itself", what, (long long)g, (long long)(k - off[g]), puller[k]);
            }
        const int64_t need = nw_net(c, g)->created + cnt[(size_t)g];   // n + turns so far + turns of this call
        if (need > c->cap_events)
            return bfail(c, SW_ERANGE, "%s: network %lld: %lld events created + %lld turns exceed cap_events = %lld", what, (long long)g,
                         (long long)nw_net(c, g)->created, (long long)cnt[(size_t)g], (long long)c->cap_events);
        if (need + 3 > c->cap_rounds)
            return bfail(c, SW_ERANGE, "%s: network %lld: %lld events need %lld rounds of capacity, cap_rounds = %lld", what, (long long)g, (long long)need,
                         (long long)(need + 3), (long long)c->cap_rounds);
        who.push_back((int)g);
        most = std::max(most, cnt[(size_t)g]);
    }
    if (n_stopped) *n_stopped = 0;
    if (who.empty()) return SW_OK;
    BHIPCHK(c, hipSetDevice(c->device));
    const int64_t CH = swbn::MAX_TURNS_PER_LAUNCH, nl = (most + CH - 1) / CH;
    // the lists of launch j: who, off, cnt of the networks that still have turns left in it
    struct Launch { size_t who, off, cnt; int64_t m; };
    std::vector<Launch> launches((size_t)nl);
    size_t bytes = 0;
    for (int64_t j = 0; j < nl; ++j) {
        int64_t mj = 0;
        for (int g : who) mj += cnt[(size_t)g] > j * CH;
        Launch& l = launches[(size_t)j];
        l.m = mj;
        l.off = bytes; bytes += (size_t)mj * 8;
        l.cnt = bytes; bytes += (size_t)mj * 8;
        l.who = bytes; bytes += nw_up64((size_t)mj * 4);
    }
    const size_t T = puller ? (size_t)off[G] : 0;
    const size_t o_pull = nw_up64(bytes), o_peer = o_pull + nw_up64(T * 4), o_t = o_peer + nw_up64(T * 4), o_sig = o_t + nw_up64(T * 8), o_end = o_sig + T * 64;
    CHK(synth_lists(c, o_end));
    for (int64_t j = 0; j < nl; ++j) {
        const Launch& l = launches[(size_t)j];
        long long* lo = (long long*)(c->up_h.p + l.off);
        long long* lc = (long long*)(c->up_h.p + l.cnt);
        int* lw = (int*)(c->up_h.p + l.who);
        int64_t at = 0;
        for (int g : who) {
            const int64_t left = cnt[(size_t)g] - j * CH;
            if (left <= 0) continue;
            lw[at] = g; lo[at] = (puller ? off[g] : 0) + j * CH; lc[at] = std::min(CH, left);
            ++at;
        }
    }
    unsigned char* d = c->staging.p;
    BHIPCHK(c, hipMemcpyAsync(d, c->up_h.p, bytes, hipMemcpyHostToDevice, c->stream));
    if (T) {
        BHIPCHK(c, hipMemcpyAsync(d + o_pull, puller, T * 4, hipMemcpyHostToDevice, c->stream));
        BHIPCHK(c, hipMemcpyAsync(d + o_peer, peer, T * 4, hipMemcpyHostToDevice, c->stream));
        if (t) BHIPCHK(c, hipMemcpyAsync(d + o_t, t, T * 8, hipMemcpyHostToDevice, c->stream));
        if (sig64) BHIPCHK(c, hipMemcpyAsync(d + o_sig, sig64, T * 64, hipMemcpyHostToDevice, c->stream));
    }
    const int64_t turns0 = [&] { int64_t s = 0; for (int g : who) s += nw_net(c, g)->turns; return s; }();
    const int64_t imp0 = [&] { int64_t s = 0; for (int g : who) s += nw_net(c, g)->imported; return s; }();
    for (int64_t j = 0; j < nl; ++j) {
        const Launch& l = launches[(size_t)j];
        hipLaunchKernelGGL(k_batch_network_turns, dim3((unsigned)l.m), dim3(64), 0, c->stream, c->recs(), c->nw_state.p, c->nw_lay, (const int*)(d + l.who),
                           (const long long*)(d + l.off), (const long long*)(d + l.cnt), T ? (const int*)(d + o_pull) : nullptr,
                           T ? (const int*)(d + o_peer) : nullptr, T && t ? (const double*)(d + o_t) : nullptr,
                           T && sig64 ? (const unsigned char*)(d + o_sig) : nullptr);
        c->nw_launches++;
    }
    BHIPCHK(c, hipGetLastError());
    CHK(network_read_back(c, who, n_stopped));
    c->nw_calls++;
    for (int g : who) { c->nw_turns += nw_net(c, g)->turns; c->nw_imported += nw_net(c, g)->imported; }
    c->nw_turns -= turns0; c->nw_imported -= imp0;
    return SW_OK;
}

int export_event_numbers(sw_batch* c, const char* what, const int64_t* first, const int64_t* count, int64_t cap, int64_t* off, int32_t* numbers,
                         int64_t* total, bool device, void* stream) {
    if (!c) return SW_EINVAL;
    if (!off) return bfail(c, SW_EINVAL, "%s: off is NULL", what);
    std::vector<int64_t> start, cnt;
    CHK(export_ranges(c, what, first, count, [&](int64_t b) { return c->nw_view[b] ? c->events[b] : (int64_t)0; }, start, cnt));
    const XArr a[1] = {{numbers, 0, 4, 1, 1, true}};
    return batch_export(c, what, start, cnt, cap, off, total, a, 1, device, stream);
}

}  // namespace

extern "C" {

int sw_network_batch_begin(sw_batch* c, const uint8_t* which, const uint64_t* seed, const double* root_t, const uint8_t* root_sig64) {
    if (!c) return SW_EINVAL;
    if (!seed) return bfail(c, SW_EINVAL, "seed is NULL");
    CHK(network_shape(c, "sw_network_batch_begin"));
    const int n = c->n, np = c->npad;
    const int64_t G = c->B / n;
    std::vector<int> who;
    for (int64_t g = 0; g < G; ++g) {
        if (which && !which[g]) continue;
        for (int i = 0; i < n; ++i) {
            const int64_t b = g * n + i;
            if (c->events[b]) return bfail(c, SW_EINVAL, "network %lld: hashgraph %lld already holds %lld events: a network begins with empty views", (long long)g, (long long)b, (long long)c->events[b]);
            if (c->sy_has[b]) return bfail(c, SW_EINVAL, "network %lld: hashgraph %lld has generator parameters (sw_synth_batch_begin)", (long long)g, (long long)b);
            if (memcmp(c->stake_rows.data() + (size_t)b * np, c->stake_rows.data() + (size_t)g * n * np, (size_t)np * 4))
                return bfail(c, SW_EINVAL, "network %lld: hashgraph %lld has another stake row than hashgraph %lld: the views of a network share their stakes", (long long)g, (long long)b, (long long)(g * n));
        }
        who.push_back((int)g);
    }
    if (who.empty()) return SW_OK;
    BHIPCHK(c, hipSetDevice(c->device));
    CHK(network_state(c));
    const size_t m = who.size();
    const size_t o_seed = 0, o_who = nw_up64(m * 8), o_t = o_who + nw_up64(m * 4), o_sig = o_t + nw_up64(m * n * 8), o_end = o_sig + m * n * 64;
    CHK(synth_lists(c, o_end));
    unsigned char* h = c->up_h.p;
    for (size_t x = 0; x < m; ++x) {
        const size_t g = (size_t)who[x];
        ((uint64_t*)(h + o_seed))[x] = seed[g];
        ((int*)(h + o_who))[x] = who[x];
        if (root_t) memcpy(h + o_t + x * n * 8, root_t + g * n, (size_t)n * 8);
        if (root_sig64) memcpy(h + o_sig + x * n * 64, root_sig64 + g * n * 64, (size_t)n * 64);
    }
    unsigned char* d = c->staging.p;
    BHIPCHK(c, hipMemcpyAsync(d, h, root_sig64 ? o_end : (root_t ? o_sig : o_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_batch_network_begin, dim3((unsigned)m), dim3(64), 0, c->stream, c->recs(), c->nw_state.p, c->nw_lay, (const int*)(d + o_who),
                       (const unsigned long long*)(d + o_seed), root_t ? (const double*)(d + o_t) : nullptr,
                       root_sig64 ? (const unsigned char*)(d + o_sig) : nullptr);
    BHIPCHK(c, hipGetLastError());
    c->nw_launches++;
    for (int g : who) {
        c->nw_begun[(size_t)g] = 1;
        for (int i = 0; i < n; ++i) c->nw_view[(size_t)g * n + i] = 1;
    }
    return network_read_back(c, who, nullptr);
}

int sw_network_batch_turns(sw_batch* c, const int64_t* off, const int32_t* puller, const int32_t* peer, const double* t, const uint8_t* sig64,
                           int64_t* n_stopped) {
    if (!c) return SW_EINVAL;
    if (n_stopped) *n_stopped = 0;
    CHK(network_shape(c, "sw_network_batch_turns"));
    if (!off) return bfail(c, SW_EINVAL, "off is NULL");
    const int64_t G = c->B / c->n;
    if (off[0] != 0) return bfail(c, SW_EINVAL, "off[0] must be 0");
    std::vector<int64_t> cnt((size_t)G);
    for (int64_t g = 0; g < G; ++g) {
        if (off[g + 1] < off[g]) return bfail(c, SW_EINVAL, "off must not decrease (network %lld)", (long long)g);
        cnt[(size_t)g] = off[g + 1] - off[g];
    }
    if (off[G] == 0) return SW_OK;
    if (!puller || !peer) return bfail(c, SW_EINVAL, "puller / peer is NULL");
    return network_go(c, "sw_network_batch_turns", cnt, off, puller, peer, t, sig64, n_stopped);
}

int sw_network_batch_run(sw_batch* c, const int64_t* T, int64_t* n_stopped) {
    if (!c) return SW_EINVAL;
    if (n_stopped) *n_stopped = 0;
    CHK(network_shape(c, "sw_network_batch_run"));
    if (!T) return bfail(c, SW_EINVAL, "T is NULL");
    const int64_t G = c->B / c->n;
    std::vector<int64_t> cnt((size_t)G);
    for (int64_t g = 0; g < G; ++g) {
        if (T[g] < 0) return bfail(c, SW_EINVAL, "T[%lld] = %lld is negative", (long long)g, (long long)T[g]);
        cnt[(size_t)g] = T[g];
    }
    return network_go(c, "sw_network_batch_run", cnt, nullptr, nullptr, nullptr, nullptr, nullptr, n_stopped);
}

int sw_network_batch_get(sw_batch* c, int64_t* out) {
    if (!c || !out) return SW_EINVAL;
    CHK(network_shape(c, "sw_network_batch_get"));
    const int64_t G = c->B / c->n;
    for (int64_t g = 0; g < G; ++g) {
        int64_t* o = out + g * SW_NETWORK_BATCH_WORDS;
        if (!c->nw_state.p || !c->nw_begun[(size_t)g]) { o[0] = o[1] = o[2] = o[3] = o[4] = 0; o[5] = -1; continue; }
        const swbn::Net* net = nw_net(c, g);
        o[0] = 1; o[1] = net->turns; o[2] = net->created; o[3] = net->stage; o[4] = net->code; o[5] = net->view;
    }
    return SW_OK;
}

int sw_network_batch_heads(sw_batch* c, int32_t* out) {
    if (!c || !out) return SW_EINVAL;
    for (int64_t b = 0; b < c->B; ++b) out[b] = c->nw_view[b] ? nw_view_words(c, b)->head : -1;
    return SW_OK;
}

int sw_network_batch_stats(sw_batch* c, int64_t out[4]) {
    if (!c || !out) return SW_EINVAL;
    out[0] = c->nw_calls; out[1] = c->nw_turns; out[2] = c->nw_imported; out[3] = c->nw_launches;
    return SW_OK;
}

int sw_get_network_event_numbers(sw_batch* c, int64_t b, int64_t first, int64_t K, int32_t* out) {
    if (!c || !out) return SW_EINVAL;
    CHK(batch_index(c, b, "sw_get_network_event_numbers"));
    if (!c->nw_view[b]) return bfail(c, SW_EINVAL, "sw_get_network_event_numbers: hashgraph %lld is not a view of a begun network", (long long)b);
    CHK(batch_event_range(c, b, first, K, c->events[b], "sw_get_network_event_numbers"));
    return batch_copy(c, out, c->nw_lay.number(c->nw_state.p, (uint64_t)b) + first, (size_t)K * 4);
}

int sw_export_network_event_numbers(sw_batch* c, const int64_t* first, const int64_t* count, int64_t cap, int64_t* off, int32_t* numbers, int64_t* total) {
    return export_event_numbers(c, "sw_export_network_event_numbers", first, count, cap, off, numbers, total, false, nullptr);
}
int sw_export_network_event_numbers_device(sw_batch* c, const int64_t* first, const int64_t* count, int64_t cap, int64_t* off, int32_t* d_numbers,
                                         int64_t* total, void* user_stream) {
    return export_event_numbers(c, "sw_export_network_event_numbers_device", first, count, cap, off, d_numbers, total, true, user_stream);
}

}  // extern "C"
