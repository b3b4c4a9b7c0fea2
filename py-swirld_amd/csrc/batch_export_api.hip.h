// Host side of the whole-batch exports (include/swirld_hip.h: sw_export_batch_*), included behind batch_api.hip.h.
// Every call: the host checks the ranges against its mirrors (sum_h of the last step's read-back, events[]), makes the
// offsets by a prefix sum over B and so knows the total before anything is enqueued; the plan (offsets, one source
// address per hashgraph and array) goes up through a pinned slot; ONE launch of k_batch_export (batch_export.hip.h)
// gathers every requested array.  Host form: into the staging buffer, one copy back per array, one synchronisation.
// Device form: into the caller's arrays, the caller's stream waits on an event, no synchronisation.
#pragma once

namespace {

// a data array of a call: out NULL = not wanted; numbers: the source is the view's number column of the network state, not a segment
struct XArr { void* out; int seg, width, cols; long long stride; bool numbers = false; };

bool on_batch_device(const sw_batch* c, const void* p, size_t bytes) {
    const char* ends[2] = {(const char*)p, (const char*)p + (bytes ? bytes - 1 : 0)};
    for (const char* q : ends) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, q) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (at.type != hipMemoryTypeDevice || at.device != c->device) return false;
    }
    return true;
}

// where array x of hashgraph b starts (NULL: a number column of a batch without network state; such a hashgraph has no entries)
const unsigned char* export_source(const sw_batch* c, int64_t b, const XArr& x) {
    if (!x.numbers) return c->seg(b, x.seg);
    if (!c->nw_state.p) return nullptr;
    return (const unsigned char*)c->nw_lay.number(c->nw_state.p, (uint64_t)b);
}

// The ring slot of this call's plan.  A slot is rewritten only once its last upload has left it: with fewer than
// XP_SLOTS exports in flight that event is long complete and the wait returns at once.
int export_slot(sw_batch* c, size_t bytes, int* slot) {
    const int s = c->xp_next;
    c->xp_next = (s + 1) % sw_batch::XP_SLOTS;
    BHIPCHK(c, (hipError_t)c->xp_up[s].ensure(hipEventDisableTiming));
    if (c->xp_busy[s]) BHIPCHK(c, hipEventSynchronize(c->xp_up[s]));
    c->xp_busy[s] = false;
    if (!c->xp_h[s].reserve(bytes)) return bfail(c, SW_ENOMEM, "pinned host memory for an export plan (%zu bytes)", bytes);
    *slot = s;
    return SW_OK;
}

// start[b], cnt[b]: the checked range of hashgraph b in ENTRIES (cnt >= 0).  Fills off and *total, then gathers.
int batch_export(sw_batch* c, const char* what, const std::vector<int64_t>& start, const std::vector<int64_t>& cnt, int64_t cap, int64_t* off,
                 int64_t* total, const XArr* arrs, int n_arrs, bool device, void* user_stream) {
    const int64_t B = c->B;
    c->xp_calls++;
    XArr want[swbx::MAX_ARRAYS];
    int na = 0;
    for (int k = 0; k < n_arrs; ++k)
        if (arrs[k].out) want[na++] = arrs[k];
    if (device)
        for (int k = 0; k < na; ++k)
            if ((uintptr_t)want[k].out & 15) return bfail(c, SW_EINVAL, "%s: a device array that is not 16-byte aligned (nothing written)", what);
    off[0] = 0;
    for (int64_t b = 0; b < B; ++b) off[b + 1] = off[b] + cnt[b];
    const int64_t T = off[B];
    if (total) *total = T;
    if (!na) return SW_OK;   // a sizing call
    if (T > cap) return bfail(c, SW_ERANGE, "%s: %lld entries, the arrays hold %lld (nothing written; off and total are filled)", what, (long long)T, (long long)cap);
    if (!T) return SW_OK;
    BHIPCHK(c, hipSetDevice(c->device));
    if (device)
        for (int k = 0; k < na; ++k)
            if (!on_batch_device(c, want[k].out, (size_t)T * want[k].cols * want[k].width))
                return bfail(c, SW_EINVAL, "%s: every data array must lie in memory of device %d (a host pointer, or another device's)", what, c->device);
    // ---- the plan: off, then B source addresses per array
    const size_t off_bytes = ((size_t)(B + 1) * 8 + 63) & ~(size_t)63, src_bytes = ((size_t)B * 8 + 63) & ~(size_t)63;
    const size_t plan_bytes = off_bytes + swbx::MAX_ARRAYS * src_bytes;   // (a function of B alone: allocated once)
    if (!c->xp_d.p) {
        unsigned char* q = nullptr;
        if (hipMalloc((void**)&q, plan_bytes) != hipSuccess) { (void)hipGetLastError(); return bfail(c, SW_ENOMEM, "hipMalloc(%zu bytes) for the export plan failed", plan_bytes); }
        c->xp_d.adopt(q, plan_bytes);
    }
    int slot = 0;
    CHK(export_slot(c, plan_bytes, &slot));
    unsigned char* h = c->xp_h[slot].p;
    memcpy(h, off, (size_t)(B + 1) * 8);
    swbx::Plan p{};
    p.off = (const long long*)c->xp_d.p;
    p.B = B; p.total = T; p.n_arrays = na;
    long long most = 0;
    size_t out_off[swbx::MAX_ARRAYS], out_bytes[swbx::MAX_ARRAYS], stage_bytes = 0;
    for (int k = 0; k < na; ++k) {
        const XArr& x = want[k];
        unsigned long long* src = (unsigned long long*)(h + off_bytes + (size_t)k * src_bytes);
        for (int64_t b = 0; b < B; ++b)
            src[b] = (unsigned long long)(uintptr_t)export_source(c, b, x) + (unsigned long long)start[b] * (unsigned long long)x.stride * (unsigned)x.width;
        out_bytes[k] = (size_t)T * x.cols * x.width;
        out_off[k] = stage_bytes;
        stage_bytes += (out_bytes[k] + 255) & ~(size_t)255;
        p.a[k].src = (const unsigned long long*)(c->xp_d.p + off_bytes + (size_t)k * src_bytes);
        p.a[k].width = x.width; p.a[k].cols = x.cols; p.a[k].stride = x.stride;
        most = std::max(most, swbx::chunks_of(T, x.cols, x.width));
    }
    const long long blocks = (most + swbx::THREADS - 1) / swbx::THREADS;
    if (blocks > 0x7fffffffll) return bfail(c, SW_ERANGE, "%s: %lld entries are more than one launch covers", what, (long long)T);
    if (!device) CHK(batch_staging(c, stage_bytes));
    for (int k = 0; k < na; ++k) p.a[k].dst = device ? (unsigned char*)want[k].out : c->staging.p + out_off[k];
    hipStream_t user = (hipStream_t)user_stream;
    if (device) {   // behind the earlier readers of the caller's arrays
        BHIPCHK(c, (hipError_t)c->ev_user.ensure(hipEventDisableTiming));
        BHIPCHK(c, hipEventRecord(c->ev_user, user));
        BHIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_user, 0));
    }
    BHIPCHK(c, hipMemcpyAsync(c->xp_d.p, h, off_bytes + (size_t)na * src_bytes, hipMemcpyHostToDevice, c->stream));
    BHIPCHK(c, hipEventRecord(c->xp_up[slot], c->stream));
    c->xp_busy[slot] = true;
    hipLaunchKernelGGL(k_batch_export, dim3((unsigned)blocks, (unsigned)na), dim3(swbx::THREADS), 0, c->stream, p);
    BHIPCHK(c, hipGetLastError());
    c->xp_launches++;
    c->xp_entries += T;
    if (device) {
        BHIPCHK(c, hipEventRecord(c->ev_user, c->stream));
        BHIPCHK(c, hipStreamWaitEvent(user, c->ev_user, 0));
        return SW_OK;
    }
    for (int k = 0; k < na; ++k) {
        BHIPCHK(c, hipMemcpyAsync(want[k].out, c->staging.p + out_off[k], out_bytes[k], hipMemcpyDeviceToHost, c->stream));
        c->xp_d2h++;
    }
    BHIPCHK(c, hipStreamSynchronize(c->stream));
    c->xp_busy[slot] = false;
    return SW_OK;
}

// [first[b], first[b] + count[b]) of limit(b) entries, with the defaults of the header (first NULL: 0; count NULL: to the end)
template <class Limit>
int export_ranges(sw_batch* c, const char* what, const int64_t* first, const int64_t* count, Limit limit, std::vector<int64_t>& start,
                  std::vector<int64_t>& cnt) {
    start.resize((size_t)c->B); cnt.resize((size_t)c->B);
    for (int64_t b = 0; b < c->B; ++b) {
        const int64_t lim = limit(b), f = first ? first[b] : 0;
        if (f < 0 || f > lim || (count && (count[b] < 0 || count[b] > lim - f)))
            return bfail(c, SW_ERANGE, "%s: [%lld, %lld) outside the %lld entries of hashgraph %lld (nothing written)", what, (long long)f,
                         (long long)(f + (count ? count[b] : 0)), (long long)lim, (long long)b);
        start[b] = f;
        cnt[b] = count ? count[b] : lim - f;
    }
    return SW_OK;
}

int export_ordered(sw_batch* c, const char* what, const int64_t* first, const int64_t* count, int64_t cap, int64_t* off, int32_t* event,
                   int32_t* rr, double* time, int64_t* total, bool device, void* stream) {
    if (!c) return SW_EINVAL;
    if (!off) return bfail(c, SW_EINVAL, "%s: off is NULL", what);
    std::vector<int64_t> start, cnt;
    CHK(export_ranges(c, what, first, count, [&](int64_t b) { return (int64_t)c->sum_h.p[b * swb_layout::SUMMARY_WORDS + swb::S_ORDERED]; }, start, cnt));
    const XArr a[3] = {{event, swb_layout::SEG_LOG_EV, 4, 1, 1}, {rr, swb_layout::SEG_LOG_RR, 4, 1, 1}, {time, swb_layout::SEG_LOG_TS, 8, 1, 1}};
    return batch_export(c, what, start, cnt, cap, off, total, a, 3, device, stream);
}

int export_new_rounds(sw_batch* c, const char* what, const uint8_t* which, int64_t cap, int64_t* off, int32_t* rounds, int64_t* total,
                      bool device, void* stream) {
    if (!c) return SW_EINVAL;
    if (!off) return bfail(c, SW_EINVAL, "%s: off is NULL", what);
    std::vector<int64_t> start((size_t)c->B, 0), cnt((size_t)c->B, 0);
    for (int64_t b = 0; b < c->B; ++b)   // (a frozen hashgraph: the step that froze it has no new_c to return)
        if ((!which || which[b]) && !c->frozen[b]) cnt[b] = c->sum_h.p[b * swb_layout::SUMMARY_WORDS + swb::S_NNEW];
    const XArr a[1] = {{rounds, swb_layout::SEG_NEW_ROUNDS, 4, 1, 1}};
    return batch_export(c, what, start, cnt, cap, off, total, a, 1, device, stream);
}

int export_events(sw_batch* c, const char* what, const int64_t* first, const int64_t* count, int64_t cap, int64_t* off, int32_t* creator,
                  int32_t* height, int32_t* round, int8_t* famous, int64_t* total, bool device, void* stream) {
    if (!c) return SW_EINVAL;
    if (!off) return bfail(c, SW_EINVAL, "%s: off is NULL", what);
    std::vector<int64_t> start, cnt;
    CHK(export_ranges(c, what, first, count, [&](int64_t b) { return c->events[b]; }, start, cnt));
    const XArr a[4] = {{creator, swb_layout::SEG_CR, 4, 1, 1}, {height, swb_layout::SEG_HT, 4, 1, 1}, {round, swb_layout::SEG_ROUND, 4, 1, 1},
                       {famous, swb_layout::SEG_FAM_EV, 1, 1, 1}};
    return batch_export(c, what, start, cnt, cap, off, total, a, 4, device, stream);
}

int export_rounds(sw_batch* c, const char* what, const int32_t* r0, const int32_t* r1, int64_t cap, int64_t* off, int32_t* witnesses,
                  int8_t* famous, uint8_t* consensus, int64_t* total, bool device, void* stream) {
    if (!c) return SW_EINVAL;
    if (!off) return bfail(c, SW_EINVAL, "%s: off is NULL", what);
    std::vector<int64_t> start((size_t)c->B), cnt((size_t)c->B);
    for (int64_t b = 0; b < c->B; ++b) {
        const int64_t R = c->sum_h.p[b * swb_layout::SUMMARY_WORDS + swb::S_ROUNDS], a = r0 ? r0[b] : 0, z = r1 ? r1[b] : R;
        if (a < 0 || z < a || z > R)
            return bfail(c, SW_ERANGE, "%s: rounds [%lld, %lld) outside the %lld rounds of hashgraph %lld (nothing written)", what, (long long)a,
                         (long long)z, (long long)R, (long long)b);
        start[b] = a;
        cnt[b] = z - a;
    }
    const XArr a[3] = {{witnesses, swb_layout::SEG_WIT, 4, c->n, c->npad}, {famous, swb_layout::SEG_FAM_SLOT, 1, c->n, c->npad},
                       {consensus, swb_layout::SEG_CONS, 1, 1, 1}};
    return batch_export(c, what, start, cnt, cap, off, total, a, 3, device, stream);
}

}  // namespace

extern "C" {

int sw_export_batch_ordered(sw_batch* c, const int64_t* first, const int64_t* count, int64_t cap, int64_t* off, int32_t* event,
                            int32_t* round_received, double* time, int64_t* total) {
    return export_ordered(c, "sw_export_batch_ordered", first, count, cap, off, event, round_received, time, total, false, nullptr);
}
int sw_export_batch_ordered_device(sw_batch* c, const int64_t* first, const int64_t* count, int64_t cap, int64_t* off, int32_t* d_event,
                                   int32_t* d_round_received, double* d_time, int64_t* total, void* user_stream) {
    return export_ordered(c, "sw_export_batch_ordered_device", first, count, cap, off, d_event, d_round_received, d_time, total, true, user_stream);
}

int sw_export_batch_new_rounds(sw_batch* c, const uint8_t* which, int64_t cap, int64_t* off, int32_t* rounds, int64_t* total) {
    return export_new_rounds(c, "sw_export_batch_new_rounds", which, cap, off, rounds, total, false, nullptr);
}
int sw_export_batch_new_rounds_device(sw_batch* c, const uint8_t* which, int64_t cap, int64_t* off, int32_t* d_rounds, int64_t* total,
                                      void* user_stream) {
    return export_new_rounds(c, "sw_export_batch_new_rounds_device", which, cap, off, d_rounds, total, true, user_stream);
}

int sw_export_batch_events(sw_batch* c, const int64_t* first, const int64_t* count, int64_t cap, int64_t* off, int32_t* creator, int32_t* height,
                           int32_t* round, int8_t* famous, int64_t* total) {
    return export_events(c, "sw_export_batch_events", first, count, cap, off, creator, height, round, famous, total, false, nullptr);
}
int sw_export_batch_events_device(sw_batch* c, const int64_t* first, const int64_t* count, int64_t cap, int64_t* off, int32_t* d_creator,
                                  int32_t* d_height, int32_t* d_round, int8_t* d_famous, int64_t* total, void* user_stream) {
    return export_events(c, "sw_export_batch_events_device", first, count, cap, off, d_creator, d_height, d_round, d_famous, total, true, user_stream);
}

int sw_export_batch_rounds(sw_batch* c, const int32_t* r0, const int32_t* r1, int64_t cap, int64_t* off, int32_t* witnesses, int8_t* famous,
                           uint8_t* consensus, int64_t* total) {
    return export_rounds(c, "sw_export_batch_rounds", r0, r1, cap, off, witnesses, famous, consensus, total, false, nullptr);
}
int sw_export_batch_rounds_device(sw_batch* c, const int32_t* r0, const int32_t* r1, int64_t cap, int64_t* off, int32_t* d_witnesses,
                                  int8_t* d_famous, uint8_t* d_consensus, int64_t* total, void* user_stream) {
    return export_rounds(c, "sw_export_batch_rounds_device", r0, r1, cap, off, d_witnesses, d_famous, d_consensus, total, true, user_stream);
}

int sw_export_batch_stats(sw_batch* c, int64_t out[4]) {
    if (!c || !out) return SW_EINVAL;
    out[0] = c->xp_calls; out[1] = c->xp_launches; out[2] = c->xp_entries; out[3] = c->xp_d2h;
    return SW_OK;
}

}  // extern "C"
