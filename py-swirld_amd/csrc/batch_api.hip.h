// Host side of the batch entry points (include/swirld_hip.h: sw_batch_*), included at the end of swirld_hip.hip.
// A batch is one device allocation (batch_layout.h), one stream, one staging buffer and the host mirrors the append
// checks need (creator and height per event); it shares nothing with a sw_ctx.
#pragma once

struct sw_batch {
    int64_t B = 0, cap_events = 0, cap_rounds = 0;
    int n = 0, npad = 0, coin_period = 0, device = 0;
    swb_layout::Layout lay;
    std::string err;
    owned::Stream stream;
    owned::DBuf<unsigned char> mem;      // the head and the slabs
    owned::DBuf<unsigned char> staging;  // what an append or a step uploads
    owned::Pinned<unsigned char> up_h;   // a step's lists, packed
    owned::Pinned<long long> sum_h;      // [B][SUMMARY_WORDS]: the last read-back
    std::vector<int64_t> events, divided;
    std::vector<std::vector<int32_t>> cr, ht;
    std::vector<int32_t> hmax;
    std::vector<char> frozen;
    // whole-batch exports (batch_export_api.hip.h): a plan is (B + 1) offsets and B source addresses per array
    static constexpr int XP_SLOTS = 4;
    owned::Pinned<unsigned char> xp_h[XP_SLOTS];   // a ring of plans, written by the host ...
    owned::Event xp_up[XP_SLOTS];                  // ... each with the event recorded behind its upload
    bool xp_busy[XP_SLOTS] = {};
    int xp_next = 0;
    owned::DBuf<unsigned char> xp_d;               // the plan the kernel reads (rewritten in stream order)
    owned::Event ev_user;                          // between the caller's stream and ours
    int64_t xp_calls = 0, xp_launches = 0, xp_entries = 0, xp_d2h = 0;   // sw_export_batch_stats
    // generated histories (batch_synth_api.hip.h): the generator state of every hashgraph, made by the first begin
    owned::DBuf<unsigned char> sy_state;
    swbs::StateLayout sy_lay{};
    std::vector<char> sy_has, sy_cur, sy_behind, sy_fed;   // per hashgraph: has parameters; the current copy of its state;
                                                          // cr / ht mirrors behind the slab; a host append since begin
    int64_t sy_calls = 0, sy_events = 0, sy_launches = 0, sy_refreshes = 0;   // sw_synth_batch_stats
    // gossip networks (batch_network_api.hip.h): the network state, made by the first begin, and the host's copy of its words
    std::vector<uint32_t> stake_rows;              // [B][npad] as uploaded at create: views of one network share a stake row
    owned::DBuf<unsigned char> nw_state;
    swbn::Layout nw_lay{};
    owned::Pinned<unsigned char> nw_h;             // the last read-back: [Net x G] [View x B]
    std::vector<char> nw_begun, nw_stopped;        // per network
    std::vector<char> nw_view;                     // per hashgraph: a view of a begun network
    int64_t nw_calls = 0, nw_turns = 0, nw_imported = 0, nw_launches = 0;   // sw_network_batch_stats
    const swb::Rec* recs() const { return (const swb::Rec*)(mem.p + lay.recs); }
    unsigned char* seg(int64_t b, int s) const { return mem.p + lay.at((uint64_t)b, s); }
};

namespace {

std::string g_batch_create_error;

int batch_synth_refresh(sw_batch* c, const int64_t* off);   // batch_synth_api.hip.h

int bfail(sw_batch* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_batch_create_error = buf;
    return code;
}

#define BHIPCHK(c, expr)                                                                                          \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess) return bfail(c, SW_EIO, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

int batch_shape_check(sw_batch* c, int64_t B, int n_members, int64_t cap_events, int64_t cap_rounds) {
    if (B < 1 || B > (1ll << 24)) return bfail(c, SW_EINVAL, "a batch holds 1 to 2^24 hashgraphs (B = %lld)", (long long)B);
    if (n_members < 1 || n_members > SW_MAX_MEMBERS) return bfail(c, SW_EINVAL, "n_members must be in [1, %d]", SW_MAX_MEMBERS);
    if (cap_events < 1 || cap_events > (1ll << 30)) return bfail(c, SW_EINVAL, "cap_events must be in [1, 2^30]");
    if (cap_rounds < 0 || cap_rounds > (1ll << 30)) return bfail(c, SW_EINVAL, "cap_rounds must be in [0, 2^30] (0: cap_events + 3)");
    if (!swb_layout::fits((uint64_t)B, (uint64_t)n_members, (uint64_t)swb_layout::npad_of(n_members), (uint64_t)cap_events, (uint64_t)cap_rounds))
        return bfail(c, SW_EINVAL, "a batch of %lld hashgraphs of %d members, %lld events and %lld rounds each needs 2^62 bytes or more",
                     (long long)B, n_members, (long long)cap_events, (long long)cap_rounds);
    return SW_OK;
}

int batch_staging(sw_batch* c, size_t bytes) {
    if (bytes <= c->staging.cap) return SW_OK;
    const size_t want = std::max(bytes, 2 * c->staging.cap);
    BHIPCHK(c, hipStreamSynchronize(c->stream));
    c->staging.reset();
    unsigned char* q = nullptr;
    if (hipMalloc((void**)&q, want) != hipSuccess) { (void)hipGetLastError(); return bfail(c, SW_ENOMEM, "hipMalloc(%zu bytes) for the batch's staging buffer failed", want); }
    c->staging.adopt(q, want);
    return SW_OK;
}

int batch_index(sw_batch* c, int64_t b, const char* what) {
    if (b < 0 || b >= c->B) return bfail(c, SW_ERANGE, "%s: hashgraph %lld outside the batch of %lld", what, (long long)b, (long long)c->B);
    return SW_OK;
}

int batch_event_range(sw_batch* c, int64_t b, int64_t first, int64_t K, int64_t limit, const char* what) {
    if (first < 0 || K < 0 || first + K > limit)
        return bfail(c, SW_ERANGE, "%s: [%lld, %lld) outside the %lld entries of hashgraph %lld", what, (long long)first, (long long)(first + K), (long long)limit, (long long)b);
    return SW_OK;
}

int batch_round_range(sw_batch* c, int64_t b, int r0, int r1, const char* what) {
    const int64_t R = c->sum_h.p[b * swb_layout::SUMMARY_WORDS + swb::S_ROUNDS];
    if (r0 < 0 || r1 < r0 || r1 > R)
        return bfail(c, SW_ERANGE, "%s: rounds [%d, %d) outside the %lld rounds of hashgraph %lld", what, r0, r1, (long long)R, (long long)b);
    return SW_OK;
}

// a slice of a slab to the caller (a plain copy; rows of npad columns give their first n)
int batch_copy(sw_batch* c, void* out, const void* src, size_t bytes) {
    if (!bytes) return SW_OK;
    BHIPCHK(c, hipSetDevice(c->device));
    BHIPCHK(c, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, c->stream));
    BHIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

int batch_copy_rows(sw_batch* c, void* out, const void* src, size_t elem, size_t rows) {
    if (!rows) return SW_OK;
    BHIPCHK(c, hipSetDevice(c->device));
    BHIPCHK(c, hipMemcpy2DAsync(out, (size_t)c->n * elem, src, (size_t)c->npad * elem, (size_t)c->n * elem, rows, hipMemcpyDeviceToHost, c->stream));
    BHIPCHK(c, hipStreamSynchronize(c->stream));
    return SW_OK;
}

}  // namespace

extern "C" {

int64_t sw_batch_bytes(int64_t B, int n_members, int64_t cap_events, int64_t cap_rounds) {
    if (batch_shape_check(nullptr, B, n_members, cap_events, cap_rounds) != SW_OK) return -1;
    return (int64_t)swb_layout::batch_bytes((uint64_t)B, (uint64_t)n_members, (uint64_t)cap_events, (uint64_t)cap_rounds);
}

const char* sw_batch_last_error(const sw_batch* b) { return b ? b->err.c_str() : g_batch_create_error.c_str(); }

int sw_batch_destroy(sw_batch* b) {
    if (!b) return SW_EINVAL;
    (void)hipSetDevice(b->device);
    if (b->stream.get()) (void)hipStreamSynchronize(b->stream);
    delete b;   // every member gives back what it holds (owned.h)
    return SW_OK;
}

int sw_batch_create(int64_t B, int n_members, const uint64_t* stake, int coin_period, int64_t cap_events, int64_t cap_rounds, int device,
                    sw_batch** out) {
    if (!out) return bfail(nullptr, SW_EINVAL, "out is NULL");
    *out = nullptr;
    CHK(batch_shape_check(nullptr, B, n_members, cap_events, cap_rounds));
    if (coin_period < 1) return bfail(nullptr, SW_EINVAL, "coin_period must be >= 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return bfail(nullptr, SW_ENODEV, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return bfail(nullptr, SW_ENODEV, "device %d out of range (%d devices)", device, ndev);
    const int n = n_members, np = swb_layout::npad_of(n);
    std::vector<uint64_t> tot((size_t)B, (uint64_t)n);
    std::vector<uint32_t> stake_h((size_t)B * np, 0);
    for (int64_t b = 0; b < B; ++b) {
        uint64_t t = 0;
        for (int i = 0; i < n; ++i) {
            const uint64_t v = stake ? stake[b * n + i] : 1;
            if (v > (1ull << 30)) return bfail(nullptr, SW_EOVERFLOW, "hashgraph %lld: stake[%d] too large for the 32-bit tally", (long long)b, i);
            t += v;
            stake_h[(size_t)b * np + i] = (uint32_t)v;
        }
        if (t >= (1ull << 30)) return bfail(nullptr, SW_EOVERFLOW, "hashgraph %lld: total stake %llu >= 2^30", (long long)b, (unsigned long long)t);
        tot[b] = t;
    }
    if (hipSetDevice(device) != hipSuccess) return bfail(nullptr, SW_EIO, "hipSetDevice(%d) failed", device);
    sw_batch* c = new sw_batch();
    auto bail = [&](int rc) { g_batch_create_error = c->err; delete c; return rc; };
    c->B = B; c->n = n; c->npad = np; c->coin_period = coin_period; c->device = device;
    c->lay = swb_layout::make((uint64_t)B, (uint64_t)n, (uint64_t)np, (uint64_t)cap_events, (uint64_t)cap_rounds);
    c->cap_events = cap_events; c->cap_rounds = (int64_t)c->lay.cap_rounds;
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return bail(bfail(c, SW_EIO, "hipStreamCreate failed"));
    c->stream.reset(st);
    unsigned char* q = nullptr;
    if (hipMalloc((void**)&q, c->lay.total) != hipSuccess) {
        (void)hipGetLastError();
        return bail(bfail(c, SW_ENOMEM, "hipMalloc(%llu bytes) failed: a batch of %lld hashgraphs, %d members, %lld events and %lld rounds each",
                          (unsigned long long)c->lay.total, (long long)B, n, (long long)cap_events, (long long)c->cap_rounds));
    }
    c->mem.adopt(q, c->lay.total);
    if (!c->sum_h.reserve((size_t)B * swb_layout::SUMMARY_WORDS)) return bail(bfail(c, SW_ENOMEM, "pinned host memory for the batch's summaries"));
    memset(c->sum_h.p, 0, (size_t)B * swb_layout::SUMMARY_WORDS * sizeof(long long));
    // the records, and the stake rows the init kernel copies into the slabs
    std::vector<unsigned char> recs_h((size_t)B * swb_layout::REC_BYTES, 0);
    for (int64_t b = 0; b < B; ++b) {
        const swb::Rec r = swb::bind(c->mem.p, c->lay, (uint64_t)b, coin_period, tot[b]);
        memcpy(recs_h.data() + (size_t)b * swb_layout::REC_BYTES, &r, sizeof r);
    }
    static_assert(sizeof(swb::Rec) % 8 == 0 && swb_layout::REC_BYTES % alignof(swb::Rec) == 0, "records are read in place");
    auto hipbail = [&](hipError_t e, const char* what) { return bail(bfail(c, SW_EIO, "%s failed: %s", what, hipGetErrorString(e))); };
    hipError_t e = hipMemcpyAsync(c->mem.p + c->lay.recs, recs_h.data(), recs_h.size(), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return hipbail(e, "hipMemcpyAsync(records)");
    int rc = batch_staging(c, stake_h.size() * sizeof(uint32_t));
    if (rc != SW_OK) return bail(rc);
    e = hipMemcpyAsync(c->staging.p, stake_h.data(), stake_h.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return hipbail(e, "hipMemcpyAsync(stake)");
    hipLaunchKernelGGL(k_batch_init, dim3((unsigned)B), dim3(64), 0, c->stream, c->recs(), (const uint32_t*)c->staging.p);
    e = hipGetLastError();
    if (e != hipSuccess) return hipbail(e, "k_batch_init");
    e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hipbail(e, "hipStreamSynchronize");
    c->events.assign((size_t)B, 0); c->divided.assign((size_t)B, 0);
    c->cr.resize((size_t)B); c->ht.resize((size_t)B);
    c->hmax.assign((size_t)B, 0); c->frozen.assign((size_t)B, 0);
    c->sy_has.assign((size_t)B, 0); c->sy_cur.assign((size_t)B, 0); c->sy_behind.assign((size_t)B, 0); c->sy_fed.assign((size_t)B, 0);
    c->stake_rows.swap(stake_h);
    c->nw_view.assign((size_t)B, 0);
    *out = c;
    return SW_OK;
}

// Node.add_event (swirld.py:114-120) for every hashgraph of the batch at once, with the checks of a single context on
// the exact path (append_exact).  Atomic over the whole batch: nothing is stored before everything is accepted.
int sw_batch_append(sw_batch* c, const int64_t* off, const int32_t* creator, const int32_t* self_parent, const int32_t* other_parent,
                    const double* t, const uint8_t* sig64) {
    if (!c) return SW_EINVAL;
    if (!off) return bfail(c, SW_EINVAL, "off is NULL");
    const int64_t B = c->B;
    if (off[0] != 0) return bfail(c, SW_EINVAL, "off[0] must be 0");
    for (int64_t b = 0; b < B; ++b)
        if (off[b + 1] < off[b]) return bfail(c, SW_EINVAL, "off must not decrease (hashgraph %lld)", (long long)b);
    const int64_t total = off[B];
    if (total == 0) return SW_OK;
    if (!creator || !self_parent || !other_parent) return bfail(c, SW_EINVAL, "creator / self_parent / other_parent is NULL");
    const int n = c->n;
    for (int64_t b = 0; b < B; ++b)
        if (off[b + 1] > off[b] && c->nw_view[b])
            return bfail(c, SW_EINVAL, "hashgraph %lld is a view of a gossip network: its events come from the network's turns", (long long)b);
    CHK(batch_synth_refresh(c, off));   // generated events are in the slab only: the mirrors of the hashgraphs this call feeds
    std::vector<int32_t> hnew((size_t)total);
    std::vector<int32_t> hmax_new(c->hmax);
    for (int64_t b = 0; b < B; ++b) {
        const int64_t K = off[b + 1] - off[b], N0 = c->events[b];
        if (!K) continue;
        if (N0 + K > c->cap_events)
            return bfail(c, SW_ERANGE, "hashgraph %lld: %lld events stored + %lld appended exceed cap_events = %lld", (long long)b, (long long)N0, (long long)K, (long long)c->cap_events);
        const int32_t *cr = creator + off[b], *sp = self_parent + off[b], *op = other_parent + off[b];
        const std::vector<int32_t>&cr0 = c->cr[b], &ht0 = c->ht[b];
        int32_t* h = hnew.data() + off[b];
        int hmax = c->hmax[b];
        for (int64_t i = 0; i < K; ++i) {
            const int64_t e = N0 + i;
            const int32_t m = cr[i], s = sp[i], o = op[i];
            if (m < 0 || m >= n) return bfail(c, SW_EINVAL, "hashgraph %lld, event %lld: creator %d out of range", (long long)b, (long long)e, m);
            if ((s < 0) != (o < 0)) return bfail(c, SW_EINVAL, "hashgraph %lld, event %lld: must have 0 or 2 parents", (long long)b, (long long)e);
            if (s >= e || o >= e) return bfail(c, SW_EINVAL, "hashgraph %lld, event %lld: parent index not earlier (not a topological order)", (long long)b, (long long)e);
            if (s < 0) { h[i] = 0; continue; }
            if ((s < N0 ? cr0[s] : cr[s - N0]) != m) return bfail(c, SW_EINVAL, "hashgraph %lld, event %lld: self-parent is by another member", (long long)b, (long long)e);
            if ((o < N0 ? cr0[o] : cr[o - N0]) == m) return bfail(c, SW_EINVAL, "hashgraph %lld, event %lld: other-parent is by the same member", (long long)b, (long long)e);
            const int32_t hs = s < N0 ? ht0[s] : h[s - N0], ho = o < N0 ? ht0[o] : h[o - N0];   // swirld.py:117-120
            h[i] = std::max(hs, ho) + 1;
            hmax = std::max(hmax, h[i]);
        }
        if ((int64_t)hmax + 3 > c->cap_rounds)
            return bfail(c, SW_ERANGE, "hashgraph %lld: height %d needs %d rounds of capacity, cap_rounds = %lld", (long long)b, hmax, hmax + 3, (long long)c->cap_rounds);
        hmax_new[b] = hmax;
    }
    BHIPCHK(c, hipSetDevice(c->device));
    // one upload per array, one kernel for the whole batch
    auto up64 = [](size_t v) { return (v + 63) & ~(size_t)63; };
    const size_t T = (size_t)total;
    const size_t o_off = 0, o_base = o_off + up64((size_t)(B + 1) * 8), o_cr = o_base + up64((size_t)B * 8), o_sp = o_cr + up64(T * 4),
                 o_op = o_sp + up64(T * 4), o_ht = o_op + up64(T * 4), o_t = o_ht + up64(T * 4), o_sig = o_t + up64(T * 8), o_end = o_sig + T * 64;
    CHK(batch_staging(c, o_end));
    unsigned char* d = c->staging.p;
    BHIPCHK(c, hipMemcpyAsync(d + o_off, off, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, c->stream));
    BHIPCHK(c, hipMemcpyAsync(d + o_base, c->events.data(), (size_t)B * 8, hipMemcpyHostToDevice, c->stream));
    BHIPCHK(c, hipMemcpyAsync(d + o_cr, creator, T * 4, hipMemcpyHostToDevice, c->stream));
    BHIPCHK(c, hipMemcpyAsync(d + o_sp, self_parent, T * 4, hipMemcpyHostToDevice, c->stream));
    BHIPCHK(c, hipMemcpyAsync(d + o_op, other_parent, T * 4, hipMemcpyHostToDevice, c->stream));
    BHIPCHK(c, hipMemcpyAsync(d + o_ht, hnew.data(), T * 4, hipMemcpyHostToDevice, c->stream));
    if (t) BHIPCHK(c, hipMemcpyAsync(d + o_t, t, T * 8, hipMemcpyHostToDevice, c->stream));
    if (sig64) BHIPCHK(c, hipMemcpyAsync(d + o_sig, sig64, T * 64, hipMemcpyHostToDevice, c->stream));
    const long long threads = 4 * total;
    hipLaunchKernelGGL(k_batch_scatter, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, c->stream, c->recs(), (long long)B,
                       (const long long*)(d + o_off), (const long long*)(d + o_base), (const int*)(d + o_cr), (const int*)(d + o_sp),
                       (const int*)(d + o_op), (const int*)(d + o_ht), t ? (const double*)(d + o_t) : nullptr,
                       sig64 ? (const uint4*)(d + o_sig) : nullptr);
    BHIPCHK(c, hipGetLastError());
    BHIPCHK(c, hipStreamSynchronize(c->stream));
    for (int64_t b = 0; b < B; ++b) {
        const int64_t K = off[b + 1] - off[b];
        if (!K) continue;
        c->cr[b].insert(c->cr[b].end(), creator + off[b], creator + off[b + 1]);
        c->ht[b].insert(c->ht[b].end(), hnew.begin() + off[b], hnew.begin() + off[b + 1]);
        c->events[b] += K;
        c->sy_fed[b] = 1;
    }
    c->hmax.swap(hmax_new);
    return SW_OK;
}

// One step of the main loop (swirld.py:325-328) for every hashgraph that takes part: one launch, one read-back.
int sw_batch_step(sw_batch* c, const int64_t* K, int64_t* n_failed) {
    if (!c) return SW_EINVAL;
    if (n_failed) *n_failed = 0;
    const int64_t B = c->B;
    int64_t m = 0, most = 0;
    for (int64_t b = 0; b < B; ++b) {
        const int64_t left = c->events[b] - c->divided[b];
        if (K && K[b] < 0) return bfail(c, SW_EINVAL, "K[%lld] = %lld is negative", (long long)b, (long long)K[b]);
        if (K && K[b] > left && !c->frozen[b])
            return bfail(c, SW_ERANGE, "K[%lld] = %lld, but hashgraph %lld has %lld undivided events", (long long)b, (long long)K[b], (long long)b, (long long)left);
        const int64_t k = c->frozen[b] ? 0 : (K ? K[b] : left);
        if (k) { ++m; most = std::max(most, k); }
    }
    if (!m) return SW_OK;
    BHIPCHK(c, hipSetDevice(c->device));
    // launch j of nl: a hashgraph of q chunks takes part in the last q launches; the last launch goes on to fame and order
    const int64_t CH = swb::MAX_DIVIDE_PER_LAUNCH;
    const int64_t nl = (most + CH - 1) / CH;
    struct Launch { size_t who, first, K; int64_t m; };
    std::vector<Launch> launches((size_t)nl);
    size_t bytes = 0;
    for (int64_t j = 0; j < nl; ++j) {
        int64_t mj = 0;
        for (int64_t b = 0; b < B; ++b) {
            const int64_t k = c->frozen[b] ? 0 : (K ? K[b] : c->events[b] - c->divided[b]);
            if (k && (k + CH - 1) / CH >= nl - j) ++mj;
        }
        Launch& l = launches[(size_t)j];
        l.m = mj;
        l.first = bytes; bytes += (size_t)mj * 8;
        l.K = bytes; bytes += (size_t)mj * 8;
        l.who = bytes; bytes += ((size_t)mj * 4 + 7) & ~(size_t)7;
    }
    if (bytes > c->up_h.cap) {
        BHIPCHK(c, hipStreamSynchronize(c->stream));
        if (!c->up_h.reserve(std::max(bytes, 2 * c->up_h.cap))) return bfail(c, SW_ENOMEM, "pinned host memory for a step's lists (%zu bytes)", bytes);
    }
    CHK(batch_staging(c, bytes));
    for (int64_t j = 0; j < nl; ++j) {
        const Launch& l = launches[(size_t)j];
        long long* first = (long long*)(c->up_h.p + l.first);
        long long* kk = (long long*)(c->up_h.p + l.K);
        int* who = (int*)(c->up_h.p + l.who);
        int64_t at = 0;
        for (int64_t b = 0; b < B; ++b) {
            const int64_t k = c->frozen[b] ? 0 : (K ? K[b] : c->events[b] - c->divided[b]);
            if (!k) continue;
            const int64_t q = (k + CH - 1) / CH, chunk = j - (nl - q);
            if (chunk < 0) continue;
            who[at] = (int)b;
            first[at] = c->divided[b] + chunk * CH;
            kk[at] = std::min(CH, k - chunk * CH);
            ++at;
        }
    }
    BHIPCHK(c, hipMemcpyAsync(c->staging.p, c->up_h.p, bytes, hipMemcpyHostToDevice, c->stream));
    for (int64_t j = 0; j < nl; ++j) {
        const Launch& l = launches[(size_t)j];
        if (!l.m) continue;
        // (every launch clears the per-step words: they are written behind the last launch's order phase only)
        const int phases = swb::PH_HEAD | (j == nl - 1 ? swb::PH_TAIL : 0);
        hipLaunchKernelGGL(k_batch_step, dim3((unsigned)l.m), dim3(64), 0, c->stream, c->recs(), (const int*)(c->staging.p + l.who),
                           (const long long*)(c->staging.p + l.first), (const long long*)(c->staging.p + l.K), phases);
    }
    BHIPCHK(c, hipGetLastError());
    BHIPCHK(c, hipMemcpyAsync(c->sum_h.p, c->mem.p + c->lay.summaries, (size_t)B * swb_layout::SUMMARY_WORDS * sizeof(long long),
                              hipMemcpyDeviceToHost, c->stream));
    BHIPCHK(c, hipStreamSynchronize(c->stream));
    int64_t failed = 0;
    for (int64_t b = 0; b < B; ++b) {
        const long long* s = c->sum_h.p + b * swb_layout::SUMMARY_WORDS;
        c->divided[b] = s[swb::S_DIVIDED];
        if (s[swb::S_STAGE] != swb::STAGE_NONE && !c->frozen[b]) { c->frozen[b] = 1; ++failed; }
    }
    if (n_failed) *n_failed = failed;
    return SW_OK;
}

int sw_batch_shape(sw_batch* c, int64_t* B, int* n_members, int* npad, int64_t* cap_events, int64_t* cap_rounds, int64_t* bytes) {
    if (!c) return SW_EINVAL;
    if (B) *B = c->B;
    if (n_members) *n_members = c->n;
    if (npad) *npad = c->npad;
    if (cap_events) *cap_events = c->cap_events;
    if (cap_rounds) *cap_rounds = c->cap_rounds;
    if (bytes) *bytes = (int64_t)c->lay.total;
    return SW_OK;
}

int sw_batch_get_summary(sw_batch* c, int64_t* out) {
    if (!c || !out) return SW_EINVAL;
    for (int64_t b = 0; b < c->B; ++b) {
        const long long* s = c->sum_h.p + b * swb_layout::SUMMARY_WORDS;
        int64_t* o = out + b * SW_BATCH_SUMMARY_WORDS;
        o[0] = c->events[b]; o[1] = s[swb::S_DIVIDED]; o[2] = s[swb::S_ROUNDS]; o[3] = s[swb::S_ORDERED];
        o[4] = s[swb::S_NNEW]; o[5] = s[swb::S_NOUT]; o[6] = s[swb::S_STAGE]; o[7] = s[swb::S_CODE]; o[8] = s[swb::S_EVENT];
    }
    return SW_OK;
}

int sw_batch_get_height(sw_batch* c, int64_t b, int64_t first, int64_t K, int32_t* out) {
    if (!c || !out) return SW_EINVAL;
    CHK(batch_index(c, b, "sw_batch_get_height"));
    CHK(batch_event_range(c, b, first, K, c->events[b], "sw_batch_get_height"));
    return batch_copy(c, out, (const int32_t*)c->seg(b, swb_layout::SEG_HT) + first, (size_t)K * 4);
}

int sw_batch_get_round(sw_batch* c, int64_t b, int64_t first, int64_t K, int32_t* out) {
    if (!c || !out) return SW_EINVAL;
    CHK(batch_index(c, b, "sw_batch_get_round"));
    CHK(batch_event_range(c, b, first, K, c->events[b], "sw_batch_get_round"));
    return batch_copy(c, out, (const int32_t*)c->seg(b, swb_layout::SEG_ROUND) + first, (size_t)K * 4);
}

int sw_batch_get_can_see(sw_batch* c, int64_t b, int64_t first, int64_t K, int32_t* out) {
    if (!c || !out) return SW_EINVAL;
    CHK(batch_index(c, b, "sw_batch_get_can_see"));
    CHK(batch_event_range(c, b, first, K, c->divided[b], "sw_batch_get_can_see"));
    return batch_copy_rows(c, out, (const int32_t*)c->seg(b, swb_layout::SEG_L) + (size_t)first * c->npad, 4, (size_t)K);
}

int sw_batch_get_witnesses(sw_batch* c, int64_t b, int r0, int r1, int32_t* out) {
    if (!c || !out) return SW_EINVAL;
    CHK(batch_index(c, b, "sw_batch_get_witnesses"));
    CHK(batch_round_range(c, b, r0, r1, "sw_batch_get_witnesses"));
    return batch_copy_rows(c, out, (const int32_t*)c->seg(b, swb_layout::SEG_WIT) + (size_t)r0 * c->npad, 4, (size_t)(r1 - r0));
}

int sw_batch_get_witness_order(sw_batch* c, int64_t b, int r, int32_t* members, int* n_out) {
    if (!c || !members || !n_out) return SW_EINVAL;
    CHK(batch_index(c, b, "sw_batch_get_witness_order"));
    CHK(batch_round_range(c, b, r, r + 1, "sw_batch_get_witness_order"));
    int32_t cnt = 0;
    CHK(batch_copy(c, &cnt, (const int32_t*)c->seg(b, swb_layout::SEG_WCNT) + r, 4));
    *n_out = cnt;
    return batch_copy(c, members, (const int32_t*)c->seg(b, swb_layout::SEG_WORDER) + (size_t)r * c->npad, (size_t)cnt * 4);
}

int sw_batch_get_famous(sw_batch* c, int64_t b, int r0, int r1, int8_t* out) {
    if (!c || !out) return SW_EINVAL;
    CHK(batch_index(c, b, "sw_batch_get_famous"));
    CHK(batch_round_range(c, b, r0, r1, "sw_batch_get_famous"));
    return batch_copy_rows(c, out, (const int8_t*)c->seg(b, swb_layout::SEG_FAM_SLOT) + (size_t)r0 * c->npad, 1, (size_t)(r1 - r0));
}

int sw_batch_get_famous_events(sw_batch* c, int64_t b, int64_t first, int64_t K, int8_t* out) {
    if (!c || !out) return SW_EINVAL;
    CHK(batch_index(c, b, "sw_batch_get_famous_events"));
    CHK(batch_event_range(c, b, first, K, c->events[b], "sw_batch_get_famous_events"));
    return batch_copy(c, out, (const int8_t*)c->seg(b, swb_layout::SEG_FAM_EV) + first, (size_t)K);
}

int sw_batch_get_consensus(sw_batch* c, int64_t b, int r0, int r1, uint8_t* out) {
    if (!c || !out) return SW_EINVAL;
    CHK(batch_index(c, b, "sw_batch_get_consensus"));
    CHK(batch_round_range(c, b, r0, r1, "sw_batch_get_consensus"));
    return batch_copy(c, out, (const uint8_t*)c->seg(b, swb_layout::SEG_CONS) + r0, (size_t)(r1 - r0));
}

int sw_batch_get_new_rounds(sw_batch* c, int64_t b, int32_t* out, int cap, int* n_out) {
    if (!c || !n_out) return SW_EINVAL;
    CHK(batch_index(c, b, "sw_batch_get_new_rounds"));
    const int cnt = (int)c->sum_h.p[b * swb_layout::SUMMARY_WORDS + swb::S_NNEW];
    *n_out = cnt;
    if (cnt > cap) return bfail(c, SW_ERANGE, "sw_batch_get_new_rounds: capacity %d < %d", cap, cnt);
    if (cnt && !out) return SW_EINVAL;
    return batch_copy(c, out, c->seg(b, swb_layout::SEG_NEW_ROUNDS), (size_t)cnt * 4);
}

int sw_batch_get_transactions(sw_batch* c, int64_t b, int64_t first, int64_t K, int32_t* events, int32_t* round_received, double* consensus_time) {
    if (!c) return SW_EINVAL;
    CHK(batch_index(c, b, "sw_batch_get_transactions"));
    CHK(batch_event_range(c, b, first, K, c->sum_h.p[b * swb_layout::SUMMARY_WORDS + swb::S_ORDERED], "sw_batch_get_transactions"));
    if (events) CHK(batch_copy(c, events, (const int32_t*)c->seg(b, swb_layout::SEG_LOG_EV) + first, (size_t)K * 4));
    if (round_received) CHK(batch_copy(c, round_received, (const int32_t*)c->seg(b, swb_layout::SEG_LOG_RR) + first, (size_t)K * 4));
    if (consensus_time) CHK(batch_copy(c, consensus_time, (const double*)c->seg(b, swb_layout::SEG_LOG_TS) + first, (size_t)K * 8));
    return SW_OK;
}

}  // extern "C"
