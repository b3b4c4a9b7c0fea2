// Stand-alone driver of csrc/owned.h (tests/test_owned_host.py builds it with AddressSanitizer and UBSan, WITHOUT the HIP
// runtime): the HIP calls the owning types make are defined here, backed by malloc / free and a table of live handles.  A
// double free, a free of a handle the table does not know (or knows as another kind), and a handle still live at the end
// make the program fail; so does any step after which the library's live-resource counts differ from the table's own.
//   owned_main dbuf | pinned | event | stream      the cases of one type; prints "ok <case>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../py-swirld_amd/csrc/owned.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

namespace {

enum Kind { DEVICE, PINNED, EVENT, STREAM, KINDS };
const char* const kind_name[KINDS] = {"device block", "pinned block", "event", "stream"};

struct Fake {
    std::map<void*, std::pair<Kind, size_t>> live;
    int64_t bytes[KINDS] = {0, 0, 0, 0}, handles[KINDS] = {0, 0, 0, 0};
    int64_t created[KINDS] = {0, 0, 0, 0};
    bool fail_next = false;          // the next allocation or creation fails
    hipError_t last = hipSuccess;
    int64_t pinned_at_last_alloc = -1;   // pinned blocks that were live when hipHostMalloc was last entered
} fake;

hipError_t make(Kind k, size_t size, void** out) {
    if (fake.fail_next) {
        fake.fail_next = false;
        fake.last = hipErrorOutOfMemory;
        return hipErrorOutOfMemory;
    }
    void* p = malloc(size ? size : 1);
    CHECK(p);
    fake.live[p] = {k, size};
    fake.bytes[k] += (int64_t)size;
    fake.handles[k]++;
    fake.created[k]++;
    *out = p;
    return hipSuccess;
}

hipError_t drop(Kind k, void* p) {
    auto it = fake.live.find(p);
    if (it == fake.live.end()) { fprintf(stderr, "free of an unknown or already freed %s %p\n", kind_name[k], p); exit(1); }
    if (it->second.first != k) { fprintf(stderr, "%p freed as a %s, made as a %s\n", p, kind_name[k], kind_name[it->second.first]); exit(1); }
    fake.bytes[k] -= (int64_t)it->second.second;
    fake.handles[k]--;
    fake.live.erase(it);
    free(p);
    return hipSuccess;
}

// the library's counts against the table's, after every step
void agree() {
    CHECK(owned::live.device_bytes.load() == fake.bytes[DEVICE]);
    CHECK(owned::live.pinned_bytes.load() == fake.bytes[PINNED]);
    CHECK(owned::live.events.load() == fake.handles[EVENT]);
    CHECK(owned::live.streams.load() == fake.handles[STREAM]);
}

template <class T>
T* device_block(size_t n) {
    T* q = nullptr;
    CHECK(hipMalloc((void**)&q, n * sizeof(T)) == hipSuccess);
    return q;
}

hipStream_t new_stream() {
    void* s = nullptr;
    CHECK(make(STREAM, 0, &s) == hipSuccess);
    return (hipStream_t)s;
}

void dbuf_cases() {
    using owned::DBuf;
    {   // the destructor frees
        DBuf<int> a;
        CHECK(!a.p && !a.cap);
        a.adopt(device_block<int>(10), 10);
        CHECK(a.p && a.cap == 10 && fake.bytes[DEVICE] == 40);
        agree();
    }
    CHECK(fake.handles[DEVICE] == 0);
    agree();
    {   // adopt over a live block frees the old one; reset frees and empties
        DBuf<double> a;
        a.adopt(device_block<double>(3), 3);
        a.adopt(device_block<double>(5), 5);
        CHECK(fake.handles[DEVICE] == 1 && fake.bytes[DEVICE] == 40);
        agree();
        a.reset();
        CHECK(!a.p && !a.cap && fake.handles[DEVICE] == 0);
        agree();
        a.reset();   // (of an empty buffer: nothing)
        agree();
    }
    {   // the moved-from object frees nothing; move-assignment over a live object frees the old block
        DBuf<int> a, b;
        a.adopt(device_block<int>(4), 4);
        int* const pa = a.p;
        DBuf<int> m(std::move(a));
        CHECK(!a.p && !a.cap && m.p == pa && m.cap == 4 && fake.handles[DEVICE] == 1);
        agree();
        b.adopt(device_block<int>(8), 8);
        CHECK(fake.handles[DEVICE] == 2);
        b = std::move(m);
        CHECK(!m.p && !m.cap && b.p == pa && b.cap == 4 && fake.handles[DEVICE] == 1 && fake.bytes[DEVICE] == 16);
        agree();
        DBuf<int>& self = b;
        b = std::move(self);   // (self-assignment keeps the block)
        CHECK(b.p == pa && fake.handles[DEVICE] == 1);
        agree();
    }
    CHECK(fake.handles[DEVICE] == 0);
    {   // release() leaves the block live and no longer counted by the object
        int* q = nullptr;
        {
            DBuf<int> a;
            a.adopt(device_block<int>(6), 6);
            q = a.release();
            CHECK(q && !a.p && !a.cap);
            CHECK(owned::live.device_bytes.load() == 0 && fake.handles[DEVICE] == 1);
        }
        CHECK(fake.handles[DEVICE] == 1);   // (the destructor had nothing to free)
        CHECK(hipFree(q) == hipSuccess);
        agree();
    }
    {   // an aliased range is neither counted nor freed: not by release(), not by reset(), not by the destructor, not by a move
        static int range[16];
        DBuf<int> a;
        a.adopt(device_block<int>(2), 2);
        a.alias(range, 16);   // (frees what it held)
        CHECK(a.p == range && a.cap == 16 && fake.handles[DEVICE] == 0);
        agree();
        CHECK(a.release() == range && !a.p && !a.cap);
        agree();
        a.alias(range, 16);
        a.reset();
        CHECK(!a.p);
        agree();
        a.alias(range, 16);
        DBuf<int> m(std::move(a));
        CHECK(m.p == range && m.aliased && !a.aliased);
        a.adopt(device_block<int>(1), 1);   // (the moved-from object owns again like a fresh one)
        agree();
    }
    CHECK(fake.handles[DEVICE] == 0);
}

void pinned_cases() {
    using owned::Pinned;
    {
        Pinned<int> a;
        CHECK(a.reserve(0) && !a.p && fake.created[PINNED] == 0);   // nothing asked for, nothing made
        CHECK(a.reserve(100) && a.p && a.cap == 100 && fake.bytes[PINNED] == 400);
        agree();
        int* const p0 = a.p;
        CHECK(a.reserve(100) && a.reserve(7) && a.p == p0 && a.cap == 100 && fake.created[PINNED] == 1);   // at or below cap: nothing happens
        agree();
        CHECK(a.reserve(101) && a.cap == 101 && fake.created[PINNED] == 2);
        CHECK(fake.pinned_at_last_alloc == 0);   // freed before it allocated
        CHECK(fake.handles[PINNED] == 1 && fake.bytes[PINNED] == 404);
        agree();
        fake.fail_next = true;   // a failed growth: empty, and the error cleared
        CHECK(!a.reserve(1000));
        CHECK(a.p == nullptr && a.cap == 0 && fake.handles[PINNED] == 0 && fake.last == hipSuccess);
        agree();
        CHECK(a.reserve(5) && a.cap == 5);   // ... and usable again
        agree();
    }
    CHECK(fake.handles[PINNED] == 0);   // the destructor frees
    agree();
    {
        Pinned<char> a, b;
        CHECK(a.reserve(64) && b.reserve(32));
        char* const pa = a.p;
        Pinned<char> m(std::move(a));
        CHECK(!a.p && !a.cap && m.p == pa && m.cap == 64 && fake.handles[PINNED] == 2);
        agree();
        b = std::move(m);   // frees b's old block
        CHECK(!m.p && !m.cap && b.p == pa && b.cap == 64 && fake.handles[PINNED] == 1 && fake.bytes[PINNED] == 64);
        agree();
        b.reset();
        CHECK(!b.p && !b.cap && fake.handles[PINNED] == 0);
        agree();
    }
}

void event_cases() {
    using owned::Event;
    {
        Event e;
        CHECK(e.get() == nullptr && fake.created[EVENT] == 0);
        fake.fail_next = true;
        CHECK(e.ensure(hipEventDisableTiming) == (int)hipErrorOutOfMemory && e.get() == nullptr);
        agree();
        CHECK(e.ensure(hipEventDisableTiming) == (int)hipSuccess && e.get() != nullptr);
        const hipEvent_t h = e.get();
        for (int i = 0; i < 5; ++i) CHECK(e.ensure(hipEventDisableTiming) == (int)hipSuccess && e.get() == h);
        CHECK(fake.created[EVENT] == 1 && (hipEvent_t)e == h);   // created once however often it is asked for
        agree();
    }
    CHECK(fake.handles[EVENT] == 0);
    agree();
    {
        Event a, b;
        CHECK(a.ensure(0) == 0 && b.ensure(0) == 0);
        const hipEvent_t ha = a.get();
        Event m(std::move(a));
        CHECK(a.get() == nullptr && m.get() == ha && fake.handles[EVENT] == 2);
        b = std::move(m);
        CHECK(m.get() == nullptr && b.get() == ha && fake.handles[EVENT] == 1);
        agree();
        CHECK(a.ensure(0) == 0 && a.get() != nullptr);   // a moved-from event can be made again
        agree();
    }
    CHECK(fake.handles[EVENT] == 0);
    {   // a growing vector of events (the pools of a context) moves them: every event is destroyed exactly once
        std::vector<Event> pool;
        for (int i = 0; i < 100; ++i) {
            pool.emplace_back();
            CHECK(pool.back().ensure(hipEventDisableTiming) == 0);
            agree();
        }
        CHECK(fake.handles[EVENT] == 100 && fake.created[EVENT] == 4 + 100);
        pool.resize(40);
        CHECK(fake.handles[EVENT] == 40);
        agree();
    }
    CHECK(fake.handles[EVENT] == 0);
}

void stream_cases() {
    using owned::Stream;
    {
        Stream s;
        CHECK(s.get() == nullptr && !s);
        const hipStream_t h = new_stream();
        CHECK(owned::live.streams.load() == 0);   // made outside: not counted yet
        s.reset(h);                                // adopted: counted
        CHECK(s.get() == h && (hipStream_t)s == h);
        agree();
        const hipStream_t h2 = new_stream();
        s.reset(h2);   // the swap of sw_create's CU-mask stream: the old one is destroyed
        CHECK(s.get() == h2 && fake.handles[STREAM] == 1);
        agree();
    }
    CHECK(fake.handles[STREAM] == 0);
    agree();
    {
        Stream a, b;
        a.reset(new_stream());
        b.reset(new_stream());
        const hipStream_t ha = a.get();
        Stream m(std::move(a));
        CHECK(a.get() == nullptr && m.get() == ha && fake.handles[STREAM] == 2);
        agree();
        b = std::move(m);
        CHECK(m.get() == nullptr && b.get() == ha && fake.handles[STREAM] == 1);
        agree();
        b.reset();
        CHECK(b.get() == nullptr && fake.handles[STREAM] == 0);
        agree();
    }
    {
        Stream arr[2];   // (stream_srt)
        for (Stream& s : arr) s.reset(new_stream());
        agree();
    }
    CHECK(fake.handles[STREAM] == 0);
}

}  // namespace

// ---- the HIP calls of owned.h --------------------------------------------------------------------------------------------------
extern "C" {
hipError_t hipMalloc(void** ptr, size_t size) { return make(DEVICE, size, ptr); }
hipError_t hipFree(void* ptr) { return drop(DEVICE, ptr); }
hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int) {
    fake.pinned_at_last_alloc = fake.handles[PINNED];
    return make(PINNED, size, ptr);
}
hipError_t hipHostFree(void* ptr) { return drop(PINNED, ptr); }
hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned) { return make(EVENT, 0, (void**)event); }
hipError_t hipEventDestroy(hipEvent_t event) { return drop(EVENT, (void*)event); }
hipError_t hipStreamDestroy(hipStream_t stream) { return drop(STREAM, (void*)stream); }
hipError_t hipGetLastError(void) { const hipError_t e = fake.last; fake.last = hipSuccess; return e; }
}

int main(int argc, char** argv) {
    const char* which = argc > 1 ? argv[1] : "";
    if (!strcmp(which, "dbuf")) dbuf_cases();
    else if (!strcmp(which, "pinned")) pinned_cases();
    else if (!strcmp(which, "event")) event_cases();
    else if (!strcmp(which, "stream")) stream_cases();
    else { fprintf(stderr, "usage: owned_main dbuf | pinned | event | stream\n"); return 2; }
    // at the end: nothing live, every count back at zero
    for (const auto& h : fake.live) fprintf(stderr, "still live at exit: %s %p\n", kind_name[h.second.first], h.first);
    CHECK(fake.live.empty());
    agree();
    CHECK(owned::live.device_bytes.load() == 0 && owned::live.pinned_bytes.load() == 0 && owned::live.events.load() == 0 && owned::live.streams.load() == 0);
    printf("ok %s\n", which);
    return 0;
}
