// Who owns what ("ownership"): every device buffer, pinned host buffer, event and stream that a context or a
// call holds is a member of one of the types below, and that member's destructor gives it back.  A new member gets an owning
// type; sw_destroy is not touched.  Every type is move-only (declaring the moves deletes the copies); a move empties its source.
// What swirld_hip.hip still acquires or gives back by hand:
//   - dgrow: the hipMalloc of a DBuf's new block (it needs fail() and the context's sync policy; the block is adopted at once);
//   - the grow of d_Sw in launch_voter_masks (it waits for stream_aux alone, not for the device);
//   - vm_flush_translations: a transient 4 MiB allocation, freed in the next line;
//   - stream creation in sw_create and plan_order_groups (priority, CU mask: the handle is adopted at once);
//   - sw_split_link / split_dissolve: the events of a SplitGroup, which several contexts share.
// The live-resource counts (sw_debug_live_resources) are kept here: up where a type acquires or adopts, down where it frees or
// releases.  The windowed can_see table is NOT counted: d_L only aliases its address range (DBuf::alias), and its physical
// chunks belong to vm_destroy.
// Host-only: <hip/hip_runtime_api.h> and the standard library, so a plain C++ compiler builds it (tests/owned_main.cpp).
#pragma once

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <cstdint>

namespace owned {

struct Live { std::atomic<int64_t> device_bytes{0}, pinned_bytes{0}, events{0}, streams{0}; };
inline Live live;   // process-wide
inline void count(std::atomic<int64_t>& a, int64_t d) { a.fetch_add(d, std::memory_order_relaxed); }

template <class T>
struct DBuf {   // a device buffer
    T* p = nullptr;
    size_t cap = 0;        // elements
    bool aliased = false;  // p points into memory that something else owns: never freed, never counted
    DBuf() = default;
    DBuf(DBuf&& o) noexcept { take(o); }
    DBuf& operator=(DBuf&& o) noexcept { if (this != &o) { reset(); take(o); } return *this; }
    ~DBuf() { reset(); }
    void adopt(T* q, size_t n) { reset(); p = q; cap = n; count(live.device_bytes, bytes()); }   // owns the hipMalloc'ed block q
    void alias(T* q, size_t n) { reset(); p = q; cap = n; aliased = true; }
    T* release() {   // forgets the block without freeing it: the caller's from now on
        T* q = p;
        if (p && !aliased) count(live.device_bytes, -bytes());
        p = nullptr; cap = 0; aliased = false;
        return q;
    }
    void reset() { if (p && !aliased) (void)hipFree(p); release(); }
private:
    int64_t bytes() const { return (int64_t)(cap * sizeof(T)); }
    void take(DBuf& o) { p = o.p; cap = o.cap; aliased = o.aliased; o.p = nullptr; o.cap = 0; o.aliased = false; }
};

template <class T>
struct Pinned {   // a pinned host buffer
    T* p = nullptr;
    size_t cap = 0;   // elements
    Pinned() = default;
    Pinned(Pinned&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Pinned& operator=(Pinned&& o) noexcept { if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~Pinned() { reset(); }
    // Room for n elements; the contents are NOT kept.  The caller has waited for whatever may still use the old block.
    // false: the allocation failed (the HIP error is cleared) and the buffer is empty.
    bool reserve(size_t n) {
        if (n <= cap) return true;
        reset();
        if (hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return false; }
        cap = n;
        count(live.pinned_bytes, (int64_t)(cap * sizeof(T)));
        return true;
    }
    void reset() {
        if (p) { (void)hipHostFree(p); count(live.pinned_bytes, -(int64_t)(cap * sizeof(T))); }
        p = nullptr; cap = 0;
    }
};

struct Event {
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); e = o.e; o.e = nullptr; } return *this; }
    ~Event() { reset(); }
    int ensure(unsigned flags) {   // creates the event on the first call; returns the hipError_t
        if (e) return hipSuccess;
        const hipError_t r = hipEventCreateWithFlags(&e, flags);
        if (r == hipSuccess) count(live.events, 1); else e = nullptr;
        return r;
    }
    hipEvent_t get() const { return e; }
    operator hipEvent_t() const { return e; }
    void reset() { if (e) { (void)hipEventDestroy(e); count(live.events, -1); } e = nullptr; }
private:
    hipEvent_t e = nullptr;
};

struct Stream {
    Stream() = default;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    Stream& operator=(Stream&& o) noexcept { if (this != &o) { reset(); s = o.s; o.s = nullptr; } return *this; }
    ~Stream() { reset(); }
    hipStream_t get() const { return s; }
    operator hipStream_t() const { return s; }
    void reset(hipStream_t created = nullptr) {   // destroys the stream it holds and adopts a created one (or none)
        if (s) { (void)hipStreamDestroy(s); count(live.streams, -1); }
        s = created;
        if (s) count(live.streams, 1);
    }
private:
    hipStream_t s = nullptr;
};

}  // namespace owned
