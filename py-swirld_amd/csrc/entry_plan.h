// The host-side planning every call form of the C-ABI shares ("entry protocol"): the rows of a device-array
// call that are checked for alignment and residency, and the staging plan of a host-array call.  No HIP here: this header
// compiles with a plain C++ compiler (tests/entry_plan_main.cpp); swirld_hip.hip puts the HIP calls around it.
#pragma once

#include <cstddef>
#include <cstdint>

namespace entry {

// One array of a call.  A row whose pointer is NULL or whose length is 0 stands for an array the call does not touch: no
// check looks at it.  (That a REQUIRED array is not NULL is what the *_pre functions check, before any row is built.)
struct Arg {
    const void* p;
    size_t bytes;
    unsigned align;   // a power of two; 1: no alignment asked
};

inline bool skipped(const Arg& a) { return !a.p || !a.bytes; }

// the first row that is not aligned as it asks, or -1
inline int first_misaligned(const Arg* a, int n) {
    for (int i = 0; i < n; ++i)
        if (!skipped(a[i]) && ((uintptr_t)a[i].p & (uintptr_t)(a[i].align - 1))) return i;
    return -1;
}

struct Carve {   // consecutive 256-byte aligned pieces of one allocation
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }
};

// The staging buffer of a host-array call: pieces carved in call order, with the copies that fill them from the caller's
// arrays before the launches (in) and bring them back behind them (out).
struct Stage {
    static constexpr int MAX_ROWS = 16;
    struct Copy { size_t off; const void* src; void* dst; size_t bytes; };
    Carve cv;
    Copy up[MAX_ROWS], down[MAX_ROWS];
    int n_up = 0, n_down = 0;
    bool full = false;   // a copy did not fit the lists (stage_up refuses the plan)

    // room for an input and the upload of it; an array the caller left out (NULL) takes no room
    size_t in(const void* src, size_t bytes) {
        if (!src) bytes = 0;
        const size_t o = cv.take(bytes);
        if (bytes && n_up == MAX_ROWS) full = true;
        else if (bytes) up[n_up++] = Copy{o, src, nullptr, bytes};
        return o;
    }
    // room for an output and the download of it; an output the caller does not want (NULL) keeps its room: the kernels write it
    size_t out(void* dst, size_t bytes) { return out(dst, bytes, bytes); }
    // ... whose download is shorter than its room, or sized later (out_bytes) by a count the device reports
    size_t out(void* dst, size_t room, size_t bytes) {
        const size_t o = cv.take(room);
        if (dst && n_down == MAX_ROWS) full = true;
        else if (dst) down[n_down++] = Copy{o, nullptr, dst, bytes};
        return o;
    }
    // ... which takes no room when the caller does not want it (the kernels skip it as well)
    size_t out_opt(void* dst, size_t bytes) { return out(dst, dst ? bytes : 0); }
    void out_bytes(const void* dst, size_t bytes) {
        for (int i = 0; i < n_down; ++i)
            if (down[i].dst == dst) down[i].bytes = bytes;
    }
    size_t scratch(size_t bytes) { return cv.take(bytes); }
    size_t total() const { return cv.off; }
};

}  // namespace entry
