// Stand-alone host program over validate.hip.h — TEST INFRASTRUCTURE (tests/test_validate_host.py builds it with
// -fsanitize=address,undefined and runs it as a child process).  It reads a case file, builds the member table, validates
// every event and prints one line of '0' / '1' verdicts.
//
// Case file, little-endian:  int32 n | n * 32 key bytes | int64 K | int64 msg_bytes | int64 whole_bytes (-1: no id check)
//   | (K + 1) int64 msg_off | msg_bytes | [ (K + 1) int64 whole_off | whole_bytes ] | K * 64 sig | K int32 creator | K * 32 id
#define SW_CRYPTO_HOST 1
#include "../py-swirld_amd/csrc/validate.hip.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {
struct Reader {
    std::vector<uint8_t> buf;
    size_t at = 0;
    bool ok = true;
    const uint8_t* take(size_t n) {
        if (n > buf.size() - at) { ok = false; return nullptr; }
        const uint8_t* p = buf.data() + at;
        at += n;
        return p;
    }
    template <class T>
    T scalar() { T v{}; const uint8_t* p = take(sizeof(T)); if (p) memcpy(&v, p, sizeof(T)); return v; }
    template <class T>
    std::vector<T> array(size_t n) { std::vector<T> v(n); const uint8_t* p = take(n * sizeof(T)); if (p && n) memcpy(v.data(), p, n * sizeof(T)); return v; }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 2; }
    Reader r;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        uint8_t tmp[65536];
        size_t got;
        while ((got = fread(tmp, 1, sizeof tmp, f)) > 0) r.buf.insert(r.buf.end(), tmp, tmp + got);
        fclose(f);
    }
    const int32_t n = r.scalar<int32_t>();
    if (!r.ok || n < 1 || n > 1024) { fprintf(stderr, "bad member count\n"); return 2; }
    const std::vector<uint8_t> pk = r.array<uint8_t>((size_t)n * 32);
    const long long K = r.scalar<long long>(), msg_bytes = r.scalar<long long>(), whole_bytes = r.scalar<long long>();
    if (!r.ok || K < 0 || K > (1 << 20) || msg_bytes < 0 || whole_bytes < -1) { fprintf(stderr, "bad sizes\n"); return 2; }
    const std::vector<long long> msg_off = r.array<long long>((size_t)K + 1);
    const std::vector<uint8_t> msgs = r.array<uint8_t>((size_t)msg_bytes);
    std::vector<long long> whole_off;
    std::vector<uint8_t> whole;
    if (whole_bytes >= 0) { whole_off = r.array<long long>((size_t)K + 1); whole = r.array<uint8_t>((size_t)whole_bytes); }
    const std::vector<uint8_t> sig = r.array<uint8_t>((size_t)K * 64);
    const std::vector<int32_t> creator = r.array<int32_t>((size_t)K);
    const std::vector<uint8_t> id = r.array<uint8_t>((size_t)K * 32);
    if (!r.ok) { fprintf(stderr, "case file too short\n"); return 2; }

    std::vector<swv::niels> tab((size_t)(n + 1) * swv::ROW);
    std::vector<uint8_t> usable((size_t)n);
    for (int m = 0; m < n; ++m) {
        swc::ge P;
        usable[m] = swv::member_point(pk.data() + (size_t)m * 32, &P) ? 1 : 0;
        if (usable[m]) swv::build_row_host(P, tab.data() + (size_t)m * swv::ROW);
    }
    swv::build_row_host(swc::ge_base(), tab.data() + (size_t)n * swv::ROW);

    // (empty vectors may have a null data(): the id check is selected by whole_bytes, not by the pointer)
    static const uint8_t none = 0;
    const swv::Payload p{msgs.empty() ? &none : msgs.data(), msg_off.data(), msg_bytes,
                         whole_bytes >= 0 ? (whole.empty() ? &none : whole.data()) : nullptr, whole_bytes >= 0 ? whole_off.data() : nullptr,
                         whole_bytes >= 0 ? whole_bytes : 0, sig.data(), creator.data(), id.data()};
    std::string out((size_t)K, '0');
    for (long long i = 0; i < K; ++i) out[(size_t)i] = swv::validate_event(p, i, n, pk.data(), usable.data(), tab.data()) ? '1' : '0';
    printf("%s\n", out.c_str());
    return 0;
}
