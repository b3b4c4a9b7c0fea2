// Stand-alone host program over turn.hip.h — TEST INFRASTRUCTURE (tests/test_turn_sign_host.py builds it with
// -fsanitize=address,undefined and runs it as a child process).  It reads a case file and prints one line of hex per case:
// for a scalar encode([s]B) by the 64 emulated lanes, for a 64-byte value its reduction mod L, for an event the 64 signature
// bytes and the 32 id bytes behind them.
//
// Case file, little-endian:  int32 cases | per case: int32 kind |
//   kind 0 (scalar):  32 bytes
//   kind 1 (event):   32 seed bytes | int32 hdr_len | hdr | int32 dl (-1: None) | max(dl, 0) data bytes | int32 arity | 32 sp | 32 op | uint64 t_bits
//   kind 2 (reduce):  64 bytes
// Every buffer handed to the signer is a heap copy of exactly its length: a read past a segment ends the program.
#define SW_CRYPTO_HOST 1
#include "../py-swirld_amd/csrc/turn.hip.h"

#include <cstdio>
#include <cstring>
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
    std::vector<uint8_t> bytes(size_t n) { std::vector<uint8_t> v(n); const uint8_t* p = take(n); if (p && n) memcpy(v.data(), p, n); return v; }
};
void hex(const uint8_t* p, size_t n) { for (size_t i = 0; i < n; ++i) printf("%02x", p[i]); }
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
    std::vector<swv::niels> row(swv::ROW);
    swv::build_row_host(swc::ge_base(), row.data());
    static const uint8_t none = 0;
    const int32_t cases = r.scalar<int32_t>();
    if (!r.ok || cases < 0 || cases > (1 << 20)) { fprintf(stderr, "bad case count\n"); return 2; }
    for (int32_t c = 0; c < cases; ++c) {
        const int32_t kind = r.scalar<int32_t>();
        if (!r.ok || kind < 0 || kind > 2) { fprintf(stderr, "case %d: bad header\n", c); return 2; }
        if (kind == 0) {
            const std::vector<uint8_t> sb = r.bytes(32);
            if (!r.ok) { fprintf(stderr, "case file too short\n"); return 2; }
            swc::u64 s[4];
            for (int i = 0; i < 4; ++i) s[i] = swc::load64_le(sb.data() + 8 * i);
            uint8_t out[32];
            swc::ge_tobytes(out, swt::coop_base_mult(row.data(), s));
            hex(out, 32);
        } else if (kind == 2) {
            const std::vector<uint8_t> h = r.bytes(64);
            if (!r.ok) { fprintf(stderr, "case file too short\n"); return 2; }
            swc::u64 a[4];
            uint8_t out[32];
            swt::sc_reduce512w(h.data(), a);
            for (int i = 0; i < 4; ++i) swc::store64_le(out + 8 * i, a[i]);
            hex(out, 32);
        } else {
            const std::vector<uint8_t> seed = r.bytes(32);
            const int32_t hdr_len = r.scalar<int32_t>();
            if (!r.ok || hdr_len < 0 || hdr_len > 1024) { fprintf(stderr, "case %d: bad class header\n", c); return 2; }
            const std::vector<uint8_t> hdr = r.bytes((size_t)hdr_len);
            const int32_t dl = r.scalar<int32_t>();
            if (!r.ok || dl < -1 || dl > tpl::MAX_DATA) { fprintf(stderr, "case %d: bad data length\n", c); return 2; }
            const std::vector<uint8_t> data = r.bytes(dl > 0 ? (size_t)dl : 0);
            const int32_t ar = r.scalar<int32_t>();
            const std::vector<uint8_t> sp = r.bytes(32), op = r.bytes(32);
            const unsigned long long t_bits = r.scalar<unsigned long long>();
            if (!r.ok || (ar != 0 && ar != 2)) { fprintf(stderr, "case %d: bad event\n", c); return 2; }
            sws::Secret s;
            uint8_t pk[32], sig[64], id[32];
            sws::expand_seed(seed.data(), &s);
            sws::public_key(row.data(), s, pk);
            const sws::Tmpl v{hdr.empty() ? &none : hdr.data(), hdr_len, data.empty() ? &none : data.data(), dl, ar, sp.data(), op.data(), t_bits, pk};
            swt::sign_event_wave(s, row.data(), v, sig, id, swt::NoStamp{});
            hex(sig, 64);
            hex(id, 32);
        }
        printf("\n");
    }
    return 0;
}
