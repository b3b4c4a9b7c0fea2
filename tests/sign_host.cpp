// Host build of the signer's arithmetic (py-swirld_amd/csrc/sign.hip.h) — TEST INFRASTRUCTURE: tests/test_sign_host.py
// builds it with g++ and holds key expansion, sc_muladd, signing and the template hasher against libsodium, Python integers,
// pickle and hashlib.  The product only ever launches the kernels.
#define SW_CRYPTO_HOST 1
#include "../py-swirld_amd/csrc/sign.hip.h"

#include <cstring>
#include <vector>

namespace {
const swv::niels* base_row() {
    static std::vector<swv::niels> row;
    if (row.empty()) {
        row.resize(swv::ROW);
        swv::build_row_host(swc::ge_base(), row.data());
    }
    return row.data();
}
void limbs(const uint8_t b[32], swc::u64 v[4]) { for (int i = 0; i < 4; ++i) v[i] = swc::load64_le(b + 8 * i); }
}  // namespace

extern "C" {

// a (32 bytes, little-endian), prefix, and the public key of a seed
void sws_host_expand(const uint8_t* seed, uint8_t* a32, uint8_t* prefix32, uint8_t* pk32) {
    sws::Secret s;
    sws::expand_seed(seed, &s);
    for (int i = 0; i < 4; ++i) swc::store64_le(a32 + 8 * i, s.a[i]);
    memcpy(prefix32, s.prefix, 32);
    sws::public_key(base_row(), s, pk32);
}

void sws_host_sc_muladd(const uint8_t* r32, const uint8_t* k32, const uint8_t* a32, uint8_t* out32) {
    swc::u64 r[4], k[4], a[4], S[4];
    limbs(r32, r); limbs(k32, k); limbs(a32, a);
    sws::sc_muladd(r, k, a, S);
    for (int i = 0; i < 4; ++i) swc::store64_le(out32 + 8 * i, S[i]);
}

void sws_host_sign_raw(const uint8_t* seed, const uint8_t* m, unsigned long long n, uint8_t* sig64) {
    sws::Secret s;
    uint8_t pk[32];
    sws::expand_seed(seed, &s);
    sws::public_key(base_row(), s, pk);
    sws::sign_message(s, pk, base_row(), sws::RawMsg{m, n}, sig64);
}

// one event through the segment iterator: dl < 0 is None, ar is 0 or 2, t_bits the timestamp's bit pattern
void sws_host_sign_event(const uint8_t* seed, const uint8_t* hdr, int hdr_len, const uint8_t* data, int dl, int ar, const uint8_t* sp32,
                         const uint8_t* op32, unsigned long long t_bits, uint8_t* sig64, uint8_t* id32) {
    sws::Secret s;
    uint8_t pk[32];
    sws::expand_seed(seed, &s);
    sws::public_key(base_row(), s, pk);
    const sws::Tmpl v{hdr, hdr_len, data, dl, ar, sp32, op32, t_bits, pk};
    sws::sign_event(s, base_row(), v, sig64, id32);
}

}  // extern "C"
