// Host build of the one-wave signer's arithmetic (py-swirld_amd/csrc/turn.hip.h) — TEST INFRASTRUCTURE:
// tests/test_turn_sign_host.py builds it with g++ and holds the cooperative base multiplication (64 emulated lanes), the
// 32-bit-step scalar reduction and whole signatures and ids against sign.hip.h's one-lane functions, Python integers,
// libsodium, pickle and hashlib.  The product only ever launches the kernels.
#define SW_CRYPTO_HOST 1
#include "../py-swirld_amd/csrc/turn.hip.h"

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

// encode([s]B): by the wave as lane 0 holds it, and by sws::base_mult.  Returns the number of lanes whose encoded sum
// differs from lane 0's (every lane of the butterfly must end with the whole sum); `stride`: every stride-th lane is looked
// at, and the last one.
int swt_host_base_mult(const uint8_t* s32, uint8_t* coop32, uint8_t* serial32, int stride) {
    swc::u64 s[4];
    limbs(s32, s);
    swc::ge_tobytes(coop32, swt::coop_base_mult(base_row(), s));
    swc::ge_tobytes(serial32, sws::base_mult(base_row(), s));
    int differ = 0;
    for (int lane = 1; lane < swt::LANES; ++lane) {
        if (lane % stride && lane != swt::LANES - 1) continue;
        uint8_t b[32];
        swc::ge_tobytes(b, swt::coop_base_mult(base_row(), s, lane));
        differ += memcmp(b, coop32, 32) != 0;
    }
    return differ;
}

// digit `lane` of the recoding, as the lane computes it
int swt_host_lane_digit(const uint8_t* s32, int lane) {
    swc::u64 s[4];
    limbs(s32, s);
    return swt::lane_digit(s, lane);
}

void swt_host_reduce(const uint8_t* h64, uint8_t* word32, uint8_t* bitwise32) {
    swc::u64 a[4], b[4];
    swt::sc_reduce512w(h64, a);
    swc::sc_reduce512(h64, b);
    for (int i = 0; i < 4; ++i) { swc::store64_le(word32 + 8 * i, a[i]); swc::store64_le(bitwise32 + 8 * i, b[i]); }
}

void swt_host_sc_muladd(const uint8_t* r32, const uint8_t* k32, const uint8_t* a32, uint8_t* out32) {
    swc::u64 r[4], k[4], a[4], S[4];
    limbs(r32, r); limbs(k32, k); limbs(a32, a);
    swt::sc_muladd_w(r, k, a, S);
    for (int i = 0; i < 4; ++i) swc::store64_le(out32 + 8 * i, S[i]);
}

// one event through the wave's signer: dl < 0 is None, ar is 0 or 2, t_bits the timestamp's bit pattern
void swt_host_sign_event(const uint8_t* seed, const uint8_t* hdr, int hdr_len, const uint8_t* data, int dl, int ar, const uint8_t* sp32,
                         const uint8_t* op32, unsigned long long t_bits, uint8_t* sig64, uint8_t* id32) {
    sws::Secret s;
    uint8_t pk[32];
    sws::expand_seed(seed, &s);
    sws::public_key(base_row(), s, pk);
    const sws::Tmpl v{hdr, hdr_len, data, dl, ar, sp32, op32, t_bits, pk};
    swt::sign_event_wave(s, base_row(), v, sig64, id32, swt::NoStamp{});
}

}  // extern "C"
