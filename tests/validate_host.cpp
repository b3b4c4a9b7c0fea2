// Host build of validate.hip.h (g++ -DSW_CRYPTO_HOST) — TEST INFRASTRUCTURE: lets the CPU suite run the very functions
// the member-table and payload-validation kernels execute against libsodium (tests/test_validate_host.py).  The product
// never loads this library; it launches the kernels of swirld_hip.hip.
#define SW_CRYPTO_HOST 1
#include "../py-swirld_amd/csrc/validate.hip.h"

extern "C" {
int swv_host_entry_bytes(void) { return (int)sizeof(swv::niels); }
int swv_host_row_entries(void) { return swv::ROW; }

// tab: (n + 1) rows of ROW entries; usable: n bytes.  Returns the number of unusable keys.
int swv_host_build(int n, const uint8_t* pk, void* tab, uint8_t* usable) {
    swv::niels* t = (swv::niels*)tab;
    int bad = 0;
    for (int m = 0; m < n; ++m) {
        swc::ge P;
        usable[m] = swv::member_point(pk + (size_t)m * 32, &P) ? 1 : 0;
        if (usable[m]) swv::build_row_host(P, t + (size_t)m * swv::ROW);
        else ++bad;
    }
    swv::build_row_host(swc::ge_base(), t + (size_t)n * swv::ROW);
    return bad;
}

void swv_host_validate(long long K, const uint8_t* msgs, const long long* msg_off, long long msg_bytes, const uint8_t* whole,
                       const long long* whole_off, long long whole_bytes, const uint8_t* sig, const int32_t* creator,
                       const uint8_t* id, int n, const uint8_t* pk, const uint8_t* usable, const void* tab, uint8_t* ok) {
    const swv::Payload p{msgs, msg_off, msg_bytes, whole, whole_off, whole_bytes, sig, creator, id};
    for (long long i = 0; i < K; ++i) ok[i] = swv::validate_event(p, i, n, pk, usable, (const swv::niels*)tab) ? 1 : 0;
}

void swv_host_recode(const uint8_t* s32, int8_t* d64) {
    uint64_t s[4];
    for (int i = 0; i < 4; ++i) s[i] = swc::load64_le(s32 + 8 * i);
    swv::recode(s, d64);
}

// canonical encodings of (y + x, y - x, 2dxy) of entry j (1..8) at position pos of row m
void swv_host_entry(const void* tab, int m, int pos, int j, uint8_t* out96) {
    const swv::niels& e = ((const swv::niels*)tab)[(size_t)m * swv::ROW + (size_t)pos * swv::PER_POS + (j - 1)];
    swc::fe_tobytes(out96, e.yplusx);
    swc::fe_tobytes(out96 + 32, e.yminusx);
    swc::fe_tobytes(out96 + 64, e.xy2d);
}

// the same entry by repeated ge_add alone: 16^pos by 4 * pos self-additions, then j - 1 additions
int swv_host_entry_by_additions(const uint8_t* pk, int negate, int pos, int j, uint8_t* out96) {
    swc::ge P;
    if (pk) {
        if (!swc::ge_frombytes(&P, pk)) return 0;
        if (negate) P = swc::ge_neg(P);
    } else {
        P = swc::ge_base();
    }
    for (int k = 0; k < 4 * pos; ++k) P = swc::ge_add(P, P);
    swc::ge R = P;
    for (int k = 1; k < j; ++k) R = swc::ge_add(R, P);
    const swv::niels e = swv::niels_of(R, swc::fe_invert(R.Z));
    swc::fe_tobytes(out96, e.yplusx);
    swc::fe_tobytes(out96 + 32, e.yminusx);
    swc::fe_tobytes(out96 + 64, e.xy2d);
    return 1;
}

int swv_host_verify_ref(const uint8_t* sig, const uint8_t* m, uint64_t mlen, const uint8_t* pk) { return swc::ed25519_verify(sig, m, mlen, pk) ? 1 : 0; }
}
