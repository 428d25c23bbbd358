// Host check of csrc/plonk_transcript.hpp, which prover and verifier share: Keccak-256 on its two known answers and around
// the block boundary (rate 136 bytes), and what both make of zeta where zeta^n = 1 and at a generic point, against plain
// restatements.  No device is touched.  Built as HIP for the headers' sake, the host side only, with the sanitizers:
//   hipcc --offload-host-only -std=c++17 -O1 -g -x hip tools/plonk_transcript_host_test.cpp -fsanitize=address,undefined -o t && ./t
#include <stdio.h>

#include "../rapidsnark-old_amd/csrc/plonk_transcript.hpp"

static int failures = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) failures++, printf("FAILED line %d: %s\n", __LINE__, #c);   \
    } while (0)

static std::string hex_of_keccak(const std::vector<uint8_t> &in) {
    uint8_t d[32];
    keccak256(d, in.data(), in.size());
    char s[65];
    for (int i = 0; i < 32; i++) snprintf(s + 2 * i, 3, "%02x", d[i]);
    return s;
}
// byte i of the longer inputs is 7 i + 1 mod 256
static std::vector<uint8_t> ramp(size_t n) {
    std::vector<uint8_t> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (uint8_t)(7 * i + 1);
    return v;
}

// L_i(zeta) = w^i Z_H(zeta) / (n (zeta - w^i)) with an inversion of its own, zeta^n != 1
static Fr lagrange_at(uint32_t log_n, const Fr &ze, uint64_t i) {
    const Fr wi = fr_pow(root_of_unity(log_n), i);
    Fr zh = ze;
    for (uint32_t k = 0; k < log_n; k++) zh = Fr::sqr(zh);
    zh = Fr::sub(zh, Fr::one());
    return Fr::mul(Fr::mul(wi, zh), Fr::inv(Fr::mul(fr_small(1ull << log_n), Fr::sub(ze, wi))));
}

int main() {
    CHECK(hex_of_keccak({}) == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470");
    CHECK(hex_of_keccak({'a', 'b', 'c'}) == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45");
    // one byte short of a block, a block, a byte more, two blocks: digests of the library before the transcript moved here
    CHECK(hex_of_keccak(ramp(135)) == "34bd7bed52ea092f88bc887256e7f06500ee814afa9a5566e22030af2ef1c5c0");
    CHECK(hex_of_keccak(ramp(136)) == "2b31811a93dfc4bdc41b6aa7790e784b987c25a2c8a0e101cfa694552dc8ae39");
    CHECK(hex_of_keccak(ramp(137)) == "a6103b089a404974c2b460048bfddd45108748fbdd9bad451f54d1fe95f8f284");
    CHECK(hex_of_keccak(ramp(272)) == "415fd325cae3a2f957fea2770d710027317ced7e7266a59905102c14fdb9959a");

    const uint32_t log_n = 3;
    const uint64_t l = 3;
    uint8_t pub[3 * 32] = {0};
    pub[0] = 11, pub[32] = 22, pub[64] = 33, pub[65] = 1;
    const Fr one = Fr::one(), w = root_of_unity(log_n);
    // zeta = 1: L1 = 1, PI = -publics[0]
    AtZeta z = at_zeta(log_n, one, pub, l);
    CHECK(z.zn == one && z.zh.is_zero() && z.l1 == one && z.pi == Fr::neg(fr_from_std(pub)));
    CHECK(zeta_powers(log_n, one).l1 == one && zeta_powers(log_n, one).pi.is_zero());
    // zeta = w: L1 = 0, PI = -publics[1]; zeta = w^5, beyond the publics: PI = 0
    z = at_zeta(log_n, w, pub, l);
    CHECK(z.zn == one && z.zh.is_zero() && z.l1.is_zero() && z.pi == Fr::neg(fr_from_std(pub + 32)));
    z = at_zeta(log_n, fr_pow(w, 5), pub, l);
    CHECK(z.zh.is_zero() && z.l1.is_zero() && z.pi.is_zero());
    // a generic point, with and without publics
    const Fr ze = fr_small(0x123456789abcdefull);
    z = at_zeta(log_n, ze, pub, l);
    Fr pi = Fr::zero();
    for (uint64_t i = 0; i < l; i++) pi = Fr::sub(pi, Fr::mul(fr_from_std(pub + i * 32), lagrange_at(log_n, ze, i)));
    CHECK(z.zn == fr_pow(ze, 8) && z.zh == Fr::sub(z.zn, one) && z.l1 == lagrange_at(log_n, ze, 0) && z.pi == pi);
    z = at_zeta(log_n, ze, nullptr, 0);
    CHECK(z.l1 == lagrange_at(log_n, ze, 0) && z.pi.is_zero());
    printf(failures ? "%d checks FAILED\n" : "plonk_transcript host checks OK\n", failures);
    return failures ? 1 : 0;
}
