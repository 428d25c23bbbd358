// The cooperative (latency) path of the pairing units: one workgroup per proof or per group of pairs, an Fq12 product
// spread over the lanes of one wave (pairing_coop.hip).  This header holds what is host + device:
// the map from lanes to the coefficients of a sliced product, which a host build checks against pairing.hpp's f12_mul,
// f12_sqr and f12_mul_line, the reading of the two thresholds, and the launchers pairing.hip calls.
//
// An Fq12 over the basis 1, w, ..., w^5 with coefficients in Fq2 (w^6 = xi): in pairing.hpp's layout the coefficient of w^k
// is Fq2 number coop_slot(k) of the six (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2), because w^2 = v.  Lane 6 i + j makes
// a_i b_j; lane k < 6 then sums c_k = sum_{i + j = k} a_i b_j + xi sum_{i + j = k + 6} a_i b_j.  A line s + t w + c w^3 has
// j in {0, 1, 3} only: 18 lanes.  The sums are exact in Fq2 and every element is kept reduced, so the result has the same
// bytes as the Karatsuba forms of pairing.hpp.
#pragma once
#include <string>

#include "pairing.hpp"
#include "verify_batch_host.hpp"

namespace zk {

constexpr uint32_t COOP_FULL = 0x3Fu, COOP_LINE = 0x0Bu;   // the j with a non-zero b_j: all six, or a line's 0, 1 and 3
constexpr int COOP_LANES_FULL = 36, COOP_LANES_LINE = 18;

ZK_HD int coop_slot(int k) { return (k & 1) * 3 + (k >> 1); }
// the (i, j) of a lane's product
ZK_HD void coop_pair_full(int lane, int &i, int &j) {
    i = lane / 6;
    j = lane % 6;
}
ZK_HD void coop_pair_line(int lane, int &i, int &j) {
    i = lane / 3;
    j = lane % 3;
    if (j == 2) j = 3;
}
// c_k from prod[6 i + j] = a_i b_j; entries whose j is not in jmask are never read
ZK_HD Fq2 coop_sum(int k, const Fq2 *prod, uint32_t jmask) {
    Fq2 lo = Fq2::zero(), hi = Fq2::zero();
    for (int i = 0; i < 6; i++) {
        const bool wrap = i > k;                      // i + j = k + 6
        const int j = wrap ? k + 6 - i : k - i;
        if (!((jmask >> j) & 1u)) continue;
        if (wrap) hi = Fq2::add(hi, prod[6 * i + j]);
        else lo = Fq2::add(lo, prod[6 * i + j]);
    }
    return Fq2::add(lo, f2_mul_xi(hi));
}

// ZKHIP_VERIFY_COOP_MAX / ZKHIP_PAIRING_COOP_MAX: the largest number of jobs a call sends down the cooperative path; 0: never
inline uint64_t coop_threshold(const char *name, const char *jobs, uint64_t dflt) {
    return env_number(name, dflt, 0, 1ull << 24, ("a number of " + std::string(jobs) + " from 0 to 2^24").c_str());
}

#if defined(__HIPCC__)
constexpr uint32_t COOP_FINAL = 1, COOP_CHECK = 2;    // k_pairing_coop's flags: final exponentiation and bytes out; point checks

// verdict[i] of n proofs, one workgroup each.  lines: n x MILLER_LINES, the kernel's own.
void launch_verify_coop(uint8_t *verdict, const uint8_t *proofs, const Fr *publics, uint64_t n, uint32_t nPublic, const G1Affine *ic, const Line *tab,
                        const Fq12 *ml_ab, const PairConsts *k, Line *lines, hipStream_t s);
// out[j]: group j's product, 384 bytes (COOP_FINAL) or the Miller value as an Fq12.  lines: n_pairs x MILLER_LINES and skip: n_pairs,
// the kernel's own; err: k_pair_check's three words, set to NO_BAD_POINT by the caller (written with COOP_CHECK only).
void launch_pairing_coop(uint8_t *out, const G1Affine *g1, const G2Affine *g2, Line *lines, uint8_t *skip, uint32_t *err, uint64_t n_pairs, uint32_t group,
                         uint32_t flags, const PairConsts *k, hipStream_t s);
#endif

}   // namespace zk
