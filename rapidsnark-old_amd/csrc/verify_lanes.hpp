// The three steps of a lane that verifies one proof, shared by pairing.hip (k_verify_check / _miller / _final: the key in
// the launch arguments, lane i has proof i) and pairing_set.hip (the key from a record in device memory, a wave per run of
// one key).  The kernels find the lane's proof, signals and slots; what is computed is here, once.  pairing.hip's file
// comment describes the equation and the tables.
#pragma once
#include "hiputil.hpp"
#include "devmem.hpp"
#include "ptcheck.hpp"
#include "pairing.hpp"
#include "paircheck.hpp"

namespace {

__device__ __noinline__ bool in_subgroup(const G2Affine &Q) {   // [r] Q = infinity
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = FrParams::P[i];
    return scalar_mul_affine(Q, r).is_inf();
}

// *status, and *vkx when the proof is well-formed.  pr: A 64 | B 128 | C 64; pub: the proof's nPublic signals
__device__ __forceinline__ void verify_check_lane(uint32_t *status, G1Affine *vkx, const uint8_t *__restrict__ pr, const Fr *__restrict__ pub,
                                                  uint32_t nPublic, const G1Affine *__restrict__ ic, const Fq &b1, const Fq2 &b2) {
    const G1Affine A = load_pt(reinterpret_cast<const G1Affine *>(pr));
    const G2Affine B = load_pt(reinterpret_cast<const G2Affine *>(pr + 64));
    const G1Affine C = load_pt(reinterpret_cast<const G1Affine *>(pr + 192));
    bool ok = !A.is_inf() && !B.is_inf() && !C.is_inf() && on_curve(A, b1) && on_curve(C, b1) && on_curve(B, b2);
    for (uint32_t j = 0; ok && j < nPublic; j++) ok = below_r(load_el(pub + j));
    if (ok) ok = in_subgroup(B);
    *status = ok ? ST_OK : ST_MALFORMED;
    if (!ok) return;
    G1XYZZ acc = G1XYZZ::from_affine(load_pt(ic));
    for (uint32_t j = 0; j < nPublic; j++) {
        const G1XYZZ t = scalar_mul_affine(load_pt(ic + 1 + j), load_el(pub + j));
        add(acc, t);
    }
    const G1Affine X = g1_to_affine(acc);
    store_el(&vkx->x, X.x);
    store_el(&vkx->y, X.y);
}

// *f_out = miller(-A, B) miller(vk_x, gamma) miller(C, delta) miller(alpha, beta) of a well-formed proof; tab: gamma's
// lines, then delta's, the same address in every lane of the wave
__device__ __forceinline__ void verify_miller_lane(Fq12 *f_out, const uint8_t *__restrict__ pr, const G1Affine *__restrict__ vkx,
                                                   const Line *__restrict__ tab, const Fq12 *ml_ab, const PairConsts *k) {
    G1Affine A = load_pt(reinterpret_cast<const G1Affine *>(pr));
    A.y = Fq::neg(A.y);
    const G2Affine B = load_pt(reinterpret_cast<const G2Affine *>(pr + 64));
    const G1Affine C = load_pt(reinterpret_cast<const G1Affine *>(pr + 192));
    const G1Affine X = load_pt(vkx);
    const bool have_x = !X.is_inf();
    const Line *tg = tab, *td = tab + MILLER_LINES;
    G2Proj T{B.x, B.y, Fq2::one()};
    G2Affine q1, q2;
    frob_twist(q1, q2, B, *k);
    Fq12 f;
    f12_one(f);
    Line l;
    int at = 0;                                       // wave-uniform: the index into both tables
    auto lines = [&]() {                              // the line just made at -A, and the tables' lines at vk_x and C
        f12_mul_line_at(f, l, A);
        if (have_x) f12_mul_line_at(f, tg[at], X);
        f12_mul_line_at(f, td[at], C);
        at++;
    };
    for (int s = 0; s < 64; s++) {
        f12_sqr(f, f);
        step_dbl(T, l, *k);
        lines();
        if (ate_bit(s)) {
            step_add(T, l, B);
            lines();
        }
    }
    step_add(T, l, q1);
    lines();
    step_add(T, l, q2);
    lines();
    f12_mul(f, f, *ml_ab);
    *f_out = f;
}

// *verdict from the proof's status word and Miller value
__device__ __forceinline__ void verify_final_lane(uint8_t *verdict, const Fq12 *f, uint32_t status, const PairConsts *k) {
    if (status != ST_OK) {
        *verdict = ZK_VERIFY_MALFORMED;
        return;
    }
    Fq12 r;
    final_exp(r, *f, *k);
    *verdict = f12_is_one(r) ? ZK_VERIFY_OK : ZK_VERIFY_INVALID;
}

}   // namespace
