// The device side that the two batch-verification units share (pairing_batch.hip: one key, DESIGN.md section 23;
// pairing_set_batch.hip: a key set, section 25): what a lane does for its proof in the check, scale and Miller kernels, the
// wave that sums a group's or segment's X, and the points a tail keeps in LDS.  The kernels stay in their units and find
// the lane's proof, signals and slot; what is computed is here, once.  On top of pairing_coop_dev.hpp, whose LDS block and
// sliced Fq12 operations both tails run on; like it, everything here has internal linkage.
#pragma once
#include "pairing_coop_dev.hpp"

namespace {

constexpr uint32_t TAIL_THREADS = 192;

struct Scalar16 {
    uint32_t v[4];
};
static_assert(sizeof(Scalar16) == 16, "layout");

__device__ __noinline__ void nl_madd(G1XYZZ &a, const G1Affine &b) { madd(a, b); }
__device__ __noinline__ void nl_dbl(G1XYZZ &a) { a = dbl(a); }

__device__ __forceinline__ Fr scalar_of(const Scalar16 *p) {
    const uint4 w = *reinterpret_cast<const uint4 *>(p);
    Fr r = Fr::zero();
    r.v[0] = w.x; r.v[1] = w.y; r.v[2] = w.z; r.v[3] = w.w;
    return r;
}

// ---------------------------------------------------------------- a lane per proof.  pr: A 64 | B 128 | C 64
// *status: k_verify_check's criteria (without vk_x), the subgroup by psi.  pub: the proof's nPublic signals
__device__ __forceinline__ void batch_check_lane(uint32_t *status, const uint8_t *__restrict__ pr, const Fr *__restrict__ pub, uint32_t nPublic,
                                                 const PairConsts *__restrict__ k, const Fq &b1, const Fq2 &b2) {
    const G1Affine A = load_pt(reinterpret_cast<const G1Affine *>(pr));
    const G2Affine B = load_pt(reinterpret_cast<const G2Affine *>(pr + 64));
    const G1Affine C = load_pt(reinterpret_cast<const G1Affine *>(pr + 192));
    bool ok = !A.is_inf() && !B.is_inf() && !C.is_inf() && nl_on_curve(A, b1) && nl_on_curve(C, b1) && nl_on_curve(B, b2);
    for (uint32_t j = 0; ok && j < nPublic; j++) ok = below_r(load_el(pub + j));
    if (ok) ok = nl_subgroup(B, k);
    *status = ok ? ST_OK : ST_MALFORMED;
}

// *ra = r A (affine), *rc = r C; a malformed proof: *rc = infinity, *ra is not written.  The scalar is not zero and below
// 2^128 < r, and A has order r: r A is never infinity.
__device__ __forceinline__ void batch_scale_lane(G1Affine *ra, G1XYZZ *rc, uint32_t status, const uint8_t *__restrict__ pr,
                                                 const Scalar16 *__restrict__ scalar) {
    if (status != ST_OK) {
        store_pt(rc, G1XYZZ::inf());
        return;
    }
    const G1Affine A = load_pt(reinterpret_cast<const G1Affine *>(pr));
    const G1Affine C = load_pt(reinterpret_cast<const G1Affine *>(pr + 192));
    const uint4 w = *reinterpret_cast<const uint4 *>(scalar);
    uint32_t k0 = w.x, k1 = w.y, k2 = w.z, k3 = w.w;
    G1XYZZ a = G1XYZZ::inf(), c = G1XYZZ::inf();
#pragma unroll 1
    for (int b = 0; b < 128; b++) {                   // from the top bit; doubling infinity keeps it
        nl_dbl(a);
        nl_dbl(c);
        if (k3 >> 31) {
            nl_madd(a, A);
            nl_madd(c, C);
        }
        k3 = (k3 << 1) | (k2 >> 31);
        k2 = (k2 << 1) | (k1 >> 31);
        k1 = (k1 << 1) | (k0 >> 31);
        k0 <<= 1;
    }
    G1Affine P;
    nl_to_affine(P, a);
    store_el(&ra->x, P.x);
    store_el(&ra->y, P.y);
    store_pt(rc, c);
}

// *f_out: the Miller value of (r A, B), ra: r A; 1 for a malformed proof, so that the products after it need no status
__device__ __forceinline__ void batch_miller_lane(Fq12 *f_out, uint32_t status, const uint8_t *__restrict__ pr, const G1Affine *__restrict__ ra,
                                                  const PairConsts *k) {
    Fq12 f;
    f12_one(f);
    if (status != ST_OK) {
        *f_out = f;
        return;
    }
    const G2Affine B = load_pt(reinterpret_cast<const G2Affine *>(pr + 64));
    const G1Affine P = load_pt(ra);
    G2Proj T{B.x, B.y, Fq2::one()};
    G2Affine q1, q2;
    frob_twist(q1, q2, B, *k);
    Line l;
    for (int s = 0; s < 64; s++) {
        f12_sqr(f, f);
        step_dbl(T, l, *k);
        f12_mul_line_at(f, l, P);
        if (ate_bit(s)) {
            step_add(T, l, B);
            f12_mul_line_at(f, l, P);
        }
    }
    step_add(T, l, q1);
    f12_mul_line_at(f, l, P);
    step_add(T, l, q2);
    f12_mul_line_at(f, l, P);
    *f_out = f;
}

// ---------------------------------------------------------------- the tails
// X = R IC_0 + sum_j S_j IC_(j+1) into L.part[0], by the 64 lanes of one wave.  S: S_0 .. S_(nPublic-1), then R
__device__ __forceinline__ void x_wave(uint32_t lane, const G1Affine *__restrict__ ic, const Fr *__restrict__ S, uint32_t nPublic, const Fq &beta) {
    G1XYZZ acc = G1XYZZ::inf();                       // term j: S_j IC_(j+1); term nPublic: R IC_0
    for (uint32_t j = lane; j <= nPublic; j += 64) {
        G1XYZZ t;
        nl_mul_glv(t, load_pt(ic + (j == nPublic ? 0 : 1 + j)), load_el(S + j), beta);
        nl_add(acc, t);
    }
    L.part[lane] = acc;
    for (uint32_t s = 32; s; s >>= 1) {
        wsync();
        if (lane < s) {
            G1XYZZ a = L.part[lane];
            const G1XYZZ b = L.part[lane + s];
            nl_add(a, b);
            L.part[lane] = a;
        }
    }
}

// what a tail keeps beside L, per segment of a pass: -R alpha, -X, -Cs, and whether each is a point at all
template <uint32_t SEGS>
struct alignas(16) TailPts {
    G1Affine pt[SEGS][3];
    uint32_t have[SEGS][3];
};

// -p into *pt, *have = p is not infinity
__device__ __forceinline__ void put_neg(G1Affine *pt, uint32_t *have, const G1XYZZ &p) {
    G1Affine P;
    nl_to_affine(P, p);
    *have = P.is_inf() ? 0u : 1u;
    P.y = Fq::neg(P.y);
    *pt = P;
}

}   // namespace
