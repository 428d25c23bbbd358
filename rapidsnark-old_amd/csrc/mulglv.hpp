// k P for a lane's own scalar by the endomorphism split (glv.hpp), G1 and G2 in one template, and the endomorphism's
// constant: what mulvec.hip's kernels run per point and pairing_coop.hip's runs per public signal.  mulvec.hip's header
// comment describes the loop.
#pragma once
#include "devmem.hpp"
#include "ptcheck.hpp"
#include "glv.hpp"

namespace zk {

// beta = 2203960485148121921418603742825762020974279258880205651966, standard form (scale.hip)
inline constexpr uint32_t BETA_STD[8] = {0x77fffffeu, 0x57634731u, 0xacdb5c4fu, 0xd4f263f1u, 0xa0d48bacu, 0x59e26bceu, 0, 0};


__device__ __forceinline__ Fq pick(bool c, const Fq &a, const Fq &b) {
    Fq r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
    return r;
}
__device__ __forceinline__ Fq2 pick(bool c, const Fq2 &a, const Fq2 &b) { return Fq2{pick(c, a.a, b.a), pick(c, a.b, b.b)}; }
__device__ __forceinline__ Fq times_fq(const Fq &x, const Fq &e) { return Fq::mul(x, e); }
__device__ __forceinline__ Fq2 times_fq(const Fq2 &x, const Fq &e) { return Fq2{Fq::mul(x.a, e), Fq::mul(x.b, e)}; }

// k P for the lane's own k (standard form, below r); e: the x-multiplier of the endomorphism that is multiplication by lambda
template <class F>
__device__ __forceinline__ XYZZ<F> mul_glv(const Affine<F> &P, const Fr &k, const Fq &e) {
    uint32_t k1[4], k2[4];
    glv_split(k.v, k1, k2);
    const F ex = times_fq(P.x, e);
    XYZZ<F> acc = XYZZ<F>::inf();
#pragma unroll 1
    for (int c = 0; c < 128; c++) {
        acc = dbl(acc);
        const bool b1 = k1[3] >> 31, b2 = k2[3] >> 31, both = b1 && b2, any = b1 || b2;
        Affine<F> T;                                                          // P = infinity: all-zero whatever the digits
        T.x = pick(both, F::neg(F::add(P.x, ex)), pick(b2, ex, P.x));
        T.y = pick(both, F::neg(P.y), P.y);
        T.x = pick(any, T.x, F::zero());
        T.y = pick(any, T.y, F::zero());
        madd(acc, T);
#pragma unroll
        for (int q = 3; q > 0; q--) {
            k1[q] = (k1[q] << 1) | (k1[q - 1] >> 31);
            k2[q] = (k2[q] << 1) | (k2[q - 1] >> 31);
        }
        k1[0] <<= 1;
        k2[0] <<= 1;
    }
    return acc;
}

template <class F>
inline Fq endo_const() {                                     // beta in G1, beta^2 on the twist
    const Fq beta = fq_std(BETA_STD);
    return sizeof(F) == sizeof(Fq) ? beta : Fq::sqr(beta);
}

}   // namespace zk
