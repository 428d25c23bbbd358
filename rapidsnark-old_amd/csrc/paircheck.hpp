// The checks the pairing units make on a proof's or a pair's points before any Miller loop, shared by pairing.hip (a lane
// per job) and pairing_coop.hip (a workgroup per job): one definition of each.
#pragma once
#include "devmem.hpp"
#include "ptcheck.hpp"

namespace zk {

constexpr uint32_t ST_OK = 0, ST_MALFORMED = 1;       // a proof's word after the checks

__device__ __forceinline__ bool below_r(const Fr &a) {
    uint32_t bw = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) (void)subb(a.v[i], FrParams::P[i], bw);
    return bw != 0;
}
template <class F>
__device__ __forceinline__ bool on_curve(const Affine<F> &p, const F &b) {
    return below_q(p.x) && below_q(p.y) && F::sqr(p.y) == F::add(F::mul(F::sqr(p.x), p.x), b);
}
__device__ __forceinline__ G1Affine g1_to_affine(const G1XYZZ &p) {
    if (p.is_inf()) return G1Affine::inf();
    const Fq t = Fq::inv(Fq::mul(p.zz, p.zzz));       // x = X/ZZ, y = Y/ZZZ by one inversion
    return G1Affine{Fq::mul(p.x, Fq::mul(t, p.zzz)), Fq::mul(p.y, Fq::mul(t, p.zz))};
}

}   // namespace zk
