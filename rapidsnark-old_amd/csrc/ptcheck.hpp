// Is this a point of the curve?  The one check every entry point that takes points from a file makes before it computes
// with them (ptau_prepare.hip, scale.hip): coordinates below q and y^2 = x^3 + b, the all-zero encoding (infinity) legal.
// Device side a kernel over a row of points, host side the constant b of G1 and of the G2 twist and a launcher that
// returns the lowest failing index.
#pragma once
#include "hiputil.hpp"
#include "devmem.hpp"

namespace zk {

__device__ __forceinline__ bool below_q(const Fq &a) {
    uint32_t bw = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) (void)subb(a.v[i], FqParams::P[i], bw);
    return bw != 0;
}
__device__ __forceinline__ bool below_q(const Fq2 &a) { return below_q(a.a) && below_q(a.b); }

// y^2 = x^3 + b (b = 3 in G1, 3 / (9 + u) on the twist), coordinates below q; the lowest failing index goes to *err
template <class F>
__global__ __launch_bounds__(256) void k_point_check(uint32_t *err, const Affine<F> *src, uint64_t n, F b) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<F> p = load_pt(src + i);
    if (p.is_inf()) return;
    const bool ok = below_q(p.x) && below_q(p.y) && F::sqr(p.y) == F::add(F::mul(F::sqr(p.x), p.x), b);
    if (!ok) atomicMin(err, (uint32_t)i);
}

inline Fq fq_std(uint32_t lo) {                      // small constant -> Montgomery
    Fq x = Fq::zero();
    x.v[0] = lo;
    return Fq::to_mont(x);
}
inline Fq fq_std(const uint32_t w[8]) {
    Fq x;
    for (int i = 0; i < 8; i++) x.v[i] = w[i];
    return Fq::to_mont(x);
}
template <class F>
F curve_b();
template <>
inline Fq curve_b<Fq>() { return fq_std(3); }
template <>
inline Fq2 curve_b<Fq2>() {
    // 3 / (9 + u) = 19485874751759354771024239261021720505790618469301721065564631296452457478373
    //             + 266929791119991161246907387137283842545076965332900288569378510910307636690 u
    static const uint32_t a[8] = {0x24a138e5u, 0x3267e6dcu, 0x59dbefa3u, 0xb5b4c5e5u, 0x1be06ac3u, 0x81be1899u, 0xceb8aaaeu, 0x2b149d40u};
    static const uint32_t b[8] = {0x85c315d2u, 0xe4a2bd06u, 0xe52d1852u, 0xa74fa084u, 0xeed8fdf4u, 0xcd2cafadu, 0x3af0fed4u, 0x009713b0u};
    return Fq2{fq_std(a), fq_std(b)};
}

// *d_err <- the lowest index in d_pts[0, n) that is not a point of the curve, NO_BAD_POINT when there is none (enqueued on s)
template <class F>
inline void launch_point_check(uint32_t *d_err, const Affine<F> *d_pts, uint64_t n, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(d_err, 0xFF, 4, s));
    if (n) ZK_LAUNCH(k_point_check<F>, dim3(nblocks(n, 256)), dim3(256), 0, s, d_err, d_pts, n, curve_b<F>());
    ZK_LAUNCH_OK("point check");
}

}   // namespace zk
