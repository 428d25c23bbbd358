// Synthetic point tables for benchmarks and full-size parity checks:
// P_i = P0 + i*Q, affine Montgomery, generated on the GPU — 2^22..2^24 valid, distinct curve
// points in milliseconds.  With P0 = k0*G, Q = kq*G every discrete log is known, so an MSM
// over the table is checkable in Fr alone (sum s_i*(k0+i*kq)) at sizes no CPU oracle reaches.
// Pass 1: each lane jumps to its segment start by double-and-add on the index, then walks
// the chain with mixed adds.  Pass 2: XYZZ -> affine with one Fermat inversion per segment
// (Montgomery's batch-inversion trick over the segment's ZZ*ZZZ products).
#include "kernels.hpp"
#include "hipcheck.hpp"
#include "devmem.hpp"

namespace zk {

#define CHAIN_SEG 64u

template <class F>
__global__ __launch_bounds__(64) void k_chain_walk(XYZZ<F> *tmp, Affine<F> P0, Affine<F> Q, uint64_t n) {
    uint64_t lo = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * CHAIN_SEG;
    if (lo >= n) return;
    XYZZ<F> acc = XYZZ<F>::inf();
    for (int bit = 63 - __clzll(lo | 1ull); bit >= 0; bit--) {
        acc = dbl(acc);
        if ((lo >> bit) & 1ull) madd(acc, Q);
    }
    madd(acc, P0);
    uint64_t hi = lo + CHAIN_SEG < n ? lo + CHAIN_SEG : n;
    for (uint64_t i = lo; i < hi; i++) {
        store_el(&tmp[i].x, acc.x); store_el(&tmp[i].y, acc.y); store_el(&tmp[i].zz, acc.zz); store_el(&tmp[i].zzz, acc.zzz);
        madd(acc, Q);
    }
}

template <class F>
__global__ __launch_bounds__(64) void k_chain_normalize(Affine<F> *out, const XYZZ<F> *tmp, F *pref, uint64_t n) {
    uint64_t lo = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * CHAIN_SEG;
    if (lo >= n) return;
    uint64_t hi = lo + CHAIN_SEG < n ? lo + CHAIN_SEG : n;
    F acc = F::one();
    for (uint64_t i = lo; i < hi; i++) {
        store_el(&pref[i], acc);
        F t = F::mul(load_el(&tmp[i].zz), load_el(&tmp[i].zzz));
        if (!t.is_zero()) acc = F::mul(acc, t);          // infinity in the chain: skipped
    }
    F inv = F::inv(acc);
    for (uint64_t i = hi; i-- > lo;) {
        F zz = load_el(&tmp[i].zz), zzz = load_el(&tmp[i].zzz);
        F t = F::mul(zz, zzz);
        if (t.is_zero()) {
            store_el(&out[i].x, F::zero()); store_el(&out[i].y, F::zero());
            continue;
        }
        F ii = F::mul(inv, load_el(&pref[i]));                // 1/(zz*zzz)
        inv = F::mul(inv, t);
        store_el(&out[i].x, F::mul(load_el(&tmp[i].x), F::mul(ii, zzz)));   // X/ZZ
        store_el(&out[i].y, F::mul(load_el(&tmp[i].y), F::mul(ii, zz)));    // Y/ZZZ
    }
}

template <class F>
static void chain(Affine<F> *d_out, XYZZ<F> *d_tmp, F *d_pref, const Affine<F> &P0, const Affine<F> &Q, uint64_t n, hipStream_t s) {
    uint64_t segs = (n + CHAIN_SEG - 1) / CHAIN_SEG;
    uint32_t blocks = (uint32_t)((segs + 63) / 64);
    ZK_LAUNCH(k_chain_walk<F>, dim3(blocks), dim3(64), 0, s, d_tmp, P0, Q, n);
    ZK_LAUNCH(k_chain_normalize<F>, dim3(blocks), dim3(64), 0, s, d_out, (const XYZZ<F> *)d_tmp, d_pref, n);
    ZK_LAUNCH_OK("synthetic chain");
}

// Batch fixed-base multiplication out[i] = k_i * B (a trapdoor-valid zkey is nothing but
// five such batches over the evaluations A_i(tau), B_i(tau), ... computed in Fr).  One lane per
// scalar, plain double-and-add over all 256 bits (no table: 5 x 2^20 points take well under a second),
// then the same batched normalisation as the chains.  k_i = 0 gives the all-zero infinity encoding.
template <class F>
__global__ __launch_bounds__(64) void k_fixed_base(XYZZ<F> *tmp, Affine<F> B, const uint32_t *scalars, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t k[8];
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = scalars[i * 8 + j];
    XYZZ<F> acc = XYZZ<F>::inf();
    for (int bit = 255; bit >= 0; bit--) {
        acc = dbl(acc);
        if ((k[bit >> 5] >> (bit & 31)) & 1u) madd(acc, B);
    }
    store_el(&tmp[i].x, acc.x); store_el(&tmp[i].y, acc.y); store_el(&tmp[i].zz, acc.zz); store_el(&tmp[i].zzz, acc.zzz);
}
template <class F>
static void fixed_base(Affine<F> *d_out, XYZZ<F> *d_tmp, F *d_pref, const Affine<F> &B, const uint32_t *d_scalars, uint64_t n, hipStream_t s) {
    ZK_LAUNCH(k_fixed_base<F>, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, s, d_tmp, B, d_scalars, n);
    uint64_t segs = (n + CHAIN_SEG - 1) / CHAIN_SEG;
    ZK_LAUNCH(k_chain_normalize<F>, dim3((uint32_t)((segs + 63) / 64)), dim3(64), 0, s, d_out, (const XYZZ<F> *)d_tmp, d_pref, n);
    ZK_LAUNCH_OK("fixed-base batch");
}
void launch_fixed_base_g1(G1Affine *d_out, G1XYZZ *d_tmp, Fq *d_pref, const G1Affine &B, const uint32_t *d_scalars, uint64_t n, hipStream_t s) {
    fixed_base<Fq>(d_out, d_tmp, d_pref, B, d_scalars, n, s);
}
void launch_fixed_base_g2(G2Affine *d_out, G2XYZZ *d_tmp, Fq2 *d_pref, const G2Affine &B, const uint32_t *d_scalars, uint64_t n, hipStream_t s) {
    fixed_base<Fq2>(d_out, d_tmp, d_pref, B, d_scalars, n, s);
}

// XYZZ -> affine (all-zero for infinity) of n points another kernel left in d_tmp: the chains' batched normalisation
void launch_normalize_g1(G1Affine *d_out, const G1XYZZ *d_tmp, Fq *d_pref, uint64_t n, hipStream_t s) {
    const uint64_t segs = (n + CHAIN_SEG - 1) / CHAIN_SEG;
    if (segs) ZK_LAUNCH(k_chain_normalize<Fq>, dim3((uint32_t)((segs + 63) / 64)), dim3(64), 0, s, d_out, d_tmp, d_pref, n);
    ZK_LAUNCH_OK("normalize g1");
}
void launch_normalize_g2(G2Affine *d_out, const G2XYZZ *d_tmp, Fq2 *d_pref, uint64_t n, hipStream_t s) {
    const uint64_t segs = (n + CHAIN_SEG - 1) / CHAIN_SEG;
    if (segs) ZK_LAUNCH(k_chain_normalize<Fq2>, dim3((uint32_t)((segs + 63) / 64)), dim3(64), 0, s, d_out, d_tmp, d_pref, n);
    ZK_LAUNCH_OK("normalize g2");
}

void launch_chain_g1(G1Affine *d_out, G1XYZZ *d_tmp, Fq *d_pref, const G1Affine &P0, const G1Affine &Q, uint64_t n, hipStream_t s) {
    chain<Fq>(d_out, d_tmp, d_pref, P0, Q, n, s);
}
void launch_chain_g2(G2Affine *d_out, G2XYZZ *d_tmp, Fq2 *d_pref, const G2Affine &P0, const G2Affine &Q, uint64_t n, hipStream_t s) {
    chain<Fq2>(d_out, d_tmp, d_pref, P0, Q, n, s);
}

}   // namespace zk
