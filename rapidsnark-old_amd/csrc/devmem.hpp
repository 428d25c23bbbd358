// Device-side moves of field elements and points between HBM and registers (and, for the scans over Fr, between the lanes
// of a wave), and the per-lane double-and-add over them: the one definition every kernel file uses (msm_*.hip, ntt.hip,
// nttpair.hip, fieldops.hip, synth.hip, r1cs.hip, setup.hip, ptau_prepare.hip, kzg.hip, frscan.hip).  The plain 8 x 32-bit forms of field.hpp / curve.hpp only: msm_lanes.hpp's Reg<>-converting
// load_affine / load_xyzz / store_xyzz*, its load_row_el and the twiddle loaders of ntt.hip / nttpair.hip stay with
// their kernels.
#pragma once
#include "field.hpp"
#include "curve.hpp"

namespace zk {

// 32-byte elements move as two 16-byte (dwordx4) accesses per lane: fully coalesced.  p must be 16-byte aligned (every
// hipMalloc'ed table of Fr / Fq / points is).
template <class F>
__device__ __forceinline__ F load_el(const F *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    uint4 lo = q[0], hi = q[1];
    F r;
    r.v[0] = lo.x; r.v[1] = lo.y; r.v[2] = lo.z; r.v[3] = lo.w;
    r.v[4] = hi.x; r.v[5] = hi.y; r.v[6] = hi.z; r.v[7] = hi.w;
    return r;
}
template <class F>
__device__ __forceinline__ void store_el(F *p, const F &r) {
    uint4 *q = reinterpret_cast<uint4 *>(p);
    q[0] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
    q[1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
}
__device__ __forceinline__ Fq2 load_el(const Fq2 *p) { return Fq2{load_el(&p->a), load_el(&p->b)}; }
__device__ __forceinline__ void store_el(Fq2 *p, const Fq2 &r) {
    store_el(&p->a, r.a);
    store_el(&p->b, r.b);
}

// ---- what the tiers of a scan over Fr share (kzg.hip: division by X - z; frscan.hip: running products)
// a's value in the lane d places up / down the wave (the lane's own where there is none)
__device__ __forceinline__ Fr shfl_down_fr(const Fr &a, uint32_t d) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = __shfl_down(a.v[i], d, 64);
    return r;
}
__device__ __forceinline__ Fr shfl_up_fr(const Fr &a, uint32_t d) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = __shfl_up(a.v[i], d, 64);
    return r;
}
// A wave-uniform element (a weight, a sum another workgroup left) loaded into VECTOR registers and kept there: the scalar
// file is what the products' carry chains and constants fill, and uniform operands held in it spilled
__device__ __forceinline__ Fr load_uniform(const Fr *p) {
    Fr r = load_el(p);
#pragma unroll
    for (int i = 0; i < 8; i++) __asm__ volatile("" : "+v"(r.v[i]));
    return r;
}
// elements [lo, lo + cnt) of n are this lane's, seg a lane; first_lane: the workgroup's first lane in the grid
__device__ __forceinline__ uint32_t lane_span(uint64_t &lo, uint64_t first_lane, uint64_t n, uint32_t seg) {
    lo = (first_lane + threadIdx.x) * seg;
    if (lo >= n) return 0;
    return n - lo < seg ? (uint32_t)(n - lo) : seg;
}

// whole points, coordinate by coordinate (no conversion: the table's form is the registers' form)
template <class F>
__device__ __forceinline__ Affine<F> load_pt(const Affine<F> *p) {
    return Affine<F>{load_el(&p->x), load_el(&p->y)};
}
template <class F>
__device__ __forceinline__ XYZZ<F> load_pt(const XYZZ<F> *p) {
    return XYZZ<F>{load_el(&p->x), load_el(&p->y), load_el(&p->zz), load_el(&p->zzz)};
}
template <class F>
__device__ __forceinline__ void store_pt(XYZZ<F> *p, const XYZZ<F> &v) {
    store_el(&p->x, v.x);
    store_el(&p->y, v.y);
    store_el(&p->zz, v.zz);
    store_el(&p->zzz, v.zzz);
}

// k P for an affine P and a 256-bit magnitude k in standard form, by double-and-add with mixed adds over the BIT LENGTH
// of k: a wave of +-1 and +-2^i scalars does one or a few steps and never waits for a 254-bit one.  The magnitude is
// shifted so that its top bit is bit 255 and the loop reads bit 31 of the top word: no run-time indexed register array.
// P = infinity gives infinity (madd ignores such an operand and dbl keeps infinity; the early return only saves the loop).
template <class F>
__device__ __forceinline__ XYZZ<F> scalar_mul_affine(const Affine<F> &P, const Fr &scalar) {
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; i++) k[i] = scalar.v[i];
    int bl = 0;
#pragma unroll
    for (int i = 7; i >= 0; i--)
        if (bl == 0 && k[i]) bl = 32 * i + 32 - __clz(k[i]);
    int s = 256 - bl;
    while (s >= 32) {
#pragma unroll
        for (int i = 7; i > 0; i--) k[i] = k[i - 1];
        k[0] = 0;
        s -= 32;
    }
    if (s) {
#pragma unroll
        for (int i = 7; i > 0; i--) k[i] = (k[i] << s) | (k[i - 1] >> (32 - s));
        k[0] <<= s;
    }
    XYZZ<F> acc = XYZZ<F>::inf();
    if (P.is_inf()) return acc;
    for (int i = 0; i < bl; i++) {
        acc = dbl(acc);
        if (k[7] >> 31) madd(acc, P);
#pragma unroll
        for (int q = 7; q > 0; q--) k[q] = (k[q] << 1) | (k[q - 1] >> 31);
        k[0] <<= 1;
    }
    return acc;
}

}   // namespace zk
