// Pippenger multi-scalar multiplication over BN254 G1 / G2 for gfx950 — replaces ffiasm
// ParallelMultiexp behind Curve::multiMulByScalar (call sites src/groth16.cpp:173,183,190,197,204).
//
// MI355X design (ffiasm keeps nThreads x 2^c per-thread bucket arrays; that makes no sense here):
//   1. msm_sort.hip — k_msm_digits : signed c-bit digits of every scalar, window-major 32-bit codes (bit 31 = sign, low bits =
//      bucket key; with window-precomputed tables every window shares ONE bucket set, and a batch of B scalar vectors
//      — several small proofs in one set of launches — gets one set per vector)
//   2. msm_sort.hip — k_bin_count / k_bin_scatter : partition the codes by their high key bits into <= 256 bins (LDS-staged);
//      k_bin_count_lds / k_bin_scatter_lds : counting sort of every bin with its histogram in LDS; k_scan_* between
//      (1-2 run ONCE per scalar vector: the witness sort is shared by MSM A, B1, B2, C,
//       which the reference recomputes four times, src/groth16.cpp:183-204)
//   3. msm_accum.hip — k_msm_accum_l1 / _l1_g2s : load-balanced segmented accumulation — every lane mixed-adds an equal share of
//      the bucket-sorted list into XYZZ accumulators in VGPRs (next point prefetched; G2 split across lane pairs);
//      k_msm_accum_pair / _wave : runs cut by chunk edges are merged by wave-parallel segmented scans, level by level
//   4. msm_reduce.hip — bucket reduction sum_k (k+1)*B_k per bucket set: k_msm_reduce_chunks / _tree (chunked running sums + LDS tree)
//      for large sets, k_msm_reduce_bits_block / _top (one binary tree of bit sums, c-1 additions deep) for small ones
//   5. host (host_tail.cpp): the serial rest — Horner over the windows (plain tables) or over the c bit sums, and the
//      final assembly: serial doublings are 30x faster on one CPU core than on one GPU lane.
// Signed digits halve the bucket count; scalars are reduced mod r first so any 256-bit
// input is accepted like the reference's raw-byte interface.
// msm_tables.hip prepares the point tables (internal Montgomery form, window pre-computation).
//
// This header: the device helpers that steps 3, 4 and the table kernels share (the sort needs none of them).
#pragma once
#include "kernels.hpp"
#include "common.hpp"
#include "field29.hpp"
#include "curve29.hpp"
#include "devmem.hpp"

namespace zk {

// a table row is read exactly once per MSM: ZK_L1_NT_GATHER (measurement builds) loads it with the non-temporal hint
template <class F>
__device__ __forceinline__ F load_row_el(const F *p) {
#if defined(ZK_L1_NT_GATHER)
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const v4u *q = reinterpret_cast<const v4u *>(p);
    v4u lo = __builtin_nontemporal_load(q), hi = __builtin_nontemporal_load(q + 1);
    F r;
    r.v[0] = lo.x; r.v[1] = lo.y; r.v[2] = lo.z; r.v[3] = lo.w;
    r.v[4] = hi.x; r.v[5] = hi.y; r.v[6] = hi.z; r.v[7] = hi.w;
    return r;
#else
    return load_el(p);
#endif
}

// Register representation of the MSM kernels: 9x29-bit signed limbs (field29.hpp).  HBM keeps
// canonical 256-bit words of the SAME (2^261) Montgomery form; Reg<> converts at load/store.
template <class FM> struct Reg;
template <> struct Reg<Fq> {
    typedef Fq29 type;
    __device__ __forceinline__ static Fq29 load(const Fq *p) { return Fq29::load(load_el(p)); }
    __device__ __forceinline__ static void store(Fq *p, const Fq29 &r) { store_el(p, Fq29::store(r)); }
    __device__ __forceinline__ static void store256(Fq *p, const Fq29 &r) { store_el(p, Fq29::to_mont256(r)); }
};
template <> struct Reg<Fq2> {
    typedef Fq2r type;
    __device__ __forceinline__ static Fq2r load(const Fq2 *p) { return Fq2r{Reg<Fq>::load(&p->a), Reg<Fq>::load(&p->b)}; }
    __device__ __forceinline__ static void store(Fq2 *p, const Fq2r &r) { Reg<Fq>::store(&p->a, r.a); Reg<Fq>::store(&p->b, r.b); }
    __device__ __forceinline__ static void store256(Fq2 *p, const Fq2r &r) { Reg<Fq>::store256(&p->a, r.a); Reg<Fq>::store256(&p->b, r.b); }
};
#define REGF typename Reg<F>::type

template <class F>
__device__ __forceinline__ Affine<REGF> load_affine(const Affine<F> *p) {
    return Affine<REGF>{Reg<F>::load(&p->x), Reg<F>::load(&p->y)};
}
template <class F>
__device__ __forceinline__ XYZZ<REGF> load_xyzz(const XYZZ<F> *p) {
    return XYZZ<REGF>{Reg<F>::load(&p->x), Reg<F>::load(&p->y), Reg<F>::load(&p->zz), Reg<F>::load(&p->zzz)};
}
template <class F>
__device__ __forceinline__ void store_xyzz(XYZZ<F> *p, const XYZZ<REGF> &v) {
    Reg<F>::store(&p->x, v.x);
    Reg<F>::store(&p->y, v.y);
    Reg<F>::store(&p->zz, v.zz);
    Reg<F>::store(&p->zzz, v.zzz);
}
// final window sums leave the device in the zkey's own 2^256 Montgomery form
template <class F>
__device__ __forceinline__ void store_xyzz_mont256(XYZZ<F> *p, const XYZZ<REGF> &v) {
    Reg<F>::store256(&p->x, v.x);
    Reg<F>::store256(&p->y, v.y);
    Reg<F>::store256(&p->zz, v.zz);
    Reg<F>::store256(&p->zzz, v.zzz);
}

template <class F>
__device__ __forceinline__ Affine<REGF> to_reg_affine(const Affine<F> &w);
template <>
__device__ __forceinline__ Affine<Fq29> to_reg_affine<Fq>(const Affine<Fq> &w) {
    return Affine<Fq29>{Fq29::load(w.x), Fq29::load(w.y)};
}
template <>
__device__ __forceinline__ Affine<Fq2r> to_reg_affine<Fq2>(const Affine<Fq2> &w) {
    return Affine<Fq2r>{Fq2r{Fq29::load(w.x.a), Fq29::load(w.x.b)}, Fq2r{Fq29::load(w.y.a), Fq29::load(w.y.b)}};
}

// Bucket sums, partial sums and reduction scratch live in HBM as the ACCUMULATORS' OWN LIMBS (G1Acc /
// G2Acc, kernels.hpp): 36 (72) int32, moved as nine 16-byte accesses per lane.  Storing them as canonical
// 256-bit words cost ~95 instructions per coordinate (exact reduction, conditional +p, limb -> word
// packing) in the most divergent spot of the level-1 loop — a bucket run ends in ~46 % of a wave's
// iterations (64 lanes, ~104 entries per bucket), and the other 63 lanes wait — and the same again to
// unpack at every load.  Lazy values are valid operands everywhere (field29.hpp); infinity stays the
// all-zero pattern.
__device__ __forceinline__ void load36(int32_t *dst, const int32_t *src) {
    const uint4 *q = reinterpret_cast<const uint4 *>(src);
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const uint4 t = q[i];
        dst[4 * i] = (int32_t)t.x; dst[4 * i + 1] = (int32_t)t.y; dst[4 * i + 2] = (int32_t)t.z; dst[4 * i + 3] = (int32_t)t.w;
    }
}
__device__ __forceinline__ void store36(int32_t *dst, const int32_t *src) {
    uint4 *q = reinterpret_cast<uint4 *>(dst);
#pragma unroll
    for (int i = 0; i < 9; i++) q[i] = make_uint4((uint32_t)src[4 * i], (uint32_t)src[4 * i + 1], (uint32_t)src[4 * i + 2], (uint32_t)src[4 * i + 3]);
}
__device__ __forceinline__ XYZZ<Fq29> unpack36(const int32_t *w) {
    XYZZ<Fq29> v;
#pragma unroll
    for (int i = 0; i < 9; i++) { v.x.l[i] = w[i]; v.y.l[i] = w[9 + i]; v.zz.l[i] = w[18 + i]; v.zzz.l[i] = w[27 + i]; }
    return v;
}
__device__ __forceinline__ void pack36(int32_t *w, const Fq29 &x, const Fq29 &y, const Fq29 &zz, const Fq29 &zzz) {
#pragma unroll
    for (int i = 0; i < 9; i++) { w[i] = x.l[i]; w[9 + i] = y.l[i]; w[18 + i] = zz.l[i]; w[27 + i] = zzz.l[i]; }
}

// Lane model of the merge / reduction kernels: one lane per G1 element; a lane PAIR per G2 element
// (even lane = real components, odd lane = imaginary components, curve29.hpp Fq2s) — half the
// registers per lane, twice the lanes, no spills.
template <class F> struct LaneModel;
template <> struct LaneModel<Fq> {
    static constexpr uint32_t LPE = 1;      // lanes per element
    typedef Fq29 R;
    typedef G1Acc Mem;
    __device__ __forceinline__ static XYZZ<R> load(const G1Acc *p) {
        int32_t w[36];
        load36(w, p->l);
        return unpack36(w);
    }
    __device__ __forceinline__ static void store(G1Acc *p, const XYZZ<R> &v) {
        int32_t w[36];
        pack36(w, v.x, v.y, v.zz, v.zzz);
        store36(p->l, w);
    }
    __device__ __forceinline__ static void store256(G1XYZZ *p, const XYZZ<R> &v) { store_xyzz_mont256(p, v); }
};
template <> struct LaneModel<Fq2> {
    static constexpr uint32_t LPE = 2;
    typedef Fq2s R;
    typedef G2Acc Mem;
    __device__ __forceinline__ static XYZZ<R> load(const G2Acc *p) {      // memory: [component][x | y | zz | zzz][limb]
        int32_t w[36];
        load36(w, p->l + 36 * (threadIdx.x & 1u));
        const XYZZ<Fq29> t = unpack36(w);
        return XYZZ<R>{R{t.x}, R{t.y}, R{t.zz}, R{t.zzz}};
    }
    __device__ __forceinline__ static void store(G2Acc *p, const XYZZ<R> &v) {
        int32_t w[36];
        pack36(w, v.x.v, v.y.v, v.zz.v, v.zzz.v);
        store36(p->l + 36 * (threadIdx.x & 1u), w);
    }
    __device__ __forceinline__ static void store256(G2XYZZ *p, const XYZZ<R> &v) {   // x.a x.b y.a y.b zz.a zz.b zzz.a zzz.b, canonical words
        Fq *c = reinterpret_cast<Fq *>(p) + (threadIdx.x & 1u);
        Reg<Fq>::store256(c, v.x.v); Reg<Fq>::store256(c + 2, v.y.v); Reg<Fq>::store256(c + 4, v.zz.v); Reg<Fq>::store256(c + 6, v.zzz.v);
    }
};
#define ACCMEM typename LaneModel<F>::Mem

static inline bool skip_followups_probe() {      // ZKHIP_PROBE_SKIP_FOLLOWUPS (-DZK_PROBES builds only, WRONG results): no partial merges, no bucket reductions
    static const bool skip = probe_env("ZKHIP_PROBE_SKIP_FOLLOWUPS") != nullptr;
    return skip;
}

}   // namespace zk
