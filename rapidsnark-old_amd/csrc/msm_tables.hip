// MSM point tables (overview: msm_lanes.hpp): conversion to the internal Montgomery form and window pre-computation.
#include "hipcheck.hpp"
#include "msm_lanes.hpp"

namespace zk {

// zkey tables arrive as x*2^256; convert every coordinate to x*2^261 in place (once, at create)
__global__ __launch_bounds__(256) void k_fq_to_internal(Fq *coords, uint64_t n) {
    uint64_t st = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += st)
        store_el(coords + i, Fq29::store(Fq29::from_mont256(load_el(coords + i))));
}
void launch_fq_to_internal(Fq *coords, uint64_t n, hipStream_t s) {
    if (!n) return;
    uint64_t g = (n + 255) / 256;
    if (g > 4096) g = 4096;
    ZK_LAUNCH(k_fq_to_internal, dim3((uint32_t)g), dim3(256), 0, s, coords, n);
    ZK_LAUNCH_OK("fq_to_internal");
}

// ---------------------------------------------------------------- window pre-computation
// T[j*n + i] = 2^(c*j) * P_i for j < W, affine, resident in HBM (x W table memory — what 288 GB
// are for).  Every window then adds into the SAME bucket set, so the bucket reduction is paid
// once and the window can grow to c = 20: 13 instead of 16 additions per point.
template <class F>
__global__ __launch_bounds__(128) void k_precomp_walk(XYZZ<F> *tmp, const Affine<F> *pts, uint64_t n, uint32_t c, uint32_t W) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typedef REGF FR;
    XYZZ<FR> acc = XYZZ<FR>::from_affine(load_affine(pts + i));
    for (uint32_t j = 1; j < W; j++) {
        for (uint32_t k = 0; k < c; k++) acc = dbl(acc);
        store_xyzz(tmp + (uint64_t)(j - 1) * n + i, acc);
    }
}
// XYZZ -> affine over segments of 64 points with one Fermat inversion per segment
template <class F>
__global__ __launch_bounds__(64) void k_precomp_normalize(Affine<F> *out, const XYZZ<F> *tmp, F *pref, uint64_t total) {
    const uint64_t lo = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 64;
    if (lo >= total) return;
    const uint64_t hi = lo + 64 < total ? lo + 64 : total;
    typedef REGF FR;
    FR acc = FR::one();
    for (uint64_t i = lo; i < hi; i++) {
        Reg<F>::store(pref + i, acc);
        FR t = FR::mul(Reg<F>::load(&tmp[i].zz), Reg<F>::load(&tmp[i].zzz));
        if (!t.is_zero()) acc = FR::mul(acc, t);          // infinity (zz = 0): skipped
    }
    FR inv = FR::inv(acc);
    for (uint64_t i = hi; i-- > lo;) {
        FR zz = Reg<F>::load(&tmp[i].zz), zzz = Reg<F>::load(&tmp[i].zzz);
        FR t = FR::mul(zz, zzz);
        if (t.is_zero()) {
            Reg<F>::store(&out[i].x, FR::zero());
            Reg<F>::store(&out[i].y, FR::zero());
            continue;
        }
        FR ii = FR::mul(inv, Reg<F>::load(pref + i));     // 1/(zz*zzz)
        inv = FR::mul(inv, t);
        Reg<F>::store(&out[i].x, FR::mul(Reg<F>::load(&tmp[i].x), FR::mul(ii, zzz)));   // X/ZZ
        Reg<F>::store(&out[i].y, FR::mul(Reg<F>::load(&tmp[i].y), FR::mul(ii, zz)));    // Y/ZZZ
    }
}
template <class F>
static void precomp_table(Affine<F> *table, XYZZ<F> *tmp, F *pref, uint64_t n, MsmPlan p, hipStream_t s) {
    if (!n || p.W < 2) return;
    ZK_LAUNCH(k_precomp_walk<F>, dim3((uint32_t)((n + 127) / 128)), dim3(128), 0, s, tmp, (const Affine<F> *)table, n, p.c, p.W);
    const uint64_t total = (uint64_t)(p.W - 1) * n, segs = (total + 63) / 64;
    ZK_LAUNCH(k_precomp_normalize<F>, dim3((uint32_t)((segs + 63) / 64)), dim3(64), 0, s, table + n, (const XYZZ<F> *)tmp, pref, total);
    ZK_LAUNCH_OK("window pre-computation");
}
// (a table with a row per second window is a table with a row per window of twice the width)
static MsmPlan table_plan(MsmPlan p) {
    if (p.precomp > 1) { p.W = msm_table_rows(p); p.c *= p.precomp; }
    return p;
}
void launch_msm_precomp_g1(G1Affine *table, G1XYZZ *tmp, Fq *pref, uint64_t n, MsmPlan p, hipStream_t s) { precomp_table<Fq>(table, tmp, pref, n, table_plan(p), s); }
void launch_msm_precomp_g2(G2Affine *table, G2XYZZ *tmp, Fq2 *pref, uint64_t n, MsmPlan p, hipStream_t s) { precomp_table<Fq2>(table, tmp, pref, n, table_plan(p), s); }

}   // namespace zk
