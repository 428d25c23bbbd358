// PLONK round 3 (include/zkhip.h, section "PLONK quotient and coset transforms"): transforms on a coset g H' of the roots
// of unity, and the quotient t = num / Z_H of a three-column PLONK proof from coset evaluations.  Nothing in the reference
// corresponds to it (it proves Groth16 only); the counterpart is round 3 of snarkjs's PLONK prover.  DESIGN.md section 29
// states the identities, the count of products and what was measured.
//
// With n = 2^log_n, m = 4n, x_i = g w_m^i (w_m zk_fr_ntt's root for m, w_m^4 = w the root for n) and Z_H = X^n - 1:
//     num = q_L a + q_R b + q_M a b + q_O c + q_C + PI
//         + alpha [ (a + beta X + gamma)(b + beta k1 X + gamma)(c + beta k2 X + gamma) z(X)
//                 - (a + beta s1 + gamma)(b + beta s2 + gamma)(c + beta s3 + gamma) z(w X) ]
//         + alpha^2 (z - 1) L1(X),                                  L1 = (X^n - 1) / (n (X - 1)) = (1 + X + .. + X^(n-1)) / n
//     t(x_i) = num(x_i) / Z_H(x_i),  Z_H(x_i) = g^n w_4^(i mod 4) - 1: four values, inverted on the host;  z(w x_i) = z(x_(i+4 mod m)).
// The transforms are nttpair.hip's passes, untouched (launch_ntt_plain over a batch; below its smallest size and at 2^28
// ntt.hip's radix-2 passes, as zk_fr_ntt).  New here: k_coset_load (standard rows -> rows times g^i in the transforms' form,
// zero-filled to m), k_coset_store (its mirror image, with the length of the result) and k_plonk_quotient.
//
// Lane map of all three: T lanes in the grid (a multiple of 256), lane l takes the points l, l + T, l + 2T, .. : `seg` of them
// (ZKHIP_QUOT_SEG, read at every call).  Neighbouring lanes touch neighbouring rows (coalesced), a lane's i mod 4 never
// changes (its 1 / Z_H is one value), and its power of g or of w_m moves on by ONE product a point (by g^T, w_m^T: the
// host's).  The starting power comes from the bits of l over a host-made record of the powers g^(2^b) (lanepow.hpp, as
// ScanConsts::wtab of frscan.hip).  Which products are formed depends on indices only and the arithmetic is exact: the bytes
// depend neither on seg nor on scheduling.  No LDS but four words for k_coset_store's length, no atomics.
//
// Forms.  I/O is STANDARD.  Everything between k_coset_load and k_coset_store is the transforms' own form: canonical words of
// x 2^261, field29.hpp's nine 29-bit limbs in registers (Fr29::mul(x, y) = x y / 2^261); no conversion between a
// transform and the quotient kernel.
#include <mutex>
#include <memory>
#include "hiputil.hpp"
#include "devmem.hpp"
#include "ptengine.hpp"
#include "field29.hpp"
#include "lanepow.hpp"
#include "plonk_internal.hpp"

namespace {

constexpr uint32_t QT_WG = 256;
constexpr uint32_t DEFAULT_SEG = 16, MAX_SEG = 4096;  // the default: profiles/plonk_quotient_timing.txt, the best call at log_n 18, 1.3 % behind the best at 22
constexpr uint32_t MAX_LOG_M = 28;
constexpr uint32_t RES_VECS = 9, EXT_VECS = 5, MAX_LOAD = 9;
enum { V_QL, V_QR, V_QM, V_QO, V_QC, V_S1, V_S2, V_S3, V_L1 };      // the resident extensions
enum { V_A, V_B, V_C, V_Z, V_PI };                                    // a proof's

typedef Fr29 F;

// ---------------------------------------------------------------- device
// A lane's power of a base: p_l = seed * base^l, moved on by pw.step = base^T a point (lanepow.hpp).  Words as the kernels
// multiply them: x 2^261 (the host makes them, pow_consts below)
struct PowConsts {
    Fr seed;
    PowTab pw;
};

__device__ __forceinline__ F ld(const Fr *p) { return F::load(load_el(p)); }
// devmem.hpp's load_uniform for the 29-bit form: a wave-uniform element pinned in VECTOR registers
__device__ __forceinline__ F ld_uniform(const Fr *p) {
    F r = ld(p);
#pragma unroll
    for (int i = 0; i < 9; i++) __asm__ volatile("" : "+v"(r.l[i]));
    return r;
}
__device__ __forceinline__ F lane_power(const PowConsts *k, uint64_t l) {
    F p = ld(&k->seed);
#pragma unroll 1
    for (uint32_t b = 0; b < POW_TAB && (l >> b); b++)
        if ((l >> b) & 1) p = F::mul(p, ld(k->pw.tab + b));
    return p;
}

// out[v][i] = src[v][i] g^i for i < n_in[v], 0 up to m, in the transforms' form.  src holds standard rows or rows in that form
// already: the seed says which (pow_consts).  src[v] NULL: every row is *fill.
// unit: g = 1, no power is kept
struct LoadArgs {
    const Fr *src[MAX_LOAD];
    uint64_t n_in[MAX_LOAD];
    const Fr *fill;
    Fr *out;
    uint64_t stride, m;
    uint32_t seg, unit;
    const PowConsts *k;
};
__global__ __launch_bounds__(QT_WG) void k_coset_load(LoadArgs A) {
    const uint64_t T = (uint64_t)gridDim.x * QT_WG, l = (uint64_t)blockIdx.x * QT_WG + threadIdx.x;
    if (l >= A.m) return;
    const uint32_t v = blockIdx.y;
    const Fr *src = A.src[v];
    const uint64_t n_in = A.n_in[v];
    Fr *out = A.out + v * A.stride;
    F p = A.unit ? ld(&A.k->seed) : lane_power(A.k, l);
    const F step = ld_uniform(&A.k->pw.step);
#pragma unroll 1
    for (uint32_t k = 0; k < A.seg; k++) {
        const uint64_t i = l + k * T;
        if (i >= A.m) break;
        if (i < n_in) {
            const F x = ld(src ? src + i : A.fill);
            store_el(out + i, F::store(F::mul(x, p)));
        } else {
            store_el(out + i, Fr::zero());
        }
        if (!A.unit) p = F::mul(p, step);
    }
}

// out[i] = in[i] g^(-i) in standard form (unit: g = 1); hi[block] = one more than the highest i of the block's lanes with
// out[i] != 0, 0 when it has none (hi NULL: not wanted).  The host takes the largest: no atomics, nothing depends on order
struct StoreArgs {
    const Fr *in;
    Fr *out;
    uint32_t *hi;
    uint64_t m;
    uint32_t seg, unit;
    const PowConsts *k;
};
__global__ __launch_bounds__(QT_WG) void k_coset_store(StoreArgs A) {
    __shared__ uint32_t sh[QT_WG / 64];
    const uint64_t T = (uint64_t)gridDim.x * QT_WG, l = (uint64_t)blockIdx.x * QT_WG + threadIdx.x;
    uint32_t top = 0;
    if (l < A.m) {
        F p = A.unit ? ld(&A.k->seed) : lane_power(A.k, l);
        const F step = ld_uniform(&A.k->pw.step);
#pragma unroll 1
        for (uint32_t k = 0; k < A.seg; k++) {
            const uint64_t i = l + k * T;
            if (i >= A.m) break;
            const F o = F::canonical(F::mul(ld(A.in + i), p));
            Fr w;
            F::to_words(w.v, o);
            store_el(A.out + i, w);
            if (!o.is_zero_raw()) top = (uint32_t)i + 1;      // i rises: the last one stands (m <= 2^28)
            if (!A.unit) p = F::mul(p, step);
        }
    }
    if (!A.hi) return;
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
        const uint32_t o = __shfl_xor(top, d, 64);
        top = o > top ? o : top;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = top;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t j = 1; j < QT_WG / 64; j++) top = sh[j] > top ? sh[j] : top;
        A.hi[blockIdx.x] = top;
    }
}

// The constants of one quotient call, words of x 2^261
struct QuotConsts {
    Fr alpha, alpha2, beta, gamma, bk1, bk2;          // bk1 = beta k1, bk2 = beta k2
    Fr zh[4];                                         // 1 / Z_H(x_i) by i mod 4
    PowConsts x;                                      // x_l = g w_m^l, step w_m^T
};
struct QuotArgs {
    const Fr *res;                                    // RES_VECS x m, resident
    const Fr *ext;                                    // EXT_VECS x m (V_PI only when has_pi)
    Fr *t;                                            // m evaluations of t
    uint64_t m;
    uint32_t seg, has_pi;
    const QuotConsts *k;
};
// 22 products a point, in pairs (field29.hpp's run2: two chains of multiply-adds interleaved):
//   a b | beta x         beta k1 x | beta k2 x      beta s1 | beta s2      beta s3 | (z - 1) L1
//   f1 f2 | g1 g2        f3 z | g3 z'               (f1 f2)(f3 z) | (g1 g2)(g3 z')
//   q_L a + q_R b | q_M (a b) + q_O c   (two products each, one reduction each)
//   alpha (P - Q) | alpha^2 ((z - 1) L1)            num / Z_H | x w_m^T
// f_j, g_j: the factors of the permutation term's two products; z' = z(w x_i) = the extension four places on, modulo m
__global__ __launch_bounds__(QT_WG) void k_plonk_quotient(QuotArgs A) {
    const uint64_t T = (uint64_t)gridDim.x * QT_WG, l = (uint64_t)blockIdx.x * QT_WG + threadIdx.x;
    if (l >= A.m) return;
    const QuotConsts *K = A.k;
    const uint64_t m = A.m;
    F x = lane_power(&K->x, l);
    const F zh = ld(K->zh + (l & 3));                 // T is a multiple of 4: i mod 4 = l mod 4 at every point of the lane
    const F alpha = ld_uniform(&K->alpha), alpha2 = ld_uniform(&K->alpha2), beta = ld_uniform(&K->beta), gamma = ld_uniform(&K->gamma);
    const F bk1 = ld_uniform(&K->bk1), bk2 = ld_uniform(&K->bk2), step = ld_uniform(&K->x.pw.step);
#pragma unroll 1
    for (uint32_t k = 0; k < A.seg; k++) {
        const uint64_t i = l + k * T;
        if (i >= m) break;
        const Fr *r = A.res + i, *e = A.ext + i;
        const F a = ld(e + V_A * m), b = ld(e + V_B * m), c = ld(e + V_C * m), z = ld(e + V_Z * m);
        F ab, bx, b1x, b2x, bs1, bs2, bs3, bz;
        F::mul2(ab, a, b, bx, beta, x);
        F::mul2(b1x, bk1, x, b2x, bk2, x);
        const F f1 = F::add(F::add(a, bx), gamma), f2 = F::add(F::add(b, b1x), gamma), f3 = F::add(F::add(c, b2x), gamma);
        F::mul2(bs1, beta, ld(r + V_S1 * m), bs2, beta, ld(r + V_S2 * m));
        F::mul2(bs3, beta, ld(r + V_S3 * m), bz, F::sub(z, F::one()), ld(r + V_L1 * m));
        const F g1 = F::add(F::add(a, bs1), gamma), g2 = F::add(F::add(b, bs2), gamma), g3 = F::add(F::add(c, bs3), gamma);
        F p12, q12, p3, q3, P, Q, G1, G2, aD, T2, t, xn;
        F::mul2(p12, f1, f2, q12, g1, g2);
        F::mul2(p3, f3, z, q3, g3, ld(A.ext + V_Z * m + ((i + 4) & (m - 1))));      // the one index edge: the rotation wraps
        F::mul2(P, p12, p3, Q, q12, q3);
        {
            const F ql = ld(r + V_QL * m), qr = ld(r + V_QR * m), qm = ld(r + V_QM * m), qo = ld(r + V_QO * m);
            F::run2(G1, F::JMulAdd2{ql, a, qr, b}, G2, F::JMulAdd2{qm, ab, qo, c});
        }
        F::mul2(aD, alpha, F::sub(P, Q), T2, alpha2, bz);
        F num = F::add(F::add(G1, G2), F::add(ld(r + V_QC * m), aD));
        num = F::add(num, T2);
        if (A.has_pi) num = F::add(num, ld(e + V_PI * m));
        F::mul2(t, num, zh, xn, x, step);
        store_el(A.t + i, F::store(t));
        x = xn;
    }
}

// ---------------------------------------------------------------- host
uint32_t seg_in_effect() { return (uint32_t)env_number("ZKHIP_QUOT_SEG", DEFAULT_SEG, 1, MAX_SEG, "a number of points per lane from 1 to 4096", ENV_LAX); }

// lanes in the grid for m points at seg a lane: whole workgroups
uint32_t blocks_of(uint64_t m, uint32_t seg) { return nblocks(m, QT_WG * seg); }

// Montgomery (2^256) words -> words of x 2^261, what the 29-bit kernels load
Fr w29(Fr a) {
    for (int i = 0; i < 5; i++) a = Fr::add(a, a);
    return a;
}
Fr raw_one() {
    Fr r = Fr::zero();
    r.v[0] = 1;
    return r;
}

enum PowKind { POW_LOAD_STD, POW_LOAD_INTERNAL, POW_STORE, POW_POINTS };
// the record of one base (Montgomery) for T lanes.  The seeds: a standard row v becomes v g^i 2^261 by one product with
// g^i 2^522; a row in the transforms' form by one with g^i 2^261; a result leaves the form by one with the plain integer
// g^(-i); the points start at g 2^261
PowConsts pow_consts(PowKind kind, Fr base, uint64_t lanes, Fr g = Fr::one()) {
    PowConsts k;
    switch (kind) {
    case POW_LOAD_STD: k.seed = w29(Fr::to_mont(w29(Fr::one()))); break;
    case POW_LOAD_INTERNAL: k.seed = w29(Fr::one()); break;
    case POW_STORE: k.seed = raw_one(); break;
    case POW_POINTS: k.seed = w29(g); break;
    }
    k.pw = pow_tab(base, lanes, w29);
    return k;
}

// One transform size: nttpair.hip's pipeline where it serves the size, else ntt.hip's radix-2 passes (as zk_fr_ntt)
struct Xform {
    uint32_t log = 0;
    bool pipeline = false;
    NttPair pair;
    DevBuf<TwEntry> fwd, inv;
    DevBuf<Fr> coset, ninv;
    NttTables t{};
    void build(uint32_t log_m, hipStream_t s) {
        log = log_m;
        pipeline = ntt_pair_supported(log_m);
        if (pipeline) {
            pair.build(log_m, log_m, 0, s, /*plain=*/true);
            return;
        }
        const uint64_t m = 1ull << log_m;
        fwd.alloc(m > 1 ? m / 2 : 1);
        inv.alloc(m > 1 ? m / 2 : 1);
        coset.alloc(m);
        ninv.alloc(1);
        launch_ntt_build_tables(fwd.p, inv.p, coset.p, ninv.p, log_m, s);
        t = NttTables{log_m, fwd.p, inv.p, coset.p, ninv.p};
    }
    static uint64_t bytes_of(uint32_t log_m) {
        const uint64_t m = 1ull << log_m;
        if (!ntt_pair_supported(log_m)) return m * sizeof(TwEntry) + (m + 1) * sizeof(Fr);
        const uint32_t t = log_m > 11 ? log_m - 11 : 0;
        return 2 * 2048 * sizeof(TwEntry) + ((t ? 2 * m : 0) + (1ull << (log_m - t)) + (t > 11 ? 2ull << t : 0)) * sizeof(Fr);
    }
    // `batch` vectors `stride` apart, natural order in and out; `data` is destroyed.  The result is where the return value
    // points: `out` on the pipeline, `data` on the radix-2 path
    Fr *run(Fr *out, Fr *data, uint64_t stride, uint32_t batch, bool inverse, hipStream_t s) const {
        if (pipeline) {
            launch_ntt_plain(out, data, stride, batch, pair, inverse, s);
            return out;
        }
        const uint64_t m = 1ull << log;
        if (!log) return data;                         // one point: the transform is the identity
        if (inverse) {
            launch_ntt_dif_inverse(data, stride, batch, t, s);
            for (uint32_t v = 0; v < batch; v++) {
                launch_bitrev_permute(data + v * stride, log, s);
                launch_fr_scale_const(data + v * stride, ninv.p, m, s);
            }
        } else {
            for (uint32_t v = 0; v < batch; v++) launch_bitrev_permute(data + v * stride, log, s);
            launch_ntt_dit_forward(data, stride, batch, t, s);
        }
        return data;
    }
};

void launch_load(LoadArgs A, uint32_t batch, hipStream_t s) {
    ZK_LAUNCH(k_coset_load, dim3(blocks_of(A.m, A.seg), batch), dim3(QT_WG), 0, s, A);
    ZK_LAUNCH_OK("coset load");
}

// What a call keeps on the device beside its vectors: the records of the powers and the blocks' lengths
struct CosetWork {
    DevBuf<PowConsts> k;                              // [0] load, [1] store
    DevBuf<uint32_t> hi;
    PowConsts h[2];                                   // the host images: they outlive the copies (the stream is drained before the next call)
    std::vector<uint32_t> hh;
    void size(uint64_t m) {
        if (!k.p) k.alloc(2);
        const uint32_t b = blocks_of(m, 1);
        if (hi.n < b) hi.alloc(b);
    }
    static uint64_t bytes_of(uint64_t m) { return 2 * sizeof(PowConsts) + (uint64_t)blocks_of(m, 1) * 4 + 64; }
};

// One transform on the coset g H' over device pointers and a stream.  Forward: n_in standard rows at `in` -> m standard rows,
// out[i] = p(g w_m^i).  Inverse: m standard rows -> the coefficients.  g, ginv: Montgomery, unit: g = 1.  a, b: two work
// vectors of m; the result is left in `out` (a third vector; `in` may be it).  t_len (may be NULL): one more than the
// highest non-zero row of the result, after the stream was drained for it
void coset_ntt_dev(Fr *out, Fr *a, Fr *b, const Fr *in, uint64_t n_in, const Xform &xf, Fr g, Fr ginv, bool unit, bool inverse, uint32_t seg,
                   CosetWork &w, uint64_t *t_len, hipStream_t s) {
    const uint64_t m = 1ull << xf.log;
    const uint32_t blocks = blocks_of(m, seg);
    const uint64_t lanes = (uint64_t)blocks * QT_WG;
    w.size(m);
    w.h[0] = pow_consts(POW_LOAD_STD, g, lanes);
    w.h[1] = pow_consts(POW_STORE, ginv, lanes);
    HIP_TRY(hipMemcpyAsync(w.k.p, w.h, sizeof w.h, hipMemcpyHostToDevice, s));
    LoadArgs L{};
    L.src[0] = in, L.n_in[0] = n_in, L.out = a, L.stride = m, L.m = m, L.seg = seg, L.unit = (unit || inverse) ? 1u : 0u, L.k = w.k.p;
    launch_load(L, 1, s);
    const Fr *r = xf.run(b, a, m, 1, inverse, s);
    StoreArgs S{r, out, t_len ? w.hi.p : nullptr, m, seg, (unit || !inverse) ? 1u : 0u, w.k.p + 1};
    ZK_LAUNCH(k_coset_store, dim3(blocks), dim3(QT_WG), 0, s, S);
    ZK_LAUNCH_OK("coset store");
    if (!t_len) return;
    w.hh.resize(blocks);
    HIP_TRY(hipMemcpyAsync(w.hh.data(), w.hi.p, blocks * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    uint64_t top = 0;
    for (uint32_t v : w.hh) top = v > top ? v : top;
    *t_len = top;
}

void fr_coset_ntt(uint8_t *out, const uint8_t *in, uint64_t n_in, uint32_t log_m, const uint8_t *shift, int inverse, int32_t device) {
    const char *who = "zk_fr_coset_ntt";
    const uint32_t seg = seg_in_effect();
    if (!out || !in) throw std::invalid_argument("null argument");
    if (log_m > MAX_LOG_M) throw std::invalid_argument(std::string(who) + ": log_m " + std::to_string(log_m) + " is above 28");
    const uint64_t m = 1ull << log_m;
    if (inverse ? n_in != m : (n_in < 1 || n_in > m))
        throw std::invalid_argument(std::string(who) + ": n_in " + std::to_string(n_in) + (inverse ? " is not 2^log_m = " : " is outside 1 .. 2^log_m = ") + std::to_string(m));
    check_below_r(who, "value", in, n_in);
    Fr g = Fr::one(), ginv = Fr::one();
    if (shift) {
        g = checked_one(who, "shift", shift);
        if (g.is_zero()) throw std::invalid_argument(std::string(who) + ": shift is zero");
        ginv = Fr::inv(g);
    }
    DeviceGuard dg(resolve_device(device));
    need_hbm(who, 3 * m * sizeof(Fr) + Xform::bytes_of(log_m) + CosetWork::bytes_of(m));
    Stream st;
    hipStream_t s = st.s;
    Xform xf;
    xf.build(log_m, s);
    DevBuf<Fr> a, b, c;
    CosetWork w;
    a.alloc(m);
    b.alloc(m);
    c.alloc(m);
    HIP_TRY(hipMemcpyAsync(c.p, in, n_in * sizeof(Fr), hipMemcpyHostToDevice, s));
    coset_ntt_dev(c.p, a.p, b.p, c.p, n_in, xf, g, ginv, !shift, inverse != 0, seg, w, nullptr, s);
    HIP_TRY(hipMemcpyAsync(out, c.p, m * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
}

}   // namespace

// ---------------------------------------------------------------- the object
struct zk_plonk_circuit {
    int device = 0;
    uint32_t log_n = 0;
    uint64_t n = 0, m = 0;
    std::mutex mu;                                    // calls on one object are serialised
    std::unique_ptr<Stream> st;
    Fr g, ginv, k1, k2, w_m;                          // Montgomery
    Fr zh[4];                                         // 1 / Z_H by i mod 4, words of x 2^261
    Xform xf;                                         // the transforms of size m
    DevBuf<Fr> res;                                   // RES_VECS x m
    DevBuf<Fr> x, y;                                  // EXT_VECS x m each: a call's vectors
    DevBuf<QuotConsts> kq;
    DevBuf<PowConsts> kl;                             // a call's load record
    QuotConsts hq;                                    // host images
    PowConsts hl;
    CosetWork cw;
    std::unique_ptr<Xform> small;                     // the transforms of size n: made by the first plonk_circuit_interpolate_dev
    DevBuf<PowConsts> ks;                             // its load and store records
    PowConsts hs[2];
    uint32_t last_launches = 0;
    size_t bytes() const {
        return res.bytes() + x.bytes() + y.bytes() + kq.bytes() + kl.bytes() + cw.k.bytes() + cw.hi.bytes() + Xform::bytes_of(log_n + 2);
    }
};

namespace {

uint64_t steady_bytes(uint32_t log_n) {
    const uint64_t m = 4ull << log_n;
    return (RES_VECS + 2 * EXT_VECS) * m * sizeof(Fr) + Xform::bytes_of(log_n + 2) + CosetWork::bytes_of(m) + sizeof(QuotConsts) + sizeof(PowConsts);
}

// the object from a view that was checked (plonk_internal.hpp: the public entry's, or a prover's)
zk_plonk_circuit *circuit_make(const CheckedView &cv, const CheckedShift &sh, int32_t device) {
    const char *who = "zk_plonk_circuit_create";
    const uint32_t seg = seg_in_effect(), log_n = cv.log_n;
    const uint8_t *const *vec = cv.vec;
    const uint64_t n = cv.n, m = 4 * n;
    const bool lagrange = cv.lagrange;
    std::unique_ptr<zk_plonk_circuit> c(new zk_plonk_circuit());
    c->log_n = log_n, c->n = n, c->m = m;
    c->k1 = cv.k1, c->k2 = cv.k2, c->g = sh.g;
    c->ginv = Fr::inv(c->g);
    c->w_m = root_of_unity(log_n + 2);
    const Fr w4 = root_of_unity(2);
    Fr zh = sh.gn;
    for (int j = 0; j < 4; j++) {                      // Z_H(x_i) = g^n w_4^(i mod 4) - 1
        c->zh[j] = w29(Fr::inv(Fr::sub(zh, Fr::one())));
        zh = Fr::mul(zh, w4);
    }
    c->device = resolve_device(device);
    DeviceGuard dg(c->device);
    // while it is made the object holds the nine vectors twice (a transform works out of place), later once beside a call's
    const uint64_t making = 2 * RES_VECS * m * sizeof(Fr) + Xform::bytes_of(log_n + 2) + Xform::bytes_of(log_n) + CosetWork::bytes_of(m);
    need_hbm(who, making > steady_bytes(log_n) ? making : steady_bytes(log_n));
    c->st.reset(new Stream());
    hipStream_t s = c->st->s;
    LaunchCount lc(c->last_launches);
    c->xf.build(log_n + 2, s);
    c->kq.alloc(1);
    c->kl.alloc(1);
    c->cw.size(m);
    DevBuf<Fr> p, q, fill;
    p.alloc(RES_VECS * m);
    q.alloc(RES_VECS * m);
    fill.alloc(1);
    for (int j = 0; j < 8; j++) HIP_TRY(hipMemcpyAsync(p.p + j * n, vec[j], n * sizeof(Fr), hipMemcpyHostToDevice, s));
    // L1's coefficients, n times 1 / n, in the form of the rows the load reads: standard, or the transforms' after the inverse transform
    const Fr ninv = lagrange ? w29(Fr::inv(fr_small(n))) : Fr::from_mont(Fr::inv(fr_small(n)));
    HIP_TRY(hipMemcpyAsync(fill.p, &ninv, sizeof ninv, hipMemcpyHostToDevice, s));
    const uint32_t blocks = blocks_of(m, seg);
    PowConsts hk[2];
    DevBuf<PowConsts> dk;
    dk.alloc(2);
    // monomial: rows in p -> extensions in q -> transformed into p.  Lagrange: rows in p -> q -> coefficients in q (one
    // batched inverse transform of size n) -> extensions in p -> transformed into q
    const Fr *rows = p.p;
    Fr *ext = q.p, *other = p.p;
    std::unique_ptr<Xform> small;
    if (lagrange) {
        small.reset(new Xform());
        small->build(log_n, s);
        hk[0] = pow_consts(POW_LOAD_STD, Fr::one(), (uint64_t)blocks_of(n, seg) * QT_WG);
        HIP_TRY(hipMemcpyAsync(dk.p, &hk[0], sizeof(PowConsts), hipMemcpyHostToDevice, s));
        LoadArgs U{};
        for (int j = 0; j < 8; j++) U.src[j] = p.p + j * n, U.n_in[j] = n;
        U.out = q.p, U.stride = n, U.m = n, U.seg = seg, U.unit = 1, U.k = dk.p;
        launch_load(U, 8, s);
        rows = small->run(q.p + 8 * n, q.p, n, 8, true, s);
        ext = p.p, other = q.p;
    }
    hk[1] = pow_consts(lagrange ? POW_LOAD_INTERNAL : POW_LOAD_STD, c->g, (uint64_t)blocks * QT_WG);
    HIP_TRY(hipMemcpyAsync(dk.p + 1, &hk[1], sizeof(PowConsts), hipMemcpyHostToDevice, s));
    LoadArgs L{};
    for (int j = 0; j < 8; j++) L.src[j] = rows + j * n, L.n_in[j] = n;
    L.src[V_L1] = nullptr, L.n_in[V_L1] = n, L.fill = fill.p;
    L.out = ext, L.stride = m, L.m = m, L.seg = seg, L.unit = 0, L.k = dk.p + 1;
    launch_load(L, RES_VECS, s);                      // the nine extensions: one batched load, one batched transform
    const Fr *r = c->xf.run(other, ext, m, RES_VECS, false, s);
    HIP_TRY(hipStreamSynchronize(s));
    DevBuf<Fr> &keep = r == p.p ? p : q;
    c->res.p = keep.p, c->res.n = keep.n;
    keep.p = nullptr, keep.n = 0;
    p.release();
    q.release();
    small.reset();
    c->x.alloc(EXT_VECS * m);
    c->y.alloc(EXT_VECS * m);
    return c.release();
}

zk_plonk_circuit *circuit_create(const zk_plonk_circuit_view *v, int32_t device) {
    const char *who = "zk_plonk_circuit_create";
    if (!v) throw std::invalid_argument("null argument");
    CheckedView cv = checked_view_dims(who, v, 1);
    checked_view_rows(who, v, cv);
    return circuit_make(cv, checked_shift(who, v->shift, cv.log_n), device);
}

// t's 4n coefficients and its length from the proof's polynomials, over device pointers and a stream: c.y holds the standard
// rows of a | b | c | z (| pi) back to back (lens[] rows each), the result is left in c.x's third vector, standard.
// Launches: one load, the batched forward transform, the quotient kernel, the inverse transform, one store
void plonk_quotient_dev(zk_plonk_circuit &c, const uint64_t lens[EXT_VECS], uint32_t vecs, Fr alpha, Fr beta, Fr gamma, uint32_t seg, uint64_t *t_len,
                        hipStream_t s) {
    const uint64_t m = c.m;
    const uint32_t blocks = blocks_of(m, seg);
    const uint64_t lanes = (uint64_t)blocks * QT_WG;
    c.hl = pow_consts(POW_LOAD_STD, c.g, lanes);
    c.hq.alpha = w29(alpha), c.hq.alpha2 = w29(Fr::sqr(alpha)), c.hq.beta = w29(beta), c.hq.gamma = w29(gamma);
    c.hq.bk1 = w29(Fr::mul(beta, c.k1)), c.hq.bk2 = w29(Fr::mul(beta, c.k2));
    for (int j = 0; j < 4; j++) c.hq.zh[j] = c.zh[j];
    c.hq.x = pow_consts(POW_POINTS, c.w_m, lanes, c.g);
    c.cw.h[1] = pow_consts(POW_STORE, c.ginv, lanes);
    HIP_TRY(hipMemcpyAsync(c.kl.p, &c.hl, sizeof c.hl, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c.kq.p, &c.hq, sizeof c.hq, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c.cw.k.p + 1, &c.cw.h[1], sizeof(PowConsts), hipMemcpyHostToDevice, s));
    LoadArgs L{};
    uint64_t at = 0;
    for (uint32_t v = 0; v < vecs; v++) {
        L.src[v] = c.y.p + at, L.n_in[v] = lens[v];
        at += lens[v];
    }
    L.out = c.x.p, L.stride = m, L.m = m, L.seg = seg, L.unit = 0, L.k = c.kl.p;
    launch_load(L, vecs, s);
    // the rows in c.y are consumed (stream order) before the transform writes there: at most 9n of its 20n rows held them
    const Fr *ext = c.xf.run(c.y.p, c.x.p, m, vecs, false, s);
    Fr *spare = ext == c.y.p ? c.x.p : c.y.p;         // the five vectors the transform left free
    QuotArgs Q{c.res.p, ext, spare, m, seg, vecs == EXT_VECS ? 1u : 0u, c.kq.p};
    ZK_LAUNCH(k_plonk_quotient, dim3(blocks), dim3(QT_WG), 0, s, Q);
    ZK_LAUNCH_OK("plonk quotient");
    const Fr *coef = c.xf.run(spare + m, spare, m, 1, true, s);
    StoreArgs S{coef, spare + 2 * m, c.cw.hi.p, m, seg, 0u, c.cw.k.p + 1};
    ZK_LAUNCH(k_coset_store, dim3(blocks), dim3(QT_WG), 0, s, S);
    ZK_LAUNCH_OK("coset store");
    if (spare != c.x.p) HIP_TRY(hipMemcpyAsync(c.x.p + 2 * m, spare + 2 * m, m * sizeof(Fr), hipMemcpyDeviceToDevice, s));
    c.cw.hh.resize(blocks);
    HIP_TRY(hipMemcpyAsync(c.cw.hh.data(), c.cw.hi.p, blocks * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    uint64_t top = 0;
    for (uint32_t v : c.cw.hh) top = v > top ? v : top;
    *t_len = top;
}

void plonk_quotient(zk_plonk_circuit *c, uint8_t *t, uint64_t *t_len, const uint8_t *const in[EXT_VECS], const uint64_t len[4], const uint8_t *alpha,
                    const uint8_t *beta, const uint8_t *gamma) {
    const char *who = "zk_plonk_quotient";
    const uint32_t seg = seg_in_effect();
    if (!c || !t || !t_len || !in[V_A] || !in[V_B] || !in[V_C] || !in[V_Z] || !alpha || !beta || !gamma) throw std::invalid_argument("null argument");
    static const char *const names[EXT_VECS] = {"a", "b", "c", "z", "pi"};
    const uint64_t n = c->n, m = c->m;
    for (int j = 0; j < 4; j++)
        if (len[j] < 1 || len[j] > 2 * n)
            throw std::invalid_argument(std::string(who) + ": " + names[j] + "_len " + std::to_string(len[j]) + " is outside 1 .. 2n = " + std::to_string(2 * n));
    const uint64_t sum = len[0] + len[1] + len[2] + len[3];
    if (sum > 5 * n + 3)
        throw std::invalid_argument(std::string(who) + ": a_len + b_len + c_len + z_len = " + std::to_string(sum) + " exceeds 5n + 3 = " + std::to_string(5 * n + 3) +
                                    ": t would have more than 4n coefficients");
    const uint32_t vecs = in[V_PI] ? EXT_VECS : EXT_VECS - 1;
    const uint64_t lens[EXT_VECS] = {len[0], len[1], len[2], len[3], n};
    for (uint32_t j = 0; j < vecs; j++) check_below_r(who, names[j], in[j], lens[j]);
    const Fr al = checked_one(who, "alpha", alpha), be = checked_one(who, "beta", beta), ga = checked_one(who, "gamma", gamma);
    std::lock_guard<std::mutex> lock(c->mu);
    DeviceGuard dg(c->device);
    LaunchCount lc(c->last_launches);
    hipStream_t s = c->st->s;
    uint64_t at = 0;
    for (uint32_t j = 0; j < vecs; j++) {
        HIP_TRY(hipMemcpyAsync(c->y.p + at, in[j], lens[j] * sizeof(Fr), hipMemcpyHostToDevice, s));
        at += lens[j];
    }
    plonk_quotient_dev(*c, lens, vecs, al, be, ga, seg, t_len, s);
    HIP_TRY(hipMemcpyAsync(t, c->x.p + 2 * m, m * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
}

}   // namespace

// ---------------------------------------------------------------- what plonkprove.hip chains (plonk_internal.hpp)
uint32_t plonk_quot_seg() { return seg_in_effect(); }

zk_plonk_circuit *plonk_circuit_make(const CheckedView &cv, const CheckedShift &shift, int32_t device) { return circuit_make(cv, shift, device); }

uint64_t plonk_circuit_need_bytes(uint32_t log_n) {
    const uint64_t m = 4ull << log_n;
    const uint64_t making = 2 * RES_VECS * m * sizeof(Fr) + Xform::bytes_of(log_n + 2) + Xform::bytes_of(log_n) + CosetWork::bytes_of(m);
    return (making > steady_bytes(log_n) ? making : steady_bytes(log_n)) + Xform::bytes_of(log_n) + 2 * sizeof(PowConsts);
}

size_t plonk_circuit_bytes(const zk_plonk_circuit *c) { return c->bytes() + (c->small ? Xform::bytes_of(c->log_n) + c->ks.bytes() : 0); }

Fr *plonk_circuit_rows(zk_plonk_circuit *c) { return c->y.p; }

const Fr *plonk_circuit_quotient_dev(zk_plonk_circuit *c, const uint64_t lens[PLONK_ROWS], uint32_t vecs, const Fr &alpha, const Fr &beta, const Fr &gamma,
                                     uint64_t *t_len, hipStream_t s) {
    static_assert(PLONK_ROWS == EXT_VECS, "a, b, c, z, pi");
    plonk_quotient_dev(*c, lens, vecs, alpha, beta, gamma, seg_in_effect(), t_len, s);
    return c->x.p + 2 * c->m;
}

void plonk_circuit_prepare_interpolate(zk_plonk_circuit *c, hipStream_t s) {
    if (c->small) return;
    std::unique_ptr<Xform> xf(new Xform());
    xf->build(c->log_n, s);
    c->ks.alloc(2);
    c->small = std::move(xf);
}

void plonk_circuit_interpolate_dev(zk_plonk_circuit *c, Fr *const out[], const Fr *in, uint32_t batch, hipStream_t s) {
    const uint32_t seg = seg_in_effect();
    const uint64_t n = c->n;
    if (batch < 1 || batch > EXT_VECS) throw std::invalid_argument("plonk_circuit_interpolate_dev: batch is outside 1 .. 5");
    plonk_circuit_prepare_interpolate(c, s);
    const uint32_t blocks = blocks_of(n, seg);
    const uint64_t lanes = (uint64_t)blocks * QT_WG;
    c->hs[0] = pow_consts(POW_LOAD_STD, Fr::one(), lanes);
    c->hs[1] = pow_consts(POW_STORE, Fr::one(), lanes);
    HIP_TRY(hipMemcpyAsync(c->ks.p, c->hs, sizeof c->hs, hipMemcpyHostToDevice, s));
    // c->x: 20n rows, free between two quotient calls.  The rows go to its first 5n, the transform may leave them in the next 5n
    LoadArgs U{};
    for (uint32_t v = 0; v < batch; v++) U.src[v] = in + v * n, U.n_in[v] = n;
    U.out = c->x.p, U.stride = n, U.m = n, U.seg = seg, U.unit = 1, U.k = c->ks.p;
    launch_load(U, batch, s);
    const Fr *r = c->small->run(c->x.p + EXT_VECS * n, c->x.p, n, batch, true, s);
    for (uint32_t v = 0; v < batch; v++) {
        StoreArgs S{r + v * n, out[v], nullptr, n, seg, 1u, c->ks.p + 1};
        ZK_LAUNCH(k_coset_store, dim3(blocks), dim3(QT_WG), 0, s, S);
    }
    ZK_LAUNCH_OK("coset store");
}

extern "C" {

int zk_fr_coset_ntt(uint8_t *out, const uint8_t *in, uint64_t n_in, uint32_t log_m, const uint8_t shift[32], int inverse, int32_t device) {
    return guarded([&] { fr_coset_ntt(out, in, n_in, log_m, shift, inverse, device); });
}

int zk_plonk_circuit_create(zk_plonk_circuit **out, const zk_plonk_circuit_view *v, int32_t device) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        *out = circuit_create(v, device);
    });
}

void zk_plonk_circuit_destroy(zk_plonk_circuit *c) { destroy_on_device(c); }

int zk_plonk_circuit_info(zk_plonk_circuit *c, zk_plonk_circuit_plan *plan) {
    return guarded([&] {
        if (!c || !plan) throw std::invalid_argument("null argument");
        info_into("zk_plonk_circuit_info", plan, [&](zk_plonk_circuit_plan &p) {
            p.seg = seg_in_effect();
            std::lock_guard<std::mutex> lock(c->mu);
            p.log_n = c->log_n;
            p.points = c->m;
            p.device_bytes = c->bytes();
            p.last_launches = c->last_launches;
        });
    });
}

int zk_plonk_quotient(zk_plonk_circuit *c, uint8_t *t, uint64_t *t_len, const uint8_t *a, uint64_t a_len, const uint8_t *b, uint64_t b_len,
                      const uint8_t *cc, uint64_t c_len, const uint8_t *z, uint64_t z_len, const uint8_t *pi, const uint8_t alpha[32],
                      const uint8_t beta[32], const uint8_t gamma[32]) {
    return guarded([&] {
        const uint8_t *const in[EXT_VECS] = {a, b, cc, z, pi};
        const uint64_t len[4] = {a_len, b_len, c_len, z_len};
        plonk_quotient(c, t, t_len, in, len, alpha, beta, gamma);
    });
}

}   // extern "C"
