// Powers of Tau, phase-2 preparation on the device (include/zkhip.h, section "Powers of Tau: prepare phase 2"): the
// Lagrange-basis sections 12 to 15 of a .ptau from its sections 2 to 5, what `snarkjs powersoftau prepare phase2` writes.
// Nothing in the reference corresponds to it: its prover reads a finished .zkey (src/main_prover.cpp:57-72).
//
// What is computed.  For every level p the 2^p points [tau^k] G, k < 2^p, become the 2^p points [L_j^(2^p)(tau)] G:
//   out_j = (1 / n) sum_k w^(-jk) in_k,   n = 2^p, w the n-th root of unity of ntt.hip (5^((r-1)/n)),
// an inverse DFT over GROUP elements, natural order in and out.  Level power + 1 of section 12 is built from the
// 2^(power+1) - 1 powers the file holds: the missing top power counts as infinity.
//
// The transform.  Decimation in frequency, one lane per butterfly (a + b, (a - b) w'), then the 1/n scale and the bit
// reversal.  The butterfly's multiplication is the whole cost: a 254-bit double-and-add whose base point differs from
// lane to lane, so there is no table to precompute.  Each stage is four launches:
//   k_ptau_bfly   a - b to a scratch row, then a + b in place                      (a general add per lane, twice)
//   normalise     the row of differences to affine, synth.hip's batched inversion  (~15 field products per point)
//   k_ptau_twmul  (a - b) w' by devmem.hpp's double-and-add with MIXED adds        (~3500 field products per point)
// so the loop pays 8M + 2S per set bit instead of the 12M + 2S of a general add.  The last pass multiplies every point
// by 1/n (k_ptau_scale) and writes it to its bit-reversed place; one more normalisation gives the file's bytes.  The
// last stage's twiddles are all 1, which the loop does in one step (it runs over the bit length of the scalar).
//
// Levels together.  Counted from the END, stage t of EVERY level has butterflies of span 2^t with the twiddle
// w_(2^(t+1))^(-j), whatever the level.  So the levels p_lo .. p_hi of a section are laid out back to back, as in the file
// (level p from point 2^p - 2^p_lo on), and stage t is one set of launches over the tail of that row that holds the
// levels above t: all the small levels cost no launches of their own.  A section is done in two such rows of about the
// same size, its top level and all the levels below it, so the peak is that of the top level.
//
// Lanes are numbered twiddle-major (lane = j * groups + g): from the stage on where a twiddle has 64 butterflies or more,
// a wave shares one scalar and the double-and-add loop does not diverge.  Nothing is accumulated with atomics; the
// result does not depend on launch order.
//
// Fields: curve.hpp's 8 x 32-bit Montgomery forms (R = 2^256), the .ptau's own bytes, as setup.hip.  Every point of a
// section is checked against the curve equation (the twist's for G2) and for coordinates below q before it is used; the
// all-zero encoding is infinity and is legal.  Membership of the G2 SUBGROUP is not checked: that is `powersoftau
// verify`'s job, and a point outside it still transforms linearly.
#include "hiputil.hpp"
#include "devmem.hpp"
#include "ptcheck.hpp"

namespace {

constexpr uint32_t NONE = NO_BAD_POINT;
constexpr uint32_t MAX_POWER = 27;                   // level power + 1 needs a 2^(power+1)-th root of unity; Fr has 2^28
constexpr uint32_t MAX_LOG_N = 28;

// ---------------------------------------------------------------- load
// A row holds the levels p_lo .. p_hi back to back: place i is point r = i + 2^p_lo - 2^p of level p = floor(log2(i + 2^p_lo))
__device__ __forceinline__ void row_place(uint64_t i, uint32_t p_lo, uint32_t &p, uint64_t &r) {
    const uint64_t u = i + (1ull << p_lo);
    p = 63u - (uint32_t)__clzll(u);
    r = u - (1ull << p);
}

// every level starts from the same powers: x[place of (p, r)] = src[r], infinity from n_src on
template <class F>
__global__ __launch_bounds__(256) void k_ptau_load(XYZZ<F> *x, const Affine<F> *src, uint64_t n_src, uint64_t cnt, uint32_t p_lo) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    uint32_t p;
    uint64_t r;
    row_place(i, p_lo, p, r);
    XYZZ<F> v = XYZZ<F>::inf();
    if (r < n_src) v = XYZZ<F>::from_affine(load_pt(src + r));
    store_pt(x + i, v);
}

// ---------------------------------------------------------------- twiddles
struct RootPowers {
    Fr w[MAX_LOG_N];                                  // w_N^(-2^i), Montgomery
};
// tab[k] = w_N^(-k), k < count, STANDARD form (the double-and-add loop reads its bits)
__global__ __launch_bounds__(256) void k_ptau_twiddles(Fr *tab, RootPowers pw, uint64_t count) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    Fr acc = Fr::one();
#pragma unroll 1
    for (uint32_t i = 0; i < MAX_LOG_N; i++)
        if ((k >> i) & 1) acc = Fr::mul(acc, pw.w[i]);
    store_el(tab + k, Fr::from_mont(acc));
}

// ---------------------------------------------------------------- the butterflies
// Stage of span `half` over the row's tail [base, base + 2 nb): lane i = j * groups + g is the butterfly of places
// lo = base + 2 half g + j and lo + half.  Two launches, so that a lane holds one sum at a time (G2: two points and the
// temporaries of an add are all the registers there are): with `diff`, a - b to diff[i] (normalised next, then multiplied), then
// with diff = NULL, a + b in place at lo.  add() takes a = b (doubling), a = -b and infinity explicitly.
template <class F>
__global__ __launch_bounds__(64) void k_ptau_bfly(XYZZ<F> *x, XYZZ<F> *diff, uint64_t nb, uint64_t groups, uint64_t half, uint64_t base) {
    const bool DIFF = diff != nullptr;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const uint64_t j = i / groups, g = i - j * groups, lo = base + 2 * half * g + j;
    XYZZ<F> b = load_pt(x + lo + half);
    if (DIFF) b.y = F::neg(b.y);
    add(b, load_pt(x + lo));
    store_pt(DIFF ? diff + i : x + lo, b);
}

// x[hi of lane i] = aff[i] * w_(2 half)^(-j); tab holds w_N^(-k), so the entry is j << tw_shift
template <class F>
__global__ __launch_bounds__(64) void k_ptau_twmul(XYZZ<F> *x, const Affine<F> *aff, uint64_t nb, uint64_t groups, uint64_t half, uint64_t base,
                                                   const Fr *tab, uint32_t tw_shift) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const uint64_t j = i / groups, g = i - j * groups, hi = base + 2 * half * g + j + half;
    store_pt(x + hi, scalar_mul_affine(load_pt(aff + i), load_el(tab + (j << tw_shift))));
}

// y[bit-reversed place of i within its level] = aff[i] / 2^p; ninv[p] = 2^(-p), standard form
template <class F>
__global__ __launch_bounds__(64) void k_ptau_scale(XYZZ<F> *y, const Affine<F> *aff, uint64_t cnt, uint32_t p_lo, const Fr *ninv) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    uint32_t p;
    uint64_t r;
    row_place(i, p_lo, p, r);
    const uint64_t rb = p ? __brevll(r) >> (64 - p) : 0;
    store_pt(y + (i - r + rb), scalar_mul_affine(load_pt(aff + i), load_el(ninv + p)));
}

// ---------------------------------------------------------------- host
// The scalars of one call: w_N^(-k) for k < N / 2 (N = 2^top, the largest level) and 2^(-p) for every level
struct Scalars {
    DevBuf<Fr> tab, ninv;
    uint32_t top = 0;
    void build(uint32_t top_, hipStream_t s) {
        top = top_;
        RootPowers pw;
        pw.w[0] = Fr::inv(root_of_unity(top));
        for (uint32_t i = 1; i < MAX_LOG_N; i++) pw.w[i] = Fr::sqr(pw.w[i - 1]);
        const uint64_t count = top ? 1ull << (top - 1) : 1;
        tab.alloc(count);
        ZK_LAUNCH(k_ptau_twiddles, dim3(nblocks(count, 256)), dim3(256), 0, s, tab.p, pw, count);
        ZK_LAUNCH_OK("ptau twiddles");
        std::vector<Fr> h(MAX_LOG_N + 1);
        Fr two = Fr::add(Fr::one(), Fr::one()), half = Fr::inv(two), acc = Fr::one();
        for (uint32_t p = 0; p <= MAX_LOG_N; p++) {
            h[p] = Fr::from_mont(acc);
            acc = Fr::mul(acc, half);
        }
        ninv.alloc(h.size());
        HIP_TRY(hipMemcpyAsync(ninv.p, h.data(), h.size() * sizeof(Fr), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));             // h and pw leave scope
    }
    static uint64_t bytes(uint32_t top_) { return (top_ ? 32ull << (top_ - 1) : 32) + 32 * (MAX_LOG_N + 1); }
};

template <class F>
struct Work {                                        // scratch of one row of `cap` points
    DevBuf<XYZZ<F>> x, y;
    DevBuf<Affine<F>> aff;
    DevBuf<F> pref;
    void alloc(uint64_t cap) {
        x.alloc(cap);
        y.alloc(cap);
        aff.alloc(cap);
        pref.alloc(cap);
    }
    static uint64_t bytes(uint64_t cap) { return cap * (2 * sizeof(XYZZ<F>) + sizeof(Affine<F>) + sizeof(F)); }
};

// Levels p_lo .. p_hi of the powers in d_src, affine in `out` (host; 2^(p_hi+1) - 2^p_lo points, level after level)
template <class F>
void run_levels(uint8_t *out, const Affine<F> *d_src, uint64_t n_src, uint32_t p_lo, uint32_t p_hi, const Scalars &sc, Work<F> &w, hipStream_t s) {
    const uint64_t cnt = (2ull << p_hi) - (1ull << p_lo);
    ZK_LAUNCH(k_ptau_load<F>, dim3(nblocks(cnt, 256)), dim3(256), 0, s, w.x.p, d_src, n_src, cnt, p_lo);
    for (uint32_t t = p_hi; t-- > 0;) {               // stage t: the levels above t, butterflies of span 2^t
        const uint32_t first = t + 1 > p_lo ? t + 1 : p_lo;
        const uint64_t base = (1ull << first) - (1ull << p_lo), nb = (cnt - base) / 2, half = 1ull << t, groups = nb / half;
        ZK_LAUNCH(k_ptau_bfly<F>, dim3(nblocks(nb, 64)), dim3(64), 0, s, w.x.p, w.y.p, nb, groups, half, base);
        ZK_LAUNCH(k_ptau_bfly<F>, dim3(nblocks(nb, 64)), dim3(64), 0, s, w.x.p, (XYZZ<F> *)nullptr, nb, groups, half, base);
        normalize(w.aff.p, w.y.p, w.pref.p, nb, s);
        ZK_LAUNCH(k_ptau_twmul<F>, dim3(nblocks(nb, 64)), dim3(64), 0, s, w.x.p, w.aff.p, nb, groups, half, base, sc.tab.p, sc.top - t - 1);
    }
    ZK_LAUNCH_OK("ptau butterflies");
    normalize(w.aff.p, w.x.p, w.pref.p, cnt, s);
    ZK_LAUNCH(k_ptau_scale<F>, dim3(nblocks(cnt, 64)), dim3(64), 0, s, w.y.p, w.aff.p, cnt, p_lo, sc.ninv.p);
    ZK_LAUNCH_OK("ptau scale");
    normalize(w.aff.p, w.y.p, w.pref.p, cnt, s);
    HIP_TRY(hipMemcpyAsync(out, w.aff.p, cnt * sizeof(Affine<F>), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
}

// d_src <- the first n_src points of `points`, each checked; -> the lowest index that is not a point of the curve, or NONE
template <class F>
uint32_t load_checked(DevBuf<Affine<F>> &d_src, const void *points, uint64_t n_src, hipStream_t s) {
    d_src.alloc(n_src ? n_src : 1);
    if (!n_src) return NONE;
    {
        StreamUploader up(s);
        up.copy(d_src.p, points, n_src * sizeof(Affine<F>));
    }
    DevBuf<uint32_t> err;
    err.alloc(1);
    launch_point_check<F>(err.p, d_src.p, n_src, s);
    uint32_t bad = NONE;
    HIP_TRY(hipMemcpyAsync(&bad, err.p, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return bad;
}

// HBM of one section whose top level is `top`: the powers, the scratch of a row of 2^top points, the scalars
template <class F>
uint64_t section_bytes(uint64_t n_src, uint32_t top) {
    return n_src * sizeof(Affine<F>) + Work<F>::bytes(1ull << top) + Scalars::bytes(top) + 4096;
}

template <class F>
void lagrange_op(uint8_t *out, const uint8_t *points, uint64_t n_points, uint32_t log_n, int32_t device, const char *who) {
    if (log_n > MAX_LOG_N) throw std::invalid_argument(std::string(who) + ": log_n " + std::to_string(log_n) + " exceeds 28");
    if (!out || (n_points && !points)) throw std::invalid_argument("null argument");
    const uint64_t n = 1ull << log_n, n_src = n_points < n ? n_points : n;
    DeviceGuard g(resolve_device(device));
    need_hbm(who, section_bytes<F>(n_src, log_n));
    Stream st;
    DevBuf<Affine<F>> d_src;
    const uint32_t bad = load_checked<F>(d_src, points, n_src, st.s);
    if (bad != NONE) throw std::invalid_argument(std::string(who) + ": point " + std::to_string(bad) + " is not on the curve");
    Scalars sc;
    sc.build(log_n, st.s);
    Work<F> w;
    w.alloc(n);
    run_levels<F>(out, d_src.p, n_src, log_n, log_n, sc, w, st.s);
}

struct Plan {                                        // what zk_ptau_prepare_sizes decides
    uint32_t power = 0;
    uint64_t n_src[4], out_bytes[4], device_bytes = 0;
    uint32_t top[4];
};

void check_view(const zk_ptau_powers_view *v, Plan &pl) {
    if (!v) throw std::invalid_argument("null argument");
    if (v->power < 1 || v->power > MAX_POWER)
        throw std::invalid_argument("ptau power " + std::to_string(v->power) + " is not supported (1 to 27: level power + 1 needs a 2^(power+1)-th root of unity)");
    pl.power = v->power;
    const uint64_t n = 1ull << v->power;
    const struct {
        int id;
        const void *p;
        uint64_t have, pts, ptb;
        uint32_t top;
    } sec[4] = {{2, v->tau_g1, v->tau_g1_bytes, 2 * n - 1, 64, v->power + 1}, {3, v->tau_g2, v->tau_g2_bytes, n, 128, v->power},
                {4, v->alpha_tau_g1, v->alpha_tau_g1_bytes, n, 64, v->power}, {5, v->beta_tau_g1, v->beta_tau_g1_bytes, n, 64, v->power}};
    for (int i = 0; i < 4; i++) {
        const auto &s = sec[i];
        if (!s.p) throw std::invalid_argument("ptau has no section " + std::to_string(s.id));
        if (s.have < s.pts * s.ptb)
            throw std::invalid_argument("ptau section " + std::to_string(s.id) + " is short: " + std::to_string(s.have) + " bytes, power " +
                                        std::to_string(v->power) + " needs " + std::to_string(s.pts * s.ptb));
        pl.n_src[i] = s.pts;
        pl.top[i] = s.top;
        pl.out_bytes[i] = ((2ull << s.top) - 1) * s.ptb;
        const uint64_t need = s.ptb == 64 ? section_bytes<Fq>(s.pts, s.top) : section_bytes<Fq2>(s.pts, s.top);
        if (need > pl.device_bytes) pl.device_bytes = need;
    }
}

template <class F>
void run_section(uint8_t *out, const void *points, uint64_t n_src, uint32_t top, int id, const Scalars &sc, hipStream_t s) {
    DevBuf<Affine<F>> d_src;
    const uint32_t bad = load_checked<F>(d_src, points, n_src, s);
    if (bad != NONE) throw std::invalid_argument("ptau section " + std::to_string(id) + ": point " + std::to_string(bad) + " is not on the curve");
    Work<F> w;
    w.alloc(1ull << top);
    // two rows of about the same size: the top level, then every level below it (level p starts at point 2^p - 1)
    run_levels<F>(out + ((1ull << top) - 1) * sizeof(Affine<F>), d_src.p, n_src, top, top, sc, w, s);
    run_levels<F>(out, d_src.p, n_src, 0, top - 1, sc, w, s);
}

void ptau_prepare(const zk_ptau_powers_view *v, int32_t device, zk_ptau_lagrange_out *out) {
    Plan pl;
    check_view(v, pl);                                // the file is checked before the device is touched
    if (!out || !out->lagrange_g1 || !out->lagrange_g2 || !out->lagrange_alpha_g1 || !out->lagrange_beta_g1)
        throw std::invalid_argument("null output buffer");
    DeviceGuard g(resolve_device(device));
    need_hbm("zk_ptau_prepare", pl.device_bytes);
    Stream st;
    Scalars sc;
    sc.build(pl.power + 1, st.s);
    run_section<Fq>(out->lagrange_g1, v->tau_g1, pl.n_src[0], pl.top[0], 2, sc, st.s);
    run_section<Fq2>(out->lagrange_g2, v->tau_g2, pl.n_src[1], pl.top[1], 3, sc, st.s);
    run_section<Fq>(out->lagrange_alpha_g1, v->alpha_tau_g1, pl.n_src[2], pl.top[2], 4, sc, st.s);
    run_section<Fq>(out->lagrange_beta_g1, v->beta_tau_g1, pl.n_src[3], pl.top[3], 5, sc, st.s);
}

}   // namespace

extern "C" {

int zk_g1_lagrange(uint8_t *out, const uint8_t *points, uint64_t n_points, uint32_t log_n, int32_t device) {
    return guarded([&] { lagrange_op<Fq>(out, points, n_points, log_n, device, "zk_g1_lagrange"); });
}
int zk_g2_lagrange(uint8_t *out, const uint8_t *points, uint64_t n_points, uint32_t log_n, int32_t device) {
    return guarded([&] { lagrange_op<Fq2>(out, points, n_points, log_n, device, "zk_g2_lagrange"); });
}

int zk_ptau_prepare_sizes(const zk_ptau_powers_view *ptau, zk_ptau_lagrange_sizes *sizes) {
    return guarded([&] {
        if (!sizes) throw std::invalid_argument("null argument");
        Plan pl;
        check_view(ptau, pl);
        sizes->lagrange_g1_bytes = pl.out_bytes[0];
        sizes->lagrange_g2_bytes = pl.out_bytes[1];
        sizes->lagrange_alpha_g1_bytes = pl.out_bytes[2];
        sizes->lagrange_beta_g1_bytes = pl.out_bytes[3];
        sizes->device_bytes = pl.device_bytes;
    });
}

int zk_ptau_prepare(const zk_ptau_powers_view *ptau, int32_t device, zk_ptau_lagrange_out *out) {
    return guarded([&] { ptau_prepare(ptau, device, out); });
}

}   // extern "C"
