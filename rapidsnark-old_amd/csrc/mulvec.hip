// n points times n DIFFERENT scalars, G1 and G2, and the Powers of Tau contribution built on it (include/zkhip.h, section
// "Powers of Tau: contribute").  Nothing in the reference corresponds to it: its prover reads a finished .zkey
// (src/main_prover.cpp:57-72); the counterpart is the arithmetic of snarkjs `powersoftau contribute`: tauG1[i] <- tau^i
// tauG1[i], tauG2[i] <- tau^i tauG2[i], alphaTauG1[i] <- alpha tau^i alphaTauG1[i], betaTauG1[i] <- beta tau^i betaTauG1[i],
// betaG2 <- beta betaG2.  No two lanes share a scalar, so nothing of scale.hip's host-made schedule applies.
//
// The kernel.  One lane per point, 64 lanes a block.  The lane splits its own scalar k = k1 + k2 lambda with both halves
// in (0, 2^128) (glv.hpp, where the bound is derived; the same function answers zk_glv_split on the host) and runs 128
// columns, most significant first.  Every column doubles the accumulator and reads the digit pair (b1, b2), the top bits
// of the two halves, which are then shifted as devmem.hpp's scalar_mul_affine shifts its scalar.  (0, 0) keeps the
// accumulator; every other pair is ONE mixed addition of an affine point made of registers the lane holds:
//     (1, 0)  P = (x, y)        (0, 1)  phi P = (e x, y)        (1, 1)  P + phi P = -phi^2 P = (-(x + e x), -y)
// (1 + lambda + lambda^2 = 0 and 1 + e + e^2 = 0, the identity scale.hip uses).  The operand is chosen with per-lane
// selects and is the all-zero point for (0, 0), which curve.hpp's madd leaves the accumulator alone for: the loop's trip
// count and every branch of its own are the same in all lanes, no register array is indexed at run time and no lane
// keeps a table in scratch or LDS.  The accumulator at infinity (the leading columns, a point at infinity) and the
// accumulator meeting +- the point it adds (small multiples, k = 0, whose split is (C - A, A + B) and whose sum is 0 P)
// are curve.hpp's explicit cases; nothing here assumes they do not happen.
//
// G1 and G2 are one template.  In G1 phi(x, y) = (beta x, y) is multiplication by lambda.  On the twist's order-r
// subgroup (beta x, y) is multiplication by lambda^2, so e = beta^2 there: the constant is the only difference.  That is
// why a G2 point must be in the SUBGROUP before it is multiplied (elsewhere phi is no multiplication by a constant):
// every point is checked first with ptengine.hpp's k_ptau_classify and, in G2, launch_subgroup; the lowest failing index
// is named.  Those kernels record it with atomicMin, which does not depend on the order of launches or lanes; nothing
// else uses atomics.
//
// Cost by operation count: 128 x (9 + 10) = 2432 field products a point, against about 254 x (9 + 10) = 4826 of
// scalar_mul_affine when the scalars of a wave differ.  ZKHIP_MULVEC_PLAIN=1 runs that loop instead (k_mul_vec<F, true>),
// one lane per point: a second route to the same bytes for the tests and the denominator of
// tools/ptau_contribute_timing.py.
//
// Scalars come from the host (zk_g*_mul_vec: 32 bytes a point) or are made by the lane (zk_g*_power_scale and the
// contribution: c base^(first_exp + i) from ptengine.hpp's table of squarings, so tau's powers never exist in host
// memory and no scalar crosses PCIe).  Points go through the device in chunks (ZKHIP_PTAU_CONTRIB_CHUNK points, 2^20
// otherwise) on chunklanes.hpp's two buffer sets, which scale.hip uses too: upload, checks, multiplication, synth.hip's
// batched normalisation and download of chunk c + 1 run on the other stream while chunk c is copied out.
//
// Fields: curve.hpp's 8 x 32-bit Montgomery forms (R = 2^256), the .ptau's own bytes, as ptau_prepare.hip and scale.hip.
#include "ptengine.hpp"
#include "chunklanes.hpp"
#include "mulglv.hpp"

namespace {

constexpr uint64_t DEFAULT_CHUNK = 1ull << 20;       // points per chunk: 64 MiB of G1 input, 128 MiB of G2
constexpr uint32_t TAB_WORDS = POW_BITS + 1;         // base^(2^i), i < 64, then the factor c (Montgomery)
// ---------------------------------------------------------------- device
// out[i] = k_i in[i], XYZZ.  k_i = sc[i] (standard form), or with POWERS tab[64] base^(e0 + i) from the squarings tab[0 .. 63]
template <class F, bool PLAIN, bool POWERS>
__global__ __launch_bounds__(64) void k_mul_vec(XYZZ<F> *__restrict__ out, const Affine<F> *__restrict__ in, uint64_t n,
                                                const Fr *__restrict__ sc, const Fr *__restrict__ tab, uint64_t e0, Fq e) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr k;
    if constexpr (POWERS) k = Fr::from_mont(Fr::mul(pow_tab(tab, e0 + i), load_el(tab + POW_BITS)));
    else k = load_el(sc + i);
    const Affine<F> P = load_pt(in + i);
    if constexpr (PLAIN) store_pt(out + i, scalar_mul_affine(P, k));
    else store_pt(out + i, mul_glv(P, k, e));
}

// ---------------------------------------------------------------- host
uint64_t chunk_points() { return env_number("ZKHIP_PTAU_CONTRIB_CHUNK", DEFAULT_CHUNK, 1, 1ull << 28, "a number of points from 1 to 2^28", ENV_LAX); }

// The squarings of the base and the factor on the device.  In the contribution they are the secrets: the host copy is
// wiped as soon as it is uploaded, the device copy before it is freed, after the lanes that read it have drained (the
// object is declared before them).
struct PowerTable {
    DevBuf<Fr> d;
    void build(Fr base, const Fr &factor, hipStream_t s) {
        Fr h[TAB_WORDS];
        for (uint32_t i = 0; i < POW_BITS; i++) {
            h[i] = base;
            base = Fr::sqr(base);
        }
        h[POW_BITS] = factor;
        if (!d.p) d.alloc(TAB_WORDS);                 // built again for the next factor: overwritten in place, never freed unwiped
        const hipError_t e1 = hipMemcpyAsync(d.p, h, sizeof h, hipMemcpyHostToDevice, s), e2 = hipStreamSynchronize(s);
        explicit_bzero(h, sizeof h);
        explicit_bzero(&base, sizeof base);
        HIP_TRY(e1);
        HIP_TRY(e2);
    }
    ~PowerTable() {
        if (d.p) (void)hipMemset(d.p, 0, d.bytes());
    }
};

template <class F>
uint64_t muller_bytes(uint64_t cap, bool host_scalars) {
    return ChunkLanes<F>::bytes(cap, host_scalars) + TAB_WORDS * sizeof(Fr) + 4096;
}

template <class F>
struct Muller {
    PowerTable tab;                                   // before the lanes (chunklanes.hpp): wiped after they have drained
    ChunkLanes<F> lanes;                              // four words of checks: ptengine.hpp's pass
    bool plain, plain_sub;
    Fq e;
    PsiConsts psi;
    Muller(uint64_t cap, bool host_scalars)
        : lanes(cap, host_scalars, 4), plain(env_switch("ZKHIP_MULVEC_PLAIN")), plain_sub(plain_subgroup()), e(endo_const<F>()),
          psi(sizeof(F) == sizeof(Fq2) ? psi_consts() : PsiConsts{}) {}     // the subgroup test's constants: G2 only
    // the checks of the lane's chunk, enqueued; inf_bad: infinity is no legal point (a .ptau's sections)
    void enqueue_checks(Lane<F> &l, bool inf_bad) { enqueue_classify<F>(l.words(), l.err.p, l.aff.p, l.cnt, inf_bad, &psi, plain_sub, l.st.s); }
    // a point of the drained lane's chunk that failed a check is an error naming `what`, the lowest index and what is wrong with it
    static void judge(const Lane<F> &l, const char *what) {
        const BadPoint b = lowest_bad(l.words());
        if (b.kind) throw std::invalid_argument(std::string(what) + ": point " + std::to_string(l.off + b.index) + " " + KIND_TEXT[b.kind]);
    }
    // out[i] = k_i in[i], i < n (host memory).  scalars given: k_i = scalars[i]; else k_i = tab's factor x base^(first_exp + i)
    void run(uint8_t *out, const uint8_t *in, uint64_t n, const uint8_t *scalars, uint64_t first_exp, bool inf_bad, const char *what) {
        lanes.run(
            out, in, n,
            [&](Lane<F> &l) {
                hipStream_t s = l.st.s;
                if (scalars) l.up.copy(l.sc.p, scalars + l.off * sizeof(Fr), l.cnt * sizeof(Fr));
                enqueue_checks(l, inf_bad);
                const dim3 grid(nblocks(l.cnt, 64)), block(64);
                const uint64_t e0 = first_exp + l.off;
                if (scalars) {
                    if (plain) ZK_LAUNCH((k_mul_vec<F, true, false>), grid, block, 0, s, l.xyzz.p, l.aff.p, l.cnt, l.sc.p, (const Fr *)nullptr, e0, e);
                    else ZK_LAUNCH((k_mul_vec<F, false, false>), grid, block, 0, s, l.xyzz.p, l.aff.p, l.cnt, l.sc.p, (const Fr *)nullptr, e0, e);
                } else {
                    if (plain) ZK_LAUNCH((k_mul_vec<F, true, true>), grid, block, 0, s, l.xyzz.p, l.aff.p, l.cnt, (const Fr *)nullptr, tab.d.p, e0, e);
                    else ZK_LAUNCH((k_mul_vec<F, false, true>), grid, block, 0, s, l.xyzz.p, l.aff.p, l.cnt, (const Fr *)nullptr, tab.d.p, e0, e);
                }
                ZK_LAUNCH_OK("point by scalar");
            },
            [&](const Lane<F> &l) { judge(l, what); });
    }
    // the checks alone, of a few points (section 6)
    void check(const uint8_t *in, uint64_t n, bool inf_bad, const char *what) {
        Lane<F> &l = lanes.lane[0];
        l.off = 0;
        l.cnt = n;
        l.up.copy(l.aff.p, in, n * sizeof(Affine<F>));
        enqueue_checks(l, inf_bad);
        HIP_TRY(hipStreamSynchronize(l.st.s));
        judge(l, what);
    }
};

// ---------------------------------------------------------------- the operators
template <class F>
void mul_vec(uint8_t *out, const uint8_t *points, const uint8_t *scalars, uint64_t n, int32_t device, const char *who) {
    if (!n) return;
    if (!out || !points || !scalars) throw std::invalid_argument("null argument");
    const uint64_t bad = first_not_below_r(scalars, n);
    if (bad < n) throw std::invalid_argument(std::string(who) + ": scalar " + std::to_string(bad) + " is not below r");
    const uint64_t chunk = chunk_points(), cap = n < chunk ? n : chunk;
    DeviceGuard g(resolve_device(device));
    need_hbm(who, muller_bytes<F>(cap, true));
    Muller<F> m(cap, true);
    m.run(out, points, n, scalars, 0, false, who);
}

template <class F>
void power_scale(uint8_t *out, const uint8_t *points, uint64_t n, const uint8_t base32[32], uint64_t first_exp, const uint8_t factor32[32],
                 int32_t device, const char *who) {
    if (!base32 || !factor32 || (n && (!out || !points))) throw std::invalid_argument("null argument");
    const Fr base = checked_scalar(base32, std::string(who) + ": the base"), factor = checked_scalar(factor32, std::string(who) + ": the factor");
    if (first_exp + n < first_exp) throw std::invalid_argument(std::string(who) + ": first_exp + n exceeds 2^64");
    if (!n) return;
    const uint64_t chunk = chunk_points(), cap = n < chunk ? n : chunk;
    DeviceGuard g(resolve_device(device));
    need_hbm(who, muller_bytes<F>(cap, false));
    Muller<F> m(cap, false);
    m.tab.build(base, factor, m.lanes.lane[0].st.s);
    m.run(out, points, n, nullptr, first_exp, false, who);
}

// ---------------------------------------------------------------- the contribution
constexpr uint32_t MAX_POWER = 28;

struct ContribPlan {
    uint32_t power = 0;
    uint64_t points[7] = {}, cap1 = 0, cap2 = 0, device_bytes = 0;      // per section 2 .. 6
};

uint64_t point_bytes(int sec) { return sec == 3 || sec == 6 ? 128 : 64; }

void check_view(const zk_ptau_file_view *v, ContribPlan &pl) {
    if (!v) throw std::invalid_argument("null argument");
    if (v->power < 1 || v->power > MAX_POWER)
        throw std::invalid_argument("ptau power " + std::to_string(v->power) + " is not supported (1 to " + std::to_string(MAX_POWER) + ")");
    for (int sec = 12; sec < 16; sec++)
        if (v->sec[sec])
            throw std::invalid_argument("the ptau file is prepared for phase 2 (it has section " + std::to_string(sec) + "): contribute before `ptauprepare`");
    pl.power = v->power;
    const uint64_t n = 1ull << v->power;
    pl.points[2] = 2 * n - 1;
    pl.points[3] = pl.points[4] = pl.points[5] = n;
    pl.points[6] = 1;
    for (int sec = 2; sec <= 6; sec++) {
        if (!v->sec[sec]) throw std::invalid_argument("ptau has no section " + std::to_string(sec));
        const uint64_t need = pl.points[sec] * point_bytes(sec);
        if (v->sec_bytes[sec] < need)
            throw std::invalid_argument("ptau section " + std::to_string(sec) + " is short: " + std::to_string(v->sec_bytes[sec]) + " bytes, power " +
                                        std::to_string(v->power) + " needs " + std::to_string(need));
    }
    const uint64_t chunk = chunk_points();
    pl.cap1 = pl.points[2] < chunk ? pl.points[2] : chunk;
    pl.cap2 = n < chunk ? n : chunk;
    const uint64_t b1 = muller_bytes<Fq>(pl.cap1, false), b2 = muller_bytes<Fq2>(pl.cap2, false);      // one group after the other
    pl.device_bytes = b1 > b2 ? b1 : b2;
}

void ptau_contribute(const zk_ptau_file_view *v, const uint8_t *tau32, const uint8_t *alpha32, const uint8_t *beta32, int32_t device,
                     zk_ptau_contrib_out *out) {
    ContribPlan pl;
    check_view(v, pl);                                // the file and the scalars are checked before the device is touched
    if (!tau32 || !alpha32 || !beta32) throw std::invalid_argument("null argument");
    if (!out || !out->tau_g1 || !out->tau_g2 || !out->alpha_tau_g1 || !out->beta_tau_g1 || !out->beta_g2) throw std::invalid_argument("null output buffer");
    struct Secrets {
        Fr tau, alpha, beta, one;
        ~Secrets() { explicit_bzero(this, sizeof *this); }
    } sec;
    const struct {
        const uint8_t *p;
        const char *name;
        Fr *to;
    } given[3] = {{tau32, "tau", &sec.tau}, {alpha32, "alpha", &sec.alpha}, {beta32, "beta", &sec.beta}};
    for (const auto &s : given) {
        bool zero = true;
        for (int i = 0; i < 32; i++) zero = zero && s.p[i] == 0;
        if (zero) throw std::invalid_argument(std::string("zk_ptau_contribute: ") + s.name + " is 0");
        *s.to = checked_scalar(s.p, std::string("zk_ptau_contribute: ") + s.name);
    }
    sec.one = Fr::one();
    DeviceGuard g(resolve_device(device));
    need_hbm("zk_ptau_contribute", pl.device_bytes);
    const uint8_t *const *in = reinterpret_cast<const uint8_t *const *>(v->sec);
    {
        Muller<Fq> m(pl.cap1, false);
        hipStream_t s = m.lanes.lane[0].st.s;
        m.tab.build(sec.tau, sec.one, s);
        m.run(out->tau_g1, in[2], pl.points[2], nullptr, 0, true, "ptau section 2");
        m.tab.build(sec.tau, sec.alpha, s);           // run() has drained both lanes
        m.run(out->alpha_tau_g1, in[4], pl.points[4], nullptr, 0, true, "ptau section 4");
        m.tab.build(sec.tau, sec.beta, s);
        m.run(out->beta_tau_g1, in[5], pl.points[5], nullptr, 0, true, "ptau section 5");
    }
    {
        Muller<Fq2> m(pl.cap2, false);
        m.tab.build(sec.tau, sec.one, m.lanes.lane[0].st.s);
        m.run(out->tau_g2, in[3], pl.points[3], nullptr, 0, true, "ptau section 3");
        m.check(in[6], 1, true, "ptau section 6");
    }
    if (zk_g2_mul(out->beta_g2, in[6], beta32) != 0) throw std::runtime_error("zk_ptau_contribute: betaG2 could not be multiplied");
}

}   // namespace

extern "C" {

int zk_glv_split(const uint8_t k[32], uint8_t k1[16], uint8_t k2[16]) {
    return guarded([&] {
        if (!k || !k1 || !k2) throw std::invalid_argument("null argument");
        if (!below(k, FrParams::P)) throw std::invalid_argument("zk_glv_split: the scalar is not below r");
        uint32_t w[8], a[4], b[4];
        memcpy(w, k, 32);
        glv_split(w, a, b);
        memcpy(k1, a, 16);
        memcpy(k2, b, 16);
    });
}

int zk_g1_mul_vec(uint8_t *out, const uint8_t *points, const uint8_t *scalars, uint64_t n, int32_t device) {
    return guarded([&] { mul_vec<Fq>(out, points, scalars, n, device, "zk_g1_mul_vec"); });
}
int zk_g2_mul_vec(uint8_t *out, const uint8_t *points, const uint8_t *scalars, uint64_t n, int32_t device) {
    return guarded([&] { mul_vec<Fq2>(out, points, scalars, n, device, "zk_g2_mul_vec"); });
}
int zk_g1_power_scale(uint8_t *out, const uint8_t *points, uint64_t n, const uint8_t base[32], uint64_t first_exp, const uint8_t factor[32], int32_t device) {
    return guarded([&] { power_scale<Fq>(out, points, n, base, first_exp, factor, device, "zk_g1_power_scale"); });
}
int zk_g2_power_scale(uint8_t *out, const uint8_t *points, uint64_t n, const uint8_t base[32], uint64_t first_exp, const uint8_t factor[32], int32_t device) {
    return guarded([&] { power_scale<Fq2>(out, points, n, base, first_exp, factor, device, "zk_g2_power_scale"); });
}

int zk_ptau_contribute_sizes(const zk_ptau_file_view *ptau, zk_ptau_contrib_sizes *sizes) {
    return guarded([&] {
        if (!sizes) throw std::invalid_argument("null argument");
        ContribPlan pl;
        check_view(ptau, pl);
        sizes->tau_g1_bytes = pl.points[2] * 64;
        sizes->tau_g2_bytes = pl.points[3] * 128;
        sizes->alpha_tau_g1_bytes = pl.points[4] * 64;
        sizes->beta_tau_g1_bytes = pl.points[5] * 64;
        sizes->beta_g2_bytes = 128;
        sizes->chunk_points = pl.cap1;
        sizes->device_bytes = pl.device_bytes;
    });
}

int zk_ptau_contribute(const zk_ptau_file_view *ptau, const uint8_t tau[32], const uint8_t alpha[32], const uint8_t beta[32], int32_t device,
                       zk_ptau_contrib_out *out) {
    return guarded([&] { ptau_contribute(ptau, tau, alpha, beta, device, out); });
}

}   // extern "C"
