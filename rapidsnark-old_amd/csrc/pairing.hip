// Pairings and Groth16 verification on the device (include/zkhip.h, section "Pairing and verification").  Nothing in the
// reference corresponds to it (it only proves); the counterpart is snarkjs `groth16 verify`.  The arithmetic is
// pairing.hpp's; this file is the lane mapping, the checks made before any pairing, and the entry points.
//
// One lane per job.  A job is a group of (P, Q) pairs that share one f: one squaring chain per group, each pair's line
// multiplied in at every step.  No lane talks to another.
//   zk_pairing: every Q is the caller's, so every pair carries a running T; it lives in device memory (192 B a pair) and
//   is loaded, stepped and stored per line.  k_miller_groups, then k_final_exp.
//   zk_vkey_verify: e(-A, B) e(alpha, beta) e(vk_x, gamma) e(C, delta) = 1.  gamma and delta are the key's: k_line_table
//   writes the MILLER_LINES line coefficients of each once, when the key is made, and k_verify_miller reads them with a
//   wave-uniform index and evaluates them at the lane's own vk_x and C; only B carries a T, in the lane's own memory.  The
//   Miller value of (alpha, beta) is made once and multiplied in.  Per proof: one variable-Q loop, two table-driven ones,
//   one Fq12 product, one final exponentiation.
//
// Checks before any pairing (k_pair_check, k_verify_check): coordinates below q, y^2 = x^3 + 3 in G1, y^2 = x^3 + 3/xi on
// the twist, and membership of the order-r subgroup of the twist by [r] Q = infinity (devmem.hpp's scalar_mul_affine over
// the 254 bits of r: the plain test, about as many Fq products as the Miller loop itself; the cooperative kernels of
// pairing_coop.hip use ptengine.hpp's endomorphism test, several times cheaper; these kernels are left as they were).  Public signals below r.  vk_x = IC_0 + sum pub_j IC_j per lane, by the same
// scalar_mul_affine and curve.hpp's add, which take every special case; vk_x = infinity is legal and contributes 1.
//
// Field form: field.hpp's 8 x 32-bit Montgomery words, the form of the .zkey's and the proof's own bytes and of every
// helper used here (ptcheck.hpp, curve.hpp, devmem.hpp).  field29.hpp's multiplier is about twice as fast; DESIGN.md
// section 17 says what that choice costs and why it was made.
#include <memory>
#include <mutex>

#include "hiputil.hpp"
#include "devmem.hpp"
#include "ptcheck.hpp"
#include "pairing.hpp"
#include "paircheck.hpp"
#include "verify_lanes.hpp"
#include "pairing_coop.hpp"
#include "pairing_internal.hpp"

namespace {

constexpr uint64_t DEFAULT_CHUNK = 1ull << 16;        // jobs per chunk
// The largest calls that take the cooperative path (pairing_coop.hip), read at every call like the chunk.  The defaults are
// the measured crossovers of profiles/verify_latency_timing.txt.
constexpr uint64_t DEFAULT_VERIFY_COOP_MAX = 1024, DEFAULT_PAIRING_COOP_MAX = 256;

static_assert(sizeof(G1Affine) == 64 && sizeof(G2Affine) == 128 && sizeof(Fq12) == 384 && sizeof(G2Proj) == 192 && sizeof(Line) == 192, "layout");

// ---------------------------------------------------------------- device: checks (in_subgroup: verify_lanes.hpp)
// err[0]: the lowest G1 index off the curve, err[1]: the lowest G2 index off the twist, err[2]: the lowest G2 index
// outside the subgroup (NO_BAD_POINT: none).  The all-zero encoding (infinity) passes.
__global__ __launch_bounds__(64) void k_pair_check(uint32_t *err, const G1Affine *__restrict__ g1, uint64_t n1, const G2Affine *__restrict__ g2,
                                                   uint64_t n2, Fq b1, Fq2 b2) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n1) {
        const G1Affine P = load_pt(g1 + i);
        if (!P.is_inf() && !on_curve(P, b1)) atomicMin(err + 0, (uint32_t)i);
    }
    if (i < n2) {
        const G2Affine Q = load_pt(g2 + i);
        if (!Q.is_inf()) {
            if (!on_curve(Q, b2)) atomicMin(err + 1, (uint32_t)i);
            else if (!in_subgroup(Q)) atomicMin(err + 2, (uint32_t)i);
        }
    }
}

// ---------------------------------------------------------------- device: constants, tables
__global__ void k_pair_consts(PairConsts *k) {
    if (blockIdx.x == 0 && threadIdx.x == 0) pair_consts_init(*k);
}

// tab[j * MILLER_LINES + i]: line i of the loop over Q[j], to be evaluated at any P (f12_mul_line_at)
__global__ __launch_bounds__(64) void k_line_table(Line *tab, const G2Affine *Q, uint32_t n, const PairConsts *k) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    line_table(tab + (uint64_t)j * MILLER_LINES, load_pt(Q + j), *k);
}

// ---------------------------------------------------------------- device: Miller loops
// f_out[j] = prod over the pairs p of group j of the Miller value of (g1[p], g2[p]); a pair with a point at infinity
// contributes 1.  T: n_pairs running points, this kernel's own.
__global__ __launch_bounds__(64) void k_miller_groups(Fq12 *f_out, const G1Affine *__restrict__ g1, const G2Affine *__restrict__ g2, G2Proj *T,
                                                      uint64_t n_pairs, uint32_t group, const PairConsts *k) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t lo = j * group;
    if (lo >= n_pairs) return;
    const uint64_t hi = n_pairs - lo < group ? n_pairs : lo + group;
    Fq12 f;
    f12_one(f);
    Line l;
    for (uint64_t p = lo; p < hi; p++) {
        const G2Affine Q = load_pt(g2 + p);
        T[p] = G2Proj{Q.x, Q.y, Fq2::one()};
    }
    for (int i = 0; i <= 64; i++) {                   // i = 64: the two Frobenius chords
        if (i < 64) f12_sqr(f, f);
        for (uint64_t p = lo; p < hi; p++) {
            const G1Affine P = load_pt(g1 + p);
            const G2Affine Q = load_pt(g2 + p);
            if (P.is_inf() || Q.is_inf()) continue;
            G2Proj t = T[p];
            if (i < 64) {
                step_dbl(t, l, *k);
                f12_mul_line_at(f, l, P);
                if (ate_bit(i)) {
                    step_add(t, l, Q);
                    f12_mul_line_at(f, l, P);
                }
            } else {
                G2Affine q1, q2;
                frob_twist(q1, q2, Q, *k);
                step_add(t, l, q1);
                f12_mul_line_at(f, l, P);
                step_add(t, l, q2);
                f12_mul_line_at(f, l, P);
            }
            T[p] = t;
        }
    }
    f_out[j] = f;
}

// out[j]: the final exponentiation of f[j] as 12 x 32 bytes little-endian, standard form
__global__ __launch_bounds__(64) void k_final_exp(uint8_t *out, const Fq12 *f, uint64_t n, const PairConsts *k) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    Fq12 r;
    final_exp(r, f[j], *k);
    const Fq *c = reinterpret_cast<const Fq *>(&r);
    Fq *o = reinterpret_cast<Fq *>(out + j * sizeof(Fq12));
    for (int i = 0; i < 12; i++) store_el(o + i, Fq::from_mont(c[i]));
}

// ---------------------------------------------------------------- device: verification
// status[i], and vk_x of proof i when it is well-formed.  proofs: A 64 | B 128 | C 64; publics: n x nPublic x 32 B
__global__ __launch_bounds__(64) void k_verify_check(uint32_t *status, G1Affine *vkx, const uint8_t *__restrict__ proofs, const Fr *__restrict__ publics,
                                                     uint64_t n, uint32_t nPublic, const G1Affine *__restrict__ ic, Fq b1, Fq2 b2) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    verify_check_lane(status + i, vkx + i, proofs + i * 256, publics + i * nPublic, nPublic, ic, b1, b2);
}

// f_out[i] = miller(-A, B) miller(vk_x, gamma) miller(C, delta) miller(alpha, beta); tab: gamma's lines, then delta's
__global__ __launch_bounds__(64) void k_verify_miller(Fq12 *f_out, const uint32_t *__restrict__ status, const uint8_t *__restrict__ proofs,
                                                      const G1Affine *__restrict__ vkx, const Line *__restrict__ tab, const Fq12 *ml_ab, uint64_t n,
                                                      const PairConsts *k) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || status[i] != ST_OK) return;
    verify_miller_lane(f_out + i, proofs + i * 256, vkx + i, tab, ml_ab, k);
}

__global__ __launch_bounds__(64) void k_verify_final(uint8_t *verdict, const Fq12 *f, const uint32_t *__restrict__ status, uint64_t n, const PairConsts *k) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    verify_final_lane(verdict + i, f + i, status[i], k);
}

}   // namespace

// ---------------------------------------------------------------- host
uint64_t zkp::chunk_jobs() { return env_number("ZKHIP_VERIFY_CHUNK", DEFAULT_CHUNK, 1, 1ull << 24, "a number of proofs from 1 to 2^24", ENV_LAX); }

uint64_t zkp::verify_coop_max() { return coop_threshold("ZKHIP_VERIFY_COOP_MAX", "proofs", DEFAULT_VERIFY_COOP_MAX); }

void zkp::Consts::make(hipStream_t s) {
    k.alloc(1);
    ZK_LAUNCH(k_pair_consts, dim3(1), dim3(1), 0, s, k.p);
    ZK_LAUNCH_OK("pairing constants");
}

namespace {

constexpr uint64_t COOP_MAX_PAIRS = 8192;             // 19 KiB of lines a pair or a proof (COOP_MAX_PROOFS): a call with more of
                                                      // them goes the lane way whatever the threshold, in chunks and constant memory
uint64_t pairing_coop_max() { return coop_threshold("ZKHIP_PAIRING_COOP_MAX", "groups", DEFAULT_PAIRING_COOP_MAX); }
thread_local int t_pairing_path = -1;

// the three words of k_pair_check after the stream has drained
struct CheckWords {
    DevBuf<uint32_t> d;
    uint32_t h[3];
    void run(const G1Affine *g1, uint64_t n1, const G2Affine *g2, uint64_t n2, hipStream_t s) {
        if (!d.p) d.alloc(3);
        HIP_TRY(hipMemsetAsync(d.p, 0xFF, 12, s));
        const uint64_t n = n1 > n2 ? n1 : n2;
        if (n) ZK_LAUNCH(k_pair_check, dim3(nblocks(n, 64)), dim3(64), 0, s, d.p, g1, n1, g2, n2, curve_b<Fq>(), curve_b<Fq2>());
        ZK_LAUNCH_OK("pairing point check");
        HIP_TRY(hipMemcpyAsync(h, d.p, 12, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
};

// every group on a workgroup of its own: one launch, the point checks inside it
void pairing_coop(uint8_t *out, const uint8_t *g1, const uint8_t *g2, uint64_t n_pairs, uint32_t group, uint64_t jobs) {
    need_hbm("zk_pairing", n_pairs * (sizeof(G1Affine) + sizeof(G2Affine) + MILLER_LINES * sizeof(Line) + 1) + jobs * sizeof(Fq12) + 65536);
    Stream st;
    hipStream_t s = st.s;
    Consts kc;
    kc.make(s);
    DevBuf<G1Affine> d1;
    DevBuf<G2Affine> d2;
    DevBuf<Line> dl;
    DevBuf<uint8_t> dskip, dout;
    DevBuf<uint32_t> derr;
    uint32_t h[3];
    d1.alloc(n_pairs);
    d2.alloc(n_pairs);
    dl.alloc(n_pairs * MILLER_LINES);
    dskip.alloc(n_pairs);
    dout.alloc(jobs * sizeof(Fq12));
    derr.alloc(3);
    HIP_TRY(hipMemcpyAsync(d1.p, g1, n_pairs * sizeof(G1Affine), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d2.p, g2, n_pairs * sizeof(G2Affine), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(derr.p, 0xFF, 12, s));
    launch_pairing_coop(dout.p, d1.p, d2.p, dl.p, dskip.p, derr.p, n_pairs, group, COOP_FINAL | COOP_CHECK, kc.k.p, s);
    HIP_TRY(hipMemcpyAsync(h, derr.p, 12, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h[0] != NO_BAD_POINT) throw std::invalid_argument("pairing: G1 point " + std::to_string(h[0]) + " is not on the curve");
    if (h[1] != NO_BAD_POINT) throw std::invalid_argument("pairing: G2 point " + std::to_string(h[1]) + " is not on the curve");
    if (h[2] != NO_BAD_POINT) throw std::invalid_argument("pairing: G2 point " + std::to_string(h[2]) + " is not in the subgroup");
    HIP_TRY(hipMemcpy(out, dout.p, jobs * sizeof(Fq12), hipMemcpyDeviceToHost));
}

void pairing(uint8_t *out, const uint8_t *g1, const uint8_t *g2, uint64_t n_pairs, uint32_t group, int32_t device) {
    if (!group) throw std::invalid_argument("zk_pairing: group is 0");
    if (!n_pairs) return;
    if (!out || !g1 || !g2) throw std::invalid_argument("null argument");
    const uint64_t jobs = (n_pairs + group - 1) / group, chunk = chunk_jobs();
    const uint64_t cap_jobs = jobs < chunk ? jobs : chunk;
    if (cap_jobs > (1ull << 31) / group) throw std::invalid_argument("zk_pairing: a chunk of " + std::to_string(cap_jobs) + " groups of " + std::to_string(group) + " pairs is too large");
    const uint64_t cap_pairs = cap_jobs * group < n_pairs ? cap_jobs * group : n_pairs;
    const bool coop = jobs <= pairing_coop_max() && n_pairs <= COOP_MAX_PAIRS;
    DeviceGuard g(resolve_device(device));
    t_pairing_path = coop ? ZK_VERIFY_PATH_COOP : ZK_VERIFY_PATH_LANES;
    if (coop) {
        pairing_coop(out, g1, g2, n_pairs, group, jobs);
        return;
    }
    need_hbm("zk_pairing", cap_pairs * (sizeof(G1Affine) + sizeof(G2Affine) + sizeof(G2Proj)) + cap_jobs * 2 * sizeof(Fq12) + 65536);
    Stream st;
    hipStream_t s = st.s;
    Consts kc;
    kc.make(s);
    DevBuf<G1Affine> d1;
    DevBuf<G2Affine> d2;
    DevBuf<G2Proj> dT;
    DevBuf<Fq12> df;
    DevBuf<uint8_t> dout;
    CheckWords cw;
    d1.alloc(cap_pairs);
    d2.alloc(cap_pairs);
    dT.alloc(cap_pairs);
    df.alloc(cap_jobs);
    dout.alloc(cap_jobs * sizeof(Fq12));
    for (uint64_t j0 = 0; j0 < jobs; j0 += cap_jobs) {
        const uint64_t nj = jobs - j0 < cap_jobs ? jobs - j0 : cap_jobs;
        const uint64_t p0 = j0 * group, np = n_pairs - p0 < nj * group ? n_pairs - p0 : nj * group;
        HIP_TRY(hipMemcpyAsync(d1.p, g1 + p0 * sizeof(G1Affine), np * sizeof(G1Affine), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d2.p, g2 + p0 * sizeof(G2Affine), np * sizeof(G2Affine), hipMemcpyHostToDevice, s));
        cw.run(d1.p, np, d2.p, np, s);
        if (cw.h[0] != NO_BAD_POINT) throw std::invalid_argument("pairing: G1 point " + std::to_string(p0 + cw.h[0]) + " is not on the curve");
        if (cw.h[1] != NO_BAD_POINT) throw std::invalid_argument("pairing: G2 point " + std::to_string(p0 + cw.h[1]) + " is not on the curve");
        if (cw.h[2] != NO_BAD_POINT) throw std::invalid_argument("pairing: G2 point " + std::to_string(p0 + cw.h[2]) + " is not in the subgroup");
        ZK_LAUNCH(k_miller_groups, dim3(nblocks(nj, 64)), dim3(64), 0, s, df.p, d1.p, d2.p, dT.p, np, group, kc.k.p);
        ZK_LAUNCH(k_final_exp, dim3(nblocks(nj, 64)), dim3(64), 0, s, dout.p, df.p, nj, kc.k.p);
        ZK_LAUNCH_OK("pairing");
        HIP_TRY(hipMemcpyAsync(out + j0 * sizeof(Fq12), dout.p, nj * sizeof(Fq12), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
}

}   // namespace

namespace {

bool all_zero(const void *p, size_t n) {
    const uint8_t *b = static_cast<const uint8_t *>(p);
    for (size_t i = 0; i < n; i++)
        if (b[i]) return false;
    return true;
}

zk_vkey *vkey_create(const zk_vkey_view *v, int32_t device) {
    if (!v || !v->vk_alpha1 || !v->vk_beta2 || !v->vk_gamma2 || !v->vk_delta2 || !v->IC) throw std::invalid_argument("null argument");
    const void *g2s[3] = {v->vk_beta2, v->vk_gamma2, v->vk_delta2};
    static const char *const g2name[3] = {"vk_beta_2", "vk_gamma_2", "vk_delta_2"};
    if (all_zero(v->vk_alpha1, sizeof(G1Affine))) throw std::invalid_argument("verification key: vk_alpha_1 is the point at infinity");
    for (int i = 0; i < 3; i++)
        if (all_zero(g2s[i], sizeof(G2Affine))) throw std::invalid_argument(std::string("verification key: ") + g2name[i] + " is the point at infinity");
    const uint64_t n1 = (uint64_t)v->nPublic + 2;     // alpha, then IC
    std::unique_ptr<zk_vkey> vk(new zk_vkey);
    vk->device = resolve_device(device);
    vk->nPublic = v->nPublic;
    memcpy(vk->alpha_h, v->vk_alpha1, sizeof vk->alpha_h);
    memcpy(vk->beta_h, v->vk_beta2, sizeof vk->beta_h);
    DeviceGuard g(vk->device);
    need_hbm("zk_vkey_create", n1 * sizeof(G1Affine) + 2 * MILLER_LINES * sizeof(Line) + 65536);
    Stream st;
    hipStream_t s = st.s;
    DevBuf<G1Affine> d1;
    DevBuf<G2Affine> d2;
    DevBuf<Line> dl;                                  // the cooperative Miller loop's lines of beta, its skip byte and error words
    DevBuf<uint8_t> dskip;
    DevBuf<uint32_t> derr;
    d1.alloc(n1);
    d2.alloc(3);
    dl.alloc(MILLER_LINES);
    dskip.alloc(1);
    derr.alloc(3);
    HIP_TRY(hipMemcpyAsync(d1.p, v->vk_alpha1, sizeof(G1Affine), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d1.p + 1, v->IC, (n1 - 1) * sizeof(G1Affine), hipMemcpyHostToDevice, s));
    for (int i = 0; i < 3; i++) HIP_TRY(hipMemcpyAsync(d2.p + i, g2s[i], sizeof(G2Affine), hipMemcpyHostToDevice, s));
    CheckWords cw;
    cw.run(d1.p, n1, d2.p, 3, s);
    if (cw.h[0] == 0) throw std::invalid_argument("verification key: vk_alpha_1 is not on the curve");
    if (cw.h[0] != NO_BAD_POINT) throw std::invalid_argument("verification key: IC point " + std::to_string(cw.h[0] - 1) + " is not on the curve");
    if (cw.h[1] != NO_BAD_POINT) throw std::invalid_argument(std::string("verification key: ") + g2name[cw.h[1]] + " is not on the curve");
    if (cw.h[2] != NO_BAD_POINT) throw std::invalid_argument(std::string("verification key: ") + g2name[cw.h[2]] + " is not in the subgroup");
    vk->kc.make(s);
    vk->ic.alloc(n1 - 1);
    vk->tab.alloc(2 * MILLER_LINES);
    vk->ml_ab.alloc(1);
    HIP_TRY(hipMemcpyAsync(vk->ic.p, d1.p + 1, (n1 - 1) * sizeof(G1Affine), hipMemcpyDeviceToDevice, s));
    ZK_LAUNCH(k_line_table, dim3(1), dim3(64), 0, s, vk->tab.p, d2.p + 1, 2u, vk->kc.k.p);
    // the Miller value of (alpha, beta): the cooperative loop, or a lane of k_miller_groups when ZKHIP_PAIRING_COOP_MAX is 0
    // (read once, after every check of the key, so a key's own error comes before a malformed variable's)
    const bool coop_ab = pairing_coop_max() != 0;
    DevBuf<G2Proj> dT;
    if (!coop_ab) {
        dT.alloc(1);
        ZK_LAUNCH(k_miller_groups, dim3(1), dim3(64), 0, s, vk->ml_ab.p, d1.p, d2.p, dT.p, (uint64_t)1, 1u, vk->kc.k.p);
    }
    ZK_LAUNCH_OK("verification key set-up");
    if (coop_ab) launch_pairing_coop(reinterpret_cast<uint8_t *>(vk->ml_ab.p), d1.p, d2.p, dl.p, dskip.p, derr.p, 1, 1, 0, vk->kc.k.p, s);
    HIP_TRY(hipStreamSynchronize(s));
    return vk.release();
}

}   // namespace

void zkp::vkey_verify_locked(zk_vkey *vk, const uint8_t *proofs, const uint8_t *publics, uint64_t n, uint8_t *verdict) {
    const uint64_t coop_max = verify_coop_max();
    const uint64_t chunk = chunk_jobs(), cap = n < chunk ? n : chunk, pub_bytes = (uint64_t)vk->nPublic * 32;
    DeviceGuard g(vk->device);
    vk->plan.coop_max = (uint32_t)coop_max;
    if (n <= coop_max && n <= COOP_MAX_PROOFS) {
        zk_vkey::Coop &c = vk->coop;
        if (!c.st) c.st.reset(new Stream);
        if (c.cap < n) {
            need_hbm("zk_vkey_verify", n * (256 + pub_bytes + 1 + MILLER_LINES * sizeof(Line)) + 65536);
            c.cap = 0;
            c.dp.alloc(n * 256);
            c.dv.alloc(n);
            c.dpub.alloc(n * vk->nPublic);
            c.lines.alloc(n * MILLER_LINES);
            c.cap = n;
        }
        hipStream_t s = c.st->s;
        HIP_TRY(hipMemcpyAsync(c.dp.p, proofs, n * 256, hipMemcpyHostToDevice, s));
        if (pub_bytes) HIP_TRY(hipMemcpyAsync(c.dpub.p, publics, n * pub_bytes, hipMemcpyHostToDevice, s));
        launch_verify_coop(c.dv.p, c.dp.p, c.dpub.p, n, vk->nPublic, vk->ic.p, vk->tab.p, vk->ml_ab.p, vk->kc.k.p, c.lines.p, s);
        HIP_TRY(hipMemcpyAsync(verdict, c.dv.p, n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        vk->plan.last_path = ZK_VERIFY_PATH_COOP;
        vk->plan.last_launches = 1;
        vk->plan.proofs_coop += n;
        return;
    }
    vk->plan.last_path = ZK_VERIFY_PATH_LANES;
    vk->plan.last_launches = 0;
    need_hbm("zk_vkey_verify", cap * (256 + pub_bytes + 4 + sizeof(G1Affine) + sizeof(Fq12) + 1) + 65536);
    Stream st;
    hipStream_t s = st.s;
    DevBuf<uint8_t> dp, dv;
    DevBuf<Fr> dpub;
    DevBuf<uint32_t> dst;
    DevBuf<G1Affine> dx;
    DevBuf<Fq12> df;
    dp.alloc(cap * 256);
    dv.alloc(cap);
    dpub.alloc(cap * vk->nPublic);
    dst.alloc(cap);
    dx.alloc(cap);
    df.alloc(cap);
    for (uint64_t off = 0; off < n; off += cap) {
        const uint64_t cnt = n - off < cap ? n - off : cap;
        const dim3 grid(nblocks(cnt, 64)), block(64);
        HIP_TRY(hipMemcpyAsync(dp.p, proofs + off * 256, cnt * 256, hipMemcpyHostToDevice, s));
        if (pub_bytes) HIP_TRY(hipMemcpyAsync(dpub.p, publics + off * pub_bytes, cnt * pub_bytes, hipMemcpyHostToDevice, s));
        ZK_LAUNCH(k_verify_check, grid, block, 0, s, dst.p, dx.p, dp.p, dpub.p, cnt, vk->nPublic, vk->ic.p, curve_b<Fq>(), curve_b<Fq2>());
        ZK_LAUNCH(k_verify_miller, grid, block, 0, s, df.p, dst.p, dp.p, dx.p, vk->tab.p, vk->ml_ab.p, cnt, vk->kc.k.p);
        ZK_LAUNCH(k_verify_final, grid, block, 0, s, dv.p, df.p, dst.p, cnt, vk->kc.k.p);
        ZK_LAUNCH_OK("verification");
        HIP_TRY(hipMemcpyAsync(verdict + off, dv.p, cnt, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        vk->plan.last_launches += 3;
        vk->plan.proofs_lanes += cnt;
    }
}

namespace {

void vkey_verify(zk_vkey *vk, const uint8_t *proofs, const uint8_t *publics, uint64_t n, uint8_t *verdict) {
    if (!vk) throw std::invalid_argument("null argument");
    if (!n) return;
    if (!proofs || !verdict || (vk->nPublic && !publics)) throw std::invalid_argument("null argument");
    std::lock_guard<std::mutex> lock(vk->mu);
    vkey_verify_locked(vk, proofs, publics, n, verdict);
}

}   // namespace

extern "C" {

int zk_pairing(uint8_t *out, const uint8_t *g1, const uint8_t *g2, uint64_t n_pairs, uint32_t group, int32_t device) {
    return guarded([&] { pairing(out, g1, g2, n_pairs, group, device); });
}

int zk_vkey_create(zk_vkey **out, const zk_vkey_view *view, int32_t device) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        *out = vkey_create(view, device);
    });
}

void zk_vkey_destroy(zk_vkey *vk) {
    if (!vk) return;
    int prev = -1;
    const bool had = hipGetDevice(&prev) == hipSuccess;
    (void)hipSetDevice(vk->device);
    delete vk;
    if (had) (void)hipSetDevice(prev);
}

int zk_vkey_info(zk_vkey *vk, zk_vkey_plan *plan) {
    return guarded([&] {
        if (!vk || !plan) throw std::invalid_argument("null argument");
        std::lock_guard<std::mutex> lock(vk->mu);
        *plan = vk->plan;
    });
}

int zk_pairing_last_path(void) { return t_pairing_path; }

int zk_vkey_verify(zk_vkey *vk, const uint8_t *proofs, const uint8_t *publics, uint64_t n, uint8_t *verdict) {
    return guarded([&] { vkey_verify(vk, proofs, publics, n, verdict); });
}

}   // extern "C"
