// PLONK rounds 4 and 5 (include/zkhip.h, section "PLONK evaluations and opening proofs"): the six evaluations at zeta and
// zeta w, the linearisation polynomial, and the two opening proofs W_zeta and W_(zeta w).  Nothing in the reference
// corresponds to it (it proves Groth16 only); the counterpart is rounds 4 and 5 of snarkjs's PLONK prover.  DESIGN.md
// section 30 states the identities, the count of products and bytes and what was measured.
//
//     r(X) = a' b' qM + a' qL + b' qR + c' qO + PI(zeta) + qC
//          + alpha [ (a' + beta zeta + gamma)(b' + beta k1 zeta + gamma)(c' + beta k2 zeta + gamma) z(X)
//                  - (a' + beta s1' + gamma)(b' + beta s2' + gamma)(c' + beta s3(X) + gamma) z'w ]
//          + alpha^2 (z(X) - 1) L1(zeta) - Z_H(zeta) (t_lo + zeta^n t_mid + zeta^2n t_hi)
//     F(X) = r + v a + v^2 b + v^3 c + v^4 s1 + v^5 s2           (a' = a(zeta), .., z'w = z(zeta w))
// Per coefficient F is a sum of 14 rows times scalars the host makes, q_C with weight 1 and one constant at index 0
// (lin_consts below).  The divisions by X - zeta and X - zeta w and the two multiplications are kzg.hip's, untouched
// (kzg_internal.hpp); the remainder of the first division is F(zeta), so r(zeta) = F(zeta) - E costs nothing.
//
// New here: k_poly_eval and k_poly_eval_finish (m polynomials, each at its own point, in two launches) and k_plonk_linearise.
// Lane map of k_poly_eval and k_plonk_linearise: plonkquot.hip's.  T lanes in the grid (a multiple of 256), lane l takes the
// coefficients l, l + T, l + 2T, .. : `seg` of them (ZKHIP_OPEN_SEG, read at every call), so neighbouring lanes touch
// neighbouring rows at any seg.  An evaluating lane runs Horner in z^T (the host's) and multiplies ONCE by z^l, from the bits
// of l over a host-made record of z^(2^b) (lanepow.hpp).  The lanes' sums meet by shuffles within a wave, in LDS across the four waves, one
// row per workgroup goes to a vector of partial sums, and k_poly_eval_finish (a workgroup per polynomial) adds those.  No
// atomics; the sums are exact field additions, so no byte depends on seg or on scheduling.
//
// Form: field.hpp's 8 x 32-bit Fr, as kzg.hip's division.  Every vector stays in STANDARD form: the scalars and the powers
// are Montgomery, and a Montgomery product of a standard value with such a scalar is standard, so F is what the division
// reads and the quotient what the sort of the multiplication reads.  One operand term per reduction: no ranges to state.
#include "lanepow.hpp"
#include "plonk_internal.hpp"
#include "plonk_transcript.hpp"

namespace {

constexpr uint32_t OP_WG = 256;
constexpr uint32_t DEFAULT_SEG = 16, MAX_SEG = 4096;  // the default: profiles/plonk_opening_timing.txt, the best whole call at log_n 22 (at 18 seg 4's is 10 % shorter)
constexpr uint32_t MAX_GRID_Y = 65535;
constexpr uint32_t CIRC_VECS = 8, WIT_VECS = 4, T_VECS = 3, EVALS = 6;
enum { C_QL, C_QR, C_QM, C_QO, C_QC, C_S1, C_S2, C_S3 };           // the resident coefficient rows, the view's order
enum { W_A, W_B, W_C, W_Z };                                        // round 4's
// the rows of F that carry a scalar, and q_C (weight 1)
enum { R_QM, R_QL, R_QR, R_QO, R_Z, R_S3, R_TLO, R_TMID, R_THI, R_A, R_B, R_C, R_S1, R_S2, LIN_SCALED, R_QC = LIN_SCALED, LIN_ROWS };

// ---------------------------------------------------------------- device
// The powers of one point z for T lanes, Montgomery: z^T and z^(2^b) (lanepow.hpp)
typedef PowTab EvalConsts;
struct EvalJob {
    const Fr *c;                                      // n coefficients, standard
    uint64_t n;
    uint32_t k, pad;                                  // the index of its point's record
};

__device__ __forceinline__ Fr shfl_xor_fr(const Fr &a, uint32_t d) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = __shfl_xor(a.v[i], d, 64);
    return r;
}
// the sum of `v` over the workgroup, in lane 0 (sh: a row per wave)
__device__ __forceinline__ Fr workgroup_sum(Fr v, Fr *sh) {
#pragma unroll 1
    for (uint32_t d = 32; d; d >>= 1) v = Fr::add(v, shfl_xor_fr(v, d));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (uint32_t j = 1; j < OP_WG / 64; j++) v = Fr::add(v, sh[j]);
    return v;
}

// partials[y * gridDim.x + x] = the sum over workgroup x's lanes of sum_k c[l + k T] z^(l + k T), for polynomial y
__global__ __launch_bounds__(OP_WG) void k_poly_eval(Fr *partials, const EvalJob *__restrict__ jobs, const EvalConsts *__restrict__ consts, uint32_t seg) {
    __shared__ Fr sh[OP_WG / 64];
    const uint64_t T = (uint64_t)gridDim.x * OP_WG, l = (uint64_t)blockIdx.x * OP_WG + threadIdx.x;
    const EvalJob job = jobs[blockIdx.y];
    const EvalConsts *K = consts + job.k;
    Fr acc = Fr::zero();
    if (l < job.n) {
        const uint64_t left = (job.n - l + T - 1) / T;                // the lane's coefficients: l + k T < n
        const uint32_t cnt = left < seg ? (uint32_t)left : seg;
        const Fr step = load_uniform(&K->step);
        const Fr *c = job.c + l;
        acc = load_el(c + (uint64_t)(cnt - 1) * T);
#pragma unroll 1
        for (uint32_t k = cnt - 1; k-- > 0;) acc = Fr::add(load_el(c + (uint64_t)k * T), Fr::mul(acc, step));
#pragma unroll 1
        for (uint32_t b = 0; b < POW_TAB && (l >> b); b++)
            if ((l >> b) & 1) acc = Fr::mul(acc, load_el(K->tab + b));
    }
    acc = workgroup_sum(acc, sh);
    if (threadIdx.x == 0) store_el(partials + (uint64_t)blockIdx.y * gridDim.x + blockIdx.x, acc);
}

// ys[y] = the sum of polynomial y's `blocks` partial sums: canonical, standard
__global__ __launch_bounds__(OP_WG) void k_poly_eval_finish(Fr *ys, const Fr *__restrict__ partials, uint32_t blocks) {
    __shared__ Fr sh[OP_WG / 64];
    const Fr *p = partials + (uint64_t)blockIdx.x * blocks;
    Fr acc = Fr::zero();
#pragma unroll 1
    for (uint32_t i = threadIdx.x; i < blocks; i += OP_WG) acc = Fr::add(acc, load_el(p + i));
    acc = workgroup_sum(acc, sh);
    if (threadIdx.x == 0) store_el(ys + blockIdx.x, acc);
}

// The scalars of one linearisation, Montgomery, and the constant of index 0, standard
struct LinConsts {
    Fr s[LIN_SCALED];
    Fr c0;
};
struct LinArgs {
    const Fr *row[LIN_ROWS];
    uint64_t len[LIN_ROWS];                           // each >= 1; a row reads as zero beyond its length
    Fr *out;
    uint64_t L;                                       // the largest length
    uint32_t seg;
    const LinConsts *k;
};
// out[i] = qC[i] + sum_r s_r row_r[i] (+ c0 at i = 0) for i < L: 14 products and 16 rows of traffic an index.  An index
// beyond a row's length loads the row's last element and drops it: every load is unconditional and may be issued early
__device__ __forceinline__ Fr row_at(const LinArgs &A, int r, uint64_t i) {
    const uint64_t len = A.len[r];
    const Fr x = load_el(A.row[r] + (i < len ? i : len - 1));
    return i < len ? x : Fr::zero();
}
__global__ __launch_bounds__(OP_WG) void k_plonk_linearise(LinArgs A) {
    const uint64_t T = (uint64_t)gridDim.x * OP_WG, l = (uint64_t)blockIdx.x * OP_WG + threadIdx.x;
    if (l >= A.L) return;
    // the 14 scalars by name, not as an array: an array indexed in a loop went to scratch
#define LIN_EACH(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13)
#define LIN_SCALAR(r) const Fr s##r = load_uniform(A.k->s + r);
#define LIN_TERM(r) acc = Fr::add(acc, Fr::mul(row_at(A, r, i), s##r));
    static_assert(LIN_SCALED == 14, "LIN_EACH names every scaled row");
    LIN_EACH(LIN_SCALAR)
#pragma unroll 1
    for (uint32_t k = 0; k < A.seg; k++) {
        const uint64_t i = l + k * T;
        if (i >= A.L) break;
        Fr acc = row_at(A, R_QC, i);
        if (i == 0) acc = Fr::add(acc, load_el(&A.k->c0));
        LIN_EACH(LIN_TERM)
        store_el(A.out + i, acc);
    }
#undef LIN_TERM
#undef LIN_SCALAR
#undef LIN_EACH
}

// ---------------------------------------------------------------- host
uint32_t seg_in_effect() { return (uint32_t)env_number("ZKHIP_OPEN_SEG", DEFAULT_SEG, 1, MAX_SEG, "a number of coefficients per lane from 1 to 4096", ENV_LAX); }

// workgroups for n coefficients at seg a lane
uint32_t blocks_of(uint64_t n, uint32_t seg) { return nblocks(n, OP_WG * seg); }

// the record of one point z (Montgomery) for T lanes
EvalConsts eval_consts(Fr z, uint64_t lanes) {
    return pow_tab(z, lanes, [](Fr a) { return a; });
}

// ys[j] = p_j(z_j) for m jobs on the device: two launches for every MAX_GRID_Y of them (a job names its point's record by
// its index within the launch's MAX_GRID_Y).  partials: m x blocks rows
void launch_eval(Fr *ys, Fr *partials, const EvalJob *jobs, const EvalConsts *consts, uint64_t m, uint32_t blocks, uint32_t seg, hipStream_t s) {
    for (uint64_t at = 0; at < m; at += MAX_GRID_Y) {
        const uint32_t cnt = (uint32_t)(m - at < MAX_GRID_Y ? m - at : MAX_GRID_Y);
        ZK_LAUNCH(k_poly_eval, dim3(blocks, cnt), dim3(OP_WG), 0, s, partials + at * blocks, jobs + at, consts + at, seg);
        ZK_LAUNCH(k_poly_eval_finish, dim3(cnt), dim3(OP_WG), 0, s, ys + at, partials + at * blocks, blocks);
    }
    ZK_LAUNCH_OK("polynomial evaluation");
}

void fr_poly_eval(uint8_t *ys, const uint8_t *coeffs, uint64_t n, uint64_t m, const uint8_t *zs, int32_t device) {
    const char *who = "zk_fr_poly_eval";
    if (!n) throw std::invalid_argument(std::string(who) + ": n is 0");
    if (!m) return;
    if (!ys || !coeffs || !zs) throw std::invalid_argument("null argument");
    if (n >= (1ull << 31)) throw std::invalid_argument(std::string(who) + ": n is not below 2^31");
    const uint32_t seg = seg_in_effect();
    for (uint64_t p = 0; p < m; p++) {
        const uint64_t bad = first_not_below_r(coeffs + p * n * 32, n);
        if (bad < n) throw std::invalid_argument(std::string(who) + ": polynomial " + std::to_string(p) + ", coefficient " + std::to_string(bad) + " is not below r");
    }
    check_below_r(who, "z", zs, m);
    const uint32_t blocks = blocks_of(n, seg);
    const uint64_t lanes = (uint64_t)blocks * OP_WG;
    DeviceGuard dg(resolve_device(device));
    need_hbm(who, (m * n + m * blocks + m) * sizeof(Fr) + m * (sizeof(EvalJob) + sizeof(EvalConsts)));
    Stream st;
    hipStream_t s = st.s;
    DevBuf<Fr> dc, part, dy;
    DevBuf<EvalJob> dj;
    DevBuf<EvalConsts> dk;
    dc.alloc(m * n);
    part.alloc(m * blocks);
    dy.alloc(m);
    dj.alloc(m);
    dk.alloc(m);
    std::vector<EvalJob> jobs(m);
    std::vector<EvalConsts> consts(m);
    for (uint64_t p = 0; p < m; p++) {
        jobs[p] = EvalJob{dc.p + p * n, n, (uint32_t)(p % MAX_GRID_Y), 0};
        consts[p] = eval_consts(fr_from_std(zs + p * 32), lanes);
    }
    HIP_TRY(hipMemcpyAsync(dc.p, coeffs, m * n * sizeof(Fr), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(dj.p, jobs.data(), m * sizeof(EvalJob), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(dk.p, consts.data(), m * sizeof(EvalConsts), hipMemcpyHostToDevice, s));
    launch_eval(dy.p, part.p, dj.p, dk.p, m, blocks, seg, s);
    HIP_TRY(hipMemcpyAsync(ys, dy.p, m * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
}

}   // namespace

// ---------------------------------------------------------------- the object
struct zk_plonk_opening {
    zk_kzg *kzg = nullptr;                            // borrowed: it outlives the object
    int device = 0;
    uint32_t log_n = 0;
    uint64_t n = 0, cap = 0;                          // cap: the kzg's max_coeffs, the longest vector a call takes
    std::mutex mu;                                    // calls on one object are serialised
    std::unique_ptr<Stream> st;
    Fr k1, k2, w;                                     // Montgomery
    DevBuf<Fr> circ;                                  // CIRC_VECS x n coefficients
    DevBuf<Fr> wit;                                   // WIT_VECS x cap: a, b, c, z from round 4
    DevBuf<Fr> tp;                                    // T_VECS x cap: the parts of t
    DevBuf<Fr> f, quot;                               // cap each: F and a quotient
    DevBuf<Fr> ev, yv, part;                          // the six values; F(zeta) and z(zeta w) again; the partial sums
    DevBuf<EvalJob> jobs;
    DevBuf<EvalConsts> ek;                            // [0] zeta, [1] zeta w
    DevBuf<LinConsts> lk;
    DivWork div;
    EvalJob hj[EVALS];                                // host images: they outlive the copies (the stream is drained before the next call)
    EvalConsts hek[2];
    LinConsts hlk;
    bool pending = false;                             // round 4's state, consumed by round 5
    uint64_t lens[WIT_VECS] = {0, 0, 0, 0};
    Fr zeta, evals[EVALS];                            // Montgomery
    uint32_t last_launches = 0;
    size_t bytes() const {
        return circ.bytes() + wit.bytes() + tp.bytes() + f.bytes() + quot.bytes() + ev.bytes() + yv.bytes() + part.bytes() + jobs.bytes() + ek.bytes() +
               lk.bytes() + div.bytes();
    }
};

namespace {

uint64_t resident_bytes(uint64_t n, uint64_t cap) {
    return (CIRC_VECS * n + (WIT_VECS + T_VECS + 2) * cap + (uint64_t)EVALS * blocks_of(cap, 1) + EVALS + 2) * sizeof(Fr) +
           DivWork::groups_of(cap, 1) * 6 * sizeof(Fr) + EVALS * sizeof(EvalJob) + 2 * sizeof(EvalConsts) + sizeof(LinConsts) + 65536;
}

// the object from a view that was checked and fits the kzg (plonk_internal.hpp: the public entry's, or a prover's)
zk_plonk_opening *opening_make(zk_kzg *kzg, const CheckedView &cv) {
    const char *who = "zk_plonk_opening_create";
    const uint8_t *const *vec = cv.vec;
    const uint64_t n = cv.n, cap = kzg->max_coeffs;
    std::unique_ptr<zk_plonk_opening> o(new zk_plonk_opening());
    o->kzg = kzg, o->device = kzg->device, o->log_n = cv.log_n, o->n = n, o->cap = cap;
    o->k1 = cv.k1, o->k2 = cv.k2;
    o->w = root_of_unity(cv.log_n);
    DeviceGuard dg(o->device);
    need_hbm(who, resident_bytes(n, cap) + (cv.lagrange ? 2 * n * sizeof(Fr) : 0));
    o->st.reset(new Stream());
    hipStream_t s = o->st->s;
    LaunchCount lc(o->last_launches);
    o->circ.alloc(CIRC_VECS * n);
    o->wit.alloc(WIT_VECS * cap);
    o->tp.alloc(T_VECS * cap);
    o->f.alloc(cap);
    o->quot.alloc(cap);
    o->ev.alloc(EVALS);
    o->yv.alloc(2);
    o->part.alloc((uint64_t)EVALS * blocks_of(cap, 1));
    o->jobs.alloc(EVALS);
    o->ek.alloc(2);
    o->lk.alloc(1);
    o->div.size(DivWork::groups_of(cap, 1));
    if (cv.lagrange) {
        // values at w^j -> coefficients: zk_fr_ntt's inverse transform on a copy, vector by vector (once in the object's life)
        std::vector<uint8_t> co(n * 32);
        for (uint32_t j = 0; j < CIRC_VECS; j++) {
            memcpy(co.data(), vec[j], n * 32);
            if (zk_fr_ntt(co.data(), n, 1) != 0) throw std::runtime_error(std::string(who) + ": " + zk_last_error());
            HIP_TRY(hipMemcpyAsync(o->circ.p + j * n, co.data(), n * sizeof(Fr), hipMemcpyHostToDevice, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
    } else {
        for (uint32_t j = 0; j < CIRC_VECS; j++) HIP_TRY(hipMemcpyAsync(o->circ.p + j * n, vec[j], n * sizeof(Fr), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return o.release();
}

zk_plonk_opening *opening_create(zk_kzg *kzg, const zk_plonk_circuit_view *v, int32_t device) {
    const char *who = "zk_plonk_opening_create";
    if (!kzg || !v) throw std::invalid_argument("null argument");
    CheckedView cv = checked_view_dims(who, v, 1);
    if (cv.n + 6 > kzg->max_coeffs)
        throw std::invalid_argument(std::string(who) + ": n + 6 = " + std::to_string(cv.n + 6) + " exceeds the kzg's max_coeffs = " + std::to_string(kzg->max_coeffs));
    if (device >= 0 && device != kzg->device)
        throw std::invalid_argument(std::string(who) + ": device " + std::to_string(device) + " is not the kzg's device " + std::to_string(kzg->device));
    checked_view_rows(who, v, cv);
    return opening_make(kzg, cv);
}

// Round 4 over the rows already in o->wit, len[] of them each: the two launches, the six values to the host, and the state
// round 5 consumes.  The caller holds the object (its mutex, or as its only owner) and has set the device
void evaluate_dev(zk_plonk_opening *o, uint8_t *evals, const uint64_t len[WIT_VECS], const Fr &ze, uint32_t seg, hipStream_t s) {
    o->pending = false;
    const uint64_t n = o->n, cap = o->cap;
    uint64_t longest = n;
    for (uint32_t j = 0; j < WIT_VECS; j++) longest = len[j] > longest ? len[j] : longest;
    const uint32_t blocks = blocks_of(longest, seg);
    const uint64_t lanes = (uint64_t)blocks * OP_WG;
    o->hek[0] = eval_consts(ze, lanes);
    o->hek[1] = eval_consts(Fr::mul(ze, o->w), lanes);
    // a, b, c, s1, s2 at zeta and z at zeta w: the order of the result
    o->hj[0] = EvalJob{o->wit.p + W_A * cap, len[W_A], 0, 0};
    o->hj[1] = EvalJob{o->wit.p + W_B * cap, len[W_B], 0, 0};
    o->hj[2] = EvalJob{o->wit.p + W_C * cap, len[W_C], 0, 0};
    o->hj[3] = EvalJob{o->circ.p + C_S1 * n, n, 0, 0};
    o->hj[4] = EvalJob{o->circ.p + C_S2 * n, n, 0, 0};
    o->hj[5] = EvalJob{o->wit.p + W_Z * cap, len[W_Z], 1, 0};
    HIP_TRY(hipMemcpyAsync(o->ek.p, o->hek, sizeof o->hek, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(o->jobs.p, o->hj, sizeof o->hj, hipMemcpyHostToDevice, s));
    launch_eval(o->ev.p, o->part.p, o->jobs.p, o->ek.p, EVALS, blocks, seg, s);
    HIP_TRY(hipMemcpyAsync(evals, o->ev.p, EVALS * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t j = 0; j < EVALS; j++) o->evals[j] = fr_from_std(evals + j * 32);
    for (uint32_t j = 0; j < WIT_VECS; j++) o->lens[j] = len[j];
    o->zeta = ze;
    o->pending = true;
}

void plonk_evaluate(zk_plonk_opening *o, uint8_t *evals, const uint8_t *const in[WIT_VECS], const uint64_t len[WIT_VECS], const uint8_t *zeta) {
    const char *who = "zk_plonk_evaluate";
    const uint32_t seg = seg_in_effect();
    if (!o || !evals || !in[W_A] || !in[W_B] || !in[W_C] || !in[W_Z] || !zeta) throw std::invalid_argument("null argument");
    static const char *const names[WIT_VECS] = {"a", "b", "c", "z"};
    for (uint32_t j = 0; j < WIT_VECS; j++)
        if (len[j] < 1 || len[j] > o->cap)
            throw std::invalid_argument(std::string(who) + ": " + names[j] + "_len " + std::to_string(len[j]) + " is outside 1 .. max_coeffs = " + std::to_string(o->cap));
    for (uint32_t j = 0; j < WIT_VECS; j++) check_below_r(who, names[j], in[j], len[j]);
    const Fr ze = checked_one(who, "zeta", zeta);
    std::lock_guard<std::mutex> lock(o->mu);
    DeviceGuard dg(o->device);
    LaunchCount lc(o->last_launches);
    hipStream_t s = o->st->s;
    o->pending = false;
    for (uint32_t j = 0; j < WIT_VECS; j++) HIP_TRY(hipMemcpyAsync(o->wit.p + j * o->cap, in[j], len[j] * sizeof(Fr), hipMemcpyHostToDevice, s));
    evaluate_dev(o, evals, len, ze, seg, s);
}

// What the host makes of the six values and the challenges (plonk_transcript.hpp's, the verifier's too): F's scalars, the
// constant of index 0, and E.  One inversion
LinConsts lin_consts(const zk_plonk_opening &o, Fr pi_zeta, Fr alpha, Fr beta, Fr gamma, Fr v, Fr *E) {
    AtZeta z = zeta_powers(o.log_n, o.zeta);
    z.pi = pi_zeta;
    const LinScalars L = lin_scalars(o.evals, z, o.zeta, o.k1, o.k2, alpha, beta, gamma, v);
    LinConsts k;
    k.s[R_QM] = L.qm, k.s[R_QL] = o.evals[0], k.s[R_QR] = o.evals[1], k.s[R_QO] = o.evals[2];
    k.s[R_Z] = L.z, k.s[R_S3] = L.s3, k.s[R_TLO] = L.tlo, k.s[R_TMID] = L.tmid, k.s[R_THI] = L.thi;
    for (int j = 0; j < 5; j++) k.s[R_A + j] = L.v[j];
    k.c0 = Fr::from_mont(L.c0);
    *E = L.E;
    return k;
}

// Round 5 over the parts of t already in o->tp, tlen[] rows each, and the pending evaluation's rows and values (the caller
// has consumed `pending`): the linearisation, the two divisions and the two multiplications.  Held as evaluate_dev
void open_dev(zk_plonk_opening *o, uint8_t *w_zeta, uint8_t *w_zeta_omega, uint8_t *r_zeta, uint8_t *f, uint64_t *f_len, const uint64_t tlen[T_VECS],
              const Fr &pz, const Fr &al, const Fr &be, const Fr &ga, const Fr &vv, uint32_t seg, uint32_t dseg, hipStream_t s, bool pad = false,
              Fr *const *qrows = nullptr) {
    zk_kzg *k = o->kzg;
    const uint64_t n = o->n, cap = o->cap;
    Fr E;
    o->hlk = lin_consts(*o, pz, al, be, ga, vv, &E);
    HIP_TRY(hipMemcpyAsync(o->lk.p, &o->hlk, sizeof o->hlk, hipMemcpyHostToDevice, s));
    LinArgs A{};
    auto row = [&](int r, const Fr *p, uint64_t len) { A.row[r] = p, A.len[r] = len, A.L = len > A.L ? len : A.L; };
    row(R_QM, o->circ.p + C_QM * n, n), row(R_QL, o->circ.p + C_QL * n, n), row(R_QR, o->circ.p + C_QR * n, n), row(R_QO, o->circ.p + C_QO * n, n);
    row(R_QC, o->circ.p + C_QC * n, n), row(R_S3, o->circ.p + C_S3 * n, n), row(R_S1, o->circ.p + C_S1 * n, n), row(R_S2, o->circ.p + C_S2 * n, n);
    row(R_A, o->wit.p + W_A * cap, o->lens[W_A]), row(R_B, o->wit.p + W_B * cap, o->lens[W_B]), row(R_C, o->wit.p + W_C * cap, o->lens[W_C]);
    row(R_Z, o->wit.p + W_Z * cap, o->lens[W_Z]);
    row(R_TLO, o->tp.p, tlen[0]), row(R_TMID, o->tp.p + cap, tlen[1]), row(R_THI, o->tp.p + 2 * cap, tlen[2]);
    A.out = o->f.p, A.seg = seg, A.k = o->lk.p;
    const uint64_t L = A.L;                            // <= cap: every length is
    ZK_LAUNCH(k_plonk_linearise, dim3(blocks_of(L, seg)), dim3(OP_WG), 0, s, A);
    ZK_LAUNCH_OK("plonk linearise");
    if (f) {
        HIP_TRY(hipMemcpyAsync(f, o->f.p, L * sizeof(Fr), hipMemcpyDeviceToHost, s));
        memset(f + L * 32, 0, (cap - L) * 32);
    }
    if (f_len) *f_len = L;
    // W_zeta: F / (X - zeta), the remainder is F(zeta); W_(zeta w): z / (X - zeta w).  F and the quotients stay on the device
    Fr fz;
    const Fr zw = Fr::mul(o->zeta, o->w);
    const Fr *src[2] = {o->f.p, o->wit.p + W_Z * cap};
    const uint64_t cnt[2] = {L, o->lens[W_Z]};
    const Fr at[2] = {o->zeta, zw};
    uint8_t *out[2] = {w_zeta, w_zeta_omega};
    for (int j = 0; j < 2; j++) {
        launch_divide(qrows ? qrows[j] : o->quot.p, o->yv.p + j, src[j], cnt[j], at[j], dseg, o->div, s);
        if (j == 0) HIP_TRY(hipMemcpyAsync(&fz, o->yv.p, sizeof fz, hipMemcpyDeviceToHost, s));
        if (qrows) {
            // the caller's rows (a prover that multiplies many proofs' quotients at once): the quotient stays where it was
            // divided to, the one row above it zeroed as `pad` zeroes it, and nothing is multiplied here
            HIP_TRY(hipMemsetAsync(qrows[j] + (cnt[j] - 1), 0, sizeof(Fr), s));
            if (j == 1) HIP_TRY(hipStreamSynchronize(s));       // F(zeta) is on the host
        } else if (cnt[j] > 1) {
            std::lock_guard<std::mutex> kl(k->mu);     // the kzg's points and the work buffers of its multiplication
            // pad (the chained prover's): the multiplication runs over one row more than the quotient has, zeroed here after the
            // division (stream order), so that it has the size of the prover's seven others and the kzg's buffers are not made
            // again; cnt[j] <= cap rows are there.  A zero scalar adds nothing: the point is the same
            if (pad) HIP_TRY(hipMemsetAsync(o->quot.p + (cnt[j] - 1), 0, sizeof(Fr), s));
            msm_resident(k->msm, out[j], k->tau.p, o->quot.p, pad ? cnt[j] : cnt[j] - 1, s);
        } else {
            memset(out[j], 0, 64);
            HIP_TRY(hipStreamSynchronize(s));
        }
    }
    const Fr r = Fr::sub(fz, Fr::from_mont(E));         // both standard
    memcpy(r_zeta, r.v, 32);
}

void plonk_open(zk_plonk_opening *o, uint8_t *w_zeta, uint8_t *w_zeta_omega, uint8_t *r_zeta, uint8_t *f, uint64_t *f_len, const uint8_t *const t[T_VECS],
                const uint64_t tlen[T_VECS], const uint8_t *pi_zeta, const uint8_t *alpha, const uint8_t *beta, const uint8_t *gamma, const uint8_t *v) {
    const char *who = "zk_plonk_open";
    const uint32_t seg = seg_in_effect(), dseg = kzg_seg_in_effect();
    if (!o || !w_zeta || !w_zeta_omega || !r_zeta || !t[0] || !t[1] || !t[2] || !alpha || !beta || !gamma || !v || (f && !f_len))
        throw std::invalid_argument("null argument");
    static const char *const names[T_VECS] = {"t_lo", "t_mid", "t_hi"};
    static const char *const lnames[T_VECS] = {"lo_len", "mid_len", "hi_len"};
    for (uint32_t j = 0; j < T_VECS; j++)
        if (tlen[j] < 1 || tlen[j] > o->cap)
            throw std::invalid_argument(std::string(who) + ": " + lnames[j] + " " + std::to_string(tlen[j]) + " is outside 1 .. max_coeffs = " + std::to_string(o->cap));
    for (uint32_t j = 0; j < T_VECS; j++) check_below_r(who, names[j], t[j], tlen[j]);
    const Fr pz = pi_zeta ? checked_one(who, "pi_zeta", pi_zeta) : Fr::zero();
    const Fr al = checked_one(who, "alpha", alpha), be = checked_one(who, "beta", beta), ga = checked_one(who, "gamma", gamma), vv = checked_one(who, "v", v);
    std::lock_guard<std::mutex> lock(o->mu);
    if (!o->pending) throw std::invalid_argument(std::string(who) + ": no evaluation is pending: call zk_plonk_evaluate first");
    o->pending = false;
    DeviceGuard dg(o->device);
    LaunchCount lc(o->last_launches);
    hipStream_t s = o->st->s;
    for (uint32_t j = 0; j < T_VECS; j++) HIP_TRY(hipMemcpyAsync(o->tp.p + j * o->cap, t[j], tlen[j] * sizeof(Fr), hipMemcpyHostToDevice, s));
    open_dev(o, w_zeta, w_zeta_omega, r_zeta, f, f_len, tlen, pz, al, be, ga, vv, seg, dseg, s);
}

}   // namespace

// ---------------------------------------------------------------- what plonkprove.hip chains (plonk_internal.hpp)
uint32_t plonk_open_seg() { return seg_in_effect(); }
zk_plonk_opening *plonk_opening_make(zk_kzg *kzg, const CheckedView &cv) { return opening_make(kzg, cv); }
uint64_t plonk_opening_need_bytes(uint64_t n, uint64_t cap, bool lagrange) { return resident_bytes(n, cap) + (lagrange ? 2 * n * sizeof(Fr) : 0); }
size_t plonk_opening_bytes(const zk_plonk_opening *o) { return o->bytes(); }
Fr *plonk_opening_wit(zk_plonk_opening *o, uint32_t j) { return o->wit.p + j * o->cap; }
Fr *plonk_opening_part(zk_plonk_opening *o, uint32_t j) { return o->tp.p + j * o->cap; }
const Fr *plonk_opening_circ(const zk_plonk_opening *o, uint32_t j) { return o->circ.p + j * o->n; }
void plonk_opening_clear(zk_plonk_opening *o, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(o->wit.p, 0, o->wit.bytes(), s));
    HIP_TRY(hipMemsetAsync(o->tp.p, 0, o->tp.bytes(), s));
}
void plonk_opening_evaluate_dev(zk_plonk_opening *o, uint8_t evals[6 * 32], const uint64_t len[4], const Fr &zeta, hipStream_t s) {
    evaluate_dev(o, evals, len, zeta, seg_in_effect(), s);
}
void plonk_opening_open_dev(zk_plonk_opening *o, uint8_t w_zeta[64], uint8_t w_zeta_omega[64], uint8_t r_zeta[32], uint8_t *f, uint64_t *f_len,
                            const uint64_t tlen[3], const Fr &pi_zeta, const Fr &alpha, const Fr &beta, const Fr &gamma, const Fr &v, hipStream_t s) {
    if (!o->pending) throw std::invalid_argument("zk_plonk_open: no evaluation is pending: call zk_plonk_evaluate first");
    o->pending = false;
    open_dev(o, w_zeta, w_zeta_omega, r_zeta, f, f_len, tlen, pi_zeta, alpha, beta, gamma, v, seg_in_effect(), kzg_seg_in_effect(), s, /*pad=*/true);
}
void plonk_opening_open_rows_dev(zk_plonk_opening *o, Fr *q_zeta, Fr *q_zeta_omega, uint8_t r_zeta[32], const uint64_t tlen[3], const Fr &pi_zeta,
                                 const Fr &alpha, const Fr &beta, const Fr &gamma, const Fr &v, hipStream_t s) {
    if (!o->pending) throw std::invalid_argument("zk_plonk_open: no evaluation is pending: call zk_plonk_evaluate first");
    o->pending = false;
    Fr *const qrows[2] = {q_zeta, q_zeta_omega};
    open_dev(o, nullptr, nullptr, r_zeta, nullptr, nullptr, tlen, pi_zeta, alpha, beta, gamma, v, seg_in_effect(), kzg_seg_in_effect(), s, /*pad=*/true, qrows);
}

extern "C" {

int zk_fr_poly_eval(uint8_t *ys, const uint8_t *coeffs, uint64_t n, uint64_t m, const uint8_t *zs, int32_t device) {
    return guarded([&] { fr_poly_eval(ys, coeffs, n, m, zs, device); });
}

int zk_plonk_opening_create(zk_plonk_opening **out, zk_kzg *kzg, const zk_plonk_circuit_view *v, int32_t device) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        *out = opening_create(kzg, v, device);
    });
}

void zk_plonk_opening_destroy(zk_plonk_opening *o) { destroy_on_device(o); }

int zk_plonk_opening_info(zk_plonk_opening *o, zk_plonk_opening_plan *plan) {
    return guarded([&] {
        if (!o || !plan) throw std::invalid_argument("null argument");
        info_into("zk_plonk_opening_info", plan, [&](zk_plonk_opening_plan &p) {
            p.seg = seg_in_effect();
            std::lock_guard<std::mutex> lock(o->mu);
            p.log_n = o->log_n;
            p.device_bytes = o->bytes();
            p.last_launches = o->last_launches;
            p.pending = o->pending ? 1u : 0u;
        });
    });
}

int zk_plonk_evaluate(zk_plonk_opening *o, uint8_t evals[6 * 32], const uint8_t *a, uint64_t a_len, const uint8_t *b, uint64_t b_len, const uint8_t *cc,
                      uint64_t c_len, const uint8_t *z, uint64_t z_len, const uint8_t zeta[32]) {
    return guarded([&] {
        const uint8_t *const in[WIT_VECS] = {a, b, cc, z};
        const uint64_t len[WIT_VECS] = {a_len, b_len, c_len, z_len};
        plonk_evaluate(o, evals, in, len, zeta);
    });
}

int zk_plonk_open(zk_plonk_opening *o, uint8_t w_zeta[64], uint8_t w_zeta_omega[64], uint8_t r_zeta[32], uint8_t *f, uint64_t *f_len, const uint8_t *t_lo,
                  uint64_t lo_len, const uint8_t *t_mid, uint64_t mid_len, const uint8_t *t_hi, uint64_t hi_len, const uint8_t pi_zeta[32],
                  const uint8_t alpha[32], const uint8_t beta[32], const uint8_t gamma[32], const uint8_t v[32]) {
    return guarded([&] {
        const uint8_t *const t[T_VECS] = {t_lo, t_mid, t_hi};
        const uint64_t tlen[T_VECS] = {lo_len, mid_len, hi_len};
        plonk_open(o, w_zeta, w_zeta_omega, r_zeta, f, f_len, t, tlen, pi_zeta, alpha, beta, gamma, v);
    });
}

}   // extern "C"
