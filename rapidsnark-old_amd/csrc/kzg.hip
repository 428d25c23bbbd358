// KZG polynomial commitments over a .ptau (include/zkhip.h, section "KZG polynomial commitments over a .ptau").  Nothing in
// the reference corresponds to it (it proves Groth16 only); the counterpart is the commitment layer of snarkjs's PLONK and
// fflonk provers, which read the same file.  DESIGN.md section 26 describes the scan and states what was measured.
//
// The object (zk_kzg) keeps on its device the first max_coeffs points of section 2 and, optionally, one level of section 12,
// both converted ONCE to the form the bucket kernels read (operators.hip's msm_generic converts per call), the line tables
// of the G2 generator and of [tau]G2 (pairing.hpp's line_table, as zk_vkey_create makes gamma's and delta's), and the work
// buffers of one multi-scalar multiplication.
//
// Division by X - z, the new kernels.  With S_i = sum_(j >= i) c_j z^(j - i) the quotient is q_(i-1) = S_i and the value is
// y = S_0: a suffix scan of the recurrence S_i = c_i + z S_(i+1).  Tiers, from the inside:
//   lane       `seg` consecutive coefficients by Horner (ZKHIP_KZG_SEG, read at every call)
//   wave       64 lanes: a suffix scan of the lanes' sums by six shuffle steps, step k weighted by z^(seg 2^k)
//   workgroup  4 waves: their sums meet in LDS (k_div_reduce) and are chained with z^(64 seg)
//   carry      the workgroups' sums are scanned by ONE workgroup (k_div_carry), every lane taking ceil(groups / 256) of them
// Three launches: k_div_reduce (wave and workgroup sums), k_div_carry (what lies behind each workgroup), k_div_apply (a
// wave takes what lies behind it into its last lane, scans again, and every lane runs Horner a second time from the value
// behind its segment, storing every step).  No atomics: which products are formed depends on indices only, and the
// arithmetic is exact, so the bytes do not depend on scheduling or on seg.  The values stay in STANDARD form throughout:
// the powers of z are Montgomery and a Montgomery product of such a power with a standard value is standard, so the
// coefficients are never converted and the quotient is what the sort of the multiplication reads.
// Field arithmetic: field.hpp's 8 x 32-bit Fr, what ptau_check.hip and mulvec.hip use for their scalars.
//
// Verification: e(C - [y]G + [z]pi, G2) = e(pi, [tau]G2), a lane per opening.  k_kzg_check: the checks and
// L = C - y G + z pi (mulglv.hpp's mul_glv, one inversion).  k_kzg_pair: one squaring chain, both tables' lines evaluated at L
// and at -pi, the final exponentiation.  No point of G2 comes from the caller, so there is no variable-Q loop and no
// subgroup test per opening.
#include "kzg_internal.hpp"
#include "verify_batch_host.hpp"

namespace {

static_assert(sizeof(G1Affine) == 64 && sizeof(G2Affine) == 128 && sizeof(Fr) == 32 && sizeof(Line) == 192, "layout");

// ---------------------------------------------------------------- device: division by X - z (the tiers' weights: DivPows, kzg_internal.hpp)
// sum_(k < cnt) c[k] z^k
__device__ __forceinline__ Fr horner(const Fr *__restrict__ c, uint32_t cnt, const Fr &z) {
    Fr t = Fr::zero();
#pragma unroll 1
    for (uint32_t k = cnt; k-- > 0;) t = Fr::add(load_el(c + k), Fr::mul(z, t));
    return t;
}

// v of lane l <- sum_(j >= l, j < 64) v_j z^((j - l) seg)
__device__ __forceinline__ Fr wave_suffix(Fr v, const DivPows *__restrict__ p, uint32_t lane) {
#pragma unroll 1
    for (uint32_t k = 0; k < 6; k++) {
        const Fr t = shfl_down_fr(v, 1u << k);
        if (lane + (1u << k) < 64) v = Fr::add(v, Fr::mul(load_uniform(p->lane + k), t));
    }
    return v;
}

// what lies behind wave w of a workgroup: `behind` the workgroup, chained through the sums of its later waves
template <class Load>
__device__ __forceinline__ Fr behind_wave(Fr behind, uint32_t w, const DivPows *__restrict__ p, Load sum_of) {
    if (w == DIV_WAVES - 1) return behind;
    const Fr pw = load_uniform(&p->wave);
#pragma unroll 1
    for (uint32_t j = DIV_WAVES - 1; j > w; j--) behind = Fr::add(sum_of(j), Fr::mul(pw, behind));
    return behind;
}

// wsum[4 g + w]: the sum of wave w of workgroup g (weights from the wave's first element), gsum[g]: the workgroup's
__global__ __launch_bounds__(DIV_WG) void k_div_reduce(Fr *wsum, Fr *gsum, const Fr *__restrict__ c, uint64_t n, uint32_t seg, const DivPows *__restrict__ p) {
    __shared__ Fr sh[DIV_WAVES];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t lo;
    const uint32_t cnt = lane_span(lo, (uint64_t)blockIdx.x * DIV_WG, n, seg);
    const Fr pz = load_uniform(&p->z);
    const Fr v = wave_suffix(horner(c + lo, cnt, pz), p, lane);
    if (lane == 0) {
        store_el(wsum + (uint64_t)blockIdx.x * DIV_WAVES + w, v);
        sh[w] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {                           // wave 0's sum and what lies behind wave 0
        const Fr rest = behind_wave(Fr::zero(), 0, p, [&](uint32_t j) { return sh[j]; });
        store_el(gsum + blockIdx.x, Fr::add(sh[0], Fr::mul(load_uniform(&p->wave), rest)));
    }
}

// behind[g] = sum_(g' > g) gsum[g'] Z^(g' - g - 1), Z = p.z the weight between workgroups; ONE workgroup, lane l takes
// gsum[l seg, (l + 1) seg)
__global__ __launch_bounds__(DIV_WG) void k_div_carry(Fr *behind, const Fr *__restrict__ gsum, uint64_t groups, uint32_t seg, const DivPows *__restrict__ p) {
    __shared__ Fr sh[DIV_WAVES];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t lo;
    const uint32_t cnt = lane_span(lo, 0, groups, seg);
    const Fr pz = load_uniform(&p->z);
    Fr own = horner(gsum + lo, cnt, pz);
    Fr v = wave_suffix(own, p, lane);
    if (lane == 0) sh[w] = v;
    __syncthreads();
    const Fr X = behind_wave(Fr::zero(), w, p, [&](uint32_t j) { return sh[j]; });
    if (lane == 63) own = Fr::add(own, Fr::mul(load_uniform(p->lane), X));
    v = wave_suffix(own, p, lane);
    Fr t = shfl_down_fr(v, 1);                        // what lies behind this lane's segment
    if (lane == 63) t = X;
#pragma unroll 1
    for (uint32_t k = cnt; k-- > 0;) {
        store_el(behind + lo + k, t);
        t = Fr::add(load_el(gsum + lo + k), Fr::mul(pz, t));
    }
}

// q[i - 1] = S_i for 1 <= i < n and *y = S_0
__global__ __launch_bounds__(DIV_WG) void k_div_apply(Fr *q, Fr *y, const Fr *__restrict__ c, const Fr *__restrict__ wsum, const Fr *__restrict__ behind,
                                                       uint64_t n, uint32_t seg, const DivPows *__restrict__ p) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t lo;
    const uint32_t cnt = lane_span(lo, (uint64_t)blockIdx.x * DIV_WG, n, seg);
    const Fr pz = load_uniform(&p->z);
    const Fr *ws = wsum + (uint64_t)blockIdx.x * DIV_WAVES;
    const Fr X = behind_wave(load_uniform(behind + blockIdx.x), w, p, [&](uint32_t j) { return load_uniform(ws + j); });
    Fr own = horner(c + lo, cnt, pz);
    if (lane == 63) own = Fr::add(own, Fr::mul(load_uniform(p->lane), X));
    const Fr v = wave_suffix(own, p, lane);
    Fr t = shfl_down_fr(v, 1);
    if (lane == 63) t = X;
#pragma unroll 1
    for (uint32_t k = cnt; k-- > 0;) {
        t = Fr::add(load_el(c + lo + k), Fr::mul(pz, t));
        if (lo + k) store_el(q + (lo + k - 1), t);
        else store_el(y, t);
    }
}

// ---------------------------------------------------------------- device: verification
__global__ __launch_bounds__(64) void k_kzg_line_tables(Line *tab, const G2Affine *Q, uint32_t n, const PairConsts *k) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    line_table(tab + (uint64_t)j * MILLER_LINES, load_pt(Q + j), *k);
}

// status[i]; and, when asked for and the opening is well-formed, L[i] = C_i - y_i G + z_i pi_i
__global__ __launch_bounds__(64) void k_kzg_check(uint32_t *status, G1Affine *L, const G1Affine *__restrict__ C, const Fr *__restrict__ z,
                                                   const Fr *__restrict__ y, const G1Affine *__restrict__ pi, uint64_t m, Fq b1, Fq endo, G1Affine G,
                                                   uint32_t want_L) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const G1Affine c = load_pt(C + i), p = load_pt(pi + i);
    const Fr zz = load_el(z + i), yy = load_el(y + i);
    const bool ok = (c.is_inf() || on_curve(c, b1)) && (p.is_inf() || on_curve(p, b1)) && below_r(zz) && below_r(yy);
    status[i] = ok ? ST_OK : ST_MALFORMED;
    if (!ok || !want_L) return;
    G1XYZZ acc = mul_glv(p, zz, endo);
    add(acc, neg(mul_glv(G, yy, endo)));
    madd(acc, c);
    const G1Affine l = g1_to_affine(acc);
    store_el(&L[i].x, l.x);
    store_el(&L[i].y, l.y);
}

// verdict[i] from e(L_i, G2) e(-pi_i, [tau]G2) = 1; tab: the generator's lines, then [tau]G2's, the same address in every
// lane of the wave
__global__ __launch_bounds__(64) void k_kzg_pair(uint8_t *verdict, const uint32_t *__restrict__ status, const G1Affine *__restrict__ L,
                                                  const G1Affine *__restrict__ pi, const Line *__restrict__ tab, uint64_t m, const PairConsts *k) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    if (status[i] != ST_OK) {
        verdict[i] = ZK_VERIFY_MALFORMED;
        return;
    }
    const G1Affine l = load_pt(L + i);
    G1Affine p = load_pt(pi + i);
    p.y = Fq::neg(p.y);
    const bool have_l = !l.is_inf(), have_p = !p.is_inf();
    const Line *tg = tab, *tt = tab + MILLER_LINES;
    Fq12 f;
    f12_one(f);
    int at = 0;                                       // wave-uniform: the index into both tables
    auto lines = [&]() {
        if (have_l) f12_mul_line_at(f, tg[at], l);
        if (have_p) f12_mul_line_at(f, tt[at], p);
        at++;
    };
    for (int s = 0; s < 64; s++) {
        f12_sqr(f, f);
        lines();
        if (ate_bit(s)) lines();
    }
    lines();                                          // the chords with pi(Q) and -pi^2(Q)
    lines();
    Fq12 r;
    final_exp(r, f, *k);
    verdict[i] = f12_is_one(r) ? ZK_VERIFY_OK : ZK_VERIFY_INVALID;
}

// ---------------------------------------------------------------- host: division
uint32_t seg_in_effect() { return kzg_seg_in_effect(); }

DivPows make_pows(const Fr &base, uint64_t seg) {
    DivPows p;
    p.z = base;
    Fr t = fr_pow(base, seg);
    for (int k = 0; k < 6; k++) {
        p.lane[k] = t;
        t = Fr::sqr(t);
    }
    p.wave = t;
    return p;
}

}   // namespace

// q[0, n - 1) and *y from c[0, n), n >= 1, all on the device, standard form; z in Montgomery form (declared in
// kzg_internal.hpp, with DivWork: plonkopen.hip divides too)
void launch_divide(Fr *q, Fr *y, const Fr *c, uint64_t n, const Fr &z, uint32_t seg, DivWork &w, hipStream_t s) {
    const uint64_t groups = DivWork::groups_of(n, seg);
    if (groups >= (1ull << 31)) throw std::invalid_argument("division: too many coefficients for ZKHIP_KZG_SEG");
    w.size(groups);
    const uint32_t cseg = (uint32_t)((groups + DIV_WG - 1) / DIV_WG);
    w.h[0] = make_pows(z, seg);
    w.h[1] = make_pows(Fr::sqr(Fr::sqr(w.h[0].wave)), cseg);       // z^(256 seg) between workgroups
    HIP_TRY(hipMemcpyAsync(w.pows.p, w.h, sizeof w.h, hipMemcpyHostToDevice, s));
    ZK_LAUNCH(k_div_reduce, dim3((uint32_t)groups), dim3(DIV_WG), 0, s, w.wsum.p, w.gsum.p, c, n, seg, w.pows.p);
    ZK_LAUNCH(k_div_carry, dim3(1), dim3(DIV_WG), 0, s, w.behind.p, w.gsum.p, groups, cseg, w.pows.p + 1);
    ZK_LAUNCH(k_div_apply, dim3((uint32_t)groups), dim3(DIV_WG), 0, s, q, y, c, w.wsum.p, w.behind.p, n, seg, w.pows.p);
    ZK_LAUNCH_OK("division by X - z");
}

namespace {

void fr_poly_divide(uint8_t *q, uint8_t *y, const uint8_t *coeffs, uint64_t n, const uint8_t *z, int32_t device) {
    if (!n) throw std::invalid_argument("zk_fr_poly_divide: n is 0");
    if (!y || !coeffs || !z || (n > 1 && !q)) throw std::invalid_argument("null argument");
    if (n >= (1ull << 31)) throw std::invalid_argument("zk_fr_poly_divide: n is not below 2^31");
    const uint32_t seg = seg_in_effect();
    const uint64_t bad = first_not_below_r(coeffs, n);
    if (bad < n) throw std::invalid_argument("zk_fr_poly_divide: coefficient " + std::to_string(bad) + " is not below r");
    if (!below(z, FrParams::P)) throw std::invalid_argument("zk_fr_poly_divide: z is not below r");
    DeviceGuard g(resolve_device(device));
    need_hbm("zk_fr_poly_divide", 2 * n * sizeof(Fr) + DivWork::groups_of(n, seg) * 6 * sizeof(Fr) + 65536);
    Stream st;
    hipStream_t s = st.s;
    DevBuf<Fr> dc, dq, dy;
    DivWork w;
    dc.alloc(n);
    dq.alloc(n > 1 ? n - 1 : 1);
    dy.alloc(1);
    HIP_TRY(hipMemcpyAsync(dc.p, coeffs, n * sizeof(Fr), hipMemcpyHostToDevice, s));
    launch_divide(dq.p, dy.p, dc.p, n, fr_from_std(z), seg, w, s);
    if (n > 1) HIP_TRY(hipMemcpyAsync(q, dq.p, (n - 1) * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(y, dy.p, sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
}

// the multiplication over resident bases (msm_resident) and the object (struct zk_kzg): kzg_internal.hpp

// ptengine.hpp's pass over n points of section `sec` from its point `first` on; psi (section 3): the subgroup test too.
// There the two points go through both kernels before the words are read: point 0 is the generator (compared before), so
// point 1 is the only one either kernel can name, and the pick's order (hostutil.hpp) says which kind comes first.
template <class F>
void classify(uint32_t sec, uint64_t first, const Affine<F> *pts, uint64_t n, bool inf_bad, uint32_t *d_err, const PsiConsts *psi, hipStream_t s) {
    uint32_t h[4];
    enqueue_classify<F>(h, d_err, pts, n, inf_bad, psi, plain_subgroup(), s);
    const BadPoint b = classified(h, s);
    if (b.kind)
        throw std::invalid_argument("zk_kzg_create: ptau section " + std::to_string(sec) + ": point " + std::to_string(first + b.index) + " " + KIND_TEXT[b.kind]);
}

zk_kzg *kzg_create(const zk_kzg_view *v, uint64_t max_coeffs, uint32_t lagrange_log_n, int32_t device) {
    if (!v) throw std::invalid_argument("null argument");
    if (v->power < 1 || v->power > 28) throw std::invalid_argument("zk_kzg_create: power " + std::to_string(v->power) + " is outside 1 .. 28");
    const uint64_t file_points = (2ull << v->power) - 1;
    if (!max_coeffs || max_coeffs > file_points || max_coeffs >= (1ull << 31))
        throw std::invalid_argument("zk_kzg_create: max_coeffs " + std::to_string(max_coeffs) + " is outside 1 .. " +
                                    std::to_string(file_points < (1ull << 31) ? file_points : (1ull << 31) - 1) + " (power " + std::to_string(v->power) + ")");
    const bool want_lag = lagrange_log_n != NO_LEVEL;
    if (want_lag && lagrange_log_n > v->power)
        throw std::invalid_argument("zk_kzg_create: Lagrange level " + std::to_string(lagrange_log_n) + " is above the file's power " + std::to_string(v->power));
    if (want_lag && !v->lagrange_g1) throw std::invalid_argument("zk_kzg_create: a Lagrange level needs a prepared file (ptau section 12 is absent)");
    if (!v->tau_g1) throw std::invalid_argument("zk_kzg_create: ptau section 2 is absent");
    if (!v->tau_g2) throw std::invalid_argument("zk_kzg_create: ptau section 3 is absent");
    auto need_bytes = [&](uint32_t sec, uint64_t have, uint64_t need) {
        if (have < need)
            throw std::invalid_argument("zk_kzg_create: ptau section " + std::to_string(sec) + " is short: " + std::to_string(have) + " bytes, " +
                                        std::to_string(need) + " needed");
    };
    const uint64_t lag_n = want_lag ? 1ull << lagrange_log_n : 0;
    need_bytes(2, v->tau_g1_bytes, max_coeffs * sizeof(G1Affine));
    need_bytes(3, v->tau_g2_bytes, 2 * sizeof(G2Affine));
    if (want_lag) need_bytes(12, v->lagrange_g1_bytes, (2 * lag_n - 1) * sizeof(G1Affine));
    Pt<Fq> g1;
    Pt<Fq2> g2;
    generators(g1, g2);
    if (memcmp(v->tau_g1, g1.b, sizeof g1.b) != 0) throw std::invalid_argument("zk_kzg_create: ptau section 2: point 0 is not the generator of G1");
    if (memcmp(v->tau_g2, g2.b, sizeof g2.b) != 0) throw std::invalid_argument("zk_kzg_create: ptau section 3: point 0 is not the generator of G2");

    std::unique_ptr<zk_kzg> k(new zk_kzg);
    k->device = resolve_device(device);
    k->power = v->power;
    k->max_coeffs = max_coeffs;
    k->lag_log = lagrange_log_n;
    k->lag_n = lag_n;
    memcpy(k->g1, g1.b, sizeof k->g1);
    memcpy(k->g2tau, static_cast<const uint8_t *>(v->tau_g2) + sizeof(G2Affine), sizeof k->g2tau);
    DeviceGuard g(k->device);
    const uint64_t nsc = max_coeffs > lag_n ? max_coeffs : lag_n;
    need_hbm("zk_kzg_create", (max_coeffs + lag_n) * sizeof(G1Affine) + 2 * nsc * sizeof(Fr) + DevMsm<Fq>::bytes(nsc) +
                                  DivWork::groups_of(nsc, 1) * 6 * sizeof(Fr) + 2 * MILLER_LINES * sizeof(Line) + 65536);
    k->st.reset(new Stream);
    hipStream_t s = k->st->s;
    StreamUploader up(s);
    DevBuf<uint32_t> derr;
    DevBuf<G2Affine> d2;
    derr.alloc(4);
    d2.alloc(2);
    const PsiConsts psi = psi_consts();
    k->tau.alloc(max_coeffs);
    up.copy(k->tau.p, v->tau_g1, max_coeffs * sizeof(G1Affine));
    classify<Fq>(2, 0, k->tau.p, max_coeffs, true, derr.p, nullptr, s);
    if (want_lag) {
        k->lag.alloc(lag_n);
        up.copy(k->lag.p, (const uint8_t *)v->lagrange_g1 + (lag_n - 1) * sizeof(G1Affine), lag_n * sizeof(G1Affine));
        classify<Fq>(12, lag_n - 1, k->lag.p, lag_n, false, derr.p, nullptr, s);       // the index within the section
    }
    HIP_TRY(hipMemcpyAsync(d2.p, v->tau_g2, 2 * sizeof(G2Affine), hipMemcpyHostToDevice, s));
    classify<Fq2>(3, 0, d2.p, 2, true, derr.p, &psi, s);
    // every point is what the file may hold: now the forms the kernels read
    launch_fq_to_internal(reinterpret_cast<Fq *>(k->tau.p), max_coeffs * 2, s);
    if (want_lag) launch_fq_to_internal(reinterpret_cast<Fq *>(k->lag.p), lag_n * 2, s);
    k->kc.make(s);
    k->tab.alloc(2 * MILLER_LINES);
    ZK_LAUNCH(k_kzg_line_tables, dim3(1), dim3(64), 0, s, k->tab.p, d2.p, 2u, k->kc.k.p);
    ZK_LAUNCH_OK("line tables");
    k->sc.alloc(nsc);
    k->quot.alloc(nsc);
    k->yv.alloc(1);
    k->div.size(DivWork::groups_of(nsc, 1));
    k->msm.size(max_coeffs);
    HIP_TRY(hipStreamSynchronize(s));
    return k.release();
}

void check_polys(const char *who, const uint8_t *coeffs, uint64_t n, uint64_t m) {
    for (uint64_t p = 0; p < m; p++) {
        const uint64_t bad = first_not_below_r(coeffs + p * n * 32, n);
        if (bad < n) throw std::invalid_argument(std::string(who) + ": polynomial " + std::to_string(p) + ", coefficient " + std::to_string(bad) + " is not below r");
    }
}

void kzg_commit(zk_kzg *k, uint8_t *out, const uint8_t *coeffs, uint64_t n, uint64_t m, uint32_t basis) {
    if (!k) throw std::invalid_argument("null argument");
    if (basis != ZK_KZG_MONOMIAL && basis != ZK_KZG_LAGRANGE) throw std::invalid_argument("zk_kzg_commit: basis " + std::to_string(basis) + " is unknown");
    if (!n) throw std::invalid_argument("zk_kzg_commit: n is 0");
    if (!m) return;
    if (!out || !coeffs) throw std::invalid_argument("null argument");
    if (basis == ZK_KZG_LAGRANGE) {
        if (k->lag_log == NO_LEVEL) throw std::invalid_argument("zk_kzg_commit: the object holds no Lagrange level");
        if (n != k->lag_n) throw std::invalid_argument("zk_kzg_commit: n = " + std::to_string(n) + ", the Lagrange level holds " + std::to_string(k->lag_n) + " points");
    } else if (n > k->max_coeffs) {
        throw std::invalid_argument("zk_kzg_commit: n = " + std::to_string(n) + " exceeds max_coeffs = " + std::to_string(k->max_coeffs));
    }
    check_polys("zk_kzg_commit", coeffs, n, m);
    std::lock_guard<std::mutex> lock(k->mu);
    DeviceGuard g(k->device);
    LaunchCount lc(k->last_launches);
    hipStream_t s = k->st->s;
    const G1Affine *bases = basis == ZK_KZG_LAGRANGE ? k->lag.p : k->tau.p;
    for (uint64_t p = 0; p < m; p++) {
        HIP_TRY(hipMemcpyAsync(k->sc.p, coeffs + p * n * 32, n * 32, hipMemcpyHostToDevice, s));      // as zk_msm_g1 uploads its scalars
        msm_resident(k->msm, out + p * 64, bases, k->sc.p, n, s);
    }
}

void kzg_open(zk_kzg *k, uint8_t *ys, uint8_t *proofs, const uint8_t *coeffs, uint64_t n, uint64_t m, const uint8_t *zs) {
    if (!k) throw std::invalid_argument("null argument");
    if (!n) throw std::invalid_argument("zk_kzg_open: n is 0");
    if (!m) return;
    if (!ys || !proofs || !coeffs || !zs) throw std::invalid_argument("null argument");
    if (n > k->max_coeffs) throw std::invalid_argument("zk_kzg_open: n = " + std::to_string(n) + " exceeds max_coeffs = " + std::to_string(k->max_coeffs));
    const uint32_t seg = seg_in_effect();
    check_polys("zk_kzg_open", coeffs, n, m);
    const uint64_t badz = first_not_below_r(zs, m);
    if (badz < m) throw std::invalid_argument("zk_kzg_open: z " + std::to_string(badz) + " is not below r");
    std::lock_guard<std::mutex> lock(k->mu);
    DeviceGuard g(k->device);
    LaunchCount lc(k->last_launches);
    hipStream_t s = k->st->s;
    for (uint64_t p = 0; p < m; p++) {
        HIP_TRY(hipMemcpyAsync(k->sc.p, coeffs + p * n * 32, n * 32, hipMemcpyHostToDevice, s));
        launch_divide(k->quot.p, k->yv.p, k->sc.p, n, fr_from_std(zs + p * 32), seg, k->div, s);
        HIP_TRY(hipMemcpyAsync(ys + p * 32, k->yv.p, 32, hipMemcpyDeviceToHost, s));
        if (n > 1) {
            msm_resident(k->msm, proofs + p * 64, k->tau.p, k->quot.p, n - 1, s);   // the quotient never leaves the device
        } else {
            memset(proofs + p * 64, 0, 64);
            HIP_TRY(hipStreamSynchronize(s));
        }
    }
}

// the buffers of one chunk of openings
struct OpenBufs {
    DevBuf<G1Affine> C, pi, L;
    DevBuf<Fr> z, y;
    DevBuf<uint32_t> st;
    DevBuf<uint8_t> v;
    void alloc(uint64_t cap) {
        C.alloc(cap);
        pi.alloc(cap);
        L.alloc(cap);
        z.alloc(cap);
        y.alloc(cap);
        st.alloc(cap);
        v.alloc(cap);
    }
    static uint64_t bytes(uint64_t cap) { return cap * (3 * sizeof(G1Affine) + 2 * sizeof(Fr) + 5) + 65536; }
    void load(const uint8_t *c, const uint8_t *zs, const uint8_t *ys, const uint8_t *p, uint64_t off, uint64_t cnt, hipStream_t s) {
        HIP_TRY(hipMemcpyAsync(C.p, c + off * 64, cnt * 64, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(pi.p, p + off * 64, cnt * 64, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(z.p, zs + off * 32, cnt * 32, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(y.p, ys + off * 32, cnt * 32, hipMemcpyHostToDevice, s));
    }
};

void launch_check(zk_kzg *k, OpenBufs &b, uint64_t cnt, bool want_L, hipStream_t s) {
    G1Affine G;
    memcpy(&G, k->g1, sizeof G);
    ZK_LAUNCH(k_kzg_check, dim3(nblocks(cnt, 64)), dim3(64), 0, s, b.st.p, b.L.p, b.C.p, b.z.p, b.y.p, b.pi.p, cnt, curve_b<Fq>(), endo_const<Fq>(), G,
              want_L ? 1u : 0u);
}

void kzg_verify(zk_kzg *k, const uint8_t *commitments, const uint8_t *zs, const uint8_t *ys, const uint8_t *proofs, uint64_t m, uint8_t *verdict) {
    if (!k) throw std::invalid_argument("null argument");
    if (!m) return;
    if (!commitments || !zs || !ys || !proofs || !verdict) throw std::invalid_argument("null argument");
    const uint64_t chunk = chunk_jobs(), cap = m < chunk ? m : chunk;
    std::lock_guard<std::mutex> lock(k->mu);
    DeviceGuard g(k->device);
    LaunchCount lc(k->last_launches);
    need_hbm("zk_kzg_verify", OpenBufs::bytes(cap));
    hipStream_t s = k->st->s;
    OpenBufs b;
    b.alloc(cap);
    for (uint64_t off = 0; off < m; off += cap) {
        const uint64_t cnt = m - off < cap ? m - off : cap;
        b.load(commitments, zs, ys, proofs, off, cnt, s);
        launch_check(k, b, cnt, true, s);
        ZK_LAUNCH(k_kzg_pair, dim3(nblocks(cnt, 64)), dim3(64), 0, s, b.v.p, b.st.p, b.L.p, b.pi.p, k->tab.p, cnt, k->kc.k.p);
        ZK_LAUNCH_OK("opening verification");
        HIP_TRY(hipMemcpyAsync(verdict + off, b.v.p, cnt, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
}

void kzg_verify_batch(zk_kzg *k, const uint8_t *commitments, const uint8_t *zs, const uint8_t *ys, const uint8_t *proofs, uint64_t m,
                      const uint8_t *scalars16, uint8_t *verdict) {
    if (!k || !verdict) throw std::invalid_argument("null argument");
    if (!m) {
        *verdict = ZK_VERIFY_OK;
        return;
    }
    if (!commitments || !zs || !ys || !proofs) throw std::invalid_argument("null argument");
    if (m >= (1ull << 31)) throw std::invalid_argument("zk_kzg_verify_batch: m is not below 2^31");
    std::vector<uint8_t> drawn;
    refuse_zero_scalars(scalars16, m, "zk_kzg_verify_batch");
    if (!scalars16) {
        drawn.resize(m * 16);
        draw_scalars(drawn.data(), m, "zk_kzg_verify_batch");
        scalars16 = drawn.data();
    }
    std::lock_guard<std::mutex> lock(k->mu);
    DeviceGuard g(k->device);
    LaunchCount lc(k->last_launches);
    need_hbm("zk_kzg_verify_batch", OpenBufs::bytes(m) + 2 * m * sizeof(Fr) + (k->bmsm.n == m ? 0 : DevMsm<Fq>::bytes(m)));
    hipStream_t s = k->st->s;
    OpenBufs b;
    b.alloc(m);
    // the checks of zk_kzg_verify, without L
    std::vector<uint32_t> status(m);
    b.load(commitments, zs, ys, proofs, 0, m, s);
    launch_check(k, b, m, false, s);
    ZK_LAUNCH_OK("opening check");
    HIP_TRY(hipMemcpyAsync(status.data(), b.st.p, m * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint64_t i = 0; i < m; i++)
        if (status[i] != ST_OK) {
            *verdict = ZK_VERIFY_MALFORMED;
            return;
        }
    // r_i, r_i z_i (32 bytes each, standard form) and sum r_i y_i
    std::vector<uint8_t> r32(m * 32, 0), rz32(m * 32);
    Fr sum = Fr::zero();
    for (uint64_t i = 0; i < m; i++) {
        memcpy(r32.data() + i * 32, scalars16 + i * 16, 16);
        const Fr r = fr_from_std(r32.data() + i * 32);       // Montgomery; times a standard value: standard
        Fr z, y;
        memcpy(z.v, zs + i * 32, 32);
        memcpy(y.v, ys + i * 32, 32);
        const Fr rz = Fr::mul(r, z);
        memcpy(rz32.data() + i * 32, rz.v, 32);
        sum = Fr::add(sum, Fr::mul(r, y));
    }
    DevBuf<Fr> dr, drz;
    dr.alloc(m);
    drz.alloc(m);
    HIP_TRY(hipMemcpyAsync(dr.p, r32.data(), m * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(drz.p, rz32.data(), m * 32, hipMemcpyHostToDevice, s));
    launch_fq_to_internal(reinterpret_cast<Fq *>(b.C.p), m * 2, s);
    launch_fq_to_internal(reinterpret_cast<Fq *>(b.pi.p), m * 2, s);
    Pt<Fq> rC, rzPi, rPi;
    msm_resident(k->bmsm, rC.b, b.C.p, dr.p, m, s);
    msm_resident(k->bmsm, rzPi.b, b.pi.p, drz.p, m, s);
    msm_resident(k->bmsm, rPi.b, b.pi.p, dr.p, m, s);
    uint8_t sum32[32];
    memcpy(sum32, sum.v, 32);
    Pt<Fq> yG;
    Group<Fq>::mul(yG.b, k->g1, sum32);               // the one fixed-base multiplication
    const Pt<Fq> L = rC - yG + rzPi;
    // one opening's pair of lines: e(L, G2) e(-sum r_i pi_i, [tau]G2) = 1
    const uint32_t ok = ST_OK;
    HIP_TRY(hipMemcpyAsync(b.L.p, L.b, 64, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b.pi.p, rPi.b, 64, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b.st.p, &ok, 4, hipMemcpyHostToDevice, s));
    ZK_LAUNCH(k_kzg_pair, dim3(1), dim3(64), 0, s, b.v.p, b.st.p, b.L.p, b.pi.p, k->tab.p, (uint64_t)1, k->kc.k.p);
    ZK_LAUNCH_OK("batch verification");
    HIP_TRY(hipMemcpyAsync(verdict, b.v.p, 1, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
}

}   // namespace

// The two kernels of the pairing check over tables of another object's making (kzg_internal.hpp: plonkverify_dev.hip's
// verifier has its own [tau]G2 and no zk_kzg).  Q: the generator of G2, then [tau]G2; tab: 2 * MILLER_LINES lines
void launch_kzg_line_tables(Line *tab, const G2Affine *Q, const PairConsts *k, hipStream_t s) {
    ZK_LAUNCH(k_kzg_line_tables, dim3(1), dim3(64), 0, s, tab, Q, 2u, k);
    ZK_LAUNCH_OK("line tables");
}
void launch_kzg_pair(uint8_t *verdict, const uint32_t *status, const G1Affine *L, const G1Affine *pi, const Line *tab, uint64_t m, const PairConsts *k,
                     hipStream_t s) {
    ZK_LAUNCH(k_kzg_pair, dim3(nblocks(m, 64)), dim3(64), 0, s, verdict, status, L, pi, tab, m, k);
    ZK_LAUNCH_OK("pairing check");
}

// ZK_VERIFY_OK iff e(L, G2) = e(pi, [tau]G2), one lane of k_kzg_pair over the object's line tables (plonk_internal.hpp: the
// last step of zk_plonk_verify).  L and pi are points of the curve in the file's form: the caller's check
uint8_t kzg_pair_one(zk_kzg *k, const uint8_t L[64], const uint8_t pi[64]) {
    std::lock_guard<std::mutex> lock(k->mu);
    DeviceGuard g(k->device);
    LaunchCount lc(k->last_launches);
    hipStream_t s = k->st->s;
    DevBuf<G1Affine> dl, dp;
    DevBuf<uint32_t> st;
    DevBuf<uint8_t> dv;
    dl.alloc(1);
    dp.alloc(1);
    st.alloc(1);
    dv.alloc(1);
    const uint32_t ok = ST_OK;
    uint8_t verdict = ZK_VERIFY_INVALID;
    HIP_TRY(hipMemcpyAsync(dl.p, L, 64, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(dp.p, pi, 64, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(st.p, &ok, 4, hipMemcpyHostToDevice, s));
    ZK_LAUNCH(k_kzg_pair, dim3(1), dim3(64), 0, s, dv.p, st.p, dl.p, dp.p, k->tab.p, (uint64_t)1, k->kc.k.p);
    ZK_LAUNCH_OK("pairing check");
    HIP_TRY(hipMemcpyAsync(&verdict, dv.p, 1, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return verdict;
}

extern "C" {

int zk_fr_poly_divide(uint8_t *q, uint8_t y[32], const uint8_t *coeffs, uint64_t n, const uint8_t z[32], int32_t device) {
    return guarded([&] { fr_poly_divide(q, y, coeffs, n, z, device); });
}

int zk_kzg_create(zk_kzg **out, const zk_kzg_view *view, uint64_t max_coeffs, uint32_t lagrange_log_n, int32_t device) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        *out = kzg_create(view, max_coeffs, lagrange_log_n, device);
    });
}

void zk_kzg_destroy(zk_kzg *k) { destroy_on_device(k); }

int zk_kzg_info(zk_kzg *k, zk_kzg_plan *plan) {
    return guarded([&] {
        if (!k || !plan) throw std::invalid_argument("null argument");
        info_into("zk_kzg_info", plan, [&](zk_kzg_plan &p) {
            std::lock_guard<std::mutex> lock(k->mu);
            p.lagrange_log_n = k->lag_log;
            p.max_coeffs = k->max_coeffs;
            p.device_bytes = k->bytes();
            p.seg = seg_in_effect();
            p.last_launches = k->last_launches;
        });
    });
}

int zk_kzg_commit(zk_kzg *k, uint8_t *out, const uint8_t *coeffs, uint64_t n, uint64_t m, uint32_t basis) {
    return guarded([&] { kzg_commit(k, out, coeffs, n, m, basis); });
}

int zk_kzg_open(zk_kzg *k, uint8_t *ys, uint8_t *proofs, const uint8_t *coeffs, uint64_t n, uint64_t m, const uint8_t *zs) {
    return guarded([&] { kzg_open(k, ys, proofs, coeffs, n, m, zs); });
}

int zk_kzg_verify(zk_kzg *k, const uint8_t *commitments, const uint8_t *zs, const uint8_t *ys, const uint8_t *proofs, uint64_t m, uint8_t *verdict) {
    return guarded([&] { kzg_verify(k, commitments, zs, ys, proofs, m, verdict); });
}

int zk_kzg_verify_batch(zk_kzg *k, const uint8_t *commitments, const uint8_t *zs, const uint8_t *ys, const uint8_t *proofs, uint64_t m,
                        const uint8_t *scalars16, uint8_t *verdict) {
    return guarded([&] { kzg_verify_batch(k, commitments, zs, ys, proofs, m, scalars16, verdict); });
}

}   // extern "C"
