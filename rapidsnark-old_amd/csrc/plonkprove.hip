// PLONK prover (include/zkhip.h, section "PLONK prover and verifier"): the five rounds of a three-column proof chained on
// one stream.  The Fiat-Shamir transcript (Keccak-256, on the host: a few hundred bytes a round) and what prover and verifier
// both make of zeta are plonk_transcript.hpp's; the verifier is plonkverify.hip.  Nothing in the reference corresponds to
// it (it proves Groth16 only); the counterpart is snarkjs's PLONK prover.  DESIGN.md section 31 states the residency, the
// launches and what was measured.
//
// The rounds are the existing units' device-pointer cores (plonk_internal.hpp): frscan.hip's permutation product,
// plonkquot.hip's quotient and inverse transform of size n, plonkopen.hip's evaluations, linearisation and openings, kzg.hip's
// division and the multiplication over the kzg's resident points.  The witness is uploaded once; after that only
// commitments, the six values, `last`, t's length, r(zeta) and the challenges cross PCIe.
//
// New here, all memory-bound and in STANDARD form (a move or one subtraction an element, no product):
//   k_wire_gather   the rows of a, b, c by values from the witness by the three maps, and PI's values from the publics
//   k_plonk_blind   a row += (r_0 + r_1 X + ..) Z_H: 2 or 3 coefficients at the bottom and as many above n
//   k_plonk_split   t -> t_lo + b10 X^n, t_mid - b10 + b11 X^n, t_hi - b11
// Lane map of the gather and the split: plonkquot.hip's.  T lanes in the grid (a multiple of 256), lane l takes the rows
// l, l + T, l + 2T, .. : `seg` of them (ZKHIP_QUOT_SEG), so neighbouring lanes read neighbouring indices and write
// neighbouring rows at any seg; only the witness row an index names is not a neighbour's (32 bytes, two 16-byte loads).
// Which element goes where depends on indices only: no byte depends on seg or on scheduling.  No LDS, no atomics.
#include <sys/random.h>

#include "plonk_prover_internal.hpp"

namespace {

constexpr uint32_t PV_WG = 256;
constexpr uint32_t MIN_LOG_N = 3;
constexpr uint32_t CIRC_VECS = PLONK_CIRC_VECS, POINTS = PLONK_POINTS, BLINDS = ZK_PLONK_BLINDS;
constexpr uint32_t ROUNDS = PLONK_ROUNDS;
enum { C_QL, C_QR, C_QM, C_QO, C_QC, C_S1, C_S2, C_S3 };           // the view's order

// ---------------------------------------------------------------- device
// out[v][i] = wit[map[v][i]] for v < 3; out[3][i] = -pub[i] for i < n_public, else 0 (row 3 only when the grid has it)
struct GatherArgs {
    const uint32_t *map;                              // 3 x n, every index below the witness's length (checked when the object is made)
    const Fr *wit, *pub;
    Fr *out;                                          // 4 x n
    uint64_t n, n_public;
    uint32_t seg;
};
__global__ __launch_bounds__(PV_WG) void k_wire_gather(GatherArgs A) {
    const uint64_t T = (uint64_t)gridDim.x * PV_WG, l = (uint64_t)blockIdx.x * PV_WG + threadIdx.x;
    const uint32_t v = blockIdx.y;
    const uint32_t *map = A.map + v * A.n;
    Fr *out = A.out + v * A.n;
#pragma unroll 1
    for (uint32_t k = 0; k < A.seg; k++) {
        const uint64_t i = l + k * T;
        if (i >= A.n) break;
        if (v < 3) store_el(out + i, load_el(A.wit + map[i]));
        else store_el(out + i, i < A.n_public ? Fr::sub(Fr::zero(), load_el(A.pub + i)) : Fr::zero());
    }
}

// row[y] += (r_0 + r_1 X + .. + r_(cnt-1) X^(cnt-1)) (X^n - 1), r_j = b[first[y] + cnt - 1 - j]: the row holds n coefficients
// and what lies above them is replaced.  A workgroup a row, a lane a coefficient
struct BlindArgs {
    Fr *row[3];
    uint32_t first[3];
    const Fr *b;
    uint64_t n;
    uint32_t cnt;
};
__global__ __launch_bounds__(64) void k_plonk_blind(BlindArgs A) {
    const uint32_t j = threadIdx.x, y = blockIdx.x;
    if (j >= A.cnt) return;
    const Fr r = load_el(A.b + A.first[y] + A.cnt - 1 - j);
    Fr *row = A.row[y];
    store_el(row + j, Fr::sub(load_el(row + j), r));
    store_el(row + A.n + j, r);
}

// lo[i] = t[i], mid[i] = t[n + i] for i < n, hi[i] = t[2n + i] for i < n + 6; lo[n] = b10, mid[0] -= b10, mid[n] = b11, hi[0] -= b11
struct SplitArgs {
    const Fr *t;                                      // 4n rows
    Fr *lo, *mid, *hi;
    const Fr *b;                                      // b10, b11
    uint64_t n;
    uint32_t seg;
};
__global__ __launch_bounds__(PV_WG) void k_plonk_split(SplitArgs A) {
    const uint64_t T = (uint64_t)gridDim.x * PV_WG, l = (uint64_t)blockIdx.x * PV_WG + threadIdx.x, n = A.n;
#pragma unroll 1
    for (uint32_t k = 0; k < A.seg; k++) {
        const uint64_t i = l + k * T;
        if (i >= n + 6) break;
        Fr hi = load_el(A.t + 2 * n + i);             // 2n + i < 3n + 6 <= 4n: n >= 8
        if (i == 0) hi = Fr::sub(hi, load_el(A.b + 1));
        store_el(A.hi + i, hi);
        if (i < n) {
            Fr mid = load_el(A.t + n + i);
            if (i == 0) mid = Fr::sub(mid, load_el(A.b));
            store_el(A.lo + i, load_el(A.t + i));
            store_el(A.mid + i, mid);
        } else if (i == n) {
            store_el(A.lo + n, load_el(A.b));
            store_el(A.mid + n, load_el(A.b + 1));
        }
    }
}

// ---------------------------------------------------------------- host
uint32_t blocks_of(uint64_t n, uint32_t seg) { return nblocks(n, PV_WG * seg); }

}   // namespace

// ---------------------------------------------------------------- the object: plonk_prover_internal.hpp
namespace {

uint64_t own_need_bytes(uint64_t n, uint64_t n_witness, uint64_t n_public) {
    return 3 * n * sizeof(uint32_t) + (3 * n + 3 + n_witness + n_public + 1 + BLINDS + 4 * n + 2 * n) * sizeof(Fr) + 65536;
}

// [p] for `len` standard rows on the device, over the kzg's resident points
void commit_dev(zk_kzg *k, uint8_t out[64], const Fr *rows, uint64_t len, hipStream_t s) {
    std::lock_guard<std::mutex> kl(k->mu);             // the kzg's points and the work buffers of its multiplication
    msm_resident(k->msm, out, k->tau.p, rows, len, s);
}

zk_plonk_prover *prover_create(zk_kzg *kzg, const zk_plonk_circuit_view *v, const uint32_t *a_map, const uint32_t *b_map, const uint32_t *c_map,
                               uint64_t n_witness, uint64_t n_public, int32_t device) {
    const char *who = "zk_plonk_prover_create";
    if (!kzg || !v || !a_map || !b_map || !c_map) throw std::invalid_argument("null argument");
    CheckedView cv = checked_view_dims(who, v, MIN_LOG_N);
    const uint64_t n = cv.n, cap = kzg->max_coeffs;
    if (n + 6 > cap)
        throw std::invalid_argument(std::string(who) + ": n + 6 = " + std::to_string(n + 6) + " exceeds the kzg's max_coeffs = " + std::to_string(cap));
    if (n_public > n) throw std::invalid_argument(std::string(who) + ": n_public " + std::to_string(n_public) + " exceeds n = " + std::to_string(n));
    if (!n_witness) throw std::invalid_argument(std::string(who) + ": n_witness is 0");
    if (n_witness > (1ull << 32)) throw std::invalid_argument(std::string(who) + ": n_witness is above 2^32");
    if (device >= 0 && device != kzg->device)
        throw std::invalid_argument(std::string(who) + ": device " + std::to_string(device) + " is not the kzg's device " + std::to_string(kzg->device));
    const uint32_t *maps[3] = {a_map, b_map, c_map};
    static const char *const mnames[3] = {"a_map", "b_map", "c_map"};
    for (int j = 0; j < 3; j++)
        for (uint64_t i = 0; i < n; i++)
            if (maps[j][i] >= n_witness)
                throw std::invalid_argument(std::string(who) + ": " + mnames[j] + " " + std::to_string(i) + " is " + std::to_string(maps[j][i]) +
                                            ", not below n_witness = " + std::to_string(n_witness));
    checked_view_rows(who, v, cv);
    const CheckedShift shift = checked_shift(who, v->shift, cv.log_n);
    std::unique_ptr<zk_plonk_prover> p(new zk_plonk_prover());
    p->kzg = kzg, p->device = kzg->device, p->log_n = cv.log_n, p->n = n, p->cap = cap, p->n_witness = n_witness, p->n_public = n_public;
    const bool lagrange = cv.lagrange;
    DeviceGuard dg(p->device);
    need_hbm(who, plonk_circuit_need_bytes(cv.log_n) + plonk_opening_need_bytes(n, cap, lagrange) + plonk_perm_need_bytes(n) + own_need_bytes(n, n_witness, n_public));
    const uint64_t at = launches_now();
    p->circ = plonk_circuit_make(cv, shift, p->device);             // from the view as checked above: its 8n rows are scanned once
    p->open = plonk_opening_make(kzg, cv);
    p->perm = plonk_perm_new();
    p->st.reset(new Stream());
    hipStream_t s = p->st->s;
    p->maps.alloc(3 * n);
    p->sig.alloc(3 * n);
    p->shifts.alloc(3);
    p->wit.alloc(n_witness);
    p->pub.alloc(n_public ? n_public : 1);
    p->blind.alloc(BLINDS);
    p->vals.alloc(4 * n);
    p->zval.alloc(n);
    p->pic.alloc(n);
    for (int j = 0; j < 3; j++) HIP_TRY(hipMemcpyAsync(p->maps.p + j * n, maps[j], n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    Fr sh[3] = {Fr::from_mont(Fr::one()), Fr::from_mont(cv.k1), Fr::from_mont(cv.k2)};
    HIP_TRY(hipMemcpyAsync(p->shifts.p, sh, sizeof sh, hipMemcpyHostToDevice, s));
    // s1 .. s3 by values at w^i: the view's rows, or zk_fr_ntt's forward transform of their coefficients (once in the object's life)
    std::vector<uint8_t> sv;
    for (int j = 0; j < 3; j++) {
        const uint8_t *src = cv.vec[C_S1 + j];
        if (!lagrange) {
            sv.assign(src, src + n * 32);
            if (zk_fr_ntt(sv.data(), n, 0) != 0) throw std::runtime_error(std::string(who) + ": " + zk_last_error());
            src = sv.data();
        }
        HIP_TRY(hipMemcpyAsync(p->sig.p + j * n, src, n * sizeof(Fr), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    plonk_opening_clear(p->open, s);
    plonk_circuit_prepare_interpolate(p->circ, s);
    // the key: the eight commitments in the transcript's order, from the coefficients rounds 4 and 5 keep
    zk_plonk_vkey &vk = p->vk;
    memset(&vk, 0, sizeof vk);
    vk.size = sizeof vk, vk.log_n = cv.log_n, vk.n_public = n_public;
    memcpy(vk.k1, v->k1, 32);
    memcpy(vk.k2, v->k2, 32);
    memcpy(vk.tau_g2, kzg->g2tau, sizeof vk.tau_g2);
    uint8_t *out[CIRC_VECS] = {vk.ql, vk.qr, vk.qm, vk.qo, vk.qc, vk.s1, vk.s2, vk.s3};
    for (uint32_t j = 0; j < CIRC_VECS; j++) commit_dev(kzg, out[j], plonk_opening_circ(p->open, j), n, s);
    p->last_launches = (uint32_t)(launches_now() - at);
    return p.release();
}

// a call's blinds: the caller's, checked, or drawn into `drawn`
const uint8_t *blinds_of(const char *who, const uint8_t *blind, uint8_t *drawn) {
    if (blind) {
        check_below_r(who, "blind", blind, BLINDS);
        return blind;
    }
    for (uint32_t j = 0; j < BLINDS; j++) draw_scalar(drawn + j * 32, who);
    return drawn;
}
struct Wipe {                                         // drawn blinds are secrets: gone from the stack however the call leaves
    uint8_t *p;
    ~Wipe() {
        volatile uint8_t *v = p;
        for (size_t i = 0; i < BLINDS * 32; i++) v[i] = 0;
    }
};

// The five rounds over what is resident: the witness in p->wit, the publics in p->pub, the blinds in p->blind (their copies
// queued on the stream by the caller, who holds p->mu and the device).  publics: the host's copy, for the transcript.
// first: the launch counter where the call began
void plonk_prove_core(zk_plonk_prover *p, const char *who, uint8_t *proof, const uint8_t *publics, uint32_t seg, uint64_t first) {
    hipStream_t s = p->st->s;
    zk_kzg *k = p->kzg;
    const uint64_t n = p->n, len = n + 6;               // every committed row is read as n + 6 coefficients: zeros above its own length
    const uint32_t log_n = p->log_n;
    uint64_t mark = launches_now();
    uint32_t rounds[ROUNDS];
    auto end_round = [&](int r) {
        const uint64_t now = launches_now();
        rounds[r] = (uint32_t)(now - mark);
        mark = now;
    };
    uint8_t out[ZK_PLONK_PROOF_BYTES];
    uint8_t *pts = out, *evals = out + POINTS * 64;
    Challenges ch;
    Fr *rows[4] = {plonk_opening_wit(p->open, 0), plonk_opening_wit(p->open, 1), plonk_opening_wit(p->open, 2), plonk_opening_wit(p->open, 3)};

    // round 1: the wires by values, their coefficients, the blinding, [a] [b] [c]
    const uint32_t vecs = p->n_public ? 4u : 3u;
    GatherArgs G{p->maps.p, p->wit.p, p->pub.p, p->vals.p, n, p->n_public, seg};
    ZK_LAUNCH(k_wire_gather, dim3(blocks_of(n, seg), vecs), dim3(PV_WG), 0, s, G);
    ZK_LAUNCH_OK("wire gather");
    Fr *const out1[4] = {rows[0], rows[1], rows[2], p->pic.p};
    plonk_circuit_interpolate_dev(p->circ, out1, p->vals.p, vecs, s);
    BlindArgs B{{rows[0], rows[1], rows[2]}, {0, 2, 4}, p->blind.p, n, 2};
    ZK_LAUNCH(k_plonk_blind, dim3(3), dim3(64), 0, s, B);
    ZK_LAUNCH_OK("blinding");
    for (uint32_t j = 0; j < 3; j++) commit_dev(k, pts + (P_A + j) * 64, rows[j], len, s);
    round1_challenges(ch, p->vk, publics, pts);
    end_round(0);

    // round 2: z by values, its coefficients, the blinding, [z]
    uint8_t beta[32], gamma[32], last[32];
    fr_to_std(beta, ch.beta);
    fr_to_std(gamma, ch.gamma);
    if (!plonk_perm_dev(p->perm, p->zval.p, last, p->vals.p, p->sig.p, p->shifts.p, log_n, beta, gamma, s))
        throw PlonkRefusal(PM_ZERO_DENOMINATOR, std::string(who) + ": a denominator of the permutation product is zero");
    if (!(fr_from_std(last) == Fr::one())) throw PlonkRefusal(PM_COPIES, std::string(who) + ": the copy constraints do not hold");
    Fr *const out2[1] = {rows[3]};
    plonk_circuit_interpolate_dev(p->circ, out2, p->zval.p, 1, s);
    BlindArgs BZ{{rows[3], nullptr, nullptr}, {6, 0, 0}, p->blind.p, n, 3};
    ZK_LAUNCH(k_plonk_blind, dim3(1), dim3(64), 0, s, BZ);
    ZK_LAUNCH_OK("blinding");
    commit_dev(k, pts + P_Z * 64, rows[3], len, s);
    round2_challenge(ch, pts);
    end_round(1);

    // round 3: the rows to the quotient's input, t, its split, [t_lo] [t_mid] [t_hi]
    const uint64_t lens[PLONK_ROWS] = {n + 2, n + 2, n + 2, n + 3, n};
    Fr *in = plonk_circuit_rows(p->circ);
    uint64_t at = 0;
    for (uint32_t j = 0; j < vecs + 1; j++) {
        HIP_TRY(hipMemcpyAsync(in + at, j < 4 ? rows[j] : p->pic.p, lens[j] * sizeof(Fr), hipMemcpyDeviceToDevice, s));
        at += lens[j];
    }
    uint64_t t_len = 0;
    const Fr *t = plonk_circuit_quotient_dev(p->circ, lens, vecs + 1, ch.alpha, ch.beta, ch.gamma, &t_len, s);
    if (t_len > 3 * n + 6) throw PlonkRefusal(PM_GATES, std::string(who) + ": the witness does not satisfy the gates");
    Fr *parts[3] = {plonk_opening_part(p->open, 0), plonk_opening_part(p->open, 1), plonk_opening_part(p->open, 2)};
    SplitArgs S{t, parts[0], parts[1], parts[2], p->blind.p + 9, n, seg};
    ZK_LAUNCH(k_plonk_split, dim3(blocks_of(n + 6, seg)), dim3(PV_WG), 0, s, S);
    ZK_LAUNCH_OK("split of t");
    for (uint32_t j = 0; j < 3; j++) commit_dev(k, pts + (P_TLO + j) * 64, parts[j], len, s);
    round3_challenge(ch, pts);
    end_round(2);

    // round 4: the six values
    const uint64_t wlen[4] = {len, len, len, len};
    plonk_opening_evaluate_dev(p->open, evals, wlen, ch.zeta, s);
    round4_challenge(ch, evals);
    end_round(3);

    // round 5: the linearisation and the two openings
    const AtZeta z = at_zeta(log_n, ch.zeta, publics, p->n_public);
    const uint64_t tlen[3] = {n + 1, n + 1, n + 6};
    uint8_t r_zeta[32];
    static const uint8_t zero[32] = {0};
    plonk_opening_open_dev(p->open, pts + P_WZ * 64, pts + P_WZW * 64, r_zeta, nullptr, nullptr, tlen, z.pi, ch.alpha, ch.beta, ch.gamma, ch.v, s);
    if (memcmp(r_zeta, zero, 32) != 0) throw PlonkRefusal(PM_GATES, std::string(who) + ": the witness does not satisfy the gates");
    end_round(4);
    HIP_TRY(hipMemsetAsync(p->blind.p, 0, p->blind.bytes(), s));      // and from the device: the next call uploads its own
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(proof, out, sizeof out);
    for (uint32_t r = 0; r < ROUNDS; r++) p->round_launches[r] = rounds[r];
    p->last_launches = (uint32_t)(launches_now() - first);
}

// One proof.  wit: `up` values go up; r1cs: they are a circom witness the caller has checked (nVars = up), which the device
// extends and whose values 1 .. n_public are the publics; else the caller's witness of n_witness values, checked here
void plonk_prove(zk_plonk_prover *p, const char *who, uint8_t *proof, const uint8_t *wit, uint64_t up, const uint8_t *publics, const uint8_t *blind, bool r1cs) {
    if (!r1cs) {
        check_below_r(who, "witness", wit, up);
        if (p->n_public) check_below_r(who, "publics", publics, p->n_public);
    }
    uint8_t drawn[BLINDS * 32];
    Wipe wipe{drawn};
    blind = blinds_of(who, blind, drawn);
    const uint32_t seg = plonk_quot_seg();
    (void)plonk_perm_seg(), (void)plonk_open_seg(), (void)kzg_seg_in_effect();      // a bad knob is an error of the call before any work
    std::lock_guard<std::mutex> lock(p->mu);
    DeviceGuard dg(p->device);
    hipStream_t s = p->st->s;
    const uint64_t first = launches_now();
    HIP_TRY(hipMemcpyAsync(p->wit.p, wit, up * sizeof(Fr), hipMemcpyHostToDevice, s));
    if (p->n_public) HIP_TRY(hipMemcpyAsync(p->pub.p, publics, p->n_public * sizeof(Fr), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(p->blind.p, blind, BLINDS * sizeof(Fr), hipMemcpyHostToDevice, s));
    if (r1cs) plonk_r1cs_extend_dev(p->r1cs, p->wit.p, s);
    plonk_prove_core(p, who, proof, publics, seg, first);
}

// the existing prover over a compiled circuit: its vectors and maps come through the host once (zk_plonk_r1cs_circuit)
zk_plonk_prover *prover_create_r1cs(zk_kzg *kzg, zk_plonk_r1cs *c, const uint8_t *shift, int32_t device) {
    if (!kzg || !c) throw std::invalid_argument("null argument");
    const PlonkR1csDims d = plonk_r1cs_dims(c);
    if (d.device != kzg->device)
        throw std::invalid_argument("zk_plonk_prover_create_r1cs: the compiled circuit's device " + std::to_string(d.device) + " is not the kzg's device " +
                                    std::to_string(kzg->device));
    std::vector<uint8_t> vec(8 * d.n * 32);
    std::vector<uint32_t> maps(3 * d.n);
    if (zk_plonk_r1cs_circuit(c, vec.data(), maps.data(), maps.data() + d.n, maps.data() + 2 * d.n) != 0)
        throw std::runtime_error(std::string("zk_plonk_prover_create_r1cs: ") + zk_last_error());
    zk_plonk_circuit_view v;
    memset(&v, 0, sizeof v);
    v.log_n = d.log_n, v.basis = ZK_KZG_LAGRANGE;
    const uint8_t **vp[CIRC_VECS] = {&v.ql, &v.qr, &v.qm, &v.qo, &v.qc, &v.s1, &v.s2, &v.s3};
    for (uint32_t j = 0; j < CIRC_VECS; j++) *vp[j] = vec.data() + j * d.n * 32;
    memcpy(v.k1, d.k1, 32);
    memcpy(v.k2, d.k2, 32);
    v.shift = shift;
    zk_plonk_prover *p = prover_create(kzg, &v, maps.data(), maps.data() + d.n, maps.data() + 2 * d.n, d.n_witness, d.n_public, device);
    p->r1cs = c;
    return p;
}

}   // namespace

void plonk_prover_core(zk_plonk_prover *p, const char *who, uint8_t *proof, const uint8_t *publics, uint32_t seg, uint64_t first) {
    plonk_prove_core(p, who, proof, publics, seg, first);
}

extern "C" {

int zk_plonk_prover_create(zk_plonk_prover **out, zk_kzg *kzg, const zk_plonk_circuit_view *view, const uint32_t *a_map, const uint32_t *b_map,
                           const uint32_t *c_map, uint64_t n_witness, uint64_t n_public, int32_t device) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        *out = prover_create(kzg, view, a_map, b_map, c_map, n_witness, n_public, device);
    });
}

void zk_plonk_prover_destroy(zk_plonk_prover *p) { destroy_on_device(p); }

int zk_plonk_prover_vkey(zk_plonk_prover *p, zk_plonk_vkey *vk) {
    return guarded([&] {
        if (!p || !vk) throw std::invalid_argument("null argument");
        if (vk->size != sizeof(zk_plonk_vkey)) throw std::invalid_argument("zk_plonk_prover_vkey: vk->size is not sizeof(zk_plonk_vkey)");
        *vk = p->vk;
    });
}

int zk_plonk_prover_info(zk_plonk_prover *p, zk_plonk_prover_plan *plan) {
    return guarded([&] {
        if (!p || !plan) throw std::invalid_argument("null argument");
        info_into("zk_plonk_prover_info", plan, [&](zk_plonk_prover_plan &q) {
            q.scan_seg = plonk_perm_seg(), q.quot_seg = plonk_quot_seg(), q.open_seg = plonk_open_seg(), q.kzg_seg = kzg_seg_in_effect();
            std::lock_guard<std::mutex> lock(p->mu);
            q.log_n = p->log_n;
            q.n_witness = p->n_witness, q.n_public = p->n_public;
            q.device_bytes = p->own_bytes() + plonk_circuit_bytes(p->circ) + plonk_opening_bytes(p->open) + plonk_perm_bytes(p->perm) + plonk_many_bytes(p->many);
            q.last_launches = p->last_launches;
            for (uint32_t r = 0; r < ROUNDS; r++) q.round_launches[r] = p->round_launches[r];
        });
    });
}

int zk_plonk_prove(zk_plonk_prover *p, uint8_t proof[ZK_PLONK_PROOF_BYTES], const uint8_t *witness, const uint8_t *publics, const uint8_t *blind) {
    return guarded([&] {
        if (!p || !proof || !witness || (p->n_public && !publics)) throw std::invalid_argument("null argument");
        plonk_prove(p, "zk_plonk_prove", proof, witness, p->n_witness, publics, blind, false);
    });
}

int zk_plonk_prover_create_r1cs(zk_plonk_prover **out, zk_kzg *kzg, zk_plonk_r1cs *compiled, const uint8_t *shift, int32_t device) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        *out = prover_create_r1cs(kzg, compiled, shift, device);
    });
}

int zk_plonk_prove_r1cs(zk_plonk_prover *p, uint8_t proof[ZK_PLONK_PROOF_BYTES], const uint8_t *wtns, uint32_t nVars, const uint8_t *blind) {
    return guarded([&] {
        const char *who = "zk_plonk_prove_r1cs";
        if (!p || !proof || !wtns) throw std::invalid_argument("null argument");
        if (!p->r1cs) throw std::invalid_argument(std::string(who) + ": the prover was not made from an r1cs (zk_plonk_prover_create_r1cs)");
        plonk_r1cs_check_witness(p->r1cs, who, wtns, nVars);
        plonk_prove(p, who, proof, wtns, nVars, wtns + 32, blind, true);      // a circom witness: the publics are w[1 .. 1 + n_public)
    });
}

}   // extern "C"
