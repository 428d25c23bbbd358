// PLONK prover and verifier (include/zkhip.h, section "PLONK prover and verifier"): the five rounds of a three-column proof
// chained on one stream, the Fiat-Shamir transcript (Keccak-256, on the host: a few hundred bytes a round) and the
// verifier.  Nothing in the reference corresponds to it (it proves Groth16 only); the counterpart is snarkjs's PLONK
// prover and verifier.  DESIGN.md section 31 states the residency, the launches and what was measured.
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

#include "plonk_internal.hpp"

namespace {

constexpr uint32_t PV_WG = 256;
constexpr uint32_t MIN_LOG_N = 3, MAX_LOG_N = 25;
constexpr uint32_t CIRC_VECS = 8, EVALS = 6, POINTS = 9, BLINDS = ZK_PLONK_BLINDS;
constexpr uint32_t ROUNDS = 5;
enum { C_QL, C_QR, C_QM, C_QO, C_QC, C_S1, C_S2, C_S3 };           // the view's order
enum { P_A, P_B, P_C, P_Z, P_TLO, P_TMID, P_THI, P_WZ, P_WZW };     // the proof's points
static_assert(ZK_PLONK_PROOF_BYTES == POINTS * 64 + EVALS * 32, "layout");

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

// ---------------------------------------------------------------- host: Keccak-256
const uint64_t KECCAK_RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,
                                0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,
                                0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,
                                0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
                                0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
const int KECCAK_ROT[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
const int KECCAK_PIL[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};

inline uint64_t rotl64(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }

void keccak_f(uint64_t st[25]) {
    for (int round = 0; round < 24; round++) {
        uint64_t bc[5];
        for (int i = 0; i < 5; i++) bc[i] = st[i] ^ st[i + 5] ^ st[i + 10] ^ st[i + 15] ^ st[i + 20];
        for (int i = 0; i < 5; i++) {
            const uint64_t t = bc[(i + 4) % 5] ^ rotl64(bc[(i + 1) % 5], 1);
            for (int j = 0; j < 25; j += 5) st[j + i] ^= t;
        }
        uint64_t t = st[1];
        for (int i = 0; i < 24; i++) {
            const int j = KECCAK_PIL[i];
            const uint64_t keep = st[j];
            st[j] = rotl64(t, KECCAK_ROT[i]);
            t = keep;
        }
        for (int j = 0; j < 25; j += 5) {
            for (int i = 0; i < 5; i++) bc[i] = st[j + i];
            for (int i = 0; i < 5; i++) st[j + i] ^= (~bc[(i + 1) % 5]) & bc[(i + 2) % 5];
        }
        st[0] ^= KECCAK_RC[round];
    }
}

// rate 136 bytes, the original padding 0x01 .. 0x80
void keccak256(uint8_t out[32], const uint8_t *data, uint64_t len) {
    constexpr uint64_t RATE = 136;
    uint64_t st[25] = {0};
    auto absorb = [&](const uint8_t *block) {
        for (uint64_t i = 0; i < RATE / 8; i++) {
            uint64_t w = 0;
            for (int b = 7; b >= 0; b--) w = (w << 8) | block[i * 8 + b];
            st[i] ^= w;
        }
        keccak_f(st);
    };
    while (len >= RATE) {
        absorb(data);
        data += RATE;
        len -= RATE;
    }
    uint8_t last[RATE] = {0};
    if (len) memcpy(last, data, len);
    last[len] ^= 0x01;
    last[RATE - 1] ^= 0x80;
    absorb(last);
    for (int i = 0; i < 32; i++) out[i] = (uint8_t)(st[i / 8] >> (8 * (i % 8)));
}

// ---------------------------------------------------------------- host: the transcript
// the file's form of a coordinate -> its standard value, little-endian words
Fq fq_plain(const uint8_t c[32]) {
    Fq x;
    memcpy(x.v, c, 32);
    return Fq::from_mont(x);
}

struct Transcript {
    std::vector<uint8_t> buf;
    void words_be(const uint32_t w[8]) {
        for (int i = 7; i >= 0; i--)
            for (int b = 3; b >= 0; b--) buf.push_back((uint8_t)(w[i] >> (8 * b)));
    }
    void scalar_std(const uint8_t s[32]) {              // 32 bytes little-endian, standard
        for (int i = 31; i >= 0; i--) buf.push_back(s[i]);
    }
    void scalar(const Fr &m) {                          // Montgomery
        const Fr x = Fr::from_mont(m);
        words_be(x.v);
    }
    void point(const uint8_t p[64]) {                   // the file's form; infinity: 64 zero bytes
        words_be(fq_plain(p).v);
        words_be(fq_plain(p + 32).v);
    }
    // the digest as a big-endian integer mod r, Montgomery; the buffer is emptied
    Fr challenge() {
        uint8_t d[32], le[32];
        keccak256(d, buf.data(), buf.size());
        buf.clear();
        for (int i = 0; i < 32; i++) le[i] = d[31 - i];
        while (!below(le, FrParams::P)) {               // 2^256 < 6 r: five rounds at the most
            uint32_t w[8];
            memcpy(w, le, 32);
            uint64_t borrow = 0;
            for (int i = 0; i < 8; i++) {
                const uint64_t t = (uint64_t)w[i] - FrParams::P[i] - borrow;
                w[i] = (uint32_t)t;
                borrow = (t >> 32) & 1;
            }
            memcpy(le, w, 32);
        }
        return fr_from_std(le);
    }
};

struct Challenges {
    Fr beta, gamma, alpha, zeta, v, u;                // Montgomery
};

void round1_challenges(Challenges &c, const zk_plonk_vkey &vk, const uint8_t *publics, const uint8_t *pts) {
    Transcript t;
    const uint8_t *vkp[CIRC_VECS] = {vk.qm, vk.ql, vk.qr, vk.qo, vk.qc, vk.s1, vk.s2, vk.s3};
    for (uint32_t j = 0; j < CIRC_VECS; j++) t.point(vkp[j]);
    for (uint64_t i = 0; i < vk.n_public; i++) t.scalar_std(publics + i * 32);
    for (uint32_t j = P_A; j <= P_C; j++) t.point(pts + j * 64);
    c.beta = t.challenge();
    t.scalar(c.beta);
    c.gamma = t.challenge();
}
void round2_challenge(Challenges &c, const uint8_t *pts) {
    Transcript t;
    t.scalar(c.beta), t.scalar(c.gamma), t.point(pts + P_Z * 64);
    c.alpha = t.challenge();
}
void round3_challenge(Challenges &c, const uint8_t *pts) {
    Transcript t;
    t.scalar(c.alpha);
    for (uint32_t j = P_TLO; j <= P_THI; j++) t.point(pts + j * 64);
    c.zeta = t.challenge();
}
void round4_challenge(Challenges &c, const uint8_t *evals) {
    Transcript t;
    t.scalar(c.zeta);
    for (uint32_t j = 0; j < EVALS; j++) t.scalar_std(evals + j * 32);
    c.v = t.challenge();
}
void round5_challenge(Challenges &c, const uint8_t *pts) {
    Transcript t;
    t.point(pts + P_WZ * 64), t.point(pts + P_WZW * 64);
    c.u = t.challenge();
}

// ---------------------------------------------------------------- host: what prover and verifier both make of zeta
struct AtZeta {
    Fr zn, zh, l1, pi;                                // zeta^n, Z_H(zeta), L1(zeta), PI(zeta): Montgomery
};
// PI(zeta) = - sum_(i < l) publics[i] L_i(zeta), L_i = w^i Z_H / (n (X - w^i)): l products and ONE inversion (the prefix
// products of the denominators).  zeta^n = 1: L_i(zeta) is 1 where zeta = w^i and 0 elsewhere
AtZeta at_zeta(uint32_t log_n, const Fr &ze, const uint8_t *publics, uint64_t l) {
    AtZeta z;
    const Fr one = Fr::one(), w = root_of_unity(log_n), nn = fr_small(1ull << log_n);
    z.zn = ze;
    for (uint32_t i = 0; i < log_n; i++) z.zn = Fr::sqr(z.zn);
    z.zh = Fr::sub(z.zn, one);
    z.pi = Fr::zero();
    if (z.zh.is_zero()) {
        z.l1 = ze == one ? one : Fr::zero();
        Fr wi = one;
        for (uint64_t i = 0; i < l; i++, wi = Fr::mul(wi, w))
            if (wi == ze) z.pi = Fr::neg(fr_from_std(publics + i * 32));
        return z;
    }
    z.l1 = Fr::mul(z.zh, Fr::inv(Fr::mul(nn, Fr::sub(ze, one))));
    if (!l) return z;
    std::vector<Fr> den(l), pre(l);
    Fr wi = one, acc = one;
    for (uint64_t i = 0; i < l; i++, wi = Fr::mul(wi, w)) {
        den[i] = Fr::mul(nn, Fr::sub(ze, wi));
        pre[i] = acc;
        acc = Fr::mul(acc, den[i]);
    }
    Fr inv = Fr::inv(acc);
    // backwards: 1 / den[i] = pre[i] inv, inv *= den[i]; w^i from w^(l-1) down by w^-1
    const Fr winv = Fr::inv(w);
    wi = fr_pow(w, l - 1);
    Fr sum = Fr::zero();
    for (uint64_t i = l; i-- > 0;) {
        const Fr li = Fr::mul(wi, Fr::mul(pre[i], inv));          // w^i / (n (zeta - w^i))
        sum = Fr::add(sum, Fr::mul(fr_from_std(publics + i * 32), li));
        inv = Fr::mul(inv, den[i]);
        wi = Fr::mul(wi, winv);
    }
    z.pi = Fr::neg(Fr::mul(sum, z.zh));
    return z;
}

void check_below_r(const char *who, const char *what, const uint8_t *v, uint64_t n) {
    const uint64_t bad = first_not_below_r(v, n);
    if (bad < n) throw std::invalid_argument(std::string(who) + ": " + what + " " + std::to_string(bad) + " is not below r");
}
Fr checked_one(const char *who, const char *what, const uint8_t *v) { return checked_scalar(v, std::string(who) + ": " + what); }

uint32_t blocks_of(uint64_t n, uint32_t seg) { return nblocks(n, PV_WG * seg); }

}   // namespace

// ---------------------------------------------------------------- the object
struct zk_plonk_prover {
    zk_kzg *kzg = nullptr;                            // borrowed: it outlives the object
    zk_plonk_r1cs *r1cs = nullptr;                    // borrowed too: the compiled circuit of a prover made by zk_plonk_prover_create_r1cs
    int device = 0;
    uint32_t log_n = 0;
    uint64_t n = 0, cap = 0, n_witness = 0, n_public = 0;
    std::mutex mu;                                    // calls on one object are serialised
    std::unique_ptr<Stream> st;
    zk_plonk_circuit *circ = nullptr;                 // round 3's extensions and work vectors: owned
    zk_plonk_opening *open = nullptr;                 // rounds 4 and 5's coefficients and a proof's rows: owned
    PlonkPerm *perm = nullptr;                        // round 2's work buffers: owned
    DevBuf<uint32_t> maps;                            // 3 x n
    DevBuf<Fr> sig, shifts;                           // s1 .. s3 by values, 3 x n; 1, k1, k2
    DevBuf<Fr> wit, pub, blind;                       // a call's witness, publics and blinds
    DevBuf<Fr> vals;                                  // 4 x n: a, b, c and PI by values
    DevBuf<Fr> zval, pic;                             // z by values; PI by coefficients
    zk_plonk_vkey vk;
    uint32_t last_launches = 0, round_launches[ROUNDS] = {0, 0, 0, 0, 0};
    size_t own_bytes() const {
        return maps.bytes() + sig.bytes() + shifts.bytes() + wit.bytes() + pub.bytes() + blind.bytes() + vals.bytes() + zval.bytes() + pic.bytes();
    }
    ~zk_plonk_prover() {
        if (perm) plonk_perm_free(perm);
        if (open) zk_plonk_opening_destroy(open);
        if (circ) zk_plonk_circuit_destroy(circ);
    }
};

namespace {

uint64_t own_need_bytes(uint64_t n, uint64_t n_witness, uint64_t n_public) {
    return 3 * n * sizeof(uint32_t) + (3 * n + 3 + n_witness + n_public + 1 + BLINDS + 4 * n + 2 * n) * sizeof(Fr) + 65536;
}

uint64_t launches_now() { return g_kernel_launches.load(std::memory_order_relaxed); }

// [p] for `len` standard rows on the device, over the kzg's resident points
void commit_dev(zk_kzg *k, uint8_t out[64], const Fr *rows, uint64_t len, hipStream_t s) {
    std::lock_guard<std::mutex> kl(k->mu);             // the kzg's points and the work buffers of its multiplication
    msm_resident(k->msm, out, k->tau.p, rows, len, s);
}

zk_plonk_prover *prover_create(zk_kzg *kzg, const zk_plonk_circuit_view *v, const uint32_t *a_map, const uint32_t *b_map, const uint32_t *c_map,
                               uint64_t n_witness, uint64_t n_public, int32_t device) {
    const char *who = "zk_plonk_prover_create";
    if (!kzg || !v || !a_map || !b_map || !c_map) throw std::invalid_argument("null argument");
    if (v->log_n < MIN_LOG_N || v->log_n > MAX_LOG_N)
        throw std::invalid_argument(std::string(who) + ": log_n " + std::to_string(v->log_n) + " is outside 3 .. 25");
    if (v->basis != ZK_KZG_MONOMIAL && v->basis != ZK_KZG_LAGRANGE) throw std::invalid_argument(std::string(who) + ": basis " + std::to_string(v->basis) + " is unknown");
    const uint64_t n = 1ull << v->log_n, cap = kzg->max_coeffs;
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
    const uint8_t *vec[CIRC_VECS] = {v->ql, v->qr, v->qm, v->qo, v->qc, v->s1, v->s2, v->s3};
    static const char *const names[CIRC_VECS] = {"ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3"};
    for (uint32_t j = 0; j < CIRC_VECS; j++) {
        if (!vec[j]) throw std::invalid_argument("null argument");
        check_below_r(who, names[j], vec[j], n);
    }
    const Fr k1 = checked_one(who, "k1", v->k1), k2 = checked_one(who, "k2", v->k2);
    if (v->shift) {
        Fr g = checked_one(who, "shift", v->shift);
        if (g.is_zero()) throw std::invalid_argument(std::string(who) + ": shift is zero");
        for (uint32_t i = 0; i < v->log_n + 2; i++) g = Fr::sqr(g);
        if (g == Fr::one()) throw std::invalid_argument(std::string(who) + ": shift^(4n) is 1: Z_H vanishes on the coset");
    }
    std::unique_ptr<zk_plonk_prover> p(new zk_plonk_prover());
    p->kzg = kzg, p->device = kzg->device, p->log_n = v->log_n, p->n = n, p->cap = cap, p->n_witness = n_witness, p->n_public = n_public;
    const bool lagrange = v->basis == ZK_KZG_LAGRANGE;
    DeviceGuard dg(p->device);
    need_hbm(who, plonk_circuit_need_bytes(v->log_n) + plonk_opening_need_bytes(n, cap, lagrange) + plonk_perm_need_bytes(n) + own_need_bytes(n, n_witness, n_public));
    const uint64_t at = launches_now();
    if (zk_plonk_circuit_create(&p->circ, v, p->device) != 0) throw std::runtime_error(std::string(who) + ": " + zk_last_error());
    if (zk_plonk_opening_create(&p->open, kzg, v, p->device) != 0) throw std::runtime_error(std::string(who) + ": " + zk_last_error());
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
    Fr sh[3] = {Fr::from_mont(Fr::one()), Fr::from_mont(k1), Fr::from_mont(k2)};
    HIP_TRY(hipMemcpyAsync(p->shifts.p, sh, sizeof sh, hipMemcpyHostToDevice, s));
    // s1 .. s3 by values at w^i: the view's rows, or zk_fr_ntt's forward transform of their coefficients (once in the object's life)
    std::vector<uint8_t> sv;
    for (int j = 0; j < 3; j++) {
        const uint8_t *src = vec[C_S1 + j];
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
    vk.size = sizeof vk, vk.log_n = v->log_n, vk.n_public = n_public;
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
        throw std::invalid_argument(std::string(who) + ": a denominator of the permutation product is zero");
    if (!(fr_from_std(last) == Fr::one())) throw std::invalid_argument(std::string(who) + ": the copy constraints do not hold");
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
    if (t_len > 3 * n + 6) throw std::invalid_argument(std::string(who) + ": the witness does not satisfy the gates");
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
    if (memcmp(r_zeta, zero, 32) != 0) throw std::invalid_argument(std::string(who) + ": the witness does not satisfy the gates");
    end_round(4);
    HIP_TRY(hipMemsetAsync(p->blind.p, 0, p->blind.bytes(), s));      // and from the device: the next call uploads its own
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(proof, out, sizeof out);
    for (uint32_t r = 0; r < ROUNDS; r++) p->round_launches[r] = rounds[r];
    p->last_launches = (uint32_t)(launches_now() - first);
}

void plonk_prove(zk_plonk_prover *p, uint8_t *proof, const uint8_t *witness, const uint8_t *publics, const uint8_t *blind) {
    const char *who = "zk_plonk_prove";
    if (!p || !proof || !witness || (p->n_public && !publics)) throw std::invalid_argument("null argument");
    check_below_r(who, "witness", witness, p->n_witness);
    if (p->n_public) check_below_r(who, "publics", publics, p->n_public);
    uint8_t drawn[BLINDS * 32];
    Wipe wipe{drawn};
    blind = blinds_of(who, blind, drawn);
    const uint32_t seg = plonk_quot_seg();
    (void)plonk_perm_seg(), (void)plonk_open_seg(), (void)kzg_seg_in_effect();      // a bad knob is an error of the call before any work
    std::lock_guard<std::mutex> lock(p->mu);
    DeviceGuard dg(p->device);
    hipStream_t s = p->st->s;
    const uint64_t first = launches_now();
    HIP_TRY(hipMemcpyAsync(p->wit.p, witness, p->n_witness * sizeof(Fr), hipMemcpyHostToDevice, s));
    if (p->n_public) HIP_TRY(hipMemcpyAsync(p->pub.p, publics, p->n_public * sizeof(Fr), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(p->blind.p, blind, BLINDS * sizeof(Fr), hipMemcpyHostToDevice, s));
    plonk_prove_core(p, who, proof, publics, seg, first);
}

// a circom witness: its nWires values go up, the device extends them, the publics are w[1 .. 1 + n_public)
void plonk_prove_r1cs(zk_plonk_prover *p, uint8_t *proof, const uint8_t *wtns, uint32_t nVars, const uint8_t *blind) {
    const char *who = "zk_plonk_prove_r1cs";
    if (!p || !proof || !wtns) throw std::invalid_argument("null argument");
    if (!p->r1cs) throw std::invalid_argument(std::string(who) + ": the prover was not made from an r1cs (zk_plonk_prover_create_r1cs)");
    plonk_r1cs_check_witness(p->r1cs, who, wtns, nVars);
    uint8_t drawn[BLINDS * 32];
    Wipe wipe{drawn};
    blind = blinds_of(who, blind, drawn);
    const uint32_t seg = plonk_quot_seg();
    (void)plonk_perm_seg(), (void)plonk_open_seg(), (void)kzg_seg_in_effect();
    const uint8_t *publics = wtns + 32;
    std::lock_guard<std::mutex> lock(p->mu);
    DeviceGuard dg(p->device);
    hipStream_t s = p->st->s;
    const uint64_t first = launches_now();
    HIP_TRY(hipMemcpyAsync(p->wit.p, wtns, (size_t)nVars * sizeof(Fr), hipMemcpyHostToDevice, s));
    if (p->n_public) HIP_TRY(hipMemcpyAsync(p->pub.p, publics, p->n_public * sizeof(Fr), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(p->blind.p, blind, BLINDS * sizeof(Fr), hipMemcpyHostToDevice, s));
    plonk_r1cs_extend_dev(p->r1cs, p->wit.p, s);
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

// ---------------------------------------------------------------- the verifier
typedef Pt<Fq> P1;

// a point of the curve in the file's form (or infinity), both coordinates below q
bool g1_well_formed(const uint8_t p[64]) {
    static const uint8_t zero[64] = {0};
    if (memcmp(p, zero, 64) == 0) return true;
    if (!below(p, FqParams::P) || !below(p + 32, FqParams::P)) return false;
    Fq x, y;
    memcpy(x.v, p, 32);
    memcpy(y.v, p + 32, 32);
    return Fq::sqr(y) == Fq::add(Fq::mul(Fq::sqr(x), x), curve_b<Fq>());
}

void plonk_verify(zk_kzg *kzg, const zk_plonk_vkey *vk, const uint8_t *proof, const uint8_t *publics, uint8_t *verdict) {
    const char *who = "zk_plonk_verify";
    if (!kzg || !vk || !proof || !verdict || (vk->n_public && !publics)) throw std::invalid_argument("null argument");
    if (vk->size != sizeof(zk_plonk_vkey)) throw std::invalid_argument(std::string(who) + ": vk->size is not sizeof(zk_plonk_vkey)");
    if (vk->log_n < MIN_LOG_N || vk->log_n > MAX_LOG_N) throw std::invalid_argument(std::string(who) + ": log_n " + std::to_string(vk->log_n) + " is outside 3 .. 25");
    const uint64_t n = 1ull << vk->log_n;
    if (vk->n_public > n) throw std::invalid_argument(std::string(who) + ": n_public " + std::to_string(vk->n_public) + " exceeds n = " + std::to_string(n));
    if (memcmp(vk->tau_g2, kzg->g2tau, sizeof vk->tau_g2) != 0) throw std::invalid_argument(std::string(who) + ": the key's [tau]G2 is not the kzg's");
    const Fr k1 = checked_one(who, "k1", vk->k1), k2 = checked_one(who, "k2", vk->k2);
    const uint8_t *vkp[CIRC_VECS] = {vk->qm, vk->ql, vk->qr, vk->qo, vk->qc, vk->s1, vk->s2, vk->s3};
    for (uint32_t j = 0; j < CIRC_VECS; j++)
        if (!g1_well_formed(vkp[j])) throw std::invalid_argument(std::string(who) + ": a commitment of the key is not a point of the curve");
    const uint8_t *pts = proof, *evals = proof + POINTS * 64;
    *verdict = ZK_VERIFY_MALFORMED;
    for (uint32_t j = 0; j < POINTS; j++)
        if (!g1_well_formed(pts + j * 64)) return;
    if (first_not_below_r(evals, EVALS) < EVALS) return;
    if (first_not_below_r(publics, vk->n_public) < vk->n_public) return;

    Challenges ch;
    round1_challenges(ch, *vk, publics, pts);
    round2_challenge(ch, pts);
    round3_challenge(ch, pts);
    round4_challenge(ch, evals);
    round5_challenge(ch, pts);
    const Fr al = ch.alpha, be = ch.beta, ga = ch.gamma, ze = ch.zeta, v = ch.v, u = ch.u;
    const AtZeta z = at_zeta(vk->log_n, ze, publics, vk->n_public);
    Fr ev[EVALS];
    for (uint32_t j = 0; j < EVALS; j++) ev[j] = fr_from_std(evals + j * 32);
    const Fr a = ev[0], b = ev[1], c = ev[2], s1 = ev[3], s2 = ev[4], zw = ev[5];
    const Fr al2l1 = Fr::mul(Fr::sqr(al), z.l1), bz = Fr::mul(be, ze);
    const Fr g12 = Fr::mul(Fr::add(Fr::add(a, Fr::mul(be, s1)), ga), Fr::add(Fr::add(b, Fr::mul(be, s2)), ga));
    const Fr g12zw_alpha = Fr::mul(Fr::mul(g12, zw), al);
    const Fr r0 = Fr::sub(Fr::add(Fr::mul(g12zw_alpha, Fr::add(c, ga)), al2l1), z.pi);
    const Fr f123 = Fr::mul(Fr::mul(Fr::add(Fr::add(a, bz), ga), Fr::add(Fr::add(b, Fr::mul(bz, k1)), ga)), Fr::add(Fr::add(c, Fr::mul(bz, k2)), ga));
    auto pt = [&](uint32_t j) { return P1(pts + j * 64); };
    // D, then F
    P1 F = P1(vk->qm).times(Fr::mul(a, b)) + P1(vk->ql).times(a) + P1(vk->qr).times(b) + P1(vk->qo).times(c) + P1(vk->qc);
    F = F + pt(P_Z).times(Fr::add(Fr::add(Fr::mul(al, f123), al2l1), u));
    F = F - P1(vk->s3).times(Fr::mul(g12zw_alpha, be));
    F = F - (pt(P_TLO) + pt(P_TMID).times(z.zn) + pt(P_THI).times(Fr::sqr(z.zn))).times(z.zh);
    const P1 batch[5] = {pt(P_A), pt(P_B), pt(P_C), P1(vk->s1), P1(vk->s2)};
    Fr vp = v, e = r0;
    for (int j = 0; j < 5; j++) {
        F = F + batch[j].times(vp);
        e = Fr::add(e, Fr::mul(vp, ev[j]));
        vp = Fr::mul(vp, v);
    }
    e = Fr::add(e, Fr::mul(u, zw));
    const P1 E = P1(kzg->g1).times(e);
    const Fr uzw = Fr::mul(u, Fr::mul(ze, root_of_unity(vk->log_n)));
    const P1 L = pt(P_WZ).times(ze) + pt(P_WZW).times(uzw) + F - E;
    const P1 W = pt(P_WZ) + pt(P_WZW).times(u);
    *verdict = kzg_pair_one(kzg, L.b, W.b);
}

}   // namespace

extern "C" {

int zk_keccak256(uint8_t out32[32], const uint8_t *data, uint64_t len) {
    return guarded([&] {
        if (!out32 || (len && !data)) throw std::invalid_argument("null argument");
        keccak256(out32, data, len);
    });
}

int zk_plonk_prover_create(zk_plonk_prover **out, zk_kzg *kzg, const zk_plonk_circuit_view *view, const uint32_t *a_map, const uint32_t *b_map,
                           const uint32_t *c_map, uint64_t n_witness, uint64_t n_public, int32_t device) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        *out = prover_create(kzg, view, a_map, b_map, c_map, n_witness, n_public, device);
    });
}

void zk_plonk_prover_destroy(zk_plonk_prover *p) {
    if (!p) return;
    int prev = -1;
    const bool switched = hipGetDevice(&prev) == hipSuccess && hipSetDevice(p->device) == hipSuccess;
    delete p;
    if (switched) (void)hipSetDevice(prev);
}

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
        if (plan->size < 4) throw std::invalid_argument("zk_plonk_prover_info: plan->size is not set");
        zk_plonk_prover_plan q{};
        q.scan_seg = plonk_perm_seg(), q.quot_seg = plonk_quot_seg(), q.open_seg = plonk_open_seg(), q.kzg_seg = kzg_seg_in_effect();
        std::lock_guard<std::mutex> lock(p->mu);
        q.size = plan->size < sizeof q ? plan->size : (uint32_t)sizeof q;
        q.log_n = p->log_n;
        q.n_witness = p->n_witness, q.n_public = p->n_public;
        q.device_bytes = p->own_bytes() + plonk_circuit_bytes(p->circ) + plonk_opening_bytes(p->open) + plonk_perm_bytes(p->perm);
        q.last_launches = p->last_launches;
        for (uint32_t r = 0; r < ROUNDS; r++) q.round_launches[r] = p->round_launches[r];
        memcpy(plan, &q, q.size);
    });
}

int zk_plonk_prove(zk_plonk_prover *p, uint8_t proof[ZK_PLONK_PROOF_BYTES], const uint8_t *witness, const uint8_t *publics, const uint8_t *blind) {
    return guarded([&] { plonk_prove(p, proof, witness, publics, blind); });
}

int zk_plonk_verify(zk_kzg *kzg, const zk_plonk_vkey *vk, const uint8_t proof[ZK_PLONK_PROOF_BYTES], const uint8_t *publics, uint8_t *verdict) {
    return guarded([&] { plonk_verify(kzg, vk, proof, publics, verdict); });
}

int zk_plonk_prover_create_r1cs(zk_plonk_prover **out, zk_kzg *kzg, zk_plonk_r1cs *compiled, const uint8_t *shift, int32_t device) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        *out = prover_create_r1cs(kzg, compiled, shift, device);
    });
}

int zk_plonk_prove_r1cs(zk_plonk_prover *p, uint8_t proof[ZK_PLONK_PROOF_BYTES], const uint8_t *wtns, uint32_t nVars, const uint8_t *blind) {
    return guarded([&] { plonk_prove_r1cs(p, proof, wtns, nVars, blind); });
}

}   // extern "C"
