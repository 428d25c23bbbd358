// n G1 points times ONE scalar, and the phase-2 contribution built on it (include/zkhip.h, section "Phase-2
// contribution").  Nothing in the reference corresponds to it: its prover reads a finished .zkey
// (src/main_prover.cpp:57-72); the counterpart is the arithmetic of snarkjs `zkey contribute`: delta <- delta d, every
// point of sections 8 (C) and 9 (H) <- d^-1 point.
//
// A scalar the whole grid shares is known to the host, which buys two things a per-lane scalar cannot have.
//
// The endomorphism.  BN254 has phi(x, y) = (beta x, y) = lambda (x, y), beta^3 = 1 in Fq, lambda^2 + lambda + 1 = 0 in
// Fr.  The host writes k = k1 + k2 lambda with |k1|, |k2| < 2^127 (split(): the nearest lattice vector to (k, 0) in the
// lattice {(a, b) : a + b lambda = 0 mod r}, whose reduced basis the extended Euclid on (r, lambda) gives), so that
// k P = k1 P + k2 phi(P) takes 127 doublings instead of 254.  The split is checked in Fr on every call.
//
// The schedule.  |k1| and |k2| are recoded together into a joint sparse form (Solinas): digits in {-1, 0, 1}, at most
// 128 columns, about half of them empty, and the signs of k1 and k2 folded into the digits.  A column that is not empty
// adds one of  +-P, +-phi(P)  or, when both digits are set, +-(P + phi(P)) or +-(P - phi(P)).  P + phi(P) is free:
// 1 + lambda + lambda^2 = 0 makes it -phi^2(P) = (beta^2 x, -y), and beta^2 x = -(x + beta x).  So every column but the
// opposite-sign ones is ONE mixed addition of an affine point made of registers the lane holds anyway; P - phi(P) has no
// such form (1 - lambda has norm 3) and is added as two.  A table entry for it would have to be XYZZ (an affine one
// costs an inversion per lane): 32 more live VGPRs to replace two mixed additions (20 products) by one general addition
// (14) on one column in ten.  The schedule reaches the kernel as a byte per column in device memory, read with a
// wave-uniform index: every branch on it is uniform, nothing is indexed in registers or kept in scratch.  It lives in a
// buffer of the call's own and not in the kernel arguments because the library can wipe the one and not the other.
//
// Special cases.  The accumulator is at infinity until the first column that is not empty, and with k in {small, +-lambda,
// +-lambda +- 1, ...} it meets +- the point it adds.  curve.hpp's dbl / madd take all of them explicitly; nothing here
// assumes they do not happen.
//
// Fields: curve.hpp's 8 x 32-bit Montgomery forms (R = 2^256), the .zkey's own bytes, as setup.hip and ptau_prepare.hip.
//
// The yardstick.  k_scale_g1_plain is devmem.hpp's scalar_mul_affine with the same shared scalar, one lane per point:
// what the project had before this file.  ZKHIP_SCALE_PLAIN=1 runs it in place of k_scale_g1: a second route to the
// same bytes for the tests, and the denominator of tools/contribute_timing.py.
#include "chunklanes.hpp"
#include "ptcheck.hpp"

namespace {

constexpr uint32_t SCALE_COLS = 130;                 // the bound on the schedule's length that zkhip.h documents (reached: 128)
constexpr uint32_t SCHED_WORDS = 1 + (SCALE_COLS + 3) / 4 + 8;   // length, a byte per column, the scalar itself (plain kernel)
constexpr uint64_t DEFAULT_CHUNK = 1ull << 20;       // points per chunk: 64 MiB of input

// ---------------------------------------------------------------- host: 256-bit integers, wrapping
struct U256 {
    uint64_t w[4];
};
typedef unsigned __int128 u128;

const U256 R_STD = {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
// lambda = 4407920970296243842393367215006156084916469457145843978461
const U256 LAMBDA = {{0x8b17ea66b99c90ddull, 0x5bfc41088d8daaa7ull, 0xb3c4d79d41a91758ull, 0}};
// beta = 2203960485148121921418603742825762020974279258880205651966, standard form
const uint32_t BETA_STD[8] = {0x77fffffeu, 0x57634731u, 0xacdb5c4fu, 0xd4f263f1u, 0xa0d48bacu, 0x59e26bceu, 0, 0};
// The reduced basis v1 = (A, -B), v2 = (C, A) of {(a, b) : a + b lambda = 0 mod r}: the extended Euclid on (r, lambda)
// gives remainders r_i = s_i r + t_i lambda, so (r_i, -t_i) is in the lattice; v1 is the first with r_i < sqrt(r), v2 the
// shorter of its two neighbours.  A^2 + B C = r.
const U256 BASIS_A = {{0x89d3256894d213e3ull, 0, 0, 0}};
const U256 BASIS_B = {{0x8211bbeb7d4f1128ull, 0x6f4d8248eeb859fcull, 0, 0}};
const U256 BASIS_C = {{0x0be4e1541221250bull, 0x6f4d8248eeb859fdull, 0, 0}};

bool geq(const U256 &a, const U256 &b) {
    for (int i = 3; i >= 0; i--)
        if (a.w[i] != b.w[i]) return a.w[i] > b.w[i];
    return true;
}
bool is_zero(const U256 &a) { return !(a.w[0] | a.w[1] | a.w[2] | a.w[3]); }
U256 sub(const U256 &a, const U256 &b) {
    U256 r;
    uint64_t bw = 0;
    for (int i = 0; i < 4; i++) {
        const u128 d = (u128)a.w[i] - b.w[i] - bw;
        r.w[i] = (uint64_t)d;
        bw = (uint64_t)(d >> 64) & 1;
    }
    return r;
}
U256 neg(const U256 &a) { return sub(U256{{0, 0, 0, 0}}, a); }
void mul_wide(const U256 &a, const U256 &b, uint64_t out[8]) {
    for (int i = 0; i < 8; i++) out[i] = 0;
    for (int i = 0; i < 4; i++) {
        uint64_t c = 0;
        for (int j = 0; j < 4; j++) {
            const u128 t = (u128)a.w[i] * b.w[j] + out[i + j] + c;
            out[i + j] = (uint64_t)t;
            c = (uint64_t)(t >> 64);
        }
        out[i + 4] = c;
    }
}
U256 mul_lo(const U256 &a, const U256 &b) {
    uint64_t t[8];
    mul_wide(a, b, t);
    U256 r = {{t[0], t[1], t[2], t[3]}};
    explicit_bzero(t, sizeof t);
    return r;
}
// round(a b / r) for a < r, b < 2^128
U256 mul_div_r_round(const U256 &a, const U256 &b) {
    uint64_t num[8];
    mul_wide(a, b, num);
    U256 half = R_STD;                                // (r - 1) / 2: r is odd, so adding it rounds to nearest
    for (int i = 0; i < 4; i++) half.w[i] = (half.w[i] >> 1) | (i < 3 ? half.w[i + 1] << 63 : 0);
    uint64_t c = 0;
    for (int i = 0; i < 8; i++) {
        const u128 s = (u128)num[i] + (i < 4 ? half.w[i] : 0) + c;
        num[i] = (uint64_t)s;
        c = (uint64_t)(s >> 64);
    }
    U256 q = {{0, 0, 0, 0}}, rem = {{0, 0, 0, 0}};    // schoolbook, a bit at a time: once per call
    for (int i = 511; i >= 0; i--) {
        for (int j = 3; j > 0; j--) {
            rem.w[j] = (rem.w[j] << 1) | (rem.w[j - 1] >> 63);
            q.w[j] = (q.w[j] << 1) | (q.w[j - 1] >> 63);
        }
        rem.w[0] = (rem.w[0] << 1) | ((num[i >> 6] >> (i & 63)) & 1);
        q.w[0] <<= 1;
        if (geq(rem, R_STD)) {
            rem = sub(rem, R_STD);
            q.w[0] |= 1;
        }
    }
    explicit_bzero(num, sizeof num);
    explicit_bzero(&rem, sizeof rem);
    return q;
}

Fr fr_mont(const U256 &a) {
    Fr x;
    for (int i = 0; i < 4; i++) {
        x.v[2 * i] = (uint32_t)a.w[i];
        x.v[2 * i + 1] = (uint32_t)(a.w[i] >> 32);
    }
    return Fr::to_mont(x);
}
U256 load_u256(const uint8_t k[32]) {
    U256 a;
    memcpy(a.w, k, 32);
    return a;
}

// ---------------------------------------------------------------- host: the plan of one scalar
// Everything here is as secret as the scalar: wipe() before the object leaves scope.
struct ScalePlan {
    uint32_t len = 0;                                 // columns; 0 for k = 0
    int8_t dp[SCALE_COLS], dphi[SCALE_COLS];          // sum_i 2^i (dp[i] + lambda dphi[i]) = k mod r
    uint32_t words[SCHED_WORDS];                      // what the kernels read (device image)
    void wipe() { explicit_bzero(this, sizeof *this); }
};

// k = k1 + k2 lambda mod r, as signs and magnitudes below 2^128
void split(const U256 &k, u128 &m1, bool &neg1, u128 &m2, bool &neg2) {
    // (k, 0) = x1 v1 + x2 v2 over the rationals with x1 = k A / r, x2 = k B / r; rounded, the difference is short
    U256 c1 = mul_div_r_round(k, BASIS_A), c2 = mul_div_r_round(k, BASIS_B);
    U256 k1 = sub(sub(k, mul_lo(c1, BASIS_A)), mul_lo(c2, BASIS_C));          // k - c1 A - c2 C
    U256 k2 = sub(mul_lo(c1, BASIS_B), mul_lo(c2, BASIS_A));                  // c1 B - c2 A
    neg1 = k1.w[3] >> 63;
    neg2 = k2.w[3] >> 63;
    if (neg1) k1 = neg(k1);
    if (neg2) k2 = neg(k2);
    const bool fits = !(k1.w[2] | k1.w[3] | k2.w[2] | k2.w[3]);
    // the proof that the schedule computes k P, made on every call: k1 + k2 lambda = k in Fr
    Fr a = fr_mont(k1), b = Fr::mul(fr_mont(k2), fr_mont(LAMBDA));
    if (neg1) a = Fr::neg(a);
    if (neg2) b = Fr::neg(b);
    const bool same = Fr::add(a, b) == fr_mont(k);
    m1 = ((u128)k1.w[1] << 64) | k1.w[0];
    m2 = ((u128)k2.w[1] << 64) | k2.w[0];
    explicit_bzero(&c1, sizeof c1);
    explicit_bzero(&c2, sizeof c2);
    explicit_bzero(&k1, sizeof k1);
    explicit_bzero(&k2, sizeof k2);
    explicit_bzero(&a, sizeof a);
    explicit_bzero(&b, sizeof b);
    if (!fits || !same) throw std::logic_error("scalar split failed its check");
}

// what a column adds: 0 nothing, else 1 + 2 * (0: x, 1: beta x, 2: beta^2 x) + (1: -y)
uint32_t op_code(uint32_t xsel, bool yneg) { return 1 + 2 * xsel + (yneg ? 1 : 0); }

void make_plan(const uint8_t k32[32], ScalePlan &pl) {
    U256 k = load_u256(k32);
    if (geq(k, R_STD)) throw std::invalid_argument("the scalar is not below r");
    memset(&pl, 0, sizeof pl);
    u128 k0, k1;
    bool n0, n1;
    split(k, k0, n0, k1, n1);
    // joint sparse form of (k0, k1) (Solinas 2001, as Hankerson, Menezes, Vanstone alg. 3.50), least significant first
    uint32_t d0 = 0, d1 = 0, len = 0;
    while (k0 || d0 || k1 || d1) {
        const uint32_t l0 = ((uint32_t)k0 + d0) & 7, l1 = ((uint32_t)k1 + d1) & 7;
        auto digit = [](uint32_t l, uint32_t other) {
            if (!(l & 1)) return 0;
            int u = (l & 3) == 1 ? 1 : -1;
            if ((l == 3 || l == 5) && (other & 3) == 2) u = -u;
            return u;
        };
        const int u0 = digit(l0, l1), u1 = digit(l1, l0);
        if (2 * (int)d0 == 1 + u0) d0 = 1 - d0;
        if (2 * (int)d1 == 1 + u1) d1 = 1 - d1;
        k0 >>= 1;
        k1 >>= 1;
        if (len >= SCALE_COLS) throw std::logic_error("scalar schedule is longer than its bound");
        pl.dp[len] = (int8_t)(n0 ? -u0 : u0);
        pl.dphi[len] = (int8_t)(n1 ? -u1 : u1);
        len++;
    }
    pl.len = len;
    pl.words[0] = len;
    for (uint32_t i = 0; i < len; i++) {
        const int a = pl.dp[i], b = pl.dphi[i];
        uint32_t ops = 0;
        if (a && b && a == b) ops = op_code(2, a > 0);                       // +-(P + phi P) = -+(beta^2 x, y)
        else if (a && b) ops = op_code(0, a < 0) | op_code(1, b < 0) << 3;   // two additions
        else if (a) ops = op_code(0, a < 0);
        else if (b) ops = op_code(1, b < 0);
        pl.words[1 + (i >> 2)] |= ops << (8 * (i & 3));
    }
    memcpy(&pl.words[SCHED_WORDS - 8], k.w, 32);
    explicit_bzero(&k, sizeof k);
    explicit_bzero(&k0, sizeof k0);
    explicit_bzero(&k1, sizeof k1);
}

// ---------------------------------------------------------------- device
// out[i] = k in[i], XYZZ.  sched: word 0 the number of columns, then a byte per column (op_code of up to two additions)
__global__ __launch_bounds__(64) void k_scale_g1(G1XYZZ *__restrict__ out, const G1Affine *__restrict__ in, uint64_t n,
                                                 const uint32_t *__restrict__ sched, Fq beta) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G1Affine P = load_pt(in + i);
    G1XYZZ acc = G1XYZZ::inf();
    if (!P.is_inf()) {
        const Fq bx = Fq::mul(P.x, beta);                                    // phi(P) = (beta x, y)
        const Fq b2x = Fq::neg(Fq::add(P.x, bx));                            // beta^2 = -1 - beta
        const Fq ny = Fq::neg(P.y);
        for (uint32_t c = sched[0]; c-- > 0;) {
            acc = dbl(acc);
            uint32_t ops = (sched[1 + (c >> 2)] >> (8 * (c & 3))) & 0xFFu;
            for (; ops & 7u; ops >>= 3) {                                    // wave-uniform: 0, 1 or 2 additions
                const uint32_t op = (ops & 7u) - 1;
                G1Affine T;
                T.x = (op >> 1) == 0 ? P.x : (op >> 1) == 1 ? bx : b2x;
                T.y = (op & 1) ? ny : P.y;
                madd(acc, T);
            }
        }
    }
    store_pt(out + i, acc);
}

// the same by devmem.hpp's double-and-add over the 254 bits of k (standard form, behind the schedule)
__global__ __launch_bounds__(64) void k_scale_g1_plain(G1XYZZ *__restrict__ out, const G1Affine *__restrict__ in, uint64_t n,
                                                       const uint32_t *__restrict__ sched) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_pt(out + i, scalar_mul_affine(load_pt(in + i), load_el(reinterpret_cast<const Fr *>(sched + SCHED_WORDS - 8))));
}

// ---------------------------------------------------------------- host: rows of points through the device, in chunks
uint64_t chunk_points() { return env_number("ZKHIP_SCALE_CHUNK", DEFAULT_CHUNK, 1, 1ull << 28, "a number of points from 1 to 2^28", ENV_LAX); }

uint64_t scaler_bytes(uint64_t cap) { return ChunkLanes<Fq>::bytes(cap, false) + 4096; }

// The schedule on the device: zeroed before it is freed, after the lanes that read it have drained (declared before them)
struct SecretSchedule {
    DevBuf<uint32_t> d;
    ~SecretSchedule() {
        if (d.p) (void)hipMemset(d.p, 0, d.bytes());
    }
};

struct Scaler {
    SecretSchedule sched;                             // before the lanes (chunklanes.hpp): wiped after they have drained
    ChunkLanes<Fq> lanes;                             // one word of checks: ptcheck.hpp's
    bool plain;
    Fq beta;
    Scaler(const ScalePlan &pl, uint64_t cap) : lanes(cap, false, 1), plain(env_switch("ZKHIP_SCALE_PLAIN")), beta(fq_std(BETA_STD)) {
        sched.d.alloc(SCHED_WORDS);
        HIP_TRY(hipMemcpy(sched.d.p, pl.words, sizeof pl.words, hipMemcpyHostToDevice));
    }
    // out[i] = k in[i], i < n (host memory, 64 bytes a point); a point that failed its check is an error naming `what` and the index
    void run(uint8_t *out, const uint8_t *in, uint64_t n, const char *what) {
        lanes.run(
            out, in, n,
            [&](Lane<Fq> &l) {
                hipStream_t s = l.st.s;
                launch_point_check<Fq>(l.err.p, l.aff.p, l.cnt, s);
                HIP_TRY(hipMemcpyAsync(l.words(), l.err.p, 4, hipMemcpyDeviceToHost, s));
                if (plain) ZK_LAUNCH(k_scale_g1_plain, dim3(nblocks(l.cnt, 64)), dim3(64), 0, s, l.xyzz.p, l.aff.p, l.cnt, sched.d.p);
                else ZK_LAUNCH(k_scale_g1, dim3(nblocks(l.cnt, 64)), dim3(64), 0, s, l.xyzz.p, l.aff.p, l.cnt, sched.d.p, beta);
                ZK_LAUNCH_OK("g1 scale");
            },
            [&](const Lane<Fq> &l) {
                const uint32_t bad = *l.words();
                if (bad != NO_BAD_POINT) throw std::invalid_argument(std::string(what) + ": point " + std::to_string(l.off + bad) + " is not on the curve");
            });
    }
};

void g1_scale(uint8_t *out, const uint8_t *points, uint64_t n, const uint8_t k[32], int32_t device) {
    if (!k || (n && (!out || !points))) throw std::invalid_argument("null argument");
    ScalePlan pl;
    struct Wipe {
        ScalePlan &p;
        ~Wipe() { p.wipe(); }
    } wipe{pl};
    try {
        make_plan(k, pl);
    } catch (const std::invalid_argument &) {
        throw std::invalid_argument("zk_g1_scale: the scalar is not below r");
    }
    if (!n) return;
    const uint64_t chunk = chunk_points(), cap = n < chunk ? n : chunk;
    DeviceGuard g(resolve_device(device));
    need_hbm("zk_g1_scale", scaler_bytes(cap));
    Scaler sc(pl, cap);
    sc.run(out, points, n, "zk_g1_scale");
}

// ---------------------------------------------------------------- the contribution
template <class F>
bool host_below_q(const F &a);
template <>
bool host_below_q<Fq>(const Fq &a) {
    for (int i = 7; i >= 0; i--)
        if (a.v[i] != FqParams::P[i]) return a.v[i] < FqParams::P[i];
    return false;
}
template <>
bool host_below_q<Fq2>(const Fq2 &a) { return host_below_q(a.a) && host_below_q(a.b); }
template <class F>
bool host_point_ok(const void *bytes) {               // a point of the curve other than infinity
    Affine<F> p;
    memcpy(&p, bytes, sizeof p);
    if (p.is_inf() || !host_below_q(p.x) || !host_below_q(p.y)) return false;
    return F::sqr(p.y) == F::add(F::mul(F::sqr(p.x), p.x), curve_b<F>());
}

struct ContribPlan {
    uint64_t nC = 0, nH = 0, cap = 0, device_bytes = 0;
};

void check_view(const zk_zkey_contrib_view *v, ContribPlan &cp) {
    if (!v) throw std::invalid_argument("null argument");
    if (!v->vk_delta1 || !v->vk_delta2) throw std::invalid_argument("zkey has no delta points");
    const struct {
        int id;
        const void *p;
        uint64_t bytes;
    } sec[2] = {{8, v->pointsC, v->pointsC_bytes}, {9, v->pointsH, v->pointsH_bytes}};
    for (const auto &s : sec) {
        if (s.bytes % sizeof(G1Affine))
            throw std::invalid_argument("zkey section " + std::to_string(s.id) + " is " + std::to_string(s.bytes) + " bytes: not a whole number of points");
        if (s.bytes && !s.p) throw std::invalid_argument("zkey has no section " + std::to_string(s.id));
    }
    if (!host_point_ok<Fq>(v->vk_delta1)) throw std::invalid_argument("zkey vk_delta_1 is not a point of the curve");
    if (!host_point_ok<Fq2>(v->vk_delta2)) throw std::invalid_argument("zkey vk_delta_2 is not a point of the curve");
    cp.nC = v->pointsC_bytes / sizeof(G1Affine);
    cp.nH = v->pointsH_bytes / sizeof(G1Affine);
    const uint64_t most = cp.nC > cp.nH ? cp.nC : cp.nH, chunk = chunk_points();
    cp.cap = most < chunk ? most : chunk;
    cp.device_bytes = scaler_bytes(cp.cap ? cp.cap : 1);
}

void zkey_contribute(const zk_zkey_contrib_view *v, const uint8_t d32[32], int32_t device, zk_zkey_contrib_out *out) {
    ContribPlan cp;
    check_view(v, cp);                                // the key and the scalar are checked before the device is touched
    if (!d32) throw std::invalid_argument("null argument");
    if (!out || !out->vk_delta1 || !out->vk_delta2 || (cp.nC && !out->pointsC) || (cp.nH && !out->pointsH))
        throw std::invalid_argument("null output buffer");
    struct Secrets {
        U256 d;
        Fr dm, dinv;
        uint8_t dinv32[32];
        ScalePlan pl;
        ~Secrets() { explicit_bzero(this, sizeof *this); }
    } sec;
    sec.d = load_u256(d32);
    if (is_zero(sec.d)) throw std::invalid_argument("zk_zkey_contribute: the contribution scalar is 0");
    if (geq(sec.d, R_STD)) throw std::invalid_argument("zk_zkey_contribute: the contribution scalar is not below r");
    sec.dm = fr_mont(sec.d);
    sec.dinv = Fr::from_mont(Fr::inv(sec.dm));
    memcpy(sec.dinv32, sec.dinv.v, 32);
    make_plan(sec.dinv32, sec.pl);
    DeviceGuard g(resolve_device(device));
    need_hbm("zk_zkey_contribute", cp.device_bytes);
    if (zk_g1_mul(out->vk_delta1, static_cast<const uint8_t *>(v->vk_delta1), d32) != 0 ||
        zk_g2_mul(out->vk_delta2, static_cast<const uint8_t *>(v->vk_delta2), d32) != 0)
        throw std::runtime_error("zk_zkey_contribute: delta could not be multiplied");
    if (!cp.cap) return;
    Scaler sc(sec.pl, cp.cap);
    sc.run(out->pointsC, static_cast<const uint8_t *>(v->pointsC), cp.nC, "zkey section 8");
    sc.run(out->pointsH, static_cast<const uint8_t *>(v->pointsH), cp.nH, "zkey section 9");
}

}   // namespace

extern "C" {

int zk_g1_scale_plan(const uint8_t k[32], int8_t *digits_p, int8_t *digits_phi, uint32_t cap, uint32_t *len) {
    return guarded([&] {
        if (!k || !len || (cap && (!digits_p || !digits_phi))) throw std::invalid_argument("null argument");
        ScalePlan pl;
        struct Wipe {
            ScalePlan &p;
            ~Wipe() { p.wipe(); }
        } wipe{pl};
        try {
            make_plan(k, pl);
        } catch (const std::invalid_argument &) {
            throw std::invalid_argument("zk_g1_scale_plan: the scalar is not below r");
        }
        *len = pl.len;
        if (pl.len > cap) throw std::invalid_argument("zk_g1_scale_plan: the schedule has " + std::to_string(pl.len) + " columns, room for " + std::to_string(cap));
        memcpy(digits_p, pl.dp, pl.len);
        memcpy(digits_phi, pl.dphi, pl.len);
    });
}

int zk_g1_scale(uint8_t *out, const uint8_t *points, uint64_t n, const uint8_t k[32], int32_t device) {
    return guarded([&] { g1_scale(out, points, n, k, device); });
}

int zk_zkey_contribute_sizes(const zk_zkey_contrib_view *zkey, zk_zkey_contrib_sizes *sizes) {
    return guarded([&] {
        if (!sizes) throw std::invalid_argument("null argument");
        ContribPlan cp;
        check_view(zkey, cp);
        sizes->pointsC_bytes = cp.nC * sizeof(G1Affine);
        sizes->pointsH_bytes = cp.nH * sizeof(G1Affine);
        sizes->chunk_points = cp.cap;
        sizes->device_bytes = cp.device_bytes;
    });
}

int zk_zkey_contribute(const zk_zkey_contrib_view *zkey, const uint8_t d[32], int32_t device, zk_zkey_contrib_out *out) {
    return guarded([&] { zkey_contribute(zkey, d, device, out); });
}

}   // extern "C"
