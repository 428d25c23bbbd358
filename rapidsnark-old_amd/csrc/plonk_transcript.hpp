// What the PLONK prover (plonkprove.hip, plonkopen.hip) and the verifier (plonkverify.hip) must agree on, host code only
// and in one copy: the layout of a proof, Keccak-256, the Fiat-Shamir transcript with its five round challenges, what both
// make of zeta (zeta^n, Z_H, L1, PI) and the scalars of the linearisation.  A few hundred bytes a round: nothing here is
// worth a kernel.  tools/plonk_transcript_host_test.cpp runs it under the address and undefined-behaviour sanitizers.
#pragma once
#include <vector>

#include "ptengine.hpp"
#include "plonk_verify_dev.hpp"

namespace zkp {

constexpr uint32_t PLONK_EVALS = 6, PLONK_POINTS = 9;
enum { P_A, P_B, P_C, P_Z, P_TLO, P_TMID, P_THI, P_WZ, P_WZW };     // the proof's points; then a b c s1 s2 z(zeta w)
static_assert(ZK_PLONK_PROOF_BYTES == PLONK_POINTS * 64 + PLONK_EVALS * 32, "layout");

// ---------------------------------------------------------------- Keccak-256
inline constexpr uint64_t KECCAK_RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,
                                             0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,
                                             0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,
                                             0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
                                             0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
inline void keccak_f(uint64_t st[25]) {
    static const int ROT[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
    static const int PIL[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
    auto rotl64 = [](uint64_t x, int k) { return (x << k) | (x >> (64 - k)); };
    for (int round = 0; round < 24; round++) {
        uint64_t bc[5];
        for (int i = 0; i < 5; i++) bc[i] = st[i] ^ st[i + 5] ^ st[i + 10] ^ st[i + 15] ^ st[i + 20];
        for (int i = 0; i < 5; i++) {
            const uint64_t t = bc[(i + 4) % 5] ^ rotl64(bc[(i + 1) % 5], 1);
            for (int j = 0; j < 25; j += 5) st[j + i] ^= t;
        }
        uint64_t t = st[1];
        for (int i = 0; i < 24; i++) {
            const int j = PIL[i];
            const uint64_t keep = st[j];
            st[j] = rotl64(t, ROT[i]);
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
inline void keccak256(uint8_t out[32], const uint8_t *data, uint64_t len) {
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

// ---------------------------------------------------------------- the transcript
// the file's form of a coordinate -> its standard value, little-endian words
inline Fq fq_plain(const uint8_t c[32]) {
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

// a point of the curve in the file's form (or infinity), both coordinates below q
inline bool g1_well_formed(const uint8_t p[64]) {
    static const uint8_t zero[64] = {0};
    if (memcmp(p, zero, 64) == 0) return true;
    if (!below(p, FqParams::P) || !below(p + 32, FqParams::P)) return false;
    Fq x, y;
    memcpy(x.v, p, 32);
    memcpy(y.v, p + 32, 32);
    return Fq::sqr(y) == Fq::add(Fq::mul(Fq::sqr(x), x), curve_b<Fq>());
}

// What a lane of the device verifier needs of a checked key (plonk_verify_dev.hpp): the sponge after the 512 bytes every
// round-1 message of the key begins with, three blocks permuted and the 13 words of the fourth absorbed
inline PlonkVerifyConsts plonk_verify_consts(const zk_plonk_vkey &vk, const Fr &k1, const Fr &k2) {
    PlonkVerifyConsts K{};
    Transcript t;
    const uint8_t *vkp[8] = {vk.qm, vk.ql, vk.qr, vk.qo, vk.qc, vk.s1, vk.s2, vk.s3};
    for (uint32_t j = 0; j < 8; j++) t.point(vkp[j]);
    for (uint32_t i = 0; i < 64; i++) {
        uint64_t w = 0;
        for (int b = 7; b >= 0; b--) w = (w << 8) | t.buf[i * 8 + b];
        K.st[i % PV_RATE_WORDS] ^= w;
        if (i % PV_RATE_WORDS == PV_RATE_WORDS - 1) keccak_f(K.st);
    }
    static_assert(64 % PV_RATE_WORDS == PV_KEY_WORDS, "the key's 512 bytes end 13 words into a block");
    for (int i = 0; i < 24; i++) K.rc[i] = KECCAK_RC[i];
    K.n_public = vk.n_public;
    K.log_n = vk.log_n;
    K.k1 = k1, K.k2 = k2;
    K.w = root_of_unity(vk.log_n);
    K.n = fr_small(1ull << vk.log_n);
    K.b = curve_b<Fq>();
    return K;
}

inline void round1_challenges(Challenges &c, const zk_plonk_vkey &vk, const uint8_t *publics, const uint8_t *pts) {
    Transcript t;
    const uint8_t *vkp[8] = {vk.qm, vk.ql, vk.qr, vk.qo, vk.qc, vk.s1, vk.s2, vk.s3};
    for (uint32_t j = 0; j < 8; j++) t.point(vkp[j]);
    for (uint64_t i = 0; i < vk.n_public; i++) t.scalar_std(publics + i * 32);
    for (uint32_t j = P_A; j <= P_C; j++) t.point(pts + j * 64);
    c.beta = t.challenge();
    t.scalar(c.beta);
    c.gamma = t.challenge();
}
inline void round2_challenge(Challenges &c, const uint8_t *pts) {
    Transcript t;
    t.scalar(c.beta), t.scalar(c.gamma), t.point(pts + P_Z * 64);
    c.alpha = t.challenge();
}
inline void round3_challenge(Challenges &c, const uint8_t *pts) {
    Transcript t;
    t.scalar(c.alpha);
    for (uint32_t j = P_TLO; j <= P_THI; j++) t.point(pts + j * 64);
    c.zeta = t.challenge();
}
inline void round4_challenge(Challenges &c, const uint8_t *evals) {
    Transcript t;
    t.scalar(c.zeta);
    for (uint32_t j = 0; j < PLONK_EVALS; j++) t.scalar_std(evals + j * 32);
    c.v = t.challenge();
}
inline void round5_challenge(Challenges &c, const uint8_t *pts) {
    Transcript t;
    t.point(pts + P_WZ * 64), t.point(pts + P_WZW * 64);
    c.u = t.challenge();
}

// ---------------------------------------------------------------- what prover and verifier both make of zeta
struct AtZeta {
    Fr zn, zh, l1, pi;                                // zeta^n, Z_H(zeta), L1(zeta), PI(zeta): Montgomery
};
// zn, zh and l1 = Z_H(zeta) / (n (zeta - 1)): ONE inversion.  zeta^n = 1: L1(zeta) is 1 at zeta = 1 and 0 at every other
// root.  pi is left zero
inline AtZeta zeta_powers(uint32_t log_n, const Fr &ze) {
    AtZeta z;
    const Fr one = Fr::one();
    z.zn = ze;
    for (uint32_t i = 0; i < log_n; i++) z.zn = Fr::sqr(z.zn);
    z.zh = Fr::sub(z.zn, one);
    z.pi = Fr::zero();
    if (z.zh.is_zero()) z.l1 = ze == one ? one : Fr::zero();
    else z.l1 = Fr::mul(z.zh, Fr::inv(Fr::mul(fr_small(1ull << log_n), Fr::sub(ze, one))));
    return z;
}
// and PI(zeta) = - sum_(i < l) publics[i] L_i(zeta), L_i = w^i Z_H / (n (X - w^i)): l products and ONE more inversion (the
// prefix products of the denominators).  zeta^n = 1: L_i(zeta) is 1 where zeta = w^i and 0 elsewhere
inline AtZeta at_zeta(uint32_t log_n, const Fr &ze, const uint8_t *publics, uint64_t l) {
    AtZeta z = zeta_powers(log_n, ze);
    const Fr one = Fr::one(), w = root_of_unity(log_n), nn = fr_small(1ull << log_n);
    if (z.zh.is_zero()) {
        Fr wi = one;
        for (uint64_t i = 0; i < l; i++, wi = Fr::mul(wi, w))
            if (wi == ze) z.pi = Fr::neg(fr_from_std(publics + i * 32));
        return z;
    }
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

// The linearisation (plonkopen.hip's header states r and F): what multiplies each committed polynomial in F, from the six
// values ev[] = a b c s1 s2 z(zeta w) and the challenges, all Montgomery.  q_L, q_R, q_O take a, b, c themselves and q_C 1.
// The prover scales its rows by these, the verifier its commitments (and [z] by u more)
struct LinScalars {
    Fr qm, z, s3, tlo, tmid, thi;
    Fr v[5];                                          // v .. v^5: of a, b, c, s1, s2
    Fr E;                                             // v a + v^2 b + v^3 c + v^4 s1 + v^5 s2
    Fr c0;                                            // r's constant: PI(zeta) - alpha (..)(..)(c + gamma) z'w - alpha^2 L1(zeta)
};
inline LinScalars lin_scalars(const Fr ev[PLONK_EVALS], const AtZeta &z, const Fr &ze, const Fr &k1, const Fr &k2, const Fr &alpha, const Fr &beta,
                              const Fr &gamma, const Fr &v) {
    const Fr a = ev[0], b = ev[1], c = ev[2], s1 = ev[3], s2 = ev[4], zw = ev[5];
    const Fr bz = Fr::mul(beta, ze), al2l1 = Fr::mul(Fr::sqr(alpha), z.l1);
    const Fr f1 = Fr::add(Fr::add(a, bz), gamma), f2 = Fr::add(Fr::add(b, Fr::mul(bz, k1)), gamma), f3 = Fr::add(Fr::add(c, Fr::mul(bz, k2)), gamma);
    const Fr g12 = Fr::mul(Fr::add(Fr::add(a, Fr::mul(beta, s1)), gamma), Fr::add(Fr::add(b, Fr::mul(beta, s2)), gamma));
    const Fr g12zw_alpha = Fr::mul(Fr::mul(g12, zw), alpha);
    LinScalars k;
    k.qm = Fr::mul(a, b);
    k.z = Fr::add(Fr::mul(alpha, Fr::mul(Fr::mul(f1, f2), f3)), al2l1);
    k.s3 = Fr::neg(Fr::mul(g12zw_alpha, beta));
    k.tlo = Fr::neg(z.zh);
    k.tmid = Fr::neg(Fr::mul(z.zh, z.zn));
    k.thi = Fr::neg(Fr::mul(z.zh, Fr::sqr(z.zn)));
    Fr vp = v;
    k.E = Fr::zero();
    for (int j = 0; j < 5; j++) {
        k.v[j] = vp;
        k.E = Fr::add(k.E, Fr::mul(vp, ev[j]));
        vp = Fr::mul(vp, v);
    }
    k.c0 = Fr::sub(Fr::sub(z.pi, Fr::mul(g12zw_alpha, Fr::add(c, gamma))), al2l1);
    return k;
}

}   // namespace zkp
