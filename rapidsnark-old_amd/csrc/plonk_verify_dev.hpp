// What one proof costs a PLONK verifier before any point is touched, as ONE __host__ __device__ function: the checks of
// the proof's bytes, the six challenges of the transcript (include/zkhip.h, section "PLONK prover and verifier"), what
// the verifier makes of zeta, and the nineteen scalars of the combination.  k_plonk_transcript (plonkverify_dev.hip) runs
// it with a lane per proof; tools/plonk_verifier_host_test.cpp runs the same text on the host against
// plonk_transcript.hpp's, which stays what prover and zk_plonk_verify use.
//
// Nothing here indexes a register array at run time.  The 25 lanes of the Keccak state are addressed by constants only:
// a word is absorbed at the sponge's position by 17 selects, and what is absorbed is read from MEMORY, 32 bytes an item,
// by one loop over all six hashes of a proof (the challenges a later hash absorbs are read back from the row the lane has
// written), so that the permutation is inlined at two places and not at forty.  Its 24 rounds are a loop; the round
// constants come with the key's record.  A 256-bit value is absorbed big-endian by taking its top two words and moving
// the other six up, the way mulglv.hpp walks its digits.
#pragma once
#include "field.hpp"

namespace zk {

constexpr uint32_t PV_POINTS = 9, PV_EVALS = 6, PV_CHALLENGES = 6, PV_PROOF_BYTES = 768, PV_KEY_POINTS = 8;
// the terms of the combination, in the order of their bases: the key's eight commitments in the transcript's order, the
// generator, the proof's nine points, and W_zeta_omega once more (by u, for the right-hand side of the pairing equation)
enum {
    PV_QM, PV_QL, PV_QR, PV_QO, PV_QC, PV_S1, PV_S2, PV_S3, PV_G, PV_A, PV_B, PV_C, PV_Z, PV_TLO, PV_TMID, PV_THI, PV_WZ, PV_WZW, PV_WZW_U, PV_TERMS
};
constexpr uint32_t PV_FIXED = PV_G + 1;               // the bases that are the same for every proof
constexpr uint32_t PV_OK = 0, PV_MALFORMED = 1;
constexpr uint32_t PV_RATE_WORDS = 17;                // 136 bytes

// What a lane needs of the key, made once (zk_plonk_verifier_create): Montgomery form
struct PlonkVerifyConsts {
    uint64_t st[25];              // the sponge after the key's eight commitments: three blocks permuted, 13 words of the fourth absorbed
    uint64_t rc[24];              // Keccak's round constants
    uint64_t n_public;
    uint32_t log_n, reserved;
    Fr k1, k2, w, n;              // w: zk_fr_ntt's root for n = 2^log_n
    Fq b;                         // 3
};
constexpr uint32_t PV_KEY_WORDS = 13;                 // 512 bytes = 3 * 136 + 13 * 8

#if defined(__HIP_DEVICE_COMPILE__)
#define PV_NI __host__ __device__ __noinline__
#else
#define PV_NI
#endif
// one copy of the product in a kernel: by value, so that the operands travel in registers
PV_NI inline Fr pv_mul(Fr a, Fr b) { return Fr::mul(a, b); }
ZK_HD Fr pv_sqr(const Fr &a) { return pv_mul(a, a); }

// ---------------------------------------------------------------- 32 bytes between memory and eight words
ZK_HD void pv_load(uint32_t w[8], const uint8_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 *q = reinterpret_cast<const uint4 *>(p);          // 16-byte aligned: rows of 32 bytes in hipMalloc'ed buffers
    const uint4 lo = q[0], hi = q[1];
    w[0] = lo.x, w[1] = lo.y, w[2] = lo.z, w[3] = lo.w, w[4] = hi.x, w[5] = hi.y, w[6] = hi.z, w[7] = hi.w;
#else
    for (int i = 0; i < 8; i++) w[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
#endif
}
ZK_HD void pv_store(uint8_t *p, const uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint4 *q = reinterpret_cast<uint4 *>(p);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
#else
    for (int i = 0; i < 32; i++) p[i] = (uint8_t)(w[i / 4] >> (8 * (i % 4)));
#endif
}
template <class F>
ZK_HD F pv_load_el(const uint8_t *p) {
    F x;
    pv_load(x.v, p);
    return x;
}
template <class PR>
ZK_HD bool pv_below(const uint32_t w[8]) {
    uint32_t bw = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) (void)subb(w[i], PR::P[i], bw);
    return bw != 0;
}

// ---------------------------------------------------------------- Keccak-f[1600], the state in 25 named places
struct PvKeccak {
    static constexpr int RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
};
ZK_HD uint64_t pv_rotl(uint64_t x, int k) { return k ? (x << k) | (x >> (64 - k)) : x; }
ZK_HD void pv_keccak_f(uint64_t a[25], const uint64_t *rc) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int round = 0; round < 24; round++) {
        uint64_t c[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; x++) {
            const uint64_t d = c[(x + 4) % 5] ^ pv_rotl(c[(x + 1) % 5], 1);
#pragma unroll
            for (int y = 0; y < 25; y += 5) a[y + x] ^= d;
        }
#pragma unroll
        for (int y = 0; y < 5; y++) {
#pragma unroll
            for (int x = 0; x < 5; x++) b[y + 5 * ((2 * x + 3 * y) % 5)] = pv_rotl(a[x + 5 * y], PvKeccak::RHO[x + 5 * y]);
        }
#pragma unroll
        for (int y = 0; y < 25; y += 5) {
#pragma unroll
            for (int x = 0; x < 5; x++) a[y + x] = b[y + x] ^ (~b[y + (x + 1) % 5] & b[y + (x + 2) % 5]);
        }
        a[0] ^= rc[round];
    }
}
// word `pos` of the rate ^= w
ZK_HD void pv_xor_at(uint64_t a[25], uint32_t pos, uint64_t w) {
#pragma unroll
    for (uint32_t i = 0; i < PV_RATE_WORDS; i++) a[i] ^= pos == i ? w : 0;
}

// the digest's 32 bytes read as a big-endian integer (eight words, the lowest first) mod r: 2^256 < 6 r, five subtractions
// at the most.  Montgomery form is the caller's to make
ZK_HD Fr pv_digest_mod_r(const uint32_t v[8]) {
    Fr x;
#pragma unroll
    for (int i = 0; i < 8; i++) x.v[i] = v[i];
#pragma unroll
    for (int k = 0; k < 5; k++) x = Fr::reduce_once(x);
    return x;
}

// ---------------------------------------------------------------- the six challenges
// ch: the proof's row of 6 x 32 bytes, beta gamma alpha zeta v u, standard form little-endian; written one by one, read
// back by the later hashes.  false: a public input is not below r (the row is then incomplete)
ZK_HD bool pv_challenges(const PlonkVerifyConsts &K, const uint8_t *proof, const uint8_t *publics, uint8_t *ch) {
    const uint8_t *evals = proof + PV_POINTS * 64;
    bool ok = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint32_t h = 0; h < PV_CHALLENGES && ok; h++) {
        // what hash h absorbs: n1 scalars at p1, n2 scalars at p2 (standard form), then n3 coordinates at p3 (Montgomery)
        const uint8_t *p1 = ch, *p2 = publics, *p3 = proof;
        uint64_t n1 = 0, n2 = 0, n3 = 0;
        if (h == 0) n2 = K.n_public, n3 = 6;                                   // publics, [a] [b] [c] (after the key)
        else if (h == 1) n1 = 1;                                               // beta
        else if (h == 2) n1 = 2, p3 = proof + 3 * 64, n3 = 2;                  // beta, gamma, [z]
        else if (h == 3) p1 = ch + 2 * 32, n1 = 1, p3 = proof + 4 * 64, n3 = 6;   // alpha, [t_lo] [t_mid] [t_hi]
        else if (h == 4) p1 = ch + 3 * 32, n1 = 1, p2 = evals, n2 = PV_EVALS;  // zeta, the six values
        else p3 = proof + 7 * 64, n3 = 4;                                      // [W_zeta] [W_zeta_omega]
        uint64_t a[25];
        uint32_t pos = h == 0 ? PV_KEY_WORDS : 0;
#pragma unroll
        for (int i = 0; i < 25; i++) a[i] = h == 0 ? K.st[i] : 0;
        const uint64_t items = n1 + n2 + n3;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (uint64_t t = 0; t < items; t++) {
            const bool coord = t >= n1 + n2;
            const uint8_t *src = t < n1 ? p1 + t * 32 : !coord ? p2 + (t - n1) * 32 : p3 + (t - n1 - n2) * 32;
            uint32_t w[8];
            pv_load(w, src);
            if (coord) {
                Fq x;
#pragma unroll
                for (int i = 0; i < 8; i++) x.v[i] = w[i];
                x = Fq::from_mont(x);
#pragma unroll
                for (int i = 0; i < 8; i++) w[i] = x.v[i];
            } else {
                ok = ok && pv_below<FrParams>(w);
            }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
            for (int j = 0; j < 4; j++) {                                      // big-endian: the top two words first
                pv_xor_at(a, pos, (uint64_t)__builtin_bswap32(w[7]) | (uint64_t)__builtin_bswap32(w[6]) << 32);
#pragma unroll
                for (int i = 7; i >= 2; i--) w[i] = w[i - 2];
                if (++pos == PV_RATE_WORDS) {
                    pv_keccak_f(a, K.rc);
                    pos = 0;
                }
            }
        }
        pv_xor_at(a, pos, 0x01);                                               // the original padding: 0x01 .. 0x80
        a[PV_RATE_WORDS - 1] ^= 0x8000000000000000ull;
        pv_keccak_f(a, K.rc);
        uint32_t v[8];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            v[7 - 2 * j] = __builtin_bswap32((uint32_t)a[j]);
            v[6 - 2 * j] = __builtin_bswap32((uint32_t)(a[j] >> 32));
        }
        const Fr c = pv_digest_mod_r(v);
        pv_store(ch + h * 32, c.v);
    }
    return ok;
}

// ---------------------------------------------------------------- what the verifier makes of zeta
struct PvAtZeta {
    Fr zn, zh, l1, pi;                                // zeta^n, Z_H(zeta), L1(zeta), PI(zeta): Montgomery
};
// plonk_transcript.hpp's at_zeta without a row per public input: sum_i p_i w^i / (zeta - w^i) is carried as N / D (N in
// standard form, since the p_i are: a Montgomery product of a standard and a Montgomery value is standard), and ONE
// inversion, of n (zeta - 1) n D, serves L1 and PI.  zeta^n = 1: L1 is 1 at zeta = 1 and 0 at every other root, and PI
// is -publics[i] where zeta = w^i
ZK_HD PvAtZeta pv_at_zeta(const PlonkVerifyConsts &K, const Fr &ze, const uint8_t *publics) {
    PvAtZeta z;
    const Fr one = Fr::one();
    z.zn = ze;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint32_t i = 0; i < K.log_n; i++) z.zn = pv_sqr(z.zn);
    z.zh = Fr::sub(z.zn, one);
    z.pi = Fr::zero();
    Fr wi = one;
    if (z.zh.is_zero()) {
        z.l1 = ze == one ? one : Fr::zero();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (uint64_t i = 0; i < K.n_public; i++) {
            if (wi == ze) z.pi = Fr::neg(Fr::to_mont(pv_load_el<Fr>(publics + i * 32)));
            wi = pv_mul(wi, K.w);
        }
        return z;
    }
    Fr N = Fr::zero(), D = one;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint64_t i = 0; i < K.n_public; i++) {
        const Fr d = Fr::sub(ze, wi);
        const Fr p = pv_load_el<Fr>(publics + i * 32);
        N = Fr::add(pv_mul(N, d), pv_mul(pv_mul(p, wi), D));
        D = pv_mul(D, d);
        wi = pv_mul(wi, K.w);
    }
    const Fr X = pv_mul(K.n, Fr::sub(ze, one)), Y = pv_mul(K.n, D);
    Fr inv = one, base = pv_mul(X, Y);                // (X Y)^(r - 2)
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = FrParams::P[i];
    e[0] -= 2;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 0; i < 256; i++) {
        if (e[0] & 1u) inv = pv_mul(inv, base);
        base = pv_sqr(base);
#pragma unroll
        for (int q = 0; q < 7; q++) e[q] = (e[q] >> 1) | (e[q + 1] << 31);
        e[7] >>= 1;
    }
    z.l1 = pv_mul(z.zh, pv_mul(inv, Y));              // Z_H / X
    z.pi = Fr::neg(pv_mul(pv_mul(z.zh, Fr::to_mont(N)), pv_mul(inv, X)));   // - Z_H N / Y
    return z;
}

// ---------------------------------------------------------------- one proof
// proof: 768 bytes; publics: K.n_public x 32 bytes (never read when that is 0); ch: the proof's row of six challenges;
// sc: PV_TERMS scalars `stride` apart, standard form (NULL: the challenges alone).  PV_MALFORMED: a point that is not on
// the curve or has a coordinate not below q, one of the six values or a public input not below r; ch is then all zero
// and sc is not written.  override_ch (tests only): six challenges, standard form, taken in place of the transcript's
ZK_HD uint32_t plonk_verify_lane(const PlonkVerifyConsts &K, const uint8_t *proof, const uint8_t *publics, uint8_t *ch, Fr *sc, uint64_t stride,
                                 const uint8_t *override_ch) {
    const uint8_t *evals = proof + PV_POINTS * 64;
    bool ok = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint32_t j = 0; j < PV_POINTS; j++) {
        const Fq x = pv_load_el<Fq>(proof + j * 64), y = pv_load_el<Fq>(proof + j * 64 + 32);
        const bool inf = x.is_zero() && y.is_zero();
        const bool on = pv_below<FqParams>(x.v) && pv_below<FqParams>(y.v) && Fq::sqr(y) == Fq::add(Fq::mul(Fq::sqr(x), x), K.b);
        ok = ok && (inf || on);
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint32_t j = 0; j < PV_EVALS; j++) {
        uint32_t w[8];
        pv_load(w, evals + j * 32);
        ok = ok && pv_below<FrParams>(w);
    }
    ok = ok && pv_challenges(K, proof, publics, ch);
    if (!ok) {
        const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (uint32_t h = 0; h < PV_CHALLENGES; h++) pv_store(ch + h * 32, zero);
        return PV_MALFORMED;
    }
    if (!sc) return PV_OK;
    const uint8_t *cs = override_ch ? override_ch : ch;
    const Fr beta = Fr::to_mont(pv_load_el<Fr>(cs)), gamma = Fr::to_mont(pv_load_el<Fr>(cs + 32)), alpha = Fr::to_mont(pv_load_el<Fr>(cs + 64)),
             ze = Fr::to_mont(pv_load_el<Fr>(cs + 96)), v = Fr::to_mont(pv_load_el<Fr>(cs + 128)), u = Fr::to_mont(pv_load_el<Fr>(cs + 160));
    const PvAtZeta z = pv_at_zeta(K, ze, publics);
    auto put = [&](uint32_t t, const Fr &x) { pv_store(reinterpret_cast<uint8_t *>(sc + t * stride), Fr::from_mont(x).v); };
    auto put_std = [&](uint32_t t, const Fr &x) { pv_store(reinterpret_cast<uint8_t *>(sc + t * stride), x.v); };
    // plonk_transcript.hpp's lin_scalars, folded: [z] takes k.z + u, W_zeta_omega u zeta w, [1] -(E - c0 + u z'w)
    const Fr a = Fr::to_mont(pv_load_el<Fr>(evals)), b = Fr::to_mont(pv_load_el<Fr>(evals + 32)), c = Fr::to_mont(pv_load_el<Fr>(evals + 64)),
             s1 = Fr::to_mont(pv_load_el<Fr>(evals + 96)), s2 = Fr::to_mont(pv_load_el<Fr>(evals + 128)), zw = Fr::to_mont(pv_load_el<Fr>(evals + 160));
    const Fr bz = pv_mul(beta, ze), al2l1 = pv_mul(pv_sqr(alpha), z.l1);
    const Fr f1 = Fr::add(Fr::add(a, bz), gamma), f2 = Fr::add(Fr::add(b, pv_mul(bz, K.k1)), gamma), f3 = Fr::add(Fr::add(c, pv_mul(bz, K.k2)), gamma);
    const Fr g12 = pv_mul(Fr::add(Fr::add(a, pv_mul(beta, s1)), gamma), Fr::add(Fr::add(b, pv_mul(beta, s2)), gamma));
    const Fr g12zw_alpha = pv_mul(pv_mul(g12, zw), alpha);
    put(PV_QM, pv_mul(a, b));
    put_std(PV_QL, pv_load_el<Fr>(evals));
    put_std(PV_QR, pv_load_el<Fr>(evals + 32));
    put_std(PV_QO, pv_load_el<Fr>(evals + 64));
    put(PV_QC, Fr::one());
    put(PV_Z, Fr::add(Fr::add(pv_mul(alpha, pv_mul(pv_mul(f1, f2), f3)), al2l1), u));
    put(PV_S3, Fr::neg(pv_mul(g12zw_alpha, beta)));
    const Fr tmid = pv_mul(z.zh, z.zn);
    put(PV_TLO, Fr::neg(z.zh));
    put(PV_TMID, Fr::neg(tmid));
    put(PV_THI, Fr::neg(pv_mul(tmid, z.zn)));
    const Fr v2 = pv_sqr(v), v3 = pv_mul(v2, v), v4 = pv_sqr(v2), v5 = pv_mul(v4, v);
    put(PV_A, v);
    put(PV_B, v2);
    put(PV_C, v3);
    put(PV_S1, v4);
    put(PV_S2, v5);
    const Fr E = Fr::add(Fr::add(Fr::add(pv_mul(v, a), pv_mul(v2, b)), Fr::add(pv_mul(v3, c), pv_mul(v4, s1))), pv_mul(v5, s2));
    const Fr c0 = Fr::sub(Fr::sub(z.pi, pv_mul(g12zw_alpha, Fr::add(c, gamma))), al2l1);
    put(PV_G, Fr::neg(Fr::add(Fr::sub(E, c0), pv_mul(u, zw))));
    put(PV_WZ, ze);
    put(PV_WZW, pv_mul(u, pv_mul(ze, K.w)));
    put(PV_WZW_U, u);
    return PV_OK;
}

}   // namespace zk
