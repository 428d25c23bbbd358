// Host check of csrc/plonk_batch_dev.hpp, the per-proof text k_plonk_batch_scale runs with a lane per proof slot: its twenty
// products r s_t against products made independently, from csrc/plonk_transcript.hpp's lin_scalars (what prover and
// zk_plonk_verify use) and a Montgomery product on the host.  Random well-formed inputs with r random, r = 1 and
// r = 2^128 - 1; scalars 0 and r - 1 fed straight to the function; a slot that takes no part (zeros everywhere, whatever
// lies in its rows).  Then the arithmetic that cuts a call into chunks and groups, over (m, chunk, group) triples, the GPU
// tests' among them.  No device is touched.  Built as HIP for the headers' sake, the host side only:
//   hipcc --offload-host-only -std=c++17 -O1 -g -x hip tools/plonk_batch_host_test.cpp -fsanitize=address,undefined -o t && ./t
#include <stdio.h>

#include "../rapidsnark-old_amd/csrc/plonk_transcript.hpp"
#include "../rapidsnark-old_amd/csrc/plonk_batch_dev.hpp"

static int failures = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) failures++, printf("FAILED line %d: %s\n", __LINE__, #c);   \
    } while (0)

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}
// a value below the modulus p: 253 random bits
static void rnd_below(uint8_t out[32]) {
    for (int i = 0; i < 4; i++) {
        const uint64_t w = rnd();
        memcpy(out + 8 * i, &w, 8);
    }
    out[31] &= 0x1f;
}
static Fq fq_pow(Fq base, const uint32_t e[8]) {
    Fq acc = Fq::one();
    for (int i = 0; i < 256; i++) {
        if ((e[i >> 5] >> (i & 31)) & 1u) acc = Fq::mul(acc, base);
        base = Fq::sqr(base);
    }
    return acc;
}
// a random point of the curve in the file's form: x drawn until x^3 + 3 is a square, y its root (q = 3 mod 4)
static void rnd_point(uint8_t out[64]) {
    uint32_t e[8];                                    // (q + 1) / 4
    uint64_t carry = 1;
    for (int i = 0; i < 8; i++) {
        const uint64_t t = (uint64_t)FqParams::P[i] + carry;
        e[i] = (uint32_t)t;
        carry = t >> 32;
    }
    for (int i = 0; i < 7; i++) e[i] = (e[i] >> 2) | (e[i + 1] << 30);
    e[7] >>= 2;
    for (;;) {
        uint8_t xb[32];
        rnd_below(xb);
        Fq x;
        memcpy(x.v, xb, 32);
        const Fq rhs = Fq::add(Fq::mul(Fq::sqr(x), x), curve_b<Fq>());
        const Fq y = fq_pow(rhs, e);
        if (!(Fq::sqr(y) == rhs)) continue;
        memcpy(out, x.v, 32);
        memcpy(out + 32, y.v, 32);
        return;
    }
}

struct Input {
    zk_plonk_vkey vk;
    uint8_t proof[ZK_PLONK_PROOF_BYTES];
    std::vector<uint8_t> publics;
};
static Input make_input(uint32_t log_n, uint64_t n_public) {
    Input in;
    memset(&in.vk, 0, sizeof in.vk);
    in.vk.size = sizeof in.vk;
    in.vk.log_n = log_n;
    in.vk.n_public = n_public;
    in.vk.k1[0] = 2, in.vk.k2[0] = 3;
    uint8_t *vkp[8] = {in.vk.qm, in.vk.ql, in.vk.qr, in.vk.qo, in.vk.qc, in.vk.s1, in.vk.s2, in.vk.s3};
    for (int j = 0; j < 8; j++) rnd_point(vkp[j]);
    for (uint32_t j = 0; j < PLONK_POINTS; j++) rnd_point(in.proof + j * 64);
    for (uint32_t j = 0; j < PLONK_EVALS; j++) rnd_below(in.proof + PLONK_POINTS * 64 + j * 32);
    in.publics.resize(n_public * 32 + 32);            // a row of room: never read
    for (uint64_t i = 0; i < n_public; i++) rnd_below(in.publics.data() + i * 32);
    return in;
}

// r (16 bytes) times a Montgomery value, standard form: the product made without plonk_batch_dev.hpp
static Fr times_r(const uint8_t r16[16], const Fr &s_mont) {
    uint8_t r32[32] = {0};
    memcpy(r32, r16, 16);
    return Fr::from_mont(Fr::mul(fr_from_std(r32), s_mont));
}

struct Products {
    Fr fx[PV_FIXED], lsc[PB_L_TERMS], wsc[PB_W_TERMS];
};
static Products run_lane(const Fr *sc, uint64_t stride, const uint8_t r16[16], bool ok) {
    Products p;
    memset(&p, 0xAA, sizeof p);
    plonk_batch_scale_lane(p.fx, 1, p.lsc, p.wsc, sc, stride, r16, ok);
    return p;
}

// the lane's twenty products for a well-formed input against lin_scalars' by r
static void compare(const Input &in, const uint8_t r16[16]) {
    const Fr k1 = fr_from_std(in.vk.k1), k2 = fr_from_std(in.vk.k2);
    const PlonkVerifyConsts K = plonk_verify_consts(in.vk, k1, k2);
    const uint8_t *pts = in.proof, *evals = in.proof + PLONK_POINTS * 64;
    uint8_t row[PV_CHALLENGES * 32];
    const uint64_t stride = 3;                        // the rows lie `stride` apart, as on the device
    std::vector<Fr> sc(PV_TERMS * stride);
    memset(sc.data(), 0x55, sc.size() * sizeof(Fr));
    CHECK(plonk_verify_lane(K, in.proof, in.publics.data(), row, sc.data(), stride, nullptr) == PV_OK);
    const Products p = run_lane(sc.data(), stride, r16, true);

    Challenges ch;
    round1_challenges(ch, in.vk, in.publics.data(), pts);
    round2_challenge(ch, pts);
    round3_challenge(ch, pts);
    round4_challenge(ch, evals);
    round5_challenge(ch, pts);
    Fr ev[PLONK_EVALS];
    for (uint32_t j = 0; j < PLONK_EVALS; j++) ev[j] = fr_from_std(evals + j * 32);
    const LinScalars k = lin_scalars(ev, at_zeta(in.vk.log_n, ch.zeta, in.publics.data(), in.vk.n_public), ch.zeta, k1, k2, ch.alpha, ch.beta, ch.gamma, ch.v);
    Fr want[PV_TERMS];
    want[PV_QM] = k.qm, want[PV_QL] = ev[0], want[PV_QR] = ev[1], want[PV_QO] = ev[2], want[PV_QC] = Fr::one();
    want[PV_S1] = k.v[3], want[PV_S2] = k.v[4], want[PV_S3] = k.s3;
    want[PV_G] = Fr::neg(Fr::add(Fr::sub(k.E, k.c0), Fr::mul(ch.u, ev[5])));
    want[PV_A] = k.v[0], want[PV_B] = k.v[1], want[PV_C] = k.v[2], want[PV_Z] = Fr::add(k.z, ch.u);
    want[PV_TLO] = k.tlo, want[PV_TMID] = k.tmid, want[PV_THI] = k.thi;
    want[PV_WZ] = ch.zeta, want[PV_WZW] = Fr::mul(ch.u, Fr::mul(ch.zeta, root_of_unity(in.vk.log_n))), want[PV_WZW_U] = ch.u;
    for (uint32_t t = 0; t < PV_FIXED; t++) CHECK(p.fx[t] == times_r(r16, want[t]));
    for (uint32_t j = 0; j < PB_L_TERMS; j++) CHECK(p.lsc[j] == times_r(r16, want[PV_FIXED + j]));
    CHECK(p.wsc[0] == times_r(r16, Fr::one()) && p.wsc[1] == times_r(r16, want[PV_WZW_U]));
    uint8_t r32[32] = {0};
    memcpy(r32, r16, 16);
    CHECK(memcmp(p.wsc[0].v, r32, 32) == 0);          // r itself, the low half
}

// every row the same standard-form scalar s: every product is r s mod r_modulus
static void uniform_rows(const uint8_t s32[32], const uint8_t r16[16]) {
    Fr sc[PV_TERMS];
    for (uint32_t t = 0; t < PV_TERMS; t++) memcpy(sc[t].v, s32, 32);
    const Products p = run_lane(sc, 1, r16, true);
    const Fr want = times_r(r16, fr_from_std(s32));
    for (uint32_t t = 0; t < PV_FIXED; t++) CHECK(p.fx[t] == want);
    for (uint32_t j = 0; j < PB_L_TERMS; j++) CHECK(p.lsc[j] == want);
    CHECK(p.wsc[1] == want);
}

struct Triple {
    uint64_t m, chunk, group, groups;
};

int main() {
    uint8_t one[16] = {1}, top[16], r16[16];
    memset(top, 0xff, 16);
    for (uint32_t log_n : {3u, 4u, 11u})
        for (uint64_t l : {0ull, 2ull, 16ull}) {
            if (l > (1ull << log_n)) continue;
            const Input in = make_input(log_n, l);
            for (int rep = 0; rep < 3; rep++) {
                const uint64_t a = rnd(), b = rnd();
                memcpy(r16, &a, 8), memcpy(r16 + 8, &b, 8);
                compare(in, r16);
            }
            compare(in, one);
            compare(in, top);
        }
    {   // scalars 0 and r - 1 in every row
        uint8_t zero[32] = {0}, last[32];
        uint32_t w[8];
        memcpy(w, FrParams::P, 32);
        w[0] -= 1;
        memcpy(last, w, 32);
        for (const uint8_t *r : {(const uint8_t *)one, (const uint8_t *)top}) {
            uniform_rows(zero, r);
            uniform_rows(last, r);
        }
        Fr sc[PV_TERMS];
        memset(sc, 0, sizeof sc);
        const Products p = run_lane(sc, 1, top, true);
        for (uint32_t t = 0; t < PV_FIXED; t++) CHECK(p.fx[t].is_zero());
    }
    {   // a slot that takes no part: zeros everywhere, and its rows (here: bytes that are no scalars) are not read
        Fr sc[PV_TERMS];
        memset(sc, 0xFF, sizeof sc);
        const Products p = run_lane(sc, 1, top, false);
        for (uint32_t t = 0; t < PV_FIXED; t++) CHECK(p.fx[t].is_zero());
        for (uint32_t j = 0; j < PB_L_TERMS; j++) CHECK(p.lsc[j].is_zero());
        CHECK(p.wsc[0].is_zero() && p.wsc[1].is_zero());
        const Products q = run_lane(nullptr, 0, top, false);
        CHECK(q.wsc[0].is_zero() && q.fx[0].is_zero());
    }
    // chunks and groups: the GPU tests' triples first
    static const Triple triples[] = {
        {130, 65536, 1, 130}, {130, 65536, 3, 44}, {130, 100, 64, 3}, {130, 64, 64, 3}, {130, 7, 1000, 19}, {130, 65536, 64, 3}, {5, 65536, 2, 3},
        {6, 65536, 2, 3},     {2, 65536, 16384, 1}, {1, 65536, 16384, 1}, {257, 65536, 16384, 1}, {65536, 65536, 1024, 64}, {65537, 65536, 65536, 2},
        {1048576, 1048576, 1048576, 1}, {1048577, 1048576, 1048576, 2}, {0, 65536, 64, 0}, {200, 1, 1, 200}, {200, 3, 2, 133}};
    for (const Triple &t : triples) {
        CHECK(pb_groups_of_call(t.m, t.chunk, t.group) == t.groups);
        if (!t.m) continue;
        // every proof lies in exactly one group, no group straddles a chunk, none is longer than the group
        const uint64_t cap = pb_cap(t.m, t.chunk), g = pb_group(cap, t.group);
        CHECK(g >= 1 && g <= t.group && g <= cap);
        uint64_t covered = 0;
        for (uint64_t off = 0; off < t.m; off += cap) {
            const uint64_t cnt = t.m - off < cap ? t.m - off : cap, ng = pb_groups_in(cnt, g);
            CHECK(ng * g >= cnt && (ng - 1) * g < cnt);
            covered += cnt;
        }
        CHECK(covered == t.m);
        CHECK(pb_l_stride(g) == 9 * g + 9 && pb_w_stride(g) == 2 * g);
    }
    printf(failures ? "%d checks FAILED\n" : "plonk_batch host checks OK\n", failures);
    return failures ? 1 : 0;
}
