// Host check of csrc/plonk_verify_dev.hpp, the per-proof text k_plonk_transcript runs with a lane per proof: its six
// challenges and its nineteen scalars against csrc/plonk_transcript.hpp's (round*_challenge, at_zeta, lin_scalars), which
// prover and zk_plonk_verify use.  Random well-formed inputs at n_public 0, 1, 2, 12 and 16 (12: the round-1 message is
// 8 x 136 bytes and the last absorbed block is padding only); the two cases no hash reaches, zeta = 1 and zeta = w^3 with
// four and more publics, by the override argument; digests in each band [k r, (k + 1) r), k = 0 .. 5, fed straight to the
// reduction; and the malformed kinds.  No device is touched.  Built as HIP for the headers' sake, the host side only:
//   hipcc --offload-host-only -std=c++17 -O1 -g -x hip tools/plonk_verifier_host_test.cpp -fsanitize=address,undefined -o t && ./t
#include <stdio.h>

#include "../rapidsnark-old_amd/csrc/plonk_transcript.hpp"

static int failures = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) failures++, printf("FAILED line %d: %s\n", __LINE__, #c);   \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
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

static bool same_std(const Fr *got_std, const Fr &want_mont) { return *got_std == Fr::from_mont(want_mont); }

// the lane against the transcript's; over: six challenges (Montgomery) in place of the hash's, or NULL
static void compare(const Input &in, const Challenges *over) {
    const Fr k1 = fr_from_std(in.vk.k1), k2 = fr_from_std(in.vk.k2);
    const PlonkVerifyConsts K = plonk_verify_consts(in.vk, k1, k2);
    const uint8_t *pts = in.proof, *evals = in.proof + PLONK_POINTS * 64;
    Challenges ch;
    round1_challenges(ch, in.vk, in.publics.data(), pts);
    round2_challenge(ch, pts);
    round3_challenge(ch, pts);
    round4_challenge(ch, evals);
    round5_challenge(ch, pts);
    uint8_t row[PV_CHALLENGES * 32], ov[PV_CHALLENGES * 32];
    Fr sc[PV_TERMS];
    memset(row, 0xAA, sizeof row);
    if (over) {
        const Fr *o[6] = {&over->beta, &over->gamma, &over->alpha, &over->zeta, &over->v, &over->u};
        for (int j = 0; j < 6; j++) fr_to_std(ov + j * 32, *o[j]);
    }
    CHECK(plonk_verify_lane(K, in.proof, in.publics.data(), row, sc, 1, over ? ov : nullptr) == PV_OK);
    const Fr *c[6] = {&ch.beta, &ch.gamma, &ch.alpha, &ch.zeta, &ch.v, &ch.u};
    for (int j = 0; j < 6; j++) {
        uint8_t want[32];
        fr_to_std(want, *c[j]);
        CHECK(memcmp(row + j * 32, want, 32) == 0);
    }
    // the challenges alone: the same row, no scalar written
    uint8_t row2[PV_CHALLENGES * 32];
    CHECK(plonk_verify_lane(K, in.proof, in.publics.data(), row2, nullptr, 0, nullptr) == PV_OK && memcmp(row, row2, sizeof row) == 0);
    if (over) ch = *over;
    Fr ev[PLONK_EVALS];
    for (uint32_t j = 0; j < PLONK_EVALS; j++) ev[j] = fr_from_std(evals + j * 32);
    const AtZeta z = at_zeta(in.vk.log_n, ch.zeta, in.publics.data(), in.vk.n_public);
    const PvAtZeta pz = pv_at_zeta(K, ch.zeta, in.publics.data());
    CHECK(pz.zn == z.zn && pz.zh == z.zh && pz.l1 == z.l1 && pz.pi == z.pi);
    const LinScalars k = lin_scalars(ev, z, ch.zeta, k1, k2, ch.alpha, ch.beta, ch.gamma, ch.v);
    CHECK(same_std(sc + PV_QM, k.qm) && same_std(sc + PV_QL, ev[0]) && same_std(sc + PV_QR, ev[1]) && same_std(sc + PV_QO, ev[2]));
    CHECK(same_std(sc + PV_QC, Fr::one()) && same_std(sc + PV_S3, k.s3));
    CHECK(same_std(sc + PV_Z, Fr::add(k.z, ch.u)));
    CHECK(same_std(sc + PV_TLO, k.tlo) && same_std(sc + PV_TMID, k.tmid) && same_std(sc + PV_THI, k.thi));
    CHECK(same_std(sc + PV_A, k.v[0]) && same_std(sc + PV_B, k.v[1]) && same_std(sc + PV_C, k.v[2]) && same_std(sc + PV_S1, k.v[3]) && same_std(sc + PV_S2, k.v[4]));
    CHECK(same_std(sc + PV_G, Fr::neg(Fr::add(Fr::sub(k.E, k.c0), Fr::mul(ch.u, ev[5])))));
    CHECK(same_std(sc + PV_WZ, ch.zeta) && same_std(sc + PV_WZW_U, ch.u));
    CHECK(same_std(sc + PV_WZW, Fr::mul(ch.u, Fr::mul(ch.zeta, root_of_unity(in.vk.log_n)))));
}

static void malformed(Input in, uint32_t at, const uint32_t modulus[8], bool in_publics) {
    const PlonkVerifyConsts K = plonk_verify_consts(in.vk, fr_from_std(in.vk.k1), fr_from_std(in.vk.k2));
    uint8_t *where = in_publics ? in.publics.data() + at : in.proof + at;
    if (modulus) memcpy(where, modulus, 32);
    else where[0] ^= 1;                               // a coordinate changed: off the curve
    uint8_t row[PV_CHALLENGES * 32], zero[PV_CHALLENGES * 32] = {0};
    Fr sc[PV_TERMS];
    memset(row, 0xAA, sizeof row);
    CHECK(plonk_verify_lane(K, in.proof, in.publics.data(), row, sc, 1, nullptr) == PV_MALFORMED);
    CHECK(memcmp(row, zero, sizeof row) == 0);
}

// k r + d as eight words
static void band_value(uint32_t out[8], uint32_t k, const uint32_t d[8]) {
    uint64_t carry = 0;
    for (int i = 0; i < 8; i++) {
        const uint64_t t = (uint64_t)FrParams::P[i] * k + d[i] + carry;
        out[i] = (uint32_t)t;
        carry = t >> 32;
    }
    CHECK(carry == 0);
}

int main() {
    static const uint64_t counts[5] = {0, 1, 2, 12, 16};
    for (uint32_t log_n : {3u, 4u, 11u})
        for (uint64_t l : counts) {
            if (l > (1ull << log_n)) continue;
            for (int rep = 0; rep < 3; rep++) compare(make_input(log_n, l), nullptr);
        }
    {   // infinity among the proof's points and in the key; publics 0 and r - 1; values 0 and r - 1
        Input in = make_input(4, 2);
        memset(in.proof + 3 * 64, 0, 64);
        memset(in.proof + 8 * 64, 0, 64);
        memset(in.vk.qc, 0, 64);
        uint32_t top[8];
        memcpy(top, FrParams::P, 32);
        top[0] -= 1;
        memset(in.publics.data(), 0, 32);
        memcpy(in.publics.data() + 32, top, 32);
        memset(in.proof + 576, 0, 32);
        memcpy(in.proof + 576 + 5 * 32, top, 32);
        compare(in, nullptr);
    }
    // the cases no hash reaches: zeta = 1 (L1 = 1, PI = -publics[0]), zeta = w^3 (L1 = 0, PI = -publics[3]; 0 beyond the publics)
    for (uint64_t l : {0ull, 2ull, 4ull, 12ull, 16ull}) {
        const Input in = make_input(4, l);
        Challenges o;
        uint8_t b[32];
        Fr *f[6] = {&o.beta, &o.gamma, &o.alpha, &o.zeta, &o.v, &o.u};
        for (int j = 0; j < 6; j++) rnd_below(b), *f[j] = fr_from_std(b);
        o.zeta = Fr::one();
        compare(in, &o);
        o.zeta = fr_pow(root_of_unity(4), 3);
        compare(in, &o);
        o.zeta = fr_pow(root_of_unity(4), 15);
        compare(in, &o);
        rnd_below(b), o.zeta = fr_from_std(b);        // and a generic point through the same argument
        compare(in, &o);
    }
    // the reduction of a digest: both ends and a random member of each band; band 5 ends at 2^256 - 1
    for (uint32_t k = 0; k < 6; k++) {
        uint32_t zero[8] = {0}, top[8], mid[8], v[8];
        memcpy(top, FrParams::P, 32);
        top[0] -= 1;
        if (k == 5) {                                 // 2^256 - 1 - 5 r
            uint32_t all[8], five[8];
            for (int i = 0; i < 8; i++) all[i] = 0xffffffffu;
            band_value(five, 5, zero);
            uint64_t borrow = 0;
            for (int i = 0; i < 8; i++) {
                const uint64_t t = (uint64_t)all[i] - five[i] - borrow;
                top[i] = (uint32_t)t;
                borrow = (t >> 32) & 1;
            }
        }
        uint8_t mb[32];
        rnd_below(mb);
        memcpy(mid, mb, 32);
        if (k == 5) mid[7] = 0, mid[6] &= 0xffffu;    // below 2^256 - 5 r, which has 252 bits
        const uint32_t *ds[3] = {zero, mid, top};
        for (const uint32_t *d : ds) {
            band_value(v, k, d);
            const Fr got = pv_digest_mod_r(v);
            CHECK(memcmp(got.v, d, 32) == 0);
        }
    }
    // malformed: a point off the curve, a coordinate = q, a value = r, a public = r
    {
        const Input in = make_input(4, 2);
        malformed(in, 2 * 64, nullptr, false);
        malformed(in, 8 * 64 + 32, nullptr, false);
        malformed(in, 5 * 64, FqParams::P, false);
        malformed(in, 576 + 3 * 32, FrParams::P, false);
        malformed(in, 32, FrParams::P, true);
        malformed(in, 0, FrParams::P, true);
    }
    printf(failures ? "%d checks FAILED\n" : "plonk_verifier host checks OK\n", failures);
    return failures ? 1 : 0;
}
