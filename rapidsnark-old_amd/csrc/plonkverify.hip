// PLONK verifier (include/zkhip.h, section "PLONK prover and verifier"): the challenges from the proof by the transcript the
// prover ran, the scalars of the linearisation the prover used (plonk_transcript.hpp holds both, in one copy), a dozen
// scalar multiplications on the host and ONE launch, kzg.hip's one-lane pairing check e(L, G2) = e(W, [tau]G2).  No kernel
// of its own.  The counterpart is snarkjs's PLONK verifier; DESIGN.md section 31.
#include "plonk_internal.hpp"
#include "plonk_transcript.hpp"

namespace {

typedef Pt<Fq> P1;

void plonk_verify(zk_kzg *kzg, const zk_plonk_vkey *vk, const uint8_t *proof, const uint8_t *publics, uint8_t *verdict) {
    const char *who = "zk_plonk_verify";
    if (!kzg || !vk || !proof || !verdict || (vk->n_public && !publics)) throw std::invalid_argument("null argument");
    if (vk->size != sizeof(zk_plonk_vkey)) throw std::invalid_argument(std::string(who) + ": vk->size is not sizeof(zk_plonk_vkey)");
    if (vk->log_n < 3 || vk->log_n > PLONK_MAX_LOG_N) throw std::invalid_argument(std::string(who) + ": log_n " + std::to_string(vk->log_n) + " is outside 3 .. 25");
    const uint64_t n = 1ull << vk->log_n;
    if (vk->n_public > n) throw std::invalid_argument(std::string(who) + ": n_public " + std::to_string(vk->n_public) + " exceeds n = " + std::to_string(n));
    if (memcmp(vk->tau_g2, kzg->g2tau, sizeof vk->tau_g2) != 0) throw std::invalid_argument(std::string(who) + ": the key's [tau]G2 is not the kzg's");
    const Fr k1 = checked_one(who, "k1", vk->k1), k2 = checked_one(who, "k2", vk->k2);
    const uint8_t *vkp[PLONK_CIRC_VECS] = {vk->qm, vk->ql, vk->qr, vk->qo, vk->qc, vk->s1, vk->s2, vk->s3};
    for (uint32_t j = 0; j < PLONK_CIRC_VECS; j++)
        if (!g1_well_formed(vkp[j])) throw std::invalid_argument(std::string(who) + ": a commitment of the key is not a point of the curve");
    const uint8_t *pts = proof, *evals = proof + PLONK_POINTS * 64;
    *verdict = ZK_VERIFY_MALFORMED;
    for (uint32_t j = 0; j < PLONK_POINTS; j++)
        if (!g1_well_formed(pts + j * 64)) return;
    if (first_not_below_r(evals, PLONK_EVALS) < PLONK_EVALS) return;
    if (first_not_below_r(publics, vk->n_public) < vk->n_public) return;

    Challenges ch;
    round1_challenges(ch, *vk, publics, pts);
    round2_challenge(ch, pts);
    round3_challenge(ch, pts);
    round4_challenge(ch, evals);
    round5_challenge(ch, pts);
    const Fr ze = ch.zeta, u = ch.u;
    Fr ev[PLONK_EVALS];
    for (uint32_t j = 0; j < PLONK_EVALS; j++) ev[j] = fr_from_std(evals + j * 32);
    const LinScalars k = lin_scalars(ev, at_zeta(vk->log_n, ze, publics, vk->n_public), ze, k1, k2, ch.alpha, ch.beta, ch.gamma, ch.v);
    auto pt = [&](uint32_t j) { return P1(pts + j * 64); };
    // F: the commitments by the scalars the prover's rows took, [z] by u more
    P1 F = P1(vk->qm).times(k.qm) + P1(vk->ql).times(ev[0]) + P1(vk->qr).times(ev[1]) + P1(vk->qo).times(ev[2]) + P1(vk->qc);
    F = F + pt(P_Z).times(Fr::add(k.z, u)) + P1(vk->s3).times(k.s3);
    F = F + pt(P_TLO).times(k.tlo) + pt(P_TMID).times(k.tmid) + pt(P_THI).times(k.thi);
    const P1 batch[5] = {pt(P_A), pt(P_B), pt(P_C), P1(vk->s1), P1(vk->s2)};
    for (int j = 0; j < 5; j++) F = F + batch[j].times(k.v[j]);
    // E: -r0 + v a + .. + v^5 s2 + u z'w, r0 the constant the prover put at index 0 of r
    const P1 E = P1(kzg->g1).times(Fr::add(Fr::sub(k.E, k.c0), Fr::mul(u, ev[5])));
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

int zk_plonk_verify(zk_kzg *kzg, const zk_plonk_vkey *vk, const uint8_t proof[ZK_PLONK_PROOF_BYTES], const uint8_t *publics, uint8_t *verdict) {
    return guarded([&] { plonk_verify(kzg, vk, proof, publics, verdict); });
}

}   // extern "C"
