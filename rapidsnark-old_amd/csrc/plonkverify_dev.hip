// PLONK verifier object (include/zkhip.h, section "PLONK prover and verifier", zk_plonk_verifier_*): made from a key alone,
// m proofs a call, each with its own verdict, and everything per proof on the device.  zk_plonk_verify (plonkverify.hip)
// stays the one-proof entry with the host's transcript; its verdicts are what this unit must give.  DESIGN.md section 33.
//
// Four launches a chunk of proofs:
//   k_plonk_transcript  a lane per proof: the checks, the six Keccak-256 challenges, zeta^n, Z_H, L1, PI and the nineteen
//                       scalars of the combination (plonk_verify_dev.hpp: the same text runs on the host in
//                       tools/plonk_verifier_host_test.cpp), written term-major so that the next kernel reads them coalesced
//   k_plonk_combine     a lane per (proof, term), term-major: mulglv.hpp's mul_glv, the lanes of a wave sharing a term and,
//                       for the nine fixed bases, the base
//   k_plonk_sum         a lane per proof: L = the sum of eighteen products, W = W_zeta + u W_zeta_omega, both affine
//   k_kzg_pair          kzg.hip's, over the object's own line tables: e(L, G2) = e(W, [tau]G2)
// Every addition is curve.hpp's complete one: a zero scalar, a base at infinity, a term that cancels the running sum and
// L or W at infinity take no special path here.  A malformed proof's lanes return at once in every kernel.
#include "plonk_verifier_internal.hpp"
#include "plonk_transcript.hpp"

namespace {

// ---------------------------------------------------------------- device
__global__ __launch_bounds__(64) void k_plonk_transcript(uint32_t *status, uint8_t *ch, Fr *sc, const uint8_t *__restrict__ proofs,
                                                          const uint8_t *__restrict__ publics, uint64_t m, uint64_t stride,
                                                          const PlonkVerifyConsts *__restrict__ K, uint32_t want_scalars) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    status[i] = plonk_verify_lane(*K, proofs + i * PV_PROOF_BYTES, publics + i * K->n_public * 32, ch + i * PV_CHALLENGES * 32,
                                  want_scalars ? sc + i : nullptr, stride, nullptr);
}

// part[t stride + i] = sc[t stride + i] B, B the key's base t below PV_FIXED and the proof's point otherwise
__global__ __launch_bounds__(64) void k_plonk_combine(G1XYZZ *part, const uint32_t *__restrict__ status, const Fr *__restrict__ sc,
                                                       const uint8_t *__restrict__ proofs, const G1Affine *__restrict__ fixed, uint64_t m, uint64_t stride,
                                                       Fq endo) {
    const uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= m * PV_TERMS) return;
    const uint32_t t = (uint32_t)(lane / m);
    const uint64_t i = lane - (uint64_t)t * m;
    if (status[i] != PV_OK) return;
    const uint32_t j = t == PV_WZW_U ? PV_POINTS - 1 : t - PV_FIXED;           // the proof's point, t >= PV_FIXED
    const G1Affine *base = t < PV_FIXED ? fixed + t : reinterpret_cast<const G1Affine *>(proofs + i * PV_PROOF_BYTES) + j;
    store_pt(part + t * stride + i, mul_glv(load_pt(base), load_el(sc + t * stride + i), endo));
}

__global__ __launch_bounds__(64) void k_plonk_sum(G1Affine *L, G1Affine *W, const uint32_t *__restrict__ status, const G1XYZZ *__restrict__ part,
                                                   const uint8_t *__restrict__ proofs, uint64_t m, uint64_t stride) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || status[i] != PV_OK) return;
    G1XYZZ acc = load_pt(part + i);
#pragma unroll 1
    for (uint32_t t = 1; t < PV_WZW_U; t++) add(acc, load_pt(part + t * stride + i));
    const G1Affine l = g1_to_affine(acc);
    acc = load_pt(part + PV_WZW_U * stride + i);
    madd(acc, load_pt(reinterpret_cast<const G1Affine *>(proofs + i * PV_PROOF_BYTES) + P_WZ));
    const G1Affine w = g1_to_affine(acc);
    store_el(&L[i].x, l.x);
    store_el(&L[i].y, l.y);
    store_el(&W[i].x, w.x);
    store_el(&W[i].y, w.y);
}

// ---------------------------------------------------------------- the object (plonk_verifier_internal.hpp)
zk_plonk_verifier *verifier_create(const zk_plonk_vkey *vk, int32_t device) {
    const char *who = "zk_plonk_verifier_create";
    if (!vk) throw std::invalid_argument("null argument");
    if (vk->size != sizeof(zk_plonk_vkey)) throw std::invalid_argument(std::string(who) + ": vk->size is not sizeof(zk_plonk_vkey)");
    if (vk->log_n < 3 || vk->log_n > PLONK_MAX_LOG_N) throw std::invalid_argument(std::string(who) + ": log_n " + std::to_string(vk->log_n) + " is outside 3 .. 25");
    const uint64_t n = 1ull << vk->log_n;
    if (vk->n_public > n) throw std::invalid_argument(std::string(who) + ": n_public " + std::to_string(vk->n_public) + " exceeds n = " + std::to_string(n));
    const Fr k1 = checked_one(who, "k1", vk->k1), k2 = checked_one(who, "k2", vk->k2);
    const uint8_t *vkp[PV_KEY_POINTS] = {vk->qm, vk->ql, vk->qr, vk->qo, vk->qc, vk->s1, vk->s2, vk->s3};
    for (uint32_t j = 0; j < PV_KEY_POINTS; j++)
        if (!g1_well_formed(vkp[j])) throw std::invalid_argument(std::string(who) + ": a commitment of the key is not a point of the curve");
    const PlonkVerifyConsts K = plonk_verify_consts(*vk, k1, k2);
    Pt<Fq> g1;
    Pt<Fq2> g2;
    generators(g1, g2);
    uint8_t fixed[PV_FIXED * 64], q2[2 * sizeof(G2Affine)];
    for (uint32_t j = 0; j < PV_KEY_POINTS; j++) memcpy(fixed + j * 64, vkp[j], 64);
    memcpy(fixed + PV_G * 64, g1.b, 64);
    memcpy(q2, g2.b, sizeof(G2Affine));
    memcpy(q2 + sizeof(G2Affine), vk->tau_g2, sizeof(G2Affine));

    std::unique_ptr<zk_plonk_verifier> v(new zk_plonk_verifier);
    v->device = resolve_device(device);
    v->log_n = vk->log_n;
    v->n_public = vk->n_public;
    v->endo = endo_const<Fq>();
    memcpy(v->q2, q2, sizeof q2);
    DeviceGuard g(v->device);
    need_hbm(who, 2 * MILLER_LINES * sizeof(Line) + sizeof fixed + sizeof q2 + sizeof K + sizeof(PairConsts) + 65536);
    v->st.reset(new Stream);
    hipStream_t s = v->st->s;
    DevBuf<uint32_t> derr;
    DevBuf<G2Affine> d2;
    derr.alloc(4);
    d2.alloc(2);
    HIP_TRY(hipMemcpyAsync(d2.p, q2, sizeof q2, hipMemcpyHostToDevice, s));
    // [tau]G2 as ptau_check.hip judges section 3's points: coordinates, the twist, the subgroup; infinity is no [tau]G2
    const PsiConsts psi = psi_consts();
    uint32_t h[4];
    enqueue_classify<Fq2>(h, derr.p, d2.p + 1, 1, true, &psi, plain_subgroup(), s);
    if (classified(h, s).kind) throw std::invalid_argument(std::string(who) + ": the key's [tau]G2 is not a point of the twist in the subgroup");
    v->kc.make(s);
    v->tab.alloc(2 * MILLER_LINES);
    launch_kzg_line_tables(v->tab.p, d2.p, v->kc.k.p, s);
    v->fixed.alloc(PV_FIXED);
    v->kv.alloc(1);
    HIP_TRY(hipMemcpyAsync(v->fixed.p, fixed, sizeof fixed, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(v->kv.p, &K, sizeof K, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    return v.release();
}

void verifier_verify(zk_plonk_verifier *v, const uint8_t *proofs, const uint8_t *publics, uint64_t m, uint8_t *verdict) {
    over_chunks(v, "zk_plonk_verifier_verify", proofs, publics, m, verdict, verdict, [&](uint64_t off, uint64_t cnt, hipStream_t s) {
        launch_transcript(v, cnt, true, s);
        launch_per_proof(v, 0, cnt, s);
        HIP_TRY(hipMemcpyAsync(verdict + off, v->verdict.p, cnt, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    });
}

void verifier_challenges(zk_plonk_verifier *v, const uint8_t *proofs, const uint8_t *publics, uint64_t m, uint8_t *challenges, uint8_t *status) {
    std::vector<uint32_t> st;
    over_chunks(v, "zk_plonk_verifier_challenges", proofs, publics, m, challenges, status, [&](uint64_t off, uint64_t cnt, hipStream_t s) {
        st.resize(cnt);
        launch_transcript(v, cnt, false, s);
        ZK_LAUNCH_OK("plonk transcript");
        HIP_TRY(hipMemcpyAsync(challenges + off * PV_CHALLENGES * 32, v->ch.p, cnt * PV_CHALLENGES * 32, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(st.data(), v->status.p, cnt * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (uint64_t i = 0; i < cnt; i++) status[off + i] = st[i] == PV_OK ? 0 : ZK_VERIFY_MALFORMED;
    });
}

}   // namespace

// ---------------------------------------------------------------- what plonkverify_batch.hip launches too (plonk_verifier_internal.hpp)
void launch_transcript(zk_plonk_verifier *v, uint64_t cnt, bool want_scalars, hipStream_t s) {
    ZK_LAUNCH(k_plonk_transcript, dim3(nblocks(cnt, 64)), dim3(64), 0, s, v->status.p, v->ch.p, v->sc.p, v->proofs.p, v->publics.p, cnt, v->cap, v->kv.p,
              want_scalars ? 1u : 0u);
}

void launch_per_proof(zk_plonk_verifier *v, uint64_t lo, uint64_t cnt, hipStream_t s) {
    const uint8_t *proofs = v->proofs.p + lo * PV_PROOF_BYTES;
    ZK_LAUNCH(k_plonk_combine, dim3(nblocks(cnt * PV_TERMS, 64)), dim3(64), 0, s, v->part.p + lo, v->status.p + lo, v->sc.p + lo, proofs, v->fixed.p, cnt, v->cap,
              v->endo);
    ZK_LAUNCH(k_plonk_sum, dim3(nblocks(cnt, 64)), dim3(64), 0, s, v->L.p + lo, v->W.p + lo, v->status.p + lo, v->part.p + lo, proofs, cnt, v->cap);
    ZK_LAUNCH_OK("plonk verification");
    launch_kzg_pair(v->verdict.p + lo, v->status.p + lo, v->L.p + lo, v->W.p + lo, v->tab.p, cnt, v->kc.k.p, s);
}

extern "C" {

int zk_plonk_verifier_create(zk_plonk_verifier **out, const zk_plonk_vkey *vk, int32_t device) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        *out = verifier_create(vk, device);
    });
}

void zk_plonk_verifier_destroy(zk_plonk_verifier *v) { destroy_on_device(v); }

int zk_plonk_verifier_info(zk_plonk_verifier *v, zk_plonk_verifier_plan *plan) {
    return guarded([&] {
        if (!v || !plan) throw std::invalid_argument("null argument");
        info_into("zk_plonk_verifier_info", plan, [&](zk_plonk_verifier_plan &p) {
            std::lock_guard<std::mutex> lock(v->mu);
            p.log_n = v->log_n;
            p.n_public = v->n_public;
            p.device_bytes = v->bytes();
            p.chunk = plonk_verify_chunk_in_effect();
            p.last_launches = v->last_launches;
            p.last_chunks = v->last_chunks;
        });
    });
}

int zk_plonk_verifier_verify(zk_plonk_verifier *v, const uint8_t *proofs, const uint8_t *publics, uint64_t m, uint8_t *verdict) {
    return guarded([&] { verifier_verify(v, proofs, publics, m, verdict); });
}

int zk_plonk_verifier_challenges(zk_plonk_verifier *v, const uint8_t *proofs, const uint8_t *publics, uint64_t m, uint8_t *challenges, uint8_t *status) {
    return guarded([&] { verifier_challenges(v, proofs, publics, m, challenges, status); });
}

}   // extern "C"
