// What plonkverify_dev.hip shares with plonkverify_batch.hip (batch verification by random combination runs on a
// zk_plonk_verifier's resident key, tables and chunk buffers): the object, the walk over the chunks of a call with its
// checks, and the launchers of the per-proof kernels.  The kernels stay in plonkverify_dev.hip, and with them the bodies of
// launch_transcript and launch_per_proof; everything else here is the text plonkverify_dev.hip held.
#pragma once
#include "plonk_internal.hpp"
#include "plonk_verify_dev.hpp"

constexpr uint64_t PLONK_VERIFY_DEFAULT_CHUNK = 65536, PLONK_VERIFY_MAX_CHUNK = 1ull << 20;   // 65536: a wave of pairing lanes on every SIMD (profiles/plonk_verifier_timing.txt)
inline uint64_t plonk_verify_chunk_in_effect() {
    return env_number("ZKHIP_PLONK_VERIFY_CHUNK", PLONK_VERIFY_DEFAULT_CHUNK, 1, PLONK_VERIFY_MAX_CHUNK, "a number of proofs from 1 to 2^20");
}

// ZKHIP_PLONK_VERIFY_GROUP, read at every batch call of an object or of a key set (plonkverify_set.hip)
constexpr uint64_t PLONK_DEFAULT_GROUP = 65536, PLONK_MAX_GROUP = 1ull << 20;   // 65536: the lowest all-valid median at 65536 proofs (profiles/plonk_verify_batch_timing.txt)
inline uint64_t plonk_verify_group_in_effect() {
    return env_number("ZKHIP_PLONK_VERIFY_GROUP", PLONK_DEFAULT_GROUP, 1, PLONK_MAX_GROUP, "a number of proofs from 1 to 2^20");
}

// zk_plonk_verifier_verify_batch's own: made by the object's first batch call, re-made when the chunk's capacity or the
// group changes.  Group g of a chunk has slots of `group` proofs whatever it holds: a short group's tail and a malformed
// proof take zero scalars
constexpr uint64_t PLONK_BATCH_SLICE = 256;           // groups a launch of the cooperative pairing: 2 pairs and 38 KiB of lines each
struct PlonkBatchBufs {
    uint64_t cap = 0, group = 0, ngroups = 0;         // what the buffers were made for; ngroups = ceil(cap / group)
    DevBuf<G1Affine> fixed;                           // the nine fixed bases in the bucket kernels' form: made once
    DevBuf<uint8_t> r16;                              // cap x 16 bytes
    DevBuf<Fr> fx, partial;                           // PV_FIXED rows of ngroups group slots: r_i s_it; PV_FIXED rows of the fold's workgroup sums
    DevBuf<Fr> lsc, wsc;                              // a group: 9 group + 9 scalars; 2 group scalars
    DevBuf<G1Affine> lpt, wpt;                        // their points, the bucket kernels' form
    DevMsm<Fq> lmsm, wmsm;
    DevBuf<G1Affine> p1;                              // the pairs of a slice: L, -W a group
    DevBuf<G2Affine> p2;                              // G2, [tau]G2 a group
    DevBuf<Line> lines;
    DevBuf<uint8_t> skip, out;
    DevBuf<uint32_t> err;
    static uint64_t fold_blocks(uint64_t group_) { return (group_ + 255) / 256; }
    static uint64_t bytes_for(uint64_t cap_, uint64_t group_) {
        const uint64_t ng = (cap_ + group_ - 1) / group_;
        return cap_ * 16 + ng * (group_ + fold_blocks(group_)) * PV_FIXED * sizeof(Fr) +
               ng * (11 * group_ + PV_FIXED) * (sizeof(Fr) + sizeof(G1Affine)) + DevMsm<Fq>::bytes(9 * group_ + PV_FIXED) + DevMsm<Fq>::bytes(2 * group_) +
               PLONK_BATCH_SLICE * (2 * (sizeof(G1Affine) + sizeof(G2Affine) + MILLER_LINES * sizeof(Line) + 1) + sizeof(Fq12)) + PV_FIXED * sizeof(G1Affine) + 65536;
    }
    size_t bytes() const {
        return fixed.bytes() + r16.bytes() + fx.bytes() + partial.bytes() + lsc.bytes() + wsc.bytes() + lpt.bytes() + wpt.bytes() + msm_bytes(lmsm) +
               msm_bytes(wmsm) + p1.bytes() + p2.bytes() + lines.bytes() + skip.bytes() + out.bytes() + err.bytes();
    }
};

struct zk_plonk_verifier {
    int device = 0;
    uint32_t log_n = 0;
    uint64_t n_public = 0;
    std::mutex mu;                                    // calls on one object are serialised
    std::unique_ptr<Stream> st;
    Consts kc;
    DevBuf<Line> tab;                                 // the G2 generator's lines, then [tau]G2's
    DevBuf<G1Affine> fixed;                           // the key's eight commitments and the generator, the file's form
    DevBuf<PlonkVerifyConsts> kv;
    Fq endo;
    uint8_t q2[2 * sizeof(G2Affine)];                 // the generator of G2 and [tau]G2, the file's form: the pairs of a batch call
    // a chunk of proofs; grown, never shrunk
    uint64_t cap = 0;
    DevBuf<uint8_t> proofs, publics, ch, verdict;
    DevBuf<uint32_t> status;
    DevBuf<Fr> sc;                                    // PV_TERMS rows of cap
    DevBuf<G1XYZZ> part;
    DevBuf<G1Affine> L, W;
    PlonkBatchBufs batch;
    uint32_t last_launches = 0, last_chunks = 0;
    static uint64_t chunk_bytes(uint64_t cap_, uint64_t n_public_) {
        return cap_ * (PV_PROOF_BYTES + (n_public_ ? n_public_ : 1) * 32 + PV_CHALLENGES * 32 + 1 + 4 + PV_TERMS * (sizeof(Fr) + sizeof(G1XYZZ)) +
                       2 * sizeof(G1Affine));
    }
    size_t bytes() const {
        return tab.bytes() + fixed.bytes() + kv.bytes() + sizeof(PairConsts) + proofs.bytes() + publics.bytes() + ch.bytes() + verdict.bytes() +
               status.bytes() + sc.bytes() + part.bytes() + L.bytes() + W.bytes() + batch.bytes();
    }
    void size(const char *who, uint64_t cap_) {
        if (cap_ <= cap) return;
        need_hbm(who, chunk_bytes(cap_, n_public));
        cap = 0;
        proofs.alloc(cap_ * PV_PROOF_BYTES);
        publics.alloc(cap_ * (n_public ? n_public : 1) * 32);
        ch.alloc(cap_ * PV_CHALLENGES * 32);
        verdict.alloc(cap_);
        status.alloc(cap_);
        sc.alloc(cap_ * PV_TERMS);
        part.alloc(cap_ * PV_TERMS);
        L.alloc(cap_);
        W.alloc(cap_);
        cap = cap_;
    }
};

// the checks every call makes, then run(off, cnt, s) for every chunk with the chunk's proofs and publics on the device.
// before(cap): once, under the lock and on the object's device, before the chunk's buffers are sized (a batch call sizes its own)
template <class Run, class Before>
void over_chunks(zk_plonk_verifier *v, const char *who, const uint8_t *proofs, const uint8_t *publics, uint64_t m, const void *out1, const void *out2, Run run,
                 Before before) {
    if (!v) throw std::invalid_argument("null argument");
    if (!m) return;
    if (m >= (1ull << 31)) throw std::invalid_argument(std::string(who) + ": m is not below 2^31");
    if (!proofs || !out1 || !out2 || (v->n_public && !publics)) throw std::invalid_argument("null argument");
    const uint64_t chunk = plonk_verify_chunk_in_effect(), cap = m < chunk ? m : chunk;
    std::lock_guard<std::mutex> lock(v->mu);
    DeviceGuard g(v->device);
    LaunchCount lc(v->last_launches);
    v->last_chunks = 0;
    before(cap);
    v->size(who, cap);
    hipStream_t s = v->st->s;
    for (uint64_t off = 0; off < m; off += cap) {
        const uint64_t cnt = m - off < cap ? m - off : cap;
        HIP_TRY(hipMemcpyAsync(v->proofs.p, proofs + off * PV_PROOF_BYTES, cnt * PV_PROOF_BYTES, hipMemcpyHostToDevice, s));
        if (v->n_public) HIP_TRY(hipMemcpyAsync(v->publics.p, publics + off * v->n_public * 32, cnt * v->n_public * 32, hipMemcpyHostToDevice, s));
        run(off, cnt, s);
        v->last_chunks++;
    }
}
template <class Run>
void over_chunks(zk_plonk_verifier *v, const char *who, const uint8_t *proofs, const uint8_t *publics, uint64_t m, const void *out1, const void *out2, Run run) {
    over_chunks(v, who, proofs, publics, m, out1, out2, run, [](uint64_t) {});
}

// plonkverify_dev.hip's kernels over the chunk the object holds.  k_plonk_transcript for proofs [0, cnt): status, the
// challenges and (want_scalars) the nineteen rows of sc
void launch_transcript(zk_plonk_verifier *v, uint64_t cnt, bool want_scalars, hipStream_t s);
// k_plonk_combine, k_plonk_sum and k_kzg_pair for proofs [lo, lo + cnt) of the chunk, from status and sc as the transcript
// left them: v->verdict[lo, lo + cnt)
void launch_per_proof(zk_plonk_verifier *v, uint64_t lo, uint64_t cnt, hipStream_t s);

// plonkverify_batch.hip's pairing step over the buffers of its caller (the object's batch buffers, or a key set's,
// plonkverify_set.hip): pass[q] = e(L, G2) e(-W, [tau]G2) = 1 for the groups at[q] of sums, L | W a group in the file's form.
// p1, lines, skip: 2 PLONK_BATCH_SLICE entries (lines: times MILLER_LINES); p2: G2, [tau]G2 PLONK_BATCH_SLICE times; out:
// PLONK_BATCH_SLICE Fq12; err: three words, all ones.  The stream is drained inside
struct PlonkPairBufs {
    G1Affine *p1;
    const G2Affine *p2;
    Line *lines;
    uint8_t *skip, *out;
    uint32_t *err;
};
void plonk_group_equations(const PlonkPairBufs &b, const PairConsts *k, std::vector<uint8_t> &pass, const uint8_t *sums, const std::vector<uint64_t> &at, hipStream_t s);
