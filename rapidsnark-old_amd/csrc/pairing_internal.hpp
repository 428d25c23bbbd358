// What the translation units of the verification entry points share on the host: the key object, the constants' holder,
// the chunk size, the cooperative threshold (pairing_set.hip reads both as zk_vkey_verify does) and the per-proof pass that
// pairing.hip defines and pairing_batch.hip sends the proofs of failed groups through.  No kernel is declared here: each unit
// keeps its own.
#pragma once
#include <memory>
#include <mutex>

#include "hiputil.hpp"
#include "pairing.hpp"

namespace zkp {

struct Consts {
    DevBuf<PairConsts> k;
    void make(hipStream_t s);                         // pairing.hip: k_pair_consts
};

uint64_t chunk_jobs();                                // ZKHIP_VERIFY_CHUNK, read at every call (pairing.hip)
uint64_t verify_coop_max();                           // ZKHIP_VERIFY_COOP_MAX, read at every call (pairing.hip)
constexpr uint64_t COOP_MAX_PROOFS = 8192;            // 19 KiB of lines a proof: a call with more of them goes the lane way whatever the threshold

}   // namespace zkp

// The key on its device: IC, the line tables of gamma and delta, the Miller value of (alpha, beta), the constants.
struct zk_vkey {
    int device = 0;
    uint32_t nPublic = 0;
    std::mutex mu;                                    // calls on one key are serialised
    Consts kc;
    DevBuf<G1Affine> ic;
    DevBuf<Line> tab;
    DevBuf<Fq12> ml_ab;
    // the cooperative path's own, kept between calls: a stream and buffers for `cap` proofs, grown when a call brings more
    struct Coop {
        std::unique_ptr<Stream> st;
        DevBuf<uint8_t> dp, dv;
        DevBuf<Fr> dpub;
        DevBuf<Line> lines;
        uint64_t cap = 0;
    } coop;
    zk_vkey_plan plan{};
    // zk_vkey_verify_batch's own.  alpha and beta as zk_vkey_create was given them (checked there); their device copies and
    // beta's lines are made by the key's first batch call, so that creating a key costs what it did.
    uint8_t alpha_h[64], beta_h[128];
    struct Batch {
        bool ready = false;
        DevBuf<G1Affine> alpha;
        DevBuf<Line> tab_beta;
    } batch;
};

namespace zkp {

// zk_vkey_verify's body for n > 0 proofs on host memory; the caller holds vk->mu and has checked the pointers
void vkey_verify_locked(zk_vkey *vk, const uint8_t *proofs, const uint8_t *publics, uint64_t n, uint8_t *verdict);

}   // namespace zkp
