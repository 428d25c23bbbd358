// What the translation units of the key-set entry points share on the host: the key record the kernels read, the set
// object, and the per-proof pass that pairing_set.hip defines and pairing_set_batch.hip sends the proofs of failed groups
// through.  No kernel is declared here: each unit keeps its own.
#pragma once
#include <memory>
#include <mutex>
#include <vector>

#include "pairing_internal.hpp"

struct KeyRec {                                       // a key as the kernels see it
    const G1Affine *ic;
    const Line *tab;                                  // gamma's lines, then delta's
    const Fq12 *ml_ab;
    uint32_t nPublic, reserved;
};
static_assert(sizeof(KeyRec) == 32, "layout");

struct zk_vkey_set {
    int device = 0;
    std::mutex mu;                                    // calls on one set are serialised; no key's mutex is taken
    std::vector<uint32_t> nPublic;                    // per key
    Consts kc;
    DevBuf<KeyRec> recs;
    // the cooperative path's own, kept between calls: a stream and buffers for `cap` proofs with `cap_pub` signals
    struct Coop {
        std::unique_ptr<Stream> st;
        DevBuf<uint8_t> dp, dv;
        DevBuf<Fr> dpub;
        DevBuf<uint32_t> dkey;
        DevBuf<uint64_t> dat;
        DevBuf<Line> lines;
        uint64_t cap = 0, cap_pub = 0;
    } coop;
    zk_vkey_set_plan plan{};
    // zk_vkey_set_verify_batch's own.  alpha and beta of every key as zk_vkey_create was given them, copied when the set
    // is made; their device copies and beta's lines are made by the set's first batch call, all keys in one launch, so
    // that no key's own batch state is read or written.
    std::vector<uint8_t> alpha_h, beta_h;             // n_keys x 64, n_keys x 128
    struct Batch {
        bool ready = false;
        DevBuf<G1Affine> alpha;                       // [key]
        DevBuf<Line> tab_beta;                        // [key][MILLER_LINES]
    } batch;
};

namespace zkp {

// zk_vkey_set_verify's body for n > 0 proofs on host memory, cooperative or lanes by their number; the caller holds
// set->mu, has set the device and has checked key_of and the pointers.  at[i]: where proof i's signals begin, in signals
// from the call's first; at[n]: the call's total.
void set_verify_locked(zk_vkey_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, const std::vector<uint64_t> &at, uint64_t n,
                       uint8_t *verdict);

}   // namespace zkp
