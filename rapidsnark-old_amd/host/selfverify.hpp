// ZKHIP_SELFVERIFY=1: `prover` and `proverServer` verify every proof they make against the witness's public signals
// before handing it out, with a verification key built from the .zkey's own sections 2 and 3 (alpha_1, beta_2, gamma_2,
// delta_2, IC) on the prover's device.  A corrupted key, a .zkey whose delta_1 and delta_2 disagree or a bad table in
// device memory give proofs that do not verify; with the switch on they are refused instead of written.  One helper for
// both programs.  Unset or 0: nothing here runs.
#pragma once
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/zkhip.h"
#include "zkfile.hpp"

namespace SelfVerify {

inline bool enabled() {
    const char *e = getenv("ZKHIP_SELFVERIFY");
    return e && *e && strcmp(e, "0") != 0;
}

inline std::string message(uint8_t verdict) { return "proof failed self-verification (verdict " + std::to_string((unsigned)verdict) + ")"; }

class Key {
    zk_vkey *h_ = nullptr;
    uint32_t nPublic_ = 0;

public:
    // hdr's vk pointers and ic (section 3) are read here and not kept
    Key(const ZKeyUtils::Header &hdr, const void *ic, uint64_t icBytes, int32_t device) : nPublic_(hdr.nPublic) {
        const uint64_t want = ZKeyUtils::Shape{hdr.nVars, hdr.nPublic, hdr.domainSize, hdr.nCoefs}.sectionBytes(3);
        if (icBytes != want)
            throw std::invalid_argument("zkey section 3 holds " + std::to_string(icBytes) + " bytes, nPublic = " + std::to_string(hdr.nPublic) + " implies " +
                                        std::to_string(want));
        zk_vkey_view view;
        view.vk_alpha1 = hdr.vk_alpha1;
        view.vk_beta2 = hdr.vk_beta2;
        view.vk_gamma2 = hdr.vk_gamma2;
        view.vk_delta2 = hdr.vk_delta2;
        view.IC = ic;
        view.nPublic = hdr.nPublic;
        if (zk_vkey_create(&h_, &view, device) != 0) throw std::runtime_error(std::string("self-verification key: ") + zk_last_error());
    }
    Key(const Key &) = delete;
    Key &operator=(const Key &) = delete;
    ~Key() { zk_vkey_destroy(h_); }

    // one zk_vkey_verify call for n proofs; witness[k]: proof k's witness values (32 bytes each: 1, then the public signals)
    std::vector<uint8_t> verdicts(const zk_proof *proofs, const uint8_t *const *witness, size_t n) const {
        std::vector<uint8_t> publics((size_t)nPublic_ * 32 * n), out(n, ZK_VERIFY_MALFORMED);
        for (size_t k = 0; k < n; k++) memcpy(publics.data() + k * nPublic_ * 32, witness[k] + 32, (size_t)nPublic_ * 32);
        if (zk_vkey_verify(h_, reinterpret_cast<const uint8_t *>(proofs), publics.empty() ? nullptr : publics.data(), n, out.data()) != 0)
            throw std::runtime_error(std::string("self-verification: ") + zk_last_error());
        return out;
    }
    // throws message(verdict) unless the proof verifies
    void require(const zk_proof &proof, const uint8_t *witness) const {
        const uint8_t v = verdicts(&proof, &witness, 1)[0];
        if (v != ZK_VERIFY_OK) throw std::runtime_error(message(v));
    }
};

}   // namespace SelfVerify
