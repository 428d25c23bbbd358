// verification_key.json as `zkeynew` and `zkeycontribute` write it: snarkjs's keys protocol, curve, nPublic, vk_alpha_1,
// vk_beta_2, vk_gamma_2, vk_delta_2 and IC, from the key's own bytes (affine Montgomery points).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/zkhip.h"
#include "../csrc/common.hpp"

inline std::string g1_json(const uint8_t *p) {
    return "[\"" + zk::HostTail::fq_mont_to_dec(p) + "\", \"" + zk::HostTail::fq_mont_to_dec(p + 32) + "\", \"1\"]";
}
inline std::string g2_json(const uint8_t *p) {
    auto d = [&](int i) { return "\"" + zk::HostTail::fq_mont_to_dec(p + 32 * i) + "\""; };
    return "[[" + d(0) + ", " + d(1) + "], [" + d(2) + ", " + d(3) + "], [\"1\", \"0\"]]";
}
// A PLONK key (zk_plonk_vkey) with snarkjs's field names for PLONK, as `plonkvkey` writes it and `plonkverifier` and
// PlonkVKey.from_json read it.  w_dec: the root of unity of 2^power, decimal.  Infinity is 0 1 0.  The file names a key of this
// project's compile and transcript: parity with snarkjs is unpinned (include/zkhip.h)
inline std::string plonk_verification_key_json(const zk_plonk_vkey &vk, const std::string &k1_dec, const std::string &k2_dec, const std::string &w_dec) {
    static const uint8_t zero[128] = {0};
    auto g1 = [&](const uint8_t *p) { return memcmp(p, zero, 64) == 0 ? std::string("[\"0\", \"1\", \"0\"]") : g1_json(p); };
    const uint8_t *pts[8] = {vk.qm, vk.ql, vk.qr, vk.qo, vk.qc, vk.s1, vk.s2, vk.s3};
    static const char *const names[8] = {"Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3"};
    std::string j = "{\n \"protocol\": \"plonk\",\n \"curve\": \"bn128\",\n \"nPublic\": " + std::to_string(vk.n_public) + ",\n \"power\": " +
                    std::to_string(vk.log_n) + ",\n \"k1\": \"" + k1_dec + "\",\n \"k2\": \"" + k2_dec + "\",\n";
    for (int i = 0; i < 8; i++) j += std::string(" \"") + names[i] + "\": " + g1(pts[i]) + ",\n";
    j += " \"X_2\": " + (memcmp(vk.tau_g2, zero, 128) == 0 ? std::string("[[\"0\", \"0\"], [\"1\", \"0\"], [\"0\", \"0\"]]") : g2_json(vk.tau_g2)) + ",\n";
    j += " \"w\": \"" + w_dec + "\"\n}";
    return j;
}

// ic: nPublic + 1 G1 points (section 3)
inline std::string verification_key_json(uint32_t nPublic, const uint8_t *alpha1, const uint8_t *beta2, const uint8_t *gamma2,
                                         const uint8_t *delta2, const uint8_t *ic) {
    std::string j = "{\n \"protocol\": \"groth16\",\n \"curve\": \"bn128\",\n \"nPublic\": " + std::to_string(nPublic) + ",\n";
    j += " \"vk_alpha_1\": " + g1_json(alpha1) + ",\n";
    j += " \"vk_beta_2\": " + g2_json(beta2) + ",\n";
    j += " \"vk_gamma_2\": " + g2_json(gamma2) + ",\n \"vk_delta_2\": " + g2_json(delta2) + ",\n \"IC\": [";
    for (uint64_t i = 0; i <= nPublic; i++) j += std::string(i ? ",\n  " : "\n  ") + g1_json(ic + 64 * i);
    j += "\n ]\n}";
    return j;
}
