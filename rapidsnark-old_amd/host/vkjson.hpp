// verification_key.json as `zkeynew` and `zkeycontribute` write it: snarkjs's keys protocol, curve, nPublic, vk_alpha_1,
// vk_beta_2, vk_gamma_2, vk_delta_2 and IC, from the key's own bytes (affine Montgomery points).
#pragma once
#include <cstdint>
#include <string>

#include "../csrc/common.hpp"

inline std::string g1_json(const uint8_t *p) {
    return "[\"" + zk::HostTail::fq_mont_to_dec(p) + "\", \"" + zk::HostTail::fq_mont_to_dec(p + 32) + "\", \"1\"]";
}
inline std::string g2_json(const uint8_t *p) {
    auto d = [&](int i) { return "\"" + zk::HostTail::fq_mont_to_dec(p + 32 * i) + "\""; };
    return "[[" + d(0) + ", " + d(1) + "], [" + d(2) + ", " + d(3) + "], [\"1\", \"0\"]]";
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
