// Host helpers that need no HIP and that every unit with entry points reaches through hiputil.hpp: a number and an on/off
// switch from the environment, the pick of the first bad point from the four words of the point pass (ptengine.hpp) with
// the texts of its kinds, and the test for a scalar that is 0 or 1.  tools/verify_batch_host_test.cpp builds it for the
// host alone (through verify_batch_host.hpp).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <stdexcept>
#include <string>

#include "field.hpp"

namespace zk {

// Decimal, from min to max; unset or empty: dflt; anything else: "<name>: <what> expected".  Strict (the group switches,
// the cooperative thresholds): the first character is a digit and nothing follows the number, so a blank, a sign or a
// suffix is refused.  Lax (the chunk sizes and the scan segments, which came first): what strtoull takes before the number,
// leading blanks and a sign, is taken; nothing may follow it.
enum EnvForm { ENV_STRICT, ENV_LAX };
inline uint64_t env_number(const char *name, uint64_t dflt, uint64_t min, uint64_t max, const char *what, EnvForm form = ENV_STRICT) {
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    char *end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (*end || (form == ENV_STRICT && (*e < '0' || *e > '9')) || v < min || v > max) throw std::invalid_argument(std::string(name) + ": " + what + " expected");
    return v;
}

// on: set, not empty and not "0"
inline bool env_switch(const char *name) {
    const char *e = getenv(name);
    return e && *e && strcmp(e, "0") != 0;
}

constexpr uint32_t NO_BAD_POINT = 0xFFFFFFFFu;

// What is wrong with a row's first bad point, from the words of the point pass: h[k] is the lowest index that fails check
// k (0: a coordinate not below q, 1: off the curve, 2: outside the subgroup, 3: at infinity where that is not legal),
// NO_BAD_POINT when none does.  kind 0: no bad point; else k + 1 of the FIRST word that holds the lowest index: a point off
// the curve has no meaningful subgroup verdict.  (A point at infinity trips no other word, so its place in the order is free.)
struct BadPoint {
    uint32_t kind, index;
};
inline BadPoint lowest_bad(const uint32_t h[4]) {
    BadPoint b{0, NO_BAD_POINT};
    for (uint32_t k = 0; k < 4; k++)
        if (h[k] < b.index) b = BadPoint{k + 1, h[k]};
    return b;
}
constexpr const char *KIND_TEXT[5] = {"", "has a coordinate that is not below q", "is not on the curve", "is not in the subgroup", "is the point at infinity"};

// w_(2^28), standard form (ntt.hip and nttpair.hip keep the device's copies), and the 2^log_n-th root zk_fr_ntt uses
// (log_n <= 28, Montgomery): the host's, for ptau_prepare.hip, ptau_check.hip, frscan.hip and the PLONK units, and for the
// programs that read or write a PLONK key file, whose `w` it is
constexpr uint32_t ROOT_2_28_STD[8] = {0x725b19f0u, 0x9bd61b6eu, 0x41112ed4u, 0x402d111eu, 0x8ef62abcu, 0x00e0a7ebu, 0xa58a7e85u, 0x2a3c09f0u};
inline Fr root_of_unity(uint32_t log_n) {
    Fr w;
    for (int i = 0; i < 8; i++) w.v[i] = ROOT_2_28_STD[i];
    w = Fr::to_mont(w);
    for (uint32_t i = log_n; i < 28; i++) w = Fr::sqr(w);
    return w;
}

// a 32-byte little-endian scalar is 0 or 1: no check scalar
inline bool is_0_or_1(const uint8_t s32[32]) {
    bool small = s32[0] < 2;
    for (int i = 1; i < 32 && small; i++) small = s32[i] == 0;
    return small;
}

}   // namespace zk
