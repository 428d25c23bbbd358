// The R1CS witness check of the host programs (`wtnscheck`, and `prover` with ZKHIP_R1CS): a checker built from a mapped
// .r1cs through libzkhip's zk_r1cs_* entry points.  Nothing in the reference corresponds to it (snarkjs `wtns check`).
#pragma once
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

#include "../../include/zkhip.h"
#include "zkfile.hpp"

namespace R1csCheck {

struct Checker {
    zk_r1cs *h = nullptr;
    std::unique_ptr<BinFileUtils::BinFile> file;
    std::unique_ptr<R1csUtils::Header> header;
    Checker(const std::string &path, int32_t device) {
        file = BinFileUtils::openExisting(path, "r1cs", 1);
        header = R1csUtils::loadHeader(file.get());
        const zk_r1cs_view v = header->view();
        if (zk_r1cs_create(&h, &v, device) != 0) throw std::runtime_error(zk_last_error());
    }
    ~Checker() { zk_r1cs_destroy(h); }
    Checker(const Checker &) = delete;
    Checker &operator=(const Checker &) = delete;

    zk_r1cs_report check(const uint8_t *witness, uint32_t nVars) {
        zk_r1cs_report rep;
        memset(&rep, 0, sizeof rep);
        rep.size = sizeof rep;
        if (zk_r1cs_check(h, witness, nVars, &rep) != 0) throw std::runtime_error(zk_last_error());
        return rep;
    }
};

inline bool passed(const zk_r1cs_report &r) { return r.failed == 0 && r.one_ok && r.first_unreduced == UINT32_MAX; }

// one line naming what is wrong first: w[0], an unreduced value, then the lowest failing constraint
inline std::string first_problem(const zk_r1cs_report &r, uint32_t nConstraints) {
    if (!r.one_ok) return "witness w[0] is not 1";
    if (r.first_unreduced != UINT32_MAX) return "witness value w[" + std::to_string(r.first_unreduced) + "] is not below r";
    return "witness fails constraint " + std::to_string(r.first_failed) + " (" + std::to_string(r.failed) + " of " +
           std::to_string(nConstraints) + " constraints fail)";
}

}   // namespace R1csCheck
