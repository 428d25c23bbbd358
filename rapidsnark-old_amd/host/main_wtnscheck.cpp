// wtnscheck <circuit.r1cs> <witness.wtns>
//
// Checks a witness against every constraint of circom's .r1cs on the GPU (libzkhip zk_r1cs_*), the counterpart of snarkjs
// `wtns check`; the reference has no such program.  Exit codes: 0 every constraint holds, w[0] = 1 and every value is below
// r; 1 the witness fails (the first failing constraint with its A.w / B.w / C.w in decimal, and how many fail, on stdout);
// 255 a bad file, mismatched sizes or no device (message on stderr, as `prover`).  ZKHIP_DEVICE=<n> picks the device.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <string>

#include "cli.hpp"
#include "r1cs_check.hpp"
#include "zkfile.hpp"

namespace {

int run(const std::string &r1csPath, const std::string &wtnsPath) {
    // both files are read and matched before the device is touched
    auto r1cs = BinFileUtils::openExisting(r1csPath, "r1cs", 1);
    auto rh = R1csUtils::loadHeader(r1cs.get());
    auto wtns = BinFileUtils::openExisting(wtnsPath, "wtns", 2);
    auto wh = WtnsUtils::loadHeader(wtns.get());
    if (!U256::is_bn254_r(wh->prime)) throw std::invalid_argument("different wtns curve");
    if (wh->nVars != rh->nWires || wtns->getSectionSize(2) < uint64_t(wh->nVars) * 32)
        throw std::invalid_argument("witness does not match the r1cs (nVars " + std::to_string(wh->nVars) + ", nWires " + std::to_string(rh->nWires) + ")");
    R1csCheck::Checker checker(r1csPath, device_from_env());
    const zk_r1cs_report rep = checker.check(static_cast<const uint8_t *>(wtns->getSectionData(2)), wh->nVars);
    if (R1csCheck::passed(rep)) {
        std::cout << "witness OK: " << rh->nConstraints << " constraints hold\n";
        return 0;
    }
    if (!rep.one_ok) std::cout << "w[0] is not 1\n";
    if (rep.first_unreduced != UINT32_MAX) std::cout << "w[" << rep.first_unreduced << "] is not below r\n";
    if (rep.failed) {
        std::cout << "constraint " << rep.first_failed << " fails: A.w = " << U256::to_dec(rep.a) << ", B.w = " << U256::to_dec(rep.b)
                  << ", C.w = " << U256::to_dec(rep.c) << "\n";
        std::cout << rep.failed << " of " << rh->nConstraints << " constraints fail\n";
    }
    return 1;
}

}   // namespace

int main(int argc, char **argv) {
    return cli_main(argc == 3, "wtnscheck <circuit.r1cs> <witness.wtns>", [&] { return run(argv[1], argv[2]); });
}
