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

#include "r1cs_check.hpp"
#include "zkfile.hpp"

namespace {

constexpr uint8_t kBn254R[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                                 0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};

int run(const std::string &r1csPath, const std::string &wtnsPath) {
    // both files are read and matched before the device is touched
    auto r1cs = BinFileUtils::openExisting(r1csPath, "r1cs", 1);
    auto rh = R1csUtils::loadHeader(r1cs.get());
    auto wtns = BinFileUtils::openExisting(wtnsPath, "wtns", 2);
    auto wh = WtnsUtils::loadHeader(wtns.get());
    if (memcmp(wh->prime.data(), kBn254R, 32) != 0) throw std::invalid_argument("different wtns curve");
    if (wh->nVars != rh->nWires || wtns->getSectionSize(2) < uint64_t(wh->nVars) * 32)
        throw std::invalid_argument("witness does not match the r1cs (nVars " + std::to_string(wh->nVars) + ", nWires " + std::to_string(rh->nWires) + ")");
    const char *dev = getenv("ZKHIP_DEVICE");
    R1csCheck::Checker checker(r1csPath, dev ? atoi(dev) : -1);
    const zk_r1cs_report rep = checker.check(static_cast<const uint8_t *>(wtns->getSectionData(2)), wh->nVars);
    if (R1csCheck::passed(rep)) {
        std::cout << "witness OK: " << rh->nConstraints << " constraints hold\n";
        return 0;
    }
    if (!rep.one_ok) std::cout << "w[0] is not 1\n";
    if (rep.first_unreduced != UINT32_MAX) std::cout << "w[" << rep.first_unreduced << "] is not below r\n";
    if (rep.failed) {
        std::cout << "constraint " << rep.first_failed << " fails: A.w = " << R1csCheck::to_dec(rep.a) << ", B.w = " << R1csCheck::to_dec(rep.b)
                  << ", C.w = " << R1csCheck::to_dec(rep.c) << "\n";
        std::cout << rep.failed << " of " << rh->nConstraints << " constraints fail\n";
    }
    return 1;
}

}   // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        std::cerr << "Invalid number of parameters:\n";
        std::cerr << "Usage: wtnscheck <circuit.r1cs> <witness.wtns>\n";
        return -1;
    }
    try {
        return run(argv[1], argv[2]);
    } catch (std::exception &e) {
        std::cerr << e.what() << '\n';
        return -1;
    }
}
