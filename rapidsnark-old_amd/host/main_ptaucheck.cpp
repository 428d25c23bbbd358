// ptaucheck <file.ptau>
//
// Is this Powers of Tau file sound?  The check of libzkhip's zk_ptau_check on the GPU: every point on its curve and (G2)
// in the subgroup, sections 2 to 5 sequences of powers of one tau (times alpha, beta), section 6 the beta of section 5,
// and, when the file is prepared for phase 2, sections 12 to 15 the Lagrange form of those powers.  The arithmetic half of
// snarkjs `powersoftau verify`; the reference has no such program.  NOT checked: the contribution transcript of section 7
// (challenge hashes, proofs of knowledge), and so not that anybody honest ever contributed.  The file is mapped, never
// read whole, and its shape is checked before the device is touched.  Exit codes, as `wtnscheck` / `verifier`: 0 with
// "OK: ..." on stdout; 1 with "INVALID: ..." on stdout, one line per failed equation or the malformed point; 255 with a
// message on stderr for everything else (bad file, no device).  ZKHIP_DEVICE=<n> picks the device.  For tests only,
// ZKHIP_PTAU_CHECK_SCALAR=<decimal> fixes the scalar of the random combination (0, 1 and values >= r are refused).
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>

#include "../../include/zkhip.h"
#include "cli.hpp"
#include "zkfile.hpp"

namespace {

const char *section_name(uint32_t sec) {
    switch (sec) {
    case 2: return "tauG1";
    case 3: return "tauG2";
    case 4: return "alphaTauG1";
    case 5: return "betaTauG1";
    case 6: return "betaG2";
    }
    return "";
}

int run(const std::string &path) {
    auto ptau = BinFileUtils::openExisting(path, "ptau", 1);
    ptau->startReadSection(1);
    if (ptau->readU32LE() != 32) throw std::invalid_argument("ptau: only 256-bit fields are supported");
    U256::Bytes q;
    memcpy(q.data(), ptau->read(32), 32);
    if (!U256::is_bn254_q(q)) throw std::invalid_argument("ptau curve not supported (q is not BN254's)");
    zk_ptau_file_view v{};
    v.power = ptau->readU32LE();
    ptau->endReadSection(false);
    for (uint32_t sec : {2u, 3u, 4u, 5u, 6u, 12u, 13u, 14u, 15u})
        if (ptau->hasSection(sec)) {
            v.sec[sec] = ptau->getSectionData(sec);
            v.sec_bytes[sec] = ptau->getSectionSize(sec);
        }
    zk_ptau_check_sizes_t sz{};
    if (zk_ptau_check_sizes(&v, &sz) != 0) throw std::invalid_argument(zk_last_error());

    uint8_t s32[32];
    const uint8_t *fixed = nullptr;
    if (const char *e = getenv("ZKHIP_PTAU_CHECK_SCALAR")) {
        uint8_t one[32] = {1};
        if (!U256::from_dec(e, s32) || !U256::less(one, s32) || !U256::less(s32, U256::kBn254R.data()))
            throw std::invalid_argument("ZKHIP_PTAU_CHECK_SCALAR: a decimal number from 2 to r - 1 expected");
        fixed = s32;
    }
    zk_ptau_report rep{};
    if (zk_ptau_check(&v, fixed, device_from_env(), &rep) != 0) throw std::runtime_error(zk_last_error());

    const char *lag = sz.prepared ? "the Lagrange sections 12 to 15 are present and were checked" : "no Lagrange sections 12 to 15 (the file is not prepared for phase 2)";
    if (rep.verdict == 0) {
        std::cout << "OK: power " << v.power << ", sections 2 to 6 are powers of one tau; " << lag << "; the contribution transcript is not checked\n";
        return 0;
    }
    if (rep.verdict == 2) {
        static const char *const kind[5] = {"", "has a coordinate that is not below q", "is not on the curve", "is not in the subgroup", "is the point at infinity"};
        std::cout << "INVALID: section " << rep.bad_section << ": point " << rep.bad_index << " " << kind[rep.bad_kind <= 4 ? rep.bad_kind : 0] << "\n";
        return 1;
    }
    if (rep.failed & 1u) std::cout << "INVALID: section 2 or 3 does not start with the generator of its group\n";
    for (uint32_t sec = 2; sec <= 5; sec++)
        if (rep.failed >> sec & 1u) std::cout << "INVALID: section " << sec << " (" << section_name(sec) << ") is not a sequence of powers of the file's tau\n";
    if (rep.failed >> 6 & 1u) std::cout << "INVALID: section 6 (betaG2) is not the beta of section 5\n";
    for (uint32_t i = 0; i < 4; i++)
        for (uint32_t p = 0; p < 32; p++)
            if (rep.lagrange_failed[i] >> p & 1u) std::cout << "INVALID: section " << 12 + i << ", level " << p << " is not the Lagrange form of section " << 2 + i << "\n";
    return 1;
}

}   // namespace

int main(int argc, char **argv) {
    return cli_main(argc == 2, "ptaucheck <file.ptau>", [&] { return run(argv[1]); });
}
