// ptauprepare <in.ptau> <out.ptau>
//
// Prepares a Powers of Tau file for phase 2 on the GPU (libzkhip zk_ptau_prepare): what snarkjs `powersoftau prepare
// phase2 in.ptau out.ptau` does, the Lagrange-basis sections 12 to 15 from the powers in sections 2 to 5, so that `zkeynew`
// takes a ceremony's own output.  The reference has no such program.  <out> holds the magic and version of <in>, its
// sections 1 to 7 byte for byte in <in>'s order, then sections 12, 13, 14, 15; other sections of <in> are not copied.  Both
// files are mapped, never read whole; the library writes each section into the output's mapping as it finishes it.  The
// input is checked before the device is touched; the output is written as <out>.partial and renamed at the end, so that a
// failure leaves no file behind.  Exit codes: 0, or 255 with a message on stderr (as `zkeynew`).  ZKHIP_DEVICE=<n> picks
// the device.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "../../include/zkhip.h"
#include "outfile.hpp"
#include "zkfile.hpp"

namespace {

int run(const std::string &inPath, const std::string &outPath) {
    struct stat a, b;
    if (stat(inPath.c_str(), &a) == 0 && stat(outPath.c_str(), &b) == 0 && a.st_dev == b.st_dev && a.st_ino == b.st_ino)
        throw std::invalid_argument("the input and the output are the same file");
    auto ptau = BinFileUtils::openExisting(inPath, "ptau", 1);
    char magicVersion[8];                                  // copied as they are
    if (!std::ifstream(inPath, std::ios::binary).read(magicVersion, 8)) throw std::runtime_error("cannot read " + inPath);
    auto ph = PtauUtils::loadHeader(ptau.get());
    if (ph->lagrange[0] && ph->lagrange[1] && ph->lagrange[2] && ph->lagrange[3])
        throw std::invalid_argument("the ptau file is already prepared for phase 2 (it has sections 12 to 15)");
    zk_ptau_powers_view pv{};
    pv.power = ph->power;
    pv.tau_g1 = ph->powers[0];
    pv.tau_g2 = ph->powers[1];
    pv.alpha_tau_g1 = ph->powers[2];
    pv.beta_tau_g1 = ph->powers[3];
    pv.tau_g1_bytes = ph->powersBytes[0];
    pv.tau_g2_bytes = ph->powersBytes[1];
    pv.alpha_tau_g1_bytes = ph->powersBytes[2];
    pv.beta_tau_g1_bytes = ph->powersBytes[3];
    zk_ptau_lagrange_sizes sz{};
    if (zk_ptau_prepare_sizes(&pv, &sz) != 0) throw std::invalid_argument(zk_last_error());

    struct Sec {
        uint32_t id;
        const uint8_t *data;
        uint64_t size;
    };
    std::vector<Sec> keep;                                 // sections 1 to 7, in the input's order
    for (uint32_t id = 1; id <= 7; id++)
        if (ptau->hasSection(id)) keep.push_back({id, static_cast<const uint8_t *>(ptau->getSectionData(id)), ptau->getSectionSize(id)});
    std::sort(keep.begin(), keep.end(), [](const Sec &x, const Sec &y) { return x.data < y.data; });
    const Sec made[4] = {{12, nullptr, sz.lagrange_g1_bytes}, {13, nullptr, sz.lagrange_g2_bytes}, {14, nullptr, sz.lagrange_alpha_g1_bytes},
                         {15, nullptr, sz.lagrange_beta_g1_bytes}};
    uint64_t total = 12;
    for (const auto &s : keep) total += 12 + s.size;
    for (const auto &s : made) total += 12 + s.size;

    MappedOutFile o(outPath, total);
    uint8_t *at = o.data;
    const uint32_t count = (uint32_t)keep.size() + 4;
    memcpy(at, magicVersion, 8);
    memcpy(at + 8, &count, 4);
    at += 12;
    auto head = [&](const Sec &s) {
        memcpy(at, &s.id, 4);
        memcpy(at + 4, &s.size, 8);
        at += 12;
    };
    for (const auto &s : keep) {
        head(s);
        memcpy(at, s.data, s.size);
        at += s.size;
    }
    uint8_t *dst[4];
    for (int i = 0; i < 4; i++) {
        head(made[i]);
        dst[i] = at;
        at += made[i].size;
    }
    zk_ptau_lagrange_out out{dst[0], dst[1], dst[2], dst[3]};
    const char *dev = getenv("ZKHIP_DEVICE");
    if (zk_ptau_prepare(&pv, dev ? atoi(dev) : -1, &out) != 0) throw std::runtime_error(zk_last_error());
    o.commit();
    std::cerr << "ptauprepare: power " << ph->power << ", sections 12 to 15: "
              << (sz.lagrange_g1_bytes + sz.lagrange_g2_bytes + sz.lagrange_alpha_g1_bytes + sz.lagrange_beta_g1_bytes) << " bytes\n";
    return 0;
}

}   // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        std::cerr << "Invalid number of parameters:\n";
        std::cerr << "Usage: ptauprepare <in.ptau> <out.ptau>\n";
        return -1;
    }
    try {
        return run(argv[1], argv[2]);
    } catch (std::exception &e) {
        std::cerr << e.what() << '\n';
        return -1;
    }
}
