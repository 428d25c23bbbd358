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
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/zkhip.h"
#include "cli.hpp"
#include "outfile.hpp"
#include "zkfile.hpp"

namespace {

int run(const std::string &inPath, const std::string &outPath) {
    ContainerOut o(inPath, outPath);
    auto ptau = BinFileUtils::openExisting(inPath, "ptau", 1);
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

    std::vector<ContainerOut::Section> secs;               // sections 1 to 7, in the input's order, then the four new ones
    for (const auto &s : ptau->sectionsInFileOrder(1, 7)) secs.push_back({s.id, s.size, s.data});
    const size_t made = secs.size();
    secs.push_back({12, sz.lagrange_g1_bytes, nullptr});
    secs.push_back({13, sz.lagrange_g2_bytes, nullptr});
    secs.push_back({14, sz.lagrange_alpha_g1_bytes, nullptr});
    secs.push_back({15, sz.lagrange_beta_g1_bytes, nullptr});
    const std::vector<uint8_t *> at = o.write(ptau->magicVersion(), secs);
    zk_ptau_lagrange_out out{at[made], at[made + 1], at[made + 2], at[made + 3]};
    if (zk_ptau_prepare(&pv, device_from_env(), &out) != 0) throw std::runtime_error(zk_last_error());
    o.commit();
    std::cerr << "ptauprepare: power " << ph->power << ", sections 12 to 15: "
              << (sz.lagrange_g1_bytes + sz.lagrange_g2_bytes + sz.lagrange_alpha_g1_bytes + sz.lagrange_beta_g1_bytes) << " bytes\n";
    return 0;
}

}   // namespace

int main(int argc, char **argv) {
    return cli_main(argc == 3, "ptauprepare <in.ptau> <out.ptau>", [&] { return run(argv[1], argv[2]); });
}
