// zkeynew <circuit.r1cs> <pot.ptau> <circuit.zkey> [verification_key.json]
//
// The phase-2 starting key of a circom circuit from a prepared Powers of Tau file, on the GPU (libzkhip
// zk_groth16_setup): what snarkjs `groth16 setup` (alias `zkey new`) writes, gamma = delta = 1, with section 10 (csHash and
// contributions) all zero.  The reference has no such program.  Both files are read and checked against each other
// before the device is touched; the outputs are written to temporary names and renamed at the end, so that a failure
// leaves no file behind.  Exit codes: 0, or 255 with a message on stderr (as `prover`).  ZKHIP_DEVICE=<n> picks the device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/zkhip.h"
#include "../csrc/common.hpp"
#include "cli.hpp"
#include "outfile.hpp"
#include "vkjson.hpp"
#include "zkfile.hpp"

namespace {

// the generators of G1, (1, 2), and of G2 (EIP-197), affine Montgomery: gamma2 = delta2 = G2, delta1 = G1
void generators(uint8_t g1[64], uint8_t g2[128]) {
    auto put = [](uint8_t *out, uint64_t a, uint64_t b, uint64_t c, uint64_t d) { memcpy(out, fq_mont(a, b, c, d).v, 32); };
    put(g1, 1, 0, 0, 0);
    put(g1 + 32, 2, 0, 0, 0);
    put(g2, 0x46debd5cd992f6edull, 0x674322d4f75edaddull, 0x426a00665e5c4479ull, 0x1800deef121f1e76ull);
    put(g2 + 32, 0x97e485b7aef312c2ull, 0xf1aa493335a9e712ull, 0x7260bfb731fb5d25ull, 0x198e9393920d483aull);
    put(g2 + 64, 0x4ce6cc0166fa7daaull, 0xe3d1e7690c43d37bull, 0x4aab71808dcb408full, 0x12c85ea5db8c6debull);
    put(g2 + 96, 0x55acdadcd122975bull, 0xbc4b313370b38ef3ull, 0xec9e99ad690c3395ull, 0x090689d0585ff075ull);
}

int run(const std::string &r1csPath, const std::string &ptauPath, const std::string &zkeyPath, const std::string &vkPath) {
    // both files are read and checked against each other before the device is touched
    auto r1cs = BinFileUtils::openExisting(r1csPath, "r1cs", 1);
    auto rh = R1csUtils::loadHeader(r1cs.get());
    auto ptau = BinFileUtils::openExisting(ptauPath, "ptau", 1);
    auto ph = PtauUtils::loadHeader(ptau.get());
    zk_r1cs_view rv = rh->view();
    zk_ptau_view pv{};
    pv.power = ph->power;
    pv.alpha1 = ph->alpha1;
    pv.beta1 = ph->beta1;
    pv.beta2 = ph->beta2;
    pv.lagrange_g1 = ph->lagrange[0];
    pv.lagrange_g2 = ph->lagrange[1];
    pv.lagrange_alpha_g1 = ph->lagrange[2];
    pv.lagrange_beta_g1 = ph->lagrange[3];
    pv.lagrange_g1_bytes = ph->lagrangeBytes[0];
    pv.lagrange_g2_bytes = ph->lagrangeBytes[1];
    pv.lagrange_alpha_g1_bytes = ph->lagrangeBytes[2];
    pv.lagrange_beta_g1_bytes = ph->lagrangeBytes[3];
    zk_setup_sizes sz{};
    if (zk_groth16_setup_sizes(&rv, &pv, &sz) != 0) throw std::invalid_argument(zk_last_error());

    const ZKeyUtils::Shape shape{sz.nVars, sz.nPublic, sz.domainSize, sz.nCoefs};
    std::vector<uint8_t> ic(shape.sectionBytes(3)), coefs(shape.sectionBytes(4)), a(shape.sectionBytes(5)), b1(shape.sectionBytes(6)),
        b2(shape.sectionBytes(7)), c(shape.sectionBytes(8)), h(shape.sectionBytes(9));
    zk_setup_out out{coefs.data(), ic.data(), a.data(), b1.data(), b2.data(), c.empty() ? nullptr : c.data(), h.data()};
    if (zk_groth16_setup(&rv, &pv, device_from_env(), &out) != 0) throw std::runtime_error(zk_last_error());

    uint8_t g1[64], g2[128];
    generators(g1, g2);
    OutFile z(zkeyPath);
    z.write("zkey", 4);
    z.u32(1);
    z.u32(10);
    z.section(1, 4);
    z.u32(1);                                             // Groth16
    z.section(2, 4 + 32 + 4 + 32 + 12 + 64 + 64 + 128 + 128 + 64 + 128);
    z.u32(32);
    z.write(ph->q.data(), 32);
    z.u32(32);
    z.write(U256::kBn254R.data(), 32);
    z.u32(sz.nVars);
    z.u32(sz.nPublic);
    z.u32(sz.domainSize);
    z.write(ph->alpha1, 64);
    z.write(ph->beta1, 64);
    z.write(ph->beta2, 128);
    z.write(g2, 128);                                     // gamma2
    z.write(g1, 64);                                      // delta1
    z.write(g2, 128);                                     // delta2
    const struct {
        uint32_t id;
        const std::vector<uint8_t> &v;
    } secs[] = {{3, ic}, {4, coefs}, {5, a}, {6, b1}, {7, b2}, {8, c}, {9, h}};
    for (const auto &s : secs) {
        z.section(s.id, s.v.size());
        z.write(s.v.data(), s.v.size());
    }
    const uint8_t sec10[68] = {};                          // csHash + 0 contributions (not computed: see INTEGRATION.md)
    z.section(10, sizeof sec10);
    z.write(sec10, sizeof sec10);

    std::unique_ptr<OutFile> vk;
    if (!vkPath.empty()) {
        vk.reset(new OutFile(vkPath));
        const std::string j = verification_key_json(sz.nPublic, static_cast<const uint8_t *>(ph->alpha1), static_cast<const uint8_t *>(ph->beta2), g2, g2, ic.data());
        vk->write(j.data(), j.size());
    }
    z.commit();
    if (vk) vk->commit();
    std::cerr << "zkeynew: 2^" << sz.log_domain << " domain, " << sz.nVars << " wires, " << sz.nCoefs << " coefficients\n";
    return 0;
}

}   // namespace

int main(int argc, char **argv) {
    return cli_main(argc == 4 || argc == 5, "zkeynew <circuit.r1cs> <pot.ptau> <circuit.zkey> [verification_key.json]",
                    [&] { return run(argv[1], argv[2], argv[3], argc == 5 ? argv[4] : ""); });
}
