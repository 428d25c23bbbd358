// plonkvkey <circuit.r1cs> <pot.ptau> <verification_key.json>
//
// The verification key of the PLONK circuit `plonkprover` proves: the circuit is compiled on the device exactly as there
// (libzkhip zk_plonk_r1cs_*, k1 = 2, k2 = 3), the eight commitments are made over the .ptau's section 2
// (zk_plonk_prover_create_r1cs, zk_plonk_prover_vkey), and the key is written with the field names of snarkjs's
// verification_key.json for PLONK (vkjson.hpp: protocol plonk, curve bn128, nPublic, power, k1, k2, Qm Ql Qr Qo Qc S1 S2 S3,
// X_2, w).  `plonkverifier` reads it; so does PlonkVKey.from_json.  The counterpart is snarkjs `zkey export
// verificationkey` after `plonk setup`; the key is one of THIS project's compile and transcript (include/zkhip.h): parity
// with snarkjs is unpinned.  Exit codes: 0 the key is written; 255 with a message on stderr for anything else: usage, an
// unreadable or ill-formed file, a .ptau too small for the circuit, no device.  Both files are read and matched before the
// device is touched.  ZKHIP_DEVICE=<n> picks the device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>

#include "../../include/zkhip.h"
#include "../csrc/hostutil.hpp"
#include "cli.hpp"
#include "outfile.hpp"
#include "vkjson.hpp"
#include "zkfile.hpp"

namespace {

struct Handles {                                       // destroyed in the order the borrowing asks for
    zk_plonk_prover *prover = nullptr;
    zk_plonk_r1cs *circuit = nullptr;
    zk_kzg *kzg = nullptr;
    ~Handles() {
        zk_plonk_prover_destroy(prover);
        zk_plonk_r1cs_destroy(circuit);
        zk_kzg_destroy(kzg);
    }
};

void must(int rc) {
    if (rc != 0) throw std::runtime_error(zk_last_error());
}

int run(const std::string &r1csPath, const std::string &ptauPath, const std::string &keyPath) {
    auto r1cs = BinFileUtils::openExisting(r1csPath, "r1cs", 1);
    auto rh = R1csUtils::loadHeader(r1cs.get());
    auto ptau = BinFileUtils::openExisting(ptauPath, "ptau", 1);
    auto ph = PtauUtils::loadHeader(ptau.get());
    if (!ph->powers[0] || !ph->powers[1]) throw std::invalid_argument("the ptau has no section 2 or 3");

    const int32_t device = device_from_env();
    Handles h;
    uint8_t k1[32] = {2}, k2[32] = {3};
    const zk_r1cs_view view = rh->view();
    must(zk_plonk_r1cs_create(&h.circuit, &view, k1, k2, device));
    zk_plonk_r1cs_plan plan;
    memset(&plan, 0, sizeof plan);
    plan.size = sizeof plan;
    must(zk_plonk_r1cs_info(h.circuit, &plan));
    const uint64_t n = 1ull << plan.log_n;
    if (n + 6 > (2ull << ph->power) - 1)
        throw std::invalid_argument("the ptau is too small: the circuit compiles to " + std::to_string(plan.rows) + " rows, n + 6 = " + std::to_string(n + 6) +
                                    " points are needed, power " + std::to_string(ph->power) + " has " + std::to_string((2ull << ph->power) - 1));
    zk_kzg_view kv;
    memset(&kv, 0, sizeof kv);
    kv.power = ph->power;
    kv.tau_g1 = ph->powers[0], kv.tau_g1_bytes = ph->powersBytes[0];
    kv.tau_g2 = ph->powers[1], kv.tau_g2_bytes = ph->powersBytes[1];
    must(zk_kzg_create(&h.kzg, &kv, n + 6, ZK_KZG_NO_LAGRANGE, device));
    must(zk_plonk_prover_create_r1cs(&h.prover, h.kzg, h.circuit, nullptr, -1));
    zk_plonk_vkey vk;
    memset(&vk, 0, sizeof vk);
    vk.size = sizeof vk;
    must(zk_plonk_prover_vkey(h.prover, &vk));

    const zk::Fr w = zk::Fr::from_mont(zk::root_of_unity(vk.log_n));
    const std::string j = plonk_verification_key_json(vk, U256::to_dec(vk.k1), U256::to_dec(vk.k2), U256::to_dec(reinterpret_cast<const uint8_t *>(w.v)));
    OutFile f(keyPath);
    f.write(j.data(), j.size());
    f.commit();
    return 0;
}

}   // namespace

int main(int argc, char **argv) {
    return cli_main(argc == 4, "plonkvkey <circuit.r1cs> <pot.ptau> <verification_key.json>", [&] { return run(argv[1], argv[2], argv[3]); });
}
