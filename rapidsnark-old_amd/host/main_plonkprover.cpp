// plonkprover <circuit.r1cs> <pot.ptau> <witness.wtns> <proof.json> <public.json>
//
// A PLONK proof on the GPU from the three files circom and a Powers of Tau ceremony write: the circuit is compiled to gates,
// wire maps and sigma on the device (libzkhip zk_plonk_r1cs_*, k1 = 2, k2 = 3), the commitments are made over the .ptau's
// section 2 (zk_kzg_*; n + 6 of its points, n the compiled circuit's rows rounded up to a power of two), the witness is
// extended on the device and proved (zk_plonk_prover_create_r1cs, zk_plonk_prove_r1cs).  The counterpart is snarkjs
// `plonk setup` followed by `plonk prove`; the layout of the compiled circuit is this project's own (include/zkhip.h), so the
// proof verifies under the key of THIS compile (zk_plonk_verify), not under a snarkjs-made key.  The reference has no such
// program.  proof.json: snarkjs's field names (A B C Z T1 T2 T3 Wxi Wxiw, eval_a eval_b eval_c eval_s1 eval_s2 eval_zw,
// protocol plonk, curve bn128), decimal strings, projective points with z = 1, infinity as 0 1 0.  public.json: as `prover`.
// Exit codes: 0 both files written; 1 the prover refuses the witness (a gate or a copy constraint does not hold: the text
// on stdout, no file written); 255 with a message on stderr for anything else: usage, an unreadable or ill-formed file, a
// witness of another circuit, a .ptau too small for the circuit, no device.  All three files are read and matched before the
// device is touched.  ZKHIP_SELFVERIFY=1 verifies the proof before anything is written; ZKHIP_DEVICE=<n> picks the device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/zkhip.h"
#include "../csrc/curve.hpp"
#include "cli.hpp"
#include "outfile.hpp"
#include "zkfile.hpp"

namespace {

using zk::Fq;

// a coordinate in the .ptau encoding (Montgomery) -> decimal
std::string coord_dec(const uint8_t *c) {
    Fq x;
    memcpy(x.v, c, 32);
    x = Fq::from_mont(x);
    return U256::to_dec(reinterpret_cast<const uint8_t *>(x.v));
}

// json.dumps(..., indent=1) of the proof's fields
std::string proof_json(const uint8_t proof[ZK_PLONK_PROOF_BYTES]) {
    static const char *const points[9] = {"A", "B", "C", "Z", "T1", "T2", "T3", "Wxi", "Wxiw"};
    static const char *const evals[6] = {"eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw"};
    static const uint8_t zero[64] = {0};
    std::string s = "{\n";
    for (int j = 0; j < 9; j++) {
        const uint8_t *p = proof + j * 64;
        const bool inf = memcmp(p, zero, 64) == 0;
        s += std::string(" \"") + points[j] + "\": [\n  \"" + (inf ? "0" : coord_dec(p)) + "\",\n  \"" + (inf ? "1" : coord_dec(p + 32)) + "\",\n  \"" +
             (inf ? "0" : "1") + "\"\n ],\n";
    }
    for (int j = 0; j < 6; j++) s += std::string(" \"") + evals[j] + "\": \"" + U256::to_dec(proof + 576 + j * 32) + "\",\n";
    s += " \"protocol\": \"plonk\",\n \"curve\": \"bn128\"\n}";
    return s;
}

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

int run(const std::string &r1csPath, const std::string &ptauPath, const std::string &wtnsPath, const std::string &proofPath, const std::string &publicPath) {
    // the three files are read and matched before the device is touched
    auto r1cs = BinFileUtils::openExisting(r1csPath, "r1cs", 1);
    auto rh = R1csUtils::loadHeader(r1cs.get());
    auto ptau = BinFileUtils::openExisting(ptauPath, "ptau", 1);
    auto ph = PtauUtils::loadHeader(ptau.get());
    auto wtns = BinFileUtils::openExisting(wtnsPath, "wtns", 2);
    auto wh = WtnsUtils::loadHeader(wtns.get());
    if (!U256::is_bn254_r(wh->prime)) throw std::invalid_argument("different wtns curve");
    if (wh->nVars != rh->nWires || wtns->getSectionSize(2) < uint64_t(wh->nVars) * 32)
        throw std::invalid_argument("witness does not match the r1cs (nVars " + std::to_string(wh->nVars) + ", nWires " + std::to_string(rh->nWires) + ")");
    if (!ph->powers[0] || !ph->powers[1]) throw std::invalid_argument("the ptau has no section 2 or 3");
    const uint8_t *values = static_cast<const uint8_t *>(wtns->getSectionData(2));
    const uint32_t nPublic = rh->nPubOut + rh->nPubIn;

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

    uint8_t proof[ZK_PLONK_PROOF_BYTES];
    if (zk_plonk_prove_r1cs(h.prover, proof, values, wh->nVars, nullptr) != 0) {
        const std::string err = zk_last_error();
        if (err.find("the witness does not satisfy the gates") != std::string::npos || err.find("the copy constraints do not hold") != std::string::npos) {
            std::cout << "INVALID: " << err << "\n";
            return 1;
        }
        throw std::runtime_error(err);
    }
    const char *sv = getenv("ZKHIP_SELFVERIFY");
    if (sv && strcmp(sv, "1") == 0) {
        zk_plonk_vkey vk;
        memset(&vk, 0, sizeof vk);
        vk.size = sizeof vk;
        must(zk_plonk_prover_vkey(h.prover, &vk));
        uint8_t verdict = ZK_VERIFY_MALFORMED;
        must(zk_plonk_verify(h.kzg, &vk, proof, nPublic ? values + 32 : nullptr, &verdict));
        if (verdict != ZK_VERIFY_OK) throw std::runtime_error("ZKHIP_SELFVERIFY: the proof does not verify (verdict " + std::to_string(verdict) + ")");
    }
    const std::string pj = proof_json(proof);
    std::vector<char> pub(zk_public_to_json(values, nPublic, nullptr, 0) + 1);
    zk_public_to_json(values, nPublic, pub.data(), pub.size());
    OutFile fp(proofPath), fq(publicPath);
    fp.write(pj.data(), pj.size());
    fq.write(pub.data(), strlen(pub.data()));
    fp.commit();
    fq.commit();
    return 0;
}

}   // namespace

int main(int argc, char **argv) {
    return cli_main(argc == 6, "plonkprover <circuit.r1cs> <pot.ptau> <witness.wtns> <proof.json> <public.json>",
                    [&] { return run(argv[1], argv[2], argv[3], argv[4], argv[5]); });
}
