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
//
// plonkprover <circuit.r1cs> <pot.ptau> <w1.wtns> <p1.json> <pub1.json> <w2.wtns> <p2.json> <pub2.json> ..
//
// Several witnesses of the one circuit, a triple each, in ONE zk_plonk_prove_r1cs_many (ZKHIP_PLONK_PROVE_BATCH proofs share a
// round's multiplication).  Every file is read and matched before the device is touched.  A witness the prover refuses is named
// on stderr ("INVALID: <w.wtns>: <why>") and its two files are not written; the others' are, and the exit code is then 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
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

// What every form of the program does first: the files are read and matched before the device is touched, then the circuit is
// compiled, the kzg made over the .ptau's points and the prover over both
struct Job {
    std::unique_ptr<BinFileUtils::BinFile> r1cs, ptau;
    std::vector<std::unique_ptr<BinFileUtils::BinFile>> wtns;
    std::vector<const uint8_t *> values;                // a witness's values, nVars of them
    uint32_t nVars = 0, nPublic = 0;
    Handles h;
};

void open_job(Job &j, const std::string &r1csPath, const std::string &ptauPath, const std::vector<std::string> &wtnsPaths) {
    j.r1cs = BinFileUtils::openExisting(r1csPath, "r1cs", 1);
    auto rh = R1csUtils::loadHeader(j.r1cs.get());
    j.ptau = BinFileUtils::openExisting(ptauPath, "ptau", 1);
    auto ph = PtauUtils::loadHeader(j.ptau.get());
    for (const std::string &path : wtnsPaths) {
        j.wtns.push_back(BinFileUtils::openExisting(path, "wtns", 2));
        auto wh = WtnsUtils::loadHeader(j.wtns.back().get());
        if (!U256::is_bn254_r(wh->prime)) throw std::invalid_argument("different wtns curve");
        if (wh->nVars != rh->nWires || j.wtns.back()->getSectionSize(2) < uint64_t(wh->nVars) * 32)
            throw std::invalid_argument("witness does not match the r1cs (nVars " + std::to_string(wh->nVars) + ", nWires " + std::to_string(rh->nWires) + ")");
        j.values.push_back(static_cast<const uint8_t *>(j.wtns.back()->getSectionData(2)));
        j.nVars = wh->nVars;
    }
    if (!ph->powers[0] || !ph->powers[1]) throw std::invalid_argument("the ptau has no section 2 or 3");
    j.nPublic = rh->nPubOut + rh->nPubIn;

    const int32_t device = device_from_env();
    Handles &h = j.h;
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
}

void write_files(const uint8_t proof[ZK_PLONK_PROOF_BYTES], const uint8_t *values, uint32_t nPublic, const std::string &proofPath, const std::string &publicPath) {
    const std::string pj = proof_json(proof);
    std::vector<char> pub(zk_public_to_json(values, nPublic, nullptr, 0) + 1);
    zk_public_to_json(values, nPublic, pub.data(), pub.size());
    OutFile fp(proofPath), fq(publicPath);
    fp.write(pj.data(), pj.size());
    fq.write(pub.data(), strlen(pub.data()));
    fp.commit();
    fq.commit();
}

int run(const std::string &r1csPath, const std::string &ptauPath, const std::string &wtnsPath, const std::string &proofPath, const std::string &publicPath) {
    Job j;
    open_job(j, r1csPath, ptauPath, {wtnsPath});
    Handles &h = j.h;
    const uint8_t *values = j.values[0];
    const uint32_t nPublic = j.nPublic;

    uint8_t proof[ZK_PLONK_PROOF_BYTES];
    if (zk_plonk_prove_r1cs(h.prover, proof, values, j.nVars, nullptr) != 0) {
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
    write_files(proof, values, nPublic, proofPath, publicPath);
    return 0;
}

// Several witnesses of one circuit: argv[3 ..] holds a triple <w.wtns> <proof.json> <public.json> a witness.  One
// zk_plonk_prove_r1cs_many; a refused witness is named on stderr, its two files are not written, and once the others' are the
// exit code is a refused witness's
int run_many(int argc, char **argv) {
    const uint32_t m = (uint32_t)(argc - 3) / 3;
    std::vector<std::string> wtnsPaths;
    for (uint32_t i = 0; i < m; i++) wtnsPaths.push_back(argv[3 + 3 * i]);
    Job j;
    open_job(j, argv[1], argv[2], wtnsPaths);
    Handles &h = j.h;
    std::vector<uint8_t> all((size_t)m * j.nVars * 32), proofs((size_t)m * ZK_PLONK_PROOF_BYTES);
    for (uint32_t i = 0; i < m; i++) memcpy(all.data() + (size_t)i * j.nVars * 32, j.values[i], (size_t)j.nVars * 32);
    std::vector<uint32_t> status(m, 0);
    must(zk_plonk_prove_r1cs_many(h.prover, m, proofs.data(), status.data(), all.data(), j.nVars, nullptr));
    const char *sv = getenv("ZKHIP_SELFVERIFY");
    if (sv && strcmp(sv, "1") == 0) {
        zk_plonk_vkey vk;
        memset(&vk, 0, sizeof vk);
        vk.size = sizeof vk;
        must(zk_plonk_prover_vkey(h.prover, &vk));
        for (uint32_t i = 0; i < m; i++) {
            if (status[i] != ZK_PLONK_MANY_MADE) continue;
            uint8_t verdict = ZK_VERIFY_MALFORMED;
            must(zk_plonk_verify(h.kzg, &vk, proofs.data() + (size_t)i * ZK_PLONK_PROOF_BYTES, j.nPublic ? j.values[i] + 32 : nullptr, &verdict));
            if (verdict != ZK_VERIFY_OK)
                throw std::runtime_error("ZKHIP_SELFVERIFY: the proof of " + wtnsPaths[i] + " does not verify (verdict " + std::to_string(verdict) + ")");
        }
    }
    static const char *const why[5] = {"", "a denominator of the permutation product is zero", "the copy constraints do not hold",
                                       "the witness does not satisfy the gates", "a value is not below r"};
    int rc = 0;
    for (uint32_t i = 0; i < m; i++) {
        if (status[i] != ZK_PLONK_MANY_MADE) {
            std::cerr << "INVALID: " << wtnsPaths[i] << ": " << (status[i] < 5 ? why[status[i]] : "refused") << "\n";
            rc = 1;
            continue;
        }
        write_files(proofs.data() + (size_t)i * ZK_PLONK_PROOF_BYTES, j.values[i], j.nPublic, argv[4 + 3 * i], argv[5 + 3 * i]);
    }
    return rc;
}

}   // namespace

int main(int argc, char **argv) {
    return cli_main(argc >= 6 && argc % 3 == 0, "plonkprover <circuit.r1cs> <pot.ptau> <witness.wtns> <proof.json> <public.json>",
                    [&] { return argc == 6 ? run(argv[1], argv[2], argv[3], argv[4], argv[5]) : run_many(argc, argv); });
}
