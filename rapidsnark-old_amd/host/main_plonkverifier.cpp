// plonkverifier <verification_key.json> <public.json> <proof.json>
//
// Verifies a PLONK proof on the GPU from the key alone (libzkhip zk_plonk_verifier_*: no .ptau), the counterpart of snarkjs
// `plonk verify`; the reference has no such program.  The key is what `plonkvkey` writes (snarkjs's field names: protocol
// plonk, curve bn128 / bn254, nPublic, power, k1, k2, Qm Ql Qr Qo Qc S1 S2 S3, X_2, w), the proof what `plonkprover` writes
// (A B C Z T1 T2 T3 Wxi Wxiw, eval_a eval_b eval_c eval_s1 eval_s2 eval_zw).  Points are decimal strings (or bare numbers); a
// third projective coordinate is honoured: 0 is the point at infinity (0 1 0), anything else divides x and y.  public.json
// may be `null`.  The key names a key of THIS project's compile and transcript (include/zkhip.h): a key made by snarkjs
// parses when its w is this library's root of unity for its power, but proofs made by snarkjs are not promised to verify.
// Exit codes: 0 "OK: the proof verifies"; 1 "INVALID: ..." on stdout, saying whether the proof is malformed (a point off the
// curve, a coordinate not below q, a value or a public signal not below r) or well-formed with a failing pairing equation;
// 255 with a message on stderr for anything else: usage, an unreadable or ill-formed file, another protocol or curve, a w
// that is not the library's, a number of public signals that is not the key's, a key the library refuses, no device.  All
// three files are read and matched before the device is touched.  ZKHIP_DEVICE=<n> picks the device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/zkhip.h"
#include "../csrc/hostutil.hpp"
#include "cli.hpp"
#include "jsonpoints.hpp"
#include "zkfile.hpp"

namespace {

using namespace JsonPoints;

void protocol_and_curve(const Value &j, const std::string &path) {
    if (const Value *p = j.find("protocol"))
        if (p->text != "plonk") throw std::invalid_argument(path + ": protocol \"" + p->text + "\" is not plonk");
    if (const Value *c = j.find("curve"))
        if (c->text != "bn128" && c->text != "bn254") throw std::invalid_argument(path + ": curve \"" + c->text + "\" is not bn128");
}

// a decimal integer below 2^64
uint64_t small(const Value &v, const std::string &what) {
    uint8_t b[32];
    decimal(v, what, b);
    for (int i = 8; i < 32; i++)
        if (b[i]) throw std::invalid_argument(what + " is not below 2^64");
    uint64_t x;
    memcpy(&x, b, 8);
    return x;
}

void key_from_json(const std::string &path, zk_plonk_vkey &vk) {
    const Value j = parse_file(path);
    if (j.type != Value::Object) throw std::invalid_argument(path + ": a key object expected");
    protocol_and_curve(j, path);
    memset(&vk, 0, sizeof vk);
    vk.size = sizeof vk;
    const uint64_t power = small(member(j, "power", path), path + ": power");
    if (power > 28) throw std::invalid_argument(path + ": power " + std::to_string(power) + " is outside 0 .. 28");
    vk.log_n = (uint32_t)power;
    vk.n_public = small(member(j, "nPublic", path), path + ": nPublic");
    decimal(member(j, "k1", path), path + ": k1", vk.k1);
    decimal(member(j, "k2", path), path + ": k2", vk.k2);
    uint8_t w[32];
    decimal(member(j, "w", path), path + ": w", w);
    const zk::Fr root = zk::Fr::from_mont(zk::root_of_unity(vk.log_n));
    if (memcmp(w, root.v, 32) != 0) throw std::invalid_argument(path + ": w is not this library's root of unity for power " + std::to_string(power));
    uint8_t *pts[8] = {vk.qm, vk.ql, vk.qr, vk.qo, vk.qc, vk.s1, vk.s2, vk.s3};
    static const char *const names[8] = {"Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3"};
    for (int i = 0; i < 8; i++) g1_point(member(j, names[i], path), names[i], pts[i]);
    g2_point(member(j, "X_2", path), "X_2", vk.tau_g2);
}

int run(const std::string &keyPath, const std::string &publicPath, const std::string &proofPath) {
    // the three files are read and matched before the device is touched
    zk_plonk_vkey vk;
    key_from_json(keyPath, vk);

    const Value pub = parse_file(publicPath);
    if (pub.type != Value::Null && pub.type != Value::Array) throw std::invalid_argument(publicPath + ": a list of public signals (or null) expected");
    std::vector<uint8_t> publics(pub.items.size() * 32);
    for (size_t i = 0; i < pub.items.size(); i++) decimal(pub.items[i], publicPath + ": public signal " + std::to_string(i), publics.data() + 32 * i);
    if (vk.n_public != pub.items.size())
        throw std::invalid_argument("the verification key is for " + std::to_string(vk.n_public) + " public signals, " + publicPath + " holds " +
                                    std::to_string(pub.items.size()));

    const Value pj = parse_file(proofPath);
    if (pj.type != Value::Object) throw std::invalid_argument(proofPath + ": a proof object expected");
    protocol_and_curve(pj, proofPath);
    uint8_t proof[ZK_PLONK_PROOF_BYTES];
    static const char *const points[9] = {"A", "B", "C", "Z", "T1", "T2", "T3", "Wxi", "Wxiw"};
    static const char *const evals[6] = {"eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw"};
    for (int i = 0; i < 9; i++) g1_point(member(pj, points[i], proofPath), points[i], proof + 64 * i);
    for (int i = 0; i < 6; i++) decimal(member(pj, evals[i], proofPath), proofPath + ": " + evals[i], proof + 576 + 32 * i);

    zk_plonk_verifier *v = nullptr;
    if (zk_plonk_verifier_create(&v, &vk, device_from_env()) != 0) throw std::runtime_error(zk_last_error());
    uint8_t verdict = ZK_VERIFY_MALFORMED;
    const int rc = zk_plonk_verifier_verify(v, proof, publics.empty() ? nullptr : publics.data(), 1, &verdict);
    const std::string err = rc ? zk_last_error() : "";
    zk_plonk_verifier_destroy(v);
    if (rc != 0) throw std::runtime_error(err);
    if (verdict == ZK_VERIFY_OK) {
        std::cout << "OK: the proof verifies\n";
        return 0;
    }
    if (verdict == ZK_VERIFY_MALFORMED)
        std::cout << "INVALID: the proof is malformed (a point off the curve, a coordinate that is not below q, or a value or public signal that is not below r)\n";
    else
        std::cout << "INVALID: the proof is well-formed but the pairing equation does not hold\n";
    return 1;
}

}   // namespace

int main(int argc, char **argv) {
    return cli_main(argc == 4, "plonkverifier <verification_key.json> <public.json> <proof.json>", [&] { return run(argv[1], argv[2], argv[3]); });
}
