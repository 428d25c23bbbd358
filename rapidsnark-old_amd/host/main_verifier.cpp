// verifier <verification_key.json | circuit.zkey> <public.json> <proof.json>
//
// Verifies a Groth16 proof on the GPU (libzkhip zk_vkey_*), the counterpart of snarkjs `groth16 verify` and of the
// `verifier` the newer rapidsnark ships next to `prover` (the same argument order); the reference of this project has no
// such program.  The key is snarkjs's verification_key.json (vk_alpha_1, vk_beta_2, vk_gamma_2, vk_delta_2, IC; protocol
// groth16, curve bn128 / bn254; vk_alphabeta_12 is ignored) or a .zkey, of which only sections 1 to 3 are read.  Points are
// decimal strings (or bare numbers); a third projective coordinate is honoured: 0 is the point at infinity, anything else
// divides x and y.  public.json may be `null` (what `prover` writes for a circuit without public signals).
// Exit codes: 0 "OK: the proof verifies"; 1 "INVALID: ..." on stdout, saying whether the proof is malformed (a point off
// its curve, outside the subgroup or at infinity, a coordinate not below q, a public signal not below r) or well-formed
// with a failing pairing equation; 255 with a message on stderr for anything else: usage, an unreadable or ill-formed file,
// another protocol or curve, a number of public signals that is not the key's, no device (as `wtnscheck`).  All three
// files are read and checked before the device is touched.  ZKHIP_DEVICE=<n> picks the device.
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
#include "jsonpoints.hpp"
#include "zkfile.hpp"

namespace {

using namespace JsonPoints;       // slurp, decimal, g1_point, g2_point, member, parse_file

struct Key {
    uint8_t alpha1[64], beta2[128], gamma2[128], delta2[128];
    std::vector<uint8_t> ic;
};

void key_from_json(const std::string &path, const std::string &text, Key &k) {
    Value j;
    try {
        j = JsonMin::parse(text);
    } catch (const std::exception &e) {
        throw std::invalid_argument(path + " is neither a verification_key.json nor a .zkey (" + e.what() + ")");
    }
    if (j.type != Value::Object) throw std::invalid_argument(path + " is neither a verification_key.json nor a .zkey");
    if (const Value *p = j.find("protocol"))
        if (p->text != "groth16") throw std::invalid_argument(path + ": protocol \"" + p->text + "\" is not groth16");
    if (const Value *c = j.find("curve"))
        if (c->text != "bn128" && c->text != "bn254") throw std::invalid_argument(path + ": curve \"" + c->text + "\" is not bn128");
    g1_point(member(j, "vk_alpha_1", path), "vk_alpha_1", k.alpha1);
    g2_point(member(j, "vk_beta_2", path), "vk_beta_2", k.beta2);
    g2_point(member(j, "vk_gamma_2", path), "vk_gamma_2", k.gamma2);
    g2_point(member(j, "vk_delta_2", path), "vk_delta_2", k.delta2);
    const Value &ic = member(j, "IC", path);
    if (ic.type != Value::Array || ic.items.empty()) throw std::invalid_argument(path + ": IC is not a list of points");
    k.ic.resize(ic.items.size() * 64);
    for (size_t i = 0; i < ic.items.size(); i++) g1_point(ic.items[i], "IC[" + std::to_string(i) + "]", k.ic.data() + 64 * i);
}

void key_from_zkey(const std::string &path, Key &k) {
    auto f = BinFileUtils::openExisting(path, "zkey", 1);
    auto h = ZKeyUtils::loadHeader(f.get());
    if (!U256::is_bn254_q(h->qPrime) || !U256::is_bn254_r(h->rPrime)) throw std::invalid_argument("zkey curve not supported");
    const uint64_t want = ZKeyUtils::Shape{h->nVars, h->nPublic, h->domainSize, h->nCoefs}.sectionBytes(3);
    if (f->getSectionSize(3) != want)
        throw std::invalid_argument("zkey section 3 holds " + std::to_string(f->getSectionSize(3)) + " bytes, nPublic = " + std::to_string(h->nPublic) + " implies " +
                                    std::to_string(want));
    memcpy(k.alpha1, h->vk_alpha1, 64);
    memcpy(k.beta2, h->vk_beta2, 128);
    memcpy(k.gamma2, h->vk_gamma2, 128);
    memcpy(k.delta2, h->vk_delta2, 128);
    const uint8_t *ic = static_cast<const uint8_t *>(f->getSectionData(3));
    k.ic.assign(ic, ic + f->getSectionSize(3));
}

int run(const std::string &keyPath, const std::string &publicPath, const std::string &proofPath) {
    // the three files are read and checked before the device is touched
    Key key;
    const std::string keyText = slurp(keyPath);
    if (keyText.compare(0, 4, "zkey") == 0) key_from_zkey(keyPath, key);
    else key_from_json(keyPath, keyText, key);

    const Value pub = parse_file(publicPath);
    if (pub.type != Value::Null && pub.type != Value::Array) throw std::invalid_argument(publicPath + ": a list of public signals (or null) expected");
    std::vector<uint8_t> publics(pub.items.size() * 32);
    for (size_t i = 0; i < pub.items.size(); i++) decimal(pub.items[i], publicPath + ": public signal " + std::to_string(i), publics.data() + 32 * i);
    if (key.ic.size() / 64 != pub.items.size() + 1)
        throw std::invalid_argument("the verification key has " + std::to_string(key.ic.size() / 64) + " IC points for " + std::to_string(pub.items.size()) +
                                    " public signals (nPublic + 1 expected)");

    const Value pj = parse_file(proofPath);
    if (pj.type != Value::Object) throw std::invalid_argument(proofPath + ": a proof object expected");
    if (const Value *p = pj.find("protocol"))
        if (p->text != "groth16") throw std::invalid_argument(proofPath + ": protocol \"" + p->text + "\" is not groth16");
    if (const Value *c = pj.find("curve"))
        if (c->text != "bn128" && c->text != "bn254") throw std::invalid_argument(proofPath + ": curve \"" + c->text + "\" is not bn128");
    uint8_t proof[256];
    g1_point(member(pj, "pi_a", proofPath), "pi_a", proof);
    g2_point(member(pj, "pi_b", proofPath), "pi_b", proof + 64);
    g1_point(member(pj, "pi_c", proofPath), "pi_c", proof + 192);

    zk_vkey_view view;
    view.vk_alpha1 = key.alpha1;
    view.vk_beta2 = key.beta2;
    view.vk_gamma2 = key.gamma2;
    view.vk_delta2 = key.delta2;
    view.IC = key.ic.data();
    view.nPublic = (uint32_t)pub.items.size();
    zk_vkey *vk = nullptr;
    if (zk_vkey_create(&vk, &view, device_from_env()) != 0) throw std::runtime_error(zk_last_error());
    uint8_t verdict = ZK_VERIFY_MALFORMED;
    const int rc = zk_vkey_verify(vk, proof, publics.empty() ? nullptr : publics.data(), 1, &verdict);
    const std::string err = rc ? zk_last_error() : "";
    zk_vkey_destroy(vk);
    if (rc != 0) throw std::runtime_error(err);
    if (verdict == ZK_VERIFY_OK) {
        std::cout << "OK: the proof verifies\n";
        return 0;
    }
    if (verdict == ZK_VERIFY_MALFORMED)
        std::cout << "INVALID: the proof is malformed (a point off its curve, outside the subgroup or at infinity, or a value that is not reduced)\n";
    else
        std::cout << "INVALID: the proof is well-formed but the pairing equation does not hold\n";
    return 1;
}

}   // namespace

int main(int argc, char **argv) {
    return cli_main(argc == 4, "verifier <verification_key.json | circuit.zkey> <public.json> <proof.json>",
                    [&] { return run(argv[1], argv[2], argv[3]); });
}
