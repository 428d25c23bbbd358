// zkeyverify <circuit.r1cs> <pot.ptau> <circuit.zkey>
//
// Is this .zkey the key of this circuit over this Powers of Tau file?  The check of libzkhip's zk_zkey_verify on the GPU,
// the arithmetic half of snarkjs `zkey verify`; the reference has no such program.  The .ptau is prepared for phase 2 and
// of a power >= the circuit's, as for `zkeynew`.  Checked: every point of the key (coordinates, curve, G2 subgroup);
// alpha1, beta1, beta2 against the .ptau; gamma2 = the G2 generator; delta1 and delta2 the same delta; section 4 against
// the circuit; sections 3 and 5 to 9 against the circuit and the .ptau's Lagrange levels, each by one random combination
// (a wrong section passes with probability below 2^29 / r).  NOT checked: section 10, the contribution transcript, and so
// not that anybody honest ever contributed to delta.  The three files are mapped, never read whole, and their shapes are
// compared before the device is touched.  Exit codes, as `ptaucheck` / `verifier` / `wtnscheck`: 0 with "OK: ..." on
// stdout; 1 with one "INVALID: ..." line per finding on stdout; 255 with a message on stderr for everything else (bad
// file, no device, too little memory).  ZKHIP_DEVICE=<n> picks the device.  For tests only,
// ZKHIP_ZKEY_VERIFY_SCALAR=<decimal> fixes the scalar of the random combinations (0, 1 and values >= r are refused).
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>

#include "../../include/zkhip.h"
#include "cli.hpp"
#include "zkfile.hpp"

namespace {

const void *section_or_null(BinFileUtils::BinFile &f, uint32_t id, uint64_t &bytes) {
    bytes = f.getSectionSize(id);
    return bytes ? f.getSectionData(id) : nullptr;
}

int run(const std::string &r1csPath, const std::string &ptauPath, const std::string &zkeyPath) {
    // the three files are mapped and compared before the device is touched, and before the scalar is drawn
    auto r1cs = BinFileUtils::openExisting(r1csPath, "r1cs", 1);
    auto rh = R1csUtils::loadHeader(r1cs.get());
    auto ptau = BinFileUtils::openExisting(ptauPath, "ptau", 1);
    auto ph = PtauUtils::loadHeader(ptau.get());
    auto zkey = BinFileUtils::openExisting(zkeyPath, "zkey", 1);
    auto zh = ZKeyUtils::loadHeader(zkey.get());
    if (!U256::is_bn254_q(zh->qPrime) || !U256::is_bn254_r(zh->rPrime)) throw std::invalid_argument("zkey curve not supported");

    const zk_r1cs_view rv = rh->view();
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
    zk_zkey_verify_view zv{};
    zk_zkey_view &k = zv.key;
    k.nVars = zh->nVars;
    k.nPublic = zh->nPublic;
    k.domainSize = zh->domainSize;
    k.vk_alpha1 = zh->vk_alpha1;
    k.vk_beta1 = zh->vk_beta1;
    k.vk_beta2 = zh->vk_beta2;
    k.vk_delta1 = zh->vk_delta1;
    k.vk_delta2 = zh->vk_delta2;
    zv.vk_gamma2 = zh->vk_gamma2;
    zv.pointsIC = section_or_null(*zkey, 3, zv.pointsIC_bytes);
    k.coefs = section_or_null(*zkey, 4, k.coefs_bytes);
    if (k.coefs_bytes < 4) throw std::invalid_argument("zkey section 4 is truncated");
    uint32_t nCoefs;
    memcpy(&nCoefs, k.coefs, 4);
    k.nCoefs = nCoefs;
    k.pointsA = section_or_null(*zkey, 5, k.pointsA_bytes);
    k.pointsB1 = section_or_null(*zkey, 6, k.pointsB1_bytes);
    k.pointsB2 = section_or_null(*zkey, 7, k.pointsB2_bytes);
    k.pointsC = section_or_null(*zkey, 8, k.pointsC_bytes);
    k.pointsH = section_or_null(*zkey, 9, k.pointsH_bytes);
    zk_zkey_verify_sizes_t sz{};
    if (zk_zkey_verify_sizes(&rv, &pv, &zv, &sz) != 0) throw std::invalid_argument(zk_last_error());

    uint8_t s32[32];
    const uint8_t *fixed = nullptr;
    if (const char *e = getenv("ZKHIP_ZKEY_VERIFY_SCALAR")) {
        uint8_t one[32] = {1};
        if (!U256::from_dec(e, s32) || !U256::less(one, s32) || !U256::less(s32, U256::kBn254R.data()))
            throw std::invalid_argument("ZKHIP_ZKEY_VERIFY_SCALAR: a decimal number from 2 to r - 1 expected");
        fixed = s32;
    }
    zk_zkey_verify_report rep{};
    rep.size = sizeof rep;
    // shapes that disagree come back as a report before a device is touched
    if (zk_zkey_verify(&rv, &pv, &zv, fixed, device_from_env(), &rep) != 0) throw std::runtime_error(zk_last_error());

    const uint32_t npub = rh->nPubOut + rh->nPubIn;
    if (rep.verdict == 0) {
        std::cout << "OK: the key of this circuit over this ptau (2^" << sz.log_domain << " domain, " << zh->nVars
                  << " wires): points, alpha, beta, gamma, delta, coefficients and sections 3 and 5 to 9 hold";
        if (rep.delta_is_generator) std::cout << "; delta is 1: a phase-2 starting key, not safe to prove with";
        std::cout << "; the contribution transcript (section 10) is not checked\n";
        return 0;
    }
    if (rep.verdict == 2) {
        static const char *const kind[5] = {"", "has a coordinate that is not below q", "is not on the curve", "is not in the subgroup", "is the point at infinity"};
        std::cout << "INVALID: section " << rep.bad_section << ": point " << rep.bad_index << " " << kind[rep.bad_kind <= 4 ? rep.bad_kind : 0] << "\n";
        return 1;
    }
    if (rep.shape_failed) {
        const uint32_t sh = rep.shape_failed;
        if (sh >> ZK_ZV_SHAPE_NVARS & 1u) std::cout << "INVALID: nVars: the key has " << zh->nVars << " wires, the circuit " << rh->nWires << "\n";
        if (sh >> ZK_ZV_SHAPE_NPUBLIC & 1u) std::cout << "INVALID: nPublic: the key has " << zh->nPublic << " public signals, the circuit " << npub << "\n";
        if (sh >> ZK_ZV_SHAPE_DOMAIN & 1u)
            std::cout << "INVALID: domain: the key has a domain of " << zh->domainSize << ", the circuit's " << rh->nConstraints << " constraints and " << npub
                      << " + 1 public-input rows need a power of two of at least 2^" << sz.log_domain << "\n";
        if (sh >> ZK_ZV_SHAPE_PTAU_UNPREPARED & 1u)
            std::cout << "INVALID: ptau: the file is not prepared for phase 2 (no Lagrange sections 12 to 15)\n";
        if (sh >> ZK_ZV_SHAPE_PTAU_POWER & 1u)
            std::cout << "INVALID: ptau: the file holds 2^" << ph->power << " and the circuit needs 2^" << sz.log_domain << "\n";
        return 1;
    }
    static const char *const what[ZK_ZV_ITEMS] = {
        "alpha1: the key's alpha1 is not alphaTauG1[0] of the ptau",
        "beta1: the key's beta1 is not betaTauG1[0] of the ptau",
        "beta2: the key's beta2 is not betaG2 of the ptau",
        "gamma2: the key's gamma2 is not the generator of G2",
        "delta: delta1 and delta2 are not the same multiple of their generators",
        "coefs",
        "A: section 5 is not this circuit's A over this ptau",
        "B1: section 6 is not this circuit's B over this ptau",
        "B2: section 7 is not this circuit's B over this ptau",
        "IC: section 3 is not this circuit's public part over this ptau",
        "C: section 8 is not this circuit's private part over this ptau and delta",
        "H: section 9 is not the odd Lagrange points of twice the domain over delta"};
    for (uint32_t i = 0; i < ZK_ZV_ITEMS; i++) {
        if (rep.failed >> i & 1u) {
            if (i == ZK_ZV_COEFS)
                std::cout << "INVALID: coefs: section 4 differs from the circuit in " << rep.coef_rows_differing << " rows, the first is row " << rep.coef_first_row << "\n";
            else std::cout << "INVALID: " << what[i] << "\n";
        }
    }
    static const char *const name[ZK_ZV_ITEMS] = {"alpha1", "beta1", "beta2", "gamma2", "delta", "coefs", "A", "B1", "B2", "IC", "C", "H"};
    for (uint32_t i = 0; i < ZK_ZV_ITEMS; i++)
        if (rep.not_checked >> i & 1u) std::cout << "NOT CHECKED: " << name[i] << ": it needs a delta that holds\n";
    return 1;
}

}   // namespace

int main(int argc, char **argv) {
    return cli_main(argc == 4, "zkeyverify <circuit.r1cs> <pot.ptau> <circuit.zkey>", [&] { return run(argv[1], argv[2], argv[3]); });
}
