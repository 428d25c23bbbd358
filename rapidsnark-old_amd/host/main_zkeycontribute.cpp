// zkeycontribute <in.zkey> <out.zkey> [verification_key.json]
//
// One phase-2 contribution to a Groth16 key on the GPU (libzkhip zk_zkey_contribute): a secret d is drawn, delta <- delta d
// in section 2 and every point of sections 8 (C) and 9 (H) <- d^-1 point, the arithmetic of snarkjs `zkey contribute`.  The
// reference has no such program.  After it the key's delta is known to nobody, provided this run's d is forgotten: d comes
// from getrandom, is never printed or written and is zeroed before the program ends.  Several parties may run the tool one
// after another, each on the previous one's output.  <out> holds the magic and version of <in> and its sections 1 to 10
// in <in>'s order: 1, 3 to 7 and 10 byte for byte, 2 with the two new delta points, 8 and 9 from the library.  Section 10
// (csHash and the contribution records) is COPIED, not extended: the result is a sound proving key, not a verifiable
// ceremony transcript, and `snarkjs zkey verify` is not expected to pass.  The optional third
// argument is `zkeynew`'s verification_key.json with the new vk_delta_2.  The input is checked before the device is touched;
// the outputs are written as <out>.partial and renamed at the end, so that a failure leaves no file behind.  Exit codes: 0,
// or 255 with a message on stderr (as `zkeynew`).  ZKHIP_DEVICE=<n> picks the device.
// FOR TESTS ONLY: ZKHIP_CONTRIB_SCALAR=<decimal> fixes d (0 < d < r).  A key contributed to with a d that anybody knows is
// as unsafe as before.
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <sys/random.h>

#include "../../include/zkhip.h"
#include "cli.hpp"
#include "outfile.hpp"
#include "vkjson.hpp"
#include "zkfile.hpp"

namespace {

bool is_zero(const uint8_t d[32]) {
    uint8_t any = 0;
    for (int i = 0; i < 32; i++) any |= d[i];
    return !any;
}
bool below_r(const uint8_t d[32]) { return U256::less(d, U256::kBn254R.data()); }

// the secret: ZKHIP_CONTRIB_SCALAR (tests only) or 32 bytes of getrandom, redrawn until 0 < d < r
void draw_scalar(uint8_t d[32]) {
    if (const char *e = getenv("ZKHIP_CONTRIB_SCALAR")) {
        if (!U256::from_dec(e, d) || is_zero(d) || !below_r(d))
            throw std::invalid_argument("ZKHIP_CONTRIB_SCALAR is not a decimal number d with 0 < d < r");
        return;
    }
    do {
        size_t got = 0;
        while (got < 32) {
            const ssize_t k = getrandom(d + got, 32 - got, 0);
            if (k < 0) throw std::runtime_error("getrandom failed");
            got += (size_t)k;
        }
        d[31] &= 0x3f;                                              // r < 2^254: uniform below 2^254, then rejected
    } while (is_zero(d) || !below_r(d));
}

int run(const std::string &inPath, const std::string &outPath, const std::string &vkPath) {
    ContainerOut o(inPath, outPath);
    auto zkey = BinFileUtils::openExisting(inPath, "zkey", 1);
    for (uint32_t id = 1; id <= 10; id++)
        if (!zkey->hasSection(id)) throw std::invalid_argument("zkey has no section " + std::to_string(id));
    auto zh = ZKeyUtils::loadHeader(zkey.get());
    if (!U256::is_bn254_q(zh->qPrime) || !U256::is_bn254_r(zh->rPrime))
        throw std::invalid_argument("zkey curve not supported (q and r are not BN254's)");
    if (zh->nVars < (uint64_t)zh->nPublic + 1) throw std::invalid_argument("zkey header: nPublic + 1 exceeds nVars");
    const uint64_t nv = zh->nVars, np1 = (uint64_t)zh->nPublic + 1, n = zh->domainSize;
    if (zkey->getSectionSize(4) < 4) throw std::invalid_argument("zkey section 4 is short: it has no record count");
    uint32_t nCoefs;
    memcpy(&nCoefs, zkey->getSectionData(4), 4);
    const ZKeyUtils::Shape shape{nv, zh->nPublic, n, nCoefs};
    for (uint32_t id = 3; id <= 9; id++) {
        const uint64_t have = zkey->getSectionSize(id), want = shape.sectionBytes(id);
        if (have != want)
            throw std::invalid_argument("zkey section " + std::to_string(id) + (have < want ? " is short: " : " is long: ") + std::to_string(have) +
                                        " bytes, the header implies " + std::to_string(want));
    }

    struct Secret {
        uint8_t d[32];
        ~Secret() { explicit_bzero(d, sizeof d); }
    } secret;
    draw_scalar(secret.d);

    zk_zkey_contrib_view zv{};
    zv.vk_delta1 = zh->vk_delta1;
    zv.vk_delta2 = zh->vk_delta2;
    zv.pointsC = zkey->getSectionSize(8) ? zkey->getSectionData(8) : nullptr;
    zv.pointsH = zkey->getSectionSize(9) ? zkey->getSectionData(9) : nullptr;
    zv.pointsC_bytes = zkey->getSectionSize(8);
    zv.pointsH_bytes = zkey->getSectionSize(9);
    zk_zkey_contrib_sizes sz{};
    if (zk_zkey_contribute_sizes(&zv, &sz) != 0) throw std::invalid_argument(zk_last_error());

    std::vector<ContainerOut::Section> secs;               // sections 1 to 10, in the input's order; 8 and 9 are the library's
    for (const auto &s : zkey->sectionsInFileOrder(1, 10)) secs.push_back({s.id, s.size, s.id == 8 || s.id == 9 ? nullptr : s.data});
    const std::vector<uint8_t *> at = o.write(zkey->magicVersion(), secs);
    std::unique_ptr<OutFile> vk;
    if (!vkPath.empty()) vk.reset(new OutFile(vkPath));
    zk_zkey_contrib_out out{};
    for (size_t i = 0; i < secs.size(); i++) {
        if (secs[i].id == 8) out.pointsC = at[i];
        if (secs[i].id == 9) out.pointsH = at[i];
        if (secs[i].id == 2) {                             // the delta points are the last G1 and the last G2 of the section
            out.vk_delta1 = at[i] + (static_cast<const uint8_t *>(zh->vk_delta1) - secs[i].src);
            out.vk_delta2 = at[i] + (static_cast<const uint8_t *>(zh->vk_delta2) - secs[i].src);
        }
    }
    if (zk_zkey_contribute(&zv, secret.d, device_from_env(), &out) != 0) throw std::runtime_error(zk_last_error());
    if (vk) {
        const std::string j = verification_key_json(zh->nPublic, static_cast<const uint8_t *>(zh->vk_alpha1), static_cast<const uint8_t *>(zh->vk_beta2),
                                                    static_cast<const uint8_t *>(zh->vk_gamma2), out.vk_delta2,
                                                    static_cast<const uint8_t *>(zkey->getSectionData(3)));
        vk->write(j.data(), j.size());
    }
    o.commit();
    if (vk) vk->commit();
    std::cerr << "zkeycontribute: " << (nv - np1) << " points of section 8 and " << n << " of section 9 scaled, delta replaced\n";
    return 0;
}

}   // namespace

int main(int argc, char **argv) {
    return cli_main(argc == 3 || argc == 4, "zkeycontribute <in.zkey> <out.zkey> [verification_key.json]",
                    [&] { return run(argv[1], argv[2], argc == 4 ? argv[3] : ""); });
}
