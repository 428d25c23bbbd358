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
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <sys/random.h>
#include <sys/stat.h>

#include "../../include/zkhip.h"
#include "outfile.hpp"
#include "vkjson.hpp"
#include "zkfile.hpp"

namespace {

constexpr uint8_t kBn254R[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                                 0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};
constexpr uint8_t kBn254Q[32] = {0x47, 0xfd, 0x7c, 0xd8, 0x16, 0x8c, 0x20, 0x3c, 0x8d, 0xca, 0x71, 0x68, 0x91, 0x6a, 0x81, 0x97,
                                 0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};

bool is_zero(const uint8_t d[32]) {
    uint8_t any = 0;
    for (int i = 0; i < 32; i++) any |= d[i];
    return !any;
}
bool below_r(const uint8_t d[32]) {                       // little-endian bytes
    for (int i = 31; i >= 0; i--)
        if (d[i] != kBn254R[i]) return d[i] < kBn254R[i];
    return false;
}

// the secret: ZKHIP_CONTRIB_SCALAR (tests only) or 32 bytes of getrandom, redrawn until 0 < d < r
void draw_scalar(uint8_t d[32]) {
    if (const char *e = getenv("ZKHIP_CONTRIB_SCALAR")) {
        const std::invalid_argument bad("ZKHIP_CONTRIB_SCALAR is not a decimal number d with 0 < d < r");
        if (!*e) throw bad;
        memset(d, 0, 32);
        for (const char *c = e; *c; c++) {
            if (*c < '0' || *c > '9') throw bad;
            unsigned carry = (unsigned)(*c - '0');                 // d = 10 d + digit, a byte at a time
            for (int i = 0; i < 32; i++) {
                const unsigned t = d[i] * 10u + carry;
                d[i] = (uint8_t)t;
                carry = t >> 8;
            }
            if (carry) throw bad;
        }
        if (is_zero(d) || !below_r(d)) throw bad;
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
    struct stat a, b;
    if (stat(inPath.c_str(), &a) == 0 && stat(outPath.c_str(), &b) == 0 && a.st_dev == b.st_dev && a.st_ino == b.st_ino)
        throw std::invalid_argument("the input and the output are the same file");
    auto zkey = BinFileUtils::openExisting(inPath, "zkey", 1);
    char magicVersion[8];                                  // copied as they are
    if (!std::ifstream(inPath, std::ios::binary).read(magicVersion, 8)) throw std::runtime_error("cannot read " + inPath);
    for (uint32_t id = 1; id <= 10; id++)
        if (!zkey->hasSection(id)) throw std::invalid_argument("zkey has no section " + std::to_string(id));
    auto zh = ZKeyUtils::loadHeader(zkey.get());
    if (memcmp(zh->qPrime.data(), kBn254Q, 32) != 0 || memcmp(zh->rPrime.data(), kBn254R, 32) != 0)
        throw std::invalid_argument("zkey curve not supported (q and r are not BN254's)");
    if (zh->nVars < (uint64_t)zh->nPublic + 1) throw std::invalid_argument("zkey header: nPublic + 1 exceeds nVars");
    const uint64_t nv = zh->nVars, np1 = (uint64_t)zh->nPublic + 1, n = zh->domainSize;
    if (zkey->getSectionSize(4) < 4) throw std::invalid_argument("zkey section 4 is short: it has no record count");
    uint32_t nCoefs;
    memcpy(&nCoefs, zkey->getSectionData(4), 4);
    const struct {
        uint32_t id;
        uint64_t want;
    } implied[] = {{3, np1 * 64}, {4, 4 + (uint64_t)nCoefs * 44}, {5, nv * 64}, {6, nv * 64}, {7, nv * 128}, {8, (nv - np1) * 64}, {9, n * 64}};
    for (const auto &s : implied) {
        const uint64_t have = zkey->getSectionSize(s.id);
        if (have != s.want)
            throw std::invalid_argument("zkey section " + std::to_string(s.id) + (have < s.want ? " is short: " : " is long: ") + std::to_string(have) +
                                        " bytes, the header implies " + std::to_string(s.want));
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

    struct Sec {
        uint32_t id;
        const uint8_t *data;
        uint64_t size;
    };
    std::vector<Sec> secs;                                 // sections 1 to 10, in the input's order
    for (uint32_t id = 1; id <= 10; id++) secs.push_back({id, static_cast<const uint8_t *>(zkey->getSectionData(id)), zkey->getSectionSize(id)});
    std::sort(secs.begin(), secs.end(), [](const Sec &x, const Sec &y) { return x.data < y.data; });
    uint64_t total = 12;
    for (const auto &s : secs) total += 12 + s.size;

    MappedOutFile o(outPath, total);
    std::unique_ptr<OutFile> vk;
    if (!vkPath.empty()) vk.reset(new OutFile(vkPath));
    uint8_t *at = o.data;
    const uint32_t count = (uint32_t)secs.size();
    memcpy(at, magicVersion, 8);
    memcpy(at + 8, &count, 4);
    at += 12;
    zk_zkey_contrib_out out{};
    for (const auto &s : secs) {
        memcpy(at, &s.id, 4);
        memcpy(at + 4, &s.size, 8);
        at += 12;
        if (s.id == 8) out.pointsC = at;
        else if (s.id == 9) out.pointsH = at;
        else memcpy(at, s.data, s.size);
        if (s.id == 2) {                                   // the delta points are the last G1 and the last G2 of the section
            out.vk_delta1 = at + (static_cast<const uint8_t *>(zh->vk_delta1) - s.data);
            out.vk_delta2 = at + (static_cast<const uint8_t *>(zh->vk_delta2) - s.data);
        }
        at += s.size;
    }
    const char *dev = getenv("ZKHIP_DEVICE");
    if (zk_zkey_contribute(&zv, secret.d, dev ? atoi(dev) : -1, &out) != 0) throw std::runtime_error(zk_last_error());
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
    if (argc != 3 && argc != 4) {
        std::cerr << "Invalid number of parameters:\n";
        std::cerr << "Usage: zkeycontribute <in.zkey> <out.zkey> [verification_key.json]\n";
        return -1;
    }
    try {
        return run(argv[1], argv[2], argc == 4 ? argv[3] : "");
    } catch (std::exception &e) {
        std::cerr << e.what() << '\n';
        return -1;
    }
}
