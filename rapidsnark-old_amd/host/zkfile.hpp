// zkfile — snarkjs binary containers (.zkey / .wtns) for the MI355X prover host.
//
// One translation unit provides the three namespaces the reference spreads over
// binfile_utils / zkey_utils / wtns_utils (src/binfile_utils.hpp:10-52, src/zkey_utils.hpp:11-36,
// src/wtns_utils.hpp:10-21) with the same public names, so code written against the reference
// (`BinFileUtils::openExisting`, `BinFile::getSectionData`, `ZKeyUtils::loadHeader`, ...) compiles
// against it unchanged.  Implementation notes:
//   * the file is mapped read-only and indexed once into a {type -> [extent]} table; there is no
//     second in-memory copy (reference quirk Q13), libzkhip uploads straight from the mapping;
//   * every cursor move is bounds-checked: a truncated file is an error, not a wild read;
//   * errors are C++ exceptions thrown BY VALUE with the reference's message texts (its
//     `throw new ...` escapes `catch (std::exception&)` and aborts — quirk Q1);
//   * primes are 32-byte little-endian arrays (no gmp on this path).
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/zkhip.h"
#include "../csrc/field64.hpp"         // libzkhip's host field: BN254's primes are its FrParams::P / FqParams::P

// 256-bit integers as the files hold them, 32 little-endian bytes: BN254's two primes, decimal text, comparison
namespace U256 {

typedef std::array<uint8_t, 32> Bytes;

constexpr Bytes from_words(const uint32_t (&w)[8]) {
    Bytes b{};
    for (int i = 0; i < 32; i++) b[i] = (uint8_t)(w[i / 4] >> (8 * (i % 4)));
    return b;
}
inline constexpr Bytes kBn254R = from_words(zk::FrParams::P), kBn254Q = from_words(zk::FqParams::P);
inline bool is_bn254_r(const Bytes &p) { return p == kBn254R; }
inline bool is_bn254_q(const Bytes &p) { return p == kBn254Q; }

inline bool less(const uint8_t a[32], const uint8_t b[32]) {
    for (int i = 31; i >= 0; i--)
        if (a[i] != b[i]) return a[i] < b[i];
    return false;
}
// decimal text -> out; false for an empty string, a character that is no digit or a value of 2^256 or more
inline bool from_dec(const std::string &text, uint8_t out[32]) {
    if (text.empty()) return false;
    uint32_t w[8] = {};
    for (const char c : text) {
        if (c < '0' || c > '9') return false;
        uint64_t carry = (uint64_t)(c - '0');               // w = 10 w + digit
        for (int i = 0; i < 8; i++) {
            const uint64_t t = (uint64_t)w[i] * 10u + carry;
            w[i] = (uint32_t)t;
            carry = t >> 32;
        }
        if (carry) return false;
    }
    memcpy(out, w, 32);
    return true;
}
// canonical base 10
inline std::string to_dec(const uint8_t le[32]) {
    uint32_t w[8];
    memcpy(w, le, 32);
    std::string s;
    for (;;) {
        bool zero = true;
        uint64_t rem = 0;
        for (int i = 7; i >= 0; i--) {
            const uint64_t cur = (rem << 32) | w[i];
            w[i] = (uint32_t)(cur / 10);
            rem = cur % 10;
            zero = zero && w[i] == 0;
        }
        s.insert(s.begin(), char('0' + rem));
        if (zero) return s;
    }
}

}   // namespace U256

// a standard-form Fq constant given as little-endian 64-bit limbs -> Montgomery
inline zk::Fq64 fq_mont(uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
    zk::Fq64 x;
    x.v[0] = a; x.v[1] = b; x.v[2] = c; x.v[3] = d;
    return zk::Fq64::to_mont(x);
}

namespace BinFileUtils {

class BinFile {
public:
    BinFile(const std::string &fileName, const std::string &type, uint32_t maxVersion);
    // the same container held in memory (a .wtns image that arrived in a request body): the image is owned by the object
    BinFile(std::string &&image, const std::string &type, uint32_t maxVersion);
    ~BinFile();
    BinFile(const BinFile &) = delete;
    BinFile &operator=(const BinFile &) = delete;

    // sequential section reads
    void startReadSection(uint32_t sectionId, uint32_t sectionPos = 0);
    void endReadSection(bool check = true);
    uint32_t readU32LE();
    uint64_t readU64LE();
    void *read(uint64_t len);

    // random access
    void *getSectionData(uint32_t sectionId, uint32_t sectionPos = 0);
    uint64_t getSectionSize(uint32_t sectionId, uint32_t sectionPos = 0);
    bool hasSection(uint32_t sectionId) const { return index_.count(sectionId) != 0; }

    // what a program that rewrites the container copies: the magic and version (the file's first 8 bytes), and those of
    // sections firstId to lastId that the file has, in the file's order
    const uint8_t *magicVersion() const { return map_; }
    struct Section {
        uint32_t id;
        const uint8_t *data;
        uint64_t size;
    };
    std::vector<Section> sectionsInFileOrder(uint32_t firstId, uint32_t lastId) const;

private:
    struct Extent {
        uint64_t begin, length;
    };
    const Extent &extent(uint32_t id, uint32_t nth) const;
    const uint8_t *take(uint64_t len);   // advance the cursor, checked

    void indexSections(const std::string &type, uint32_t maxVersion);
    uint8_t *map_ = nullptr;
    uint64_t mapLen_ = 0;
    std::string owned_;                  // in-memory images (map_ points into it; nothing to unmap)
    uint64_t cursor_ = 0;
    std::map<uint32_t, std::vector<Extent>> index_;
    const Extent *open_ = nullptr;
};

std::unique_ptr<BinFile> openExisting(const std::string &filename, const std::string &type, uint32_t maxVersion);
std::unique_ptr<BinFile> fromMemory(std::string &&image, const std::string &type, uint32_t maxVersion);

}   // namespace BinFileUtils

namespace ZKeyUtils {

// zkey sections 1-2 + the record count of section 4 (src/zkey_utils.cpp:17-52)
class Header {
public:
    uint32_t n8q = 0;
    std::array<uint8_t, 32> qPrime{};
    uint32_t n8r = 0;
    std::array<uint8_t, 32> rPrime{};
    uint32_t nVars = 0, nPublic = 0, domainSize = 0;
    uint64_t nCoefs = 0;
    void *vk_alpha1 = nullptr, *vk_beta1 = nullptr, *vk_beta2 = nullptr;
    void *vk_gamma2 = nullptr, *vk_delta1 = nullptr, *vk_delta2 = nullptr;
};
std::unique_ptr<Header> loadHeader(BinFileUtils::BinFile *f);

// the byte size a key's header implies for sections 3 to 9; section 4 is sized from its own leading record count
struct Shape {
    uint64_t nVars, nPublic, domainSize, nCoefs;
    uint64_t sectionBytes(uint32_t id) const {
        switch (id) {
        case 3: return (nPublic + 1) * 64;              // IC
        case 4: return 4 + 44 * nCoefs;
        case 5: case 6: return nVars * 64;              // A, B1
        case 7: return nVars * 128;                     // B2
        case 8: return (nVars - nPublic - 1) * 64;      // C
        case 9: return domainSize * 64;                 // H
        }
        throw std::logic_error("zkey section " + std::to_string(id) + " has no implied size");
    }
};

}   // namespace ZKeyUtils

namespace WtnsUtils {

// wtns section 1 (src/wtns_utils.cpp:12-25)
class Header {
public:
    uint32_t n8 = 0;
    std::array<uint8_t, 32> prime{};
    uint32_t nVars = 0;
};
std::unique_ptr<Header> loadHeader(BinFileUtils::BinFile *f);

}   // namespace WtnsUtils

namespace R1csUtils {

// circom .r1cs section 1 + the extent of section 2 (constraints, left encoded: libzkhip decodes it on the device).
// Not read by the reference; refuses other primes ("r1cs curve not supported") and custom gates (sections 4 / 5).
class Header {
public:
    uint32_t n8 = 0;
    std::array<uint8_t, 32> prime{};
    uint32_t nWires = 0, nPubOut = 0, nPubIn = 0, nPrvIn = 0;
    uint64_t nLabels = 0;
    uint32_t nConstraints = 0;
    const void *constraints = nullptr;
    uint64_t constraintsBytes = 0;
    zk_r1cs_view view() const { return zk_r1cs_view{nWires, nPubOut, nPubIn, nPrvIn, nConstraints, constraints, constraintsBytes}; }
};
std::unique_ptr<Header> loadHeader(BinFileUtils::BinFile *f);

}   // namespace R1csUtils

namespace PtauUtils {

// A Powers of Tau file (snarkjs .ptau, magic "ptau", version 1): section 1 (n8, q, power, ceremonyPower), the points
// alpha1 = alphaTauG1[0] (section 4), beta1 = betaTauG1[0] (section 5), beta2 (section 6), and the extents of the
// Lagrange-basis sections 12 to 15 (`powersoftau prepare phase2`; NULL / 0 when the file is not prepared), left in the
// mapping: only the levels a setup needs are ever read; and the extents of the powers themselves, sections 2 to 5, what
// `ptauprepare` reads.  Refuses other fields / curves, and alpha1 / beta1 / beta2 that
// are not points of BN254's G1 / G2 curve (checked here, on the host).
class Header {
public:
    uint32_t n8 = 0;
    std::array<uint8_t, 32> q{};
    uint32_t power = 0, ceremonyPower = 0;
    const void *alpha1 = nullptr, *beta1 = nullptr, *beta2 = nullptr;
    const void *lagrange[4] = {nullptr, nullptr, nullptr, nullptr};      // sections 12, 13, 14, 15
    uint64_t lagrangeBytes[4] = {0, 0, 0, 0};
    const void *powers[4] = {nullptr, nullptr, nullptr, nullptr};        // sections 2, 3, 4, 5 (NULL: the file has none)
    uint64_t powersBytes[4] = {0, 0, 0, 0};
};
std::unique_ptr<Header> loadHeader(BinFileUtils::BinFile *f);

}   // namespace PtauUtils
