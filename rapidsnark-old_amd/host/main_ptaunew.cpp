// ptaunew <power> <out.ptau>
//
// The file a Powers of Tau ceremony starts from, what snarkjs `powersoftau new bn128 <power> out.ptau` writes: section 1
// (n8 = 32, q, power, ceremonyPower = power), sections 2, 4 and 5 filled with the generator of G1 (2^(power+1) - 1, 2^power
// and 2^power points), section 3 with 2^power generators of G2, section 6 the generator of G2, section 7 a contribution
// count of zero: tau = alpha = beta = 1.  The reference has no such program.  Host only, no device is touched; the file is
// written through a mapping as <out>.partial and renamed at the end.  The power must be 1 to 28.  Exit codes: 0, or 255
// with a message on stderr (as `zkeynew`).  The next step is `ptaucontribute`, once per party.
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "cli.hpp"
#include "outfile.hpp"
#include "zkfile.hpp"

namespace {

void put(uint8_t *at, const zk::Fq64 &x) { memcpy(at, x.v, 32); }

// `count` copies of the `bytes`-long pattern at `at`, by doubling
void fill(uint8_t *at, const uint8_t *pattern, uint64_t bytes, uint64_t count) {
    if (!count) return;
    memcpy(at, pattern, bytes);
    uint64_t have = 1;
    while (have < count) {
        const uint64_t more = have < count - have ? have : count - have;
        memcpy(at + have * bytes, at, more * bytes);
        have += more;
    }
}

int run(const std::string &powerText, const std::string &outPath) {
    char *end = nullptr;
    const unsigned long power = strtoul(powerText.c_str(), &end, 10);
    if (powerText.empty() || *end || powerText[0] < '0' || powerText[0] > '9' || power < 1 || power > 28)
        throw std::invalid_argument("ptaunew: the power must be a number from 1 to 28");
    uint8_t g1[64], g2[128];
    put(g1, fq_mont(1, 0, 0, 0));                                   // (1, 2)
    put(g1 + 32, fq_mont(2, 0, 0, 0));
    // the generator of G2 of EIP-197: x = x.a + x.b u, y = y.a + y.b u
    put(g2, fq_mont(0x46debd5cd992f6edull, 0x674322d4f75edaddull, 0x426a00665e5c4479ull, 0x1800deef121f1e76ull));
    put(g2 + 32, fq_mont(0x97e485b7aef312c2ull, 0xf1aa493335a9e712ull, 0x7260bfb731fb5d25ull, 0x198e9393920d483aull));
    put(g2 + 64, fq_mont(0x4ce6cc0166fa7daaull, 0xe3d1e7690c43d37bull, 0x4aab71808dcb408full, 0x12c85ea5db8c6debull));
    put(g2 + 96, fq_mont(0x55acdadcd122975bull, 0xbc4b313370b38ef3ull, 0xec9e99ad690c3395ull, 0x090689d0585ff075ull));

    uint8_t header[4 + 32 + 8];
    const uint32_t n8 = 32, pw = (uint32_t)power, none = 0;
    memcpy(header, &n8, 4);
    memcpy(header + 4, U256::kBn254Q.data(), 32);
    memcpy(header + 36, &pw, 4);
    memcpy(header + 40, &pw, 4);
    const uint64_t n = 1ull << power;
    const struct {
        uint64_t count, bytes;
        const uint8_t *point;
    } rows[5] = {{2 * n - 1, 64, g1}, {n, 128, g2}, {n, 64, g1}, {n, 64, g1}, {1, 128, g2}};
    std::vector<ContainerOut::Section> secs;
    secs.push_back({1, sizeof header, header});
    for (uint32_t i = 0; i < 5; i++) secs.push_back({2 + i, rows[i].count * rows[i].bytes, nullptr});
    secs.push_back({7, 4, reinterpret_cast<const uint8_t *>(&none)});
    ContainerOut o(std::string(), outPath);                         // no input file to be the same as
    const uint8_t magicVersion[8] = {'p', 't', 'a', 'u', 1, 0, 0, 0};
    const std::vector<uint8_t *> at = o.write(magicVersion, secs);
    for (uint32_t i = 0; i < 5; i++) fill(at[1 + i], rows[i].point, rows[i].bytes, rows[i].count);
    o.commit();
    std::cerr << "ptaunew: power " << power << ", tau = alpha = beta = 1: contribute before use\n";
    return 0;
}

}   // namespace

int main(int argc, char **argv) {
    return cli_main(argc == 3, "ptaunew <power> <out.ptau>", [&] { return run(argv[1], argv[2]); });
}
