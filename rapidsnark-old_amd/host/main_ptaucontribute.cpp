// ptaucontribute <in.ptau> <out.ptau>
//
// One contribution to a Powers of Tau file on the GPU (libzkhip zk_ptau_contribute): secrets tau, alpha, beta are drawn,
// tauG1[i] <- tau^i tauG1[i] and tauG2[i] <- tau^i tauG2[i] (sections 2, 3), alphaTauG1[i] <- alpha tau^i alphaTauG1[i]
// (4), betaTauG1[i] <- beta tau^i betaTauG1[i] (5), betaG2 <- beta betaG2 (6), the arithmetic of snarkjs `powersoftau
// contribute`.  The reference has no such program.  After it the file's tau, alpha and beta are known to nobody, provided
// this run's three scalars are forgotten: they come from getrandom, are never printed or written and are zeroed before the
// program ends.  Several parties run the tool one after another, each on the previous one's output, starting from
// `ptaunew`'s file; the result is sound if ONE of them forgot their scalars.  <out> holds the magic and version of <in> and
// its sections 1 to 7 in <in>'s order: 1 and 7 byte for byte, 2 to 6 from the library.  Section 7 (the contribution
// records: public keys, challenge hashes) is COPIED, not extended: the result is a sound file, not a ceremony transcript,
// and `snarkjs powersoftau verify` is not expected to accept it; `ptaucheck` checks the
// arithmetic.  An input that already has the Lagrange sections 12 to 15 is refused: contribute before `ptauprepare`.  The
// input is checked before the device is touched; the output is written as <out>.partial and renamed at the end, so that a
// failure leaves no file behind.  Exit codes: 0, or 255 with a message on stderr (as `zkeynew`).  ZKHIP_DEVICE=<n> picks the
// device.
// FOR TESTS ONLY: ZKHIP_PTAU_CONTRIB_SCALARS=<tau>,<alpha>,<beta> (decimal, 0 < each < r) fixes the scalars.  A file
// contributed to with scalars that anybody knows is as unsafe as before.
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include <sys/random.h>

#include "../../include/zkhip.h"
#include "cli.hpp"
#include "outfile.hpp"
#include "zkfile.hpp"

namespace {

struct Secrets {
    uint8_t s[3][32];                                      // tau, alpha, beta
    ~Secrets() { explicit_bzero(s, sizeof s); }
};

bool in_range(const uint8_t d[32], uint8_t least) {         // least <= d < r
    bool small = d[0] < least;
    for (int i = 1; i < 32 && small; i++) small = d[i] == 0;
    return !small && U256::less(d, U256::kBn254R.data());
}

// the secrets: ZKHIP_PTAU_CONTRIB_SCALARS (tests only) or 32 bytes of getrandom each, redrawn until 2 <= s < r
void draw_scalars(Secrets &sec) {
    if (const char *e = getenv("ZKHIP_PTAU_CONTRIB_SCALARS")) {
        const std::string text(e);
        size_t at = 0;
        bool ok = true;
        for (int i = 0; i < 3 && ok; i++) {
            const size_t comma = i < 2 ? text.find(',', at) : text.size();
            ok = comma != std::string::npos && U256::from_dec(text.substr(at, comma - at), sec.s[i]) && in_range(sec.s[i], 1);
            at = comma + 1;
        }
        if (!ok) throw std::invalid_argument("ZKHIP_PTAU_CONTRIB_SCALARS is not three decimal numbers tau,alpha,beta with 0 < each < r");
        return;
    }
    for (auto &d : sec.s)
        do {
            size_t got = 0;
            while (got < 32) {
                const ssize_t k = getrandom(d + got, 32 - got, 0);
                if (k < 0) throw std::runtime_error("getrandom failed");
                got += (size_t)k;
            }
            d[31] &= 0x3f;                                             // r < 2^254: uniform below 2^254, then rejected
        } while (!in_range(d, 2));
}

int run(const std::string &inPath, const std::string &outPath) {
    ContainerOut o(inPath, outPath);
    auto ptau = BinFileUtils::openExisting(inPath, "ptau", 1);
    ptau->startReadSection(1);
    if (ptau->readU32LE() != 32) throw std::invalid_argument("ptau: only 256-bit fields are supported");
    U256::Bytes q;
    memcpy(q.data(), ptau->read(32), 32);
    if (!U256::is_bn254_q(q)) throw std::invalid_argument("ptau curve not supported (q is not BN254's)");
    zk_ptau_file_view v{};
    v.power = ptau->readU32LE();
    ptau->endReadSection(false);
    for (uint32_t sec : {2u, 3u, 4u, 5u, 6u, 12u, 13u, 14u, 15u})
        if (ptau->hasSection(sec)) {
            v.sec[sec] = ptau->getSectionData(sec);
            v.sec_bytes[sec] = ptau->getSectionSize(sec);
        }
    zk_ptau_contrib_sizes sz{};
    if (zk_ptau_contribute_sizes(&v, &sz) != 0) throw std::invalid_argument(zk_last_error());

    Secrets secret;
    draw_scalars(secret);

    const uint64_t made[7] = {0, 0, sz.tau_g1_bytes, sz.tau_g2_bytes, sz.alpha_tau_g1_bytes, sz.beta_tau_g1_bytes, sz.beta_g2_bytes};
    std::vector<ContainerOut::Section> secs;               // sections 1 to 7, in the input's order; 2 to 6 are the library's
    for (const auto &s : ptau->sectionsInFileOrder(1, 7)) {
        if (s.id >= 2 && s.id <= 6) secs.push_back({s.id, made[s.id], nullptr});
        else secs.push_back({s.id, s.size, s.data});
    }
    const std::vector<uint8_t *> at = o.write(ptau->magicVersion(), secs);
    uint8_t *to[7] = {};
    for (size_t i = 0; i < secs.size(); i++)
        if (secs[i].id >= 2 && secs[i].id <= 6) to[secs[i].id] = at[i];
    zk_ptau_contrib_out out{to[2], to[3], to[4], to[5], to[6]};
    if (zk_ptau_contribute(&v, secret.s[0], secret.s[1], secret.s[2], device_from_env(), &out) != 0) throw std::runtime_error(zk_last_error());
    o.commit();
    std::cerr << "ptaucontribute: power " << v.power << ", sections 2 to 6 multiplied by the powers of a new tau, alpha and beta; section 7 copied\n";
    return 0;
}

}   // namespace

int main(int argc, char **argv) {
    return cli_main(argc == 3, "ptaucontribute <in.ptau> <out.ptau>", [&] { return run(argv[1], argv[2]); });
}
