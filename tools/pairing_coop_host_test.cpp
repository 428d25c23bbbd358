// Host check of the cooperative pairing path's lane map (csrc/pairing_coop.hpp): the sliced Fq12 product, squaring and line
// product, run lane by lane as the kernel's wave runs them, against pairing.hpp's f12_mul, f12_sqr and f12_mul_line on
// random elements; and the reading of the two thresholds.  tests/test_verify_coop_host.py builds and runs it.
#include <stdio.h>
#include <string.h>
#include <random>

#include "pairing_coop.hpp"

using namespace zk;

static std::mt19937_64 rng(20240611);

static Fq rand_fq() {                                 // a reduced element in Montgomery form: the product of two raw draws
    Fq a, b;
    for (int i = 0; i < 8; i++) {
        a.v[i] = (u32)rng();
        b.v[i] = (u32)rng();
    }
    a.v[7] &= 0x0FFFFFFFu;                            // below q
    b.v[7] &= 0x0FFFFFFFu;
    return Fq::mul(a, b);
}
static Fq2 rand_f2() { return Fq2{rand_fq(), rand_fq()}; }

static void to_w(Fq2 w[6], const Fq12 &a) {
    const Fq2 *s = reinterpret_cast<const Fq2 *>(&a);
    for (int k = 0; k < 6; k++) w[k] = s[coop_slot(k)];
}
static bool same(const Fq2 w[6], const Fq12 &a) {
    const Fq2 *s = reinterpret_cast<const Fq2 *>(&a);
    for (int k = 0; k < 6; k++)
        if (memcmp(&w[k], &s[coop_slot(k)], sizeof(Fq2)) != 0) return false;
    return true;
}
// what c_mul does: 36 lanes, then six sums
static void sliced_mul(Fq2 r[6], const Fq2 a[6], const Fq2 b[6]) {
    Fq2 prod[36];
    for (int lane = 0; lane < COOP_LANES_FULL; lane++) {
        int i, j;
        coop_pair_full(lane, i, j);
        prod[lane] = Fq2::mul(a[i], b[j]);
    }
    for (int k = 0; k < 6; k++) r[k] = coop_sum(k, prod, COOP_FULL);
}
// what c_line does: 18 lanes; the other 18 entries hold rubbish that must not be read
static void sliced_line(Fq2 f[6], const Fq2 &a, const Fq2 &b, const Fq2 &c) {
    Fq2 prod[36];
    for (int i = 0; i < 36; i++) prod[i] = rand_f2();
    for (int lane = 0; lane < COOP_LANES_LINE; lane++) {
        int i, j;
        coop_pair_line(lane, i, j);
        prod[6 * i + j] = Fq2::mul(f[i], j == 0 ? a : j == 1 ? b : c);
    }
    Fq2 r[6];
    for (int k = 0; k < 6; k++) r[k] = coop_sum(k, prod, COOP_LINE);
    for (int k = 0; k < 6; k++) f[k] = r[k];
}

static int expect_threshold(const char *value, bool good, uint64_t want) {
    if (value) setenv("ZKHIP_VERIFY_COOP_MAX", value, 1);
    else unsetenv("ZKHIP_VERIFY_COOP_MAX");
    try {
        const uint64_t v = coop_threshold("ZKHIP_VERIFY_COOP_MAX", "proofs", 77);
        if (!good || v != want) {
            printf("threshold '%s': got %llu\n", value ? value : "(unset)", (unsigned long long)v);
            return 1;
        }
    } catch (const std::invalid_argument &e) {
        if (good || strcmp(e.what(), "ZKHIP_VERIFY_COOP_MAX: a number of proofs from 0 to 2^24 expected") != 0) {
            printf("threshold '%s': %s\n", value, e.what());
            return 1;
        }
    }
    return 0;
}

int main() {
    int bad = 0;
    bool seen[6] = {false, false, false, false, false, false};
    for (int k = 0; k < 6; k++) seen[coop_slot(k)] = true;
    for (int k = 0; k < 6; k++) bad += !seen[k];
    for (int round = 0; round < 50; round++) {
        Fq12 a, b, want;
        Fq2 *as = reinterpret_cast<Fq2 *>(&a), *bs = reinterpret_cast<Fq2 *>(&b);
        for (int i = 0; i < 6; i++) {
            as[i] = rand_f2();
            bs[i] = rand_f2();
        }
        if (round == 0) f12_one(b);
        Fq2 aw[6], bw[6], rw[6];
        to_w(aw, a);
        to_w(bw, b);
        f12_mul(want, a, b);
        sliced_mul(rw, aw, bw);
        if (!same(rw, want)) bad++, printf("round %d: product differs\n", round);
        f12_sqr(want, a);
        sliced_mul(rw, aw, aw);
        if (!same(rw, want)) bad++, printf("round %d: square differs\n", round);
        const Fq2 s = rand_f2(), t = rand_f2(), c = rand_f2();
        want = a;
        f12_mul_line(want, s, t, c);
        sliced_line(aw, s, t, c);
        if (!same(aw, want)) bad++, printf("round %d: line product differs\n", round);
    }
    bad += expect_threshold(nullptr, true, 77);
    bad += expect_threshold("", true, 77);
    bad += expect_threshold("0", true, 0);
    bad += expect_threshold("4", true, 4);
    bad += expect_threshold("16777216", true, 1ull << 24);
    bad += expect_threshold("16777217", false, 0);
    bad += expect_threshold("-1", false, 0);
    bad += expect_threshold("4x", false, 0);
    bad += expect_threshold(" 4", false, 0);
    bad += expect_threshold("many", false, 0);
    if (bad) return 1;
    printf("OK: sliced product, square and line product equal pairing.hpp's\n");
    return 0;
}
