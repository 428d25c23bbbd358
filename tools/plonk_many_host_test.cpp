// csrc/plonk_many_plan.hpp alone, as a stand-alone program (tests/test_plonk_prove_many_host.py builds it with the address and
// undefined-behaviour sanitizers and runs it): the chunks of m proofs, the width rule and its knob, both limits of the batched
// multiplication at their edges with their messages, the out-of-memory message, and slots whose regions do not overlap.
#include <stdio.h>
#include <string.h>

#include <utility>
#include <vector>

#include "plonk_many_plan.hpp"

using namespace zk;

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            failures++;                                                   \
        }                                                                 \
    } while (0)

template <class Fn>
static std::string thrown(Fn fn) {
    try {
        fn();
    } catch (const std::exception &e) {
        return e.what();
    }
    return "";
}

static void chunking() {
    for (uint32_t B : {1u, 2u, 3u, 4u, 8u, 64u})
        for (uint64_t m = 0; m <= 3ull * B + 1; m++) {
            const uint64_t chunks = pm_chunks(m, B);
            CHECK(chunks == (m + B - 1) / B && (m == 0) == (chunks == 0));
            uint64_t next = 0;
            for (uint64_t g = 0; g < chunks; g++) {
                const uint32_t cnt = pm_chunk_count(m, g, B);
                CHECK(pm_chunk_first(g, B) == next && cnt >= 1 && cnt <= B);
                CHECK(g + 1 == chunks || cnt == B);          // only the last chunk is short
                next += cnt;
            }
            CHECK(next == m && pm_chunk_count(m, chunks, B) == 0);
        }
}

static void width_rule() {
    unsetenv("ZKHIP_PLONK_PROVE_BATCH");
    for (uint32_t log_n = 3; log_n <= 25; log_n++) {
        const uint32_t d = pm_default_width(log_n);
        CHECK(d >= 1 && d <= PM_MAX_WIDTH && pm_width(log_n) == d);
        CHECK(d == (log_n <= 16 ? 16u : 1u));                // what the measurement left committed
    }
    setenv("ZKHIP_PLONK_PROVE_BATCH", "", 1);
    CHECK(pm_width(11) == pm_default_width(11));
    for (uint32_t B = 1; B <= 64; B++) {
        setenv("ZKHIP_PLONK_PROVE_BATCH", std::to_string(B).c_str(), 1);
        for (uint32_t log_n : {3u, 16u, 17u, 25u}) CHECK(pm_width(log_n) == B);
    }
    for (const char *bad : {"0", "65", "-1", " 4", "4 ", "4x", "+4", "x", "18446744073709551617"}) {
        setenv("ZKHIP_PLONK_PROVE_BATCH", bad, 1);
        CHECK(thrown([] { pm_width(11); }) == "ZKHIP_PLONK_PROVE_BATCH: a number of proofs from 1 to 64 expected");
    }
    unsetenv("ZKHIP_PLONK_PROVE_BATCH");
}

static void limits() {
    // the header's own example: 2^20 rows, 13 windows
    const uint64_t len = (1ull << 20) + 6;
    CHECK(pm_entries(64, len, 13) == 2617260672ull && pm_width_that_fits(len, 13) == 52);
    CHECK(thrown([&] { pm_check_limits("zk_plonk_prove_many", 64, len, 13); }) ==
          "zk_plonk_prove_many: a chunk of 64 proofs is too large: 3 x 64 x 1048582 scalars x 13 windows = 2617260672 >= 2^31 table rows; "
          "ZKHIP_PLONK_PROVE_BATCH=52 would fit");
    CHECK(thrown([&] { pm_check_limits("zk_plonk_prove_many", 52, len, 13); }).empty());
    CHECK(!thrown([&] { pm_check_limits("zk_plonk_prove_many", 53, len, 13); }).empty());
    // the edges, exactly: 3 B len W = 2^31 - 3 passes, 2^31 is refused for its rows; 2^32 - 6 for its rows, 2^32 for its entries
    struct Edge {
        uint32_t B;
        uint64_t len;
        uint32_t W;
        const char *words;
    };
    const uint64_t two31 = 1ull << 31, two32 = 1ull << 32;
    for (const Edge &e : {Edge{1, 715827882ull, 1, ""}, Edge{2, 178956970ull, 2, ""}, Edge{4, 22369621ull, 8, ""},
                          Edge{4, 22369622ull, 8, ">= 2^31 table rows"}, Edge{8, 11184811ull, 16, ">= 2^32 sort entries"},
                          Edge{8, 11184810ull, 16, ">= 2^31 table rows"}, Edge{64, 1ull << 25, 1, ">= 2^32 sort entries"}}) {
        const uint64_t ent = pm_entries(e.B, e.len, e.W);
        const std::string got = thrown([&] { pm_check_limits("who", e.B, e.len, e.W); });
        if (!*e.words) {
            CHECK(ent < two31 && got.empty());
            continue;
        }
        CHECK(got.find(e.words) != std::string::npos && got.rfind("who: a chunk of " + std::to_string(e.B) + " proofs is too large: ", 0) == 0);
        CHECK((strstr(e.words, "2^32") != nullptr) == (ent >= two32) && ent >= two31);
        const uint32_t fit = pm_width_that_fits(e.len, e.W);
        CHECK(fit < e.B && (fit == 0 || pm_entries(fit, e.len, e.W) < two31) && (fit == PM_MAX_WIDTH || pm_entries(fit + 1, e.len, e.W) >= two31));
        CHECK(got.find(pm_fit_words(fit)) != std::string::npos);
    }
    CHECK(pm_entries(1, 715827882ull, 1) == two31 - 2 && pm_entries(4, 22369621ull, 8) == two31 - 32 && pm_width_that_fits(1ull << 25, 1) == 21);
    CHECK(pm_entries(4, 22369622ull, 8) >= two31 && pm_entries(8, 11184811ull, 16) >= two32 && pm_entries(8, 11184810ull, 16) < two32);
    CHECK(pm_fit_words(0) == "no width above 1 fits: ZKHIP_PLONK_PROVE_BATCH=1 proves one at a time" && pm_fit_words(1) == pm_fit_words(0));
    CHECK(pm_fit_words(7) == "ZKHIP_PLONK_PROVE_BATCH=7 would fit");
    // every log_n fits at some width with no fewer windows than the plan takes there (86 at 3 bits, 13 at the 20 bits of the largest)
    for (uint32_t log_n = 3; log_n <= 25; log_n++) CHECK(pm_width_that_fits((1ull << log_n) + 6, log_n < 8 ? 128 : log_n < 20 ? 32 : 13) >= 1);
    CHECK(pm_width_that_fits((1ull << 25) + 6, 13) == 1 && pm_width_that_fits((1ull << 24) + 6, 13) == 3);
    // HBM: need_hbm's margin, a thirty-second and 256 MiB
    const uint64_t MiB = 1ull << 20;
    CHECK(pm_hbm_margin(0) == 256 * MiB && pm_hbm_margin(32 * MiB) == 257 * MiB);
    CHECK(pm_hbm_fits(1024 * MiB, 1024 * MiB + 32 * MiB + 256 * MiB) && !pm_hbm_fits(1024 * MiB, 1024 * MiB + 32 * MiB + 256 * MiB - 1));
    CHECK(pm_hbm_message("zk_plonk_prove_many", 16, 1024 * MiB, 1000 * MiB, 12) ==
          "zk_plonk_prove_many: out of memory (a chunk of 16 proofs needs 1312 MiB of HBM, 1000 MiB free); ZKHIP_PLONK_PROVE_BATCH=12 would fit");
}

static void slots() {
    for (uint32_t B : {1u, 2u, 3u, 8u, 64u})
        for (uint64_t n : {(uint64_t)8, (uint64_t)64, (uint64_t)256, (uint64_t)2048})
            for (uint64_t n_public : {(uint64_t)0, (uint64_t)2, n}) {
                const uint64_t n_witness = 3 * n - 5;
                const PmLayout L = pm_layout(B, n, n_witness, n_public);
                CHECK(L.len == n + 6 && L.pub_stride == (n_public ? n_public : 1));
                // every region, with its rows a proof, in the slab's order: back to back, none overlapping, the slab's end the last's
                const std::vector<std::pair<uint64_t, uint64_t>> regions = {
                    {L.wit, n_witness}, {L.pub, L.pub_stride}, {L.blind, PM_BLINDS}, {L.vals, 4 * n}, {L.zval, n}, {L.pic, n}, {L.t, 3 * n + 6},
                    {L.round[0], 3 * L.len}, {L.round[1], L.len}, {L.round[2], 3 * L.len}, {L.round[3], 2 * L.len}};
                uint64_t at = 0;
                for (const auto &r : regions) {
                    CHECK(r.first == at);
                    at += r.second * B;
                }
                CHECK(at == L.rows && L.bytes() == at * 32);
                CHECK(L.committed_at() == L.round[0] && L.committed_rows() == 9 * L.len * B);
            }
    uint32_t vecs = 0;
    for (uint32_t v : PM_ROUND_VECS) {
        vecs += v;
        CHECK(v <= PM_MAX_VECS);
    }
    CHECK(vecs == 9);
}

static void statuses() {
    CHECK(std::string(pm_status_text(PM_ZERO_DENOMINATOR)) == "a denominator of the permutation product is zero");
    CHECK(std::string(pm_status_text(PM_COPIES)) == "the copy constraints do not hold");
    CHECK(std::string(pm_status_text(PM_GATES)) == "the witness does not satisfy the gates");
    CHECK(std::string(pm_status_text(PM_NOT_BELOW_R)) == "a value is not below r" && std::string(pm_status_text(9)) == "unknown status");
    CHECK(pm_refusal("zk_plonk_prove_many", 3, pm_status_text(PM_COPIES)) == "zk_plonk_prove_many: proof 3: the copy constraints do not hold");
}

int main() {
    chunking();
    width_rule();
    limits();
    slots();
    statuses();
    if (failures) return 1;
    printf("plonk_many host checks OK\n");
    return 0;
}
