// The host plan of zk_plonk_prove_many (include/zkhip.h, section "PLONK prover and verifier"), in plain
// C++ with nothing of HIP, so that tools/plonk_many_host_test.cpp checks it as a stand-alone program:
//   the status a proof of the call gets, and the text that goes with a refusal;
//   the chunk width B (ZKHIP_PLONK_PROVE_BATCH, and the default by log_n) and the chunks of m proofs;
//   where a chunk's state lies in the one slab of Fr rows the prover keeps for it (the slots);
//   the two limits of the batched multiplication (the sort's entries and the table's rows, hiputil.hpp's set_plan) and the
//   message of a request that does not fit HBM, each naming the width that would fit.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <stdexcept>
#include <string>

namespace zk {

// ---------------------------------------------------------------- a proof's status (zkhip.h: ZK_PLONK_MANY_*)
constexpr uint32_t PM_MADE = 0, PM_ZERO_DENOMINATOR = 1, PM_COPIES = 2, PM_GATES = 3, PM_NOT_BELOW_R = 4;
inline const char *pm_status_text(uint32_t status) {
    switch (status) {
    case PM_MADE: return "made";
    case PM_ZERO_DENOMINATOR: return "a denominator of the permutation product is zero";
    case PM_COPIES: return "the copy constraints do not hold";
    case PM_GATES: return "the witness does not satisfy the gates";
    case PM_NOT_BELOW_R: return "a value is not below r";
    }
    return "unknown status";
}
// "<who>: proof <i>: <what>"
inline std::string pm_refusal(const char *who, uint64_t proof, const std::string &what) {
    return std::string(who) + ": proof " + std::to_string(proof) + ": " + what;
}

// ---------------------------------------------------------------- the chunk width
constexpr uint32_t PM_MAX_WIDTH = 64, PM_BLINDS = 11;
constexpr uint32_t PM_ROUND_VECS[4] = {3, 1, 3, 2};   // vectors a proof gives the multiplication of rounds 1, 2, 3 and 5
constexpr uint32_t PM_MAX_VECS = 3;                   // the most of them: the buffers hold 3 B vectors
// The default by log_n.  The rule zk_prove_batch_submit has for Groth16 (8 up to 2^16, 4 at 2^17, 1 above) is where this
// started from; what is committed is what profiles/plonk_prove_many_timing.txt measured: 16, the widest
// width of the sweep, was the fastest at 2^11, 2^14 and 2^16, 2.3 to 3.2 times the loop; a smaller circuit is bound by launches and
// drains more, not less.  From 2^17 on nothing was measured and the call is the loop
inline uint32_t pm_default_width(uint32_t log_n) { return log_n <= 16 ? 16 : 1; }
// ZKHIP_PLONK_PROVE_BATCH: decimal, 1 .. 64, nothing before or after the number; unset or empty: the default
inline uint32_t pm_width(uint32_t log_n) {
    const char *e = getenv("ZKHIP_PLONK_PROVE_BATCH");
    if (!e || !*e) return pm_default_width(log_n);
    char *end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (*end || *e < '0' || *e > '9' || v < 1 || v > PM_MAX_WIDTH) throw std::invalid_argument("ZKHIP_PLONK_PROVE_BATCH: a number of proofs from 1 to 64 expected");
    return (uint32_t)v;
}
inline uint64_t pm_chunks(uint64_t m, uint32_t B) { return (m + B - 1) / B; }
// the proofs of chunk g: [first, first + count)
inline uint64_t pm_chunk_first(uint64_t g, uint32_t B) { return g * B; }
inline uint32_t pm_chunk_count(uint64_t m, uint64_t g, uint32_t B) {
    const uint64_t first = g * B;
    return first >= m ? 0u : (uint32_t)(m - first < B ? m - first : B);
}

// ---------------------------------------------------------------- the slots
// One slab of Fr rows.  Every region holds B proofs back to back, so that a per-proof base is a stride from one pointer, and
// the committed rows of a round are ONE run of (vectors a proof) x B vectors of n + 6 rows: what the multiplication takes.
struct PmLayout {
    uint32_t B = 0;
    uint64_t n = 0, len = 0, n_witness = 0, pub_stride = 0;
    uint64_t wit = 0, pub = 0, blind = 0;             // the inputs: n_witness, max(n_public, 1) and 11 rows a proof
    uint64_t vals = 0, zval = 0, pic = 0, t = 0;      // 4n (a, b, c, PI by values), n, n and 3n + 6 rows a proof
    uint64_t round[4] = {0, 0, 0, 0};                 // a b c | z | t_lo t_mid t_hi | W_zeta W_zeta_omega: PM_ROUND_VECS[r] x len a proof
    uint64_t rows = 0;                                // the slab
    uint64_t committed_at() const { return round[0]; }
    uint64_t committed_rows() const { return rows - round[0]; }      // cleared when the slots are made
    uint64_t bytes() const { return rows * 32; }
};
inline PmLayout pm_layout(uint32_t B, uint64_t n, uint64_t n_witness, uint64_t n_public) {
    PmLayout L;
    L.B = B, L.n = n, L.len = n + 6, L.n_witness = n_witness, L.pub_stride = n_public ? n_public : 1;
    uint64_t at = 0;
    auto take = [&](uint64_t rows_a_proof) {
        const uint64_t here = at;
        at += rows_a_proof * B;
        return here;
    };
    L.wit = take(n_witness), L.pub = take(L.pub_stride), L.blind = take(PM_BLINDS);
    L.vals = take(4 * n), L.zval = take(n), L.pic = take(n), L.t = take(3 * n + 6);
    for (int r = 0; r < 4; r++) L.round[r] = take(PM_ROUND_VECS[r] * L.len);
    L.rows = at;
    return L;
}

// ---------------------------------------------------------------- the limits
// The sort's entries are 32-bit with the sign in bit 31, and an entry names a table row before it is folded back to its
// vector's: 3 B (n + 6) W must stay below 2^32 entries and 2^31 rows (hiputil.hpp's set_plan states both).  W: the windows
inline uint64_t pm_entries(uint32_t B, uint64_t len, uint32_t W) { return (uint64_t)PM_MAX_VECS * B * len * W; }
// the largest width from 1 to 64 whose multiplications fit both, 0 when none does
inline uint32_t pm_width_that_fits(uint64_t len, uint32_t W) {
    uint32_t B = PM_MAX_WIDTH;
    while (B && pm_entries(B, len, W) >= (1ull << 31)) B--;
    return B;
}
inline std::string pm_fit_words(uint32_t fit) {
    return fit > 1 ? "ZKHIP_PLONK_PROVE_BATCH=" + std::to_string(fit) + " would fit"
                   : std::string("no width above 1 fits: ZKHIP_PLONK_PROVE_BATCH=1 proves one at a time");
}
inline void pm_check_limits(const char *who, uint32_t B, uint64_t len, uint32_t W) {
    const uint64_t e = pm_entries(B, len, W);
    if (e < (1ull << 31)) return;
    const std::string head = std::string(who) + ": a chunk of " + std::to_string(B) + " proofs is too large: 3 x " + std::to_string(B) + " x " +
                             std::to_string(len) + " scalars x " + std::to_string(W) + " windows = " + std::to_string(e);
    if (e >= (1ull << 32)) throw std::invalid_argument(head + " >= 2^32 sort entries; " + pm_fit_words(pm_width_that_fits(len, W)));
    throw std::invalid_argument(head + " >= 2^31 table rows; " + pm_fit_words(pm_width_that_fits(len, W)));
}
// need_hbm's rule and words (hiputil.hpp), with the width that would fit
inline uint64_t pm_hbm_margin(uint64_t need) { return need / 32 + ((uint64_t)256 << 20); }
inline bool pm_hbm_fits(uint64_t need, uint64_t free_bytes) { return free_bytes >= need + pm_hbm_margin(need); }
inline std::string pm_hbm_message(const char *who, uint32_t B, uint64_t need, uint64_t free_bytes, uint32_t fit) {
    return std::string(who) + ": out of memory (a chunk of " + std::to_string(B) + " proofs needs " + std::to_string((need + pm_hbm_margin(need)) >> 20) +
           " MiB of HBM, " + std::to_string(free_bytes >> 20) + " MiB free); " + pm_fit_words(fit);
}

}   // namespace zk
