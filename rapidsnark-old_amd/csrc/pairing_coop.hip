// The latency path of verification and of zk_pairing: a workgroup per proof (k_verify_coop) or per group of pairs
// (k_pairing_coop) where pairing.hip gives a lane.  Same arithmetic (pairing.hpp), same checks (paircheck.hpp), same
// results; pairing.hip's host side chooses between the two by the number of jobs.  DESIGN.md section 22.
//
// Division of work.  What does not depend on the running value f is made first, by waves that run side by side:
//   k_verify_coop, 3 waves:  wave 0 (one lane) the MILLER_LINES lines of B into the proof's own slice of `lines`; wave 1 (one
//   lane) B's subgroup test by the endomorphism (ptengine.hpp); wave 2 vk_x, a lane per public signal with mulglv.hpp's
//   split multiplication, summed by a tree through LDS and made affine.  Before that, one barrier earlier, the format
//   checks (coordinates, curve equations, signals below r) on a lane each: a malformed proof ends there and nothing is
//   computed with its values.
//   k_pairing_coop, 2 waves:  wave 0 the lines of the group's pairs, a lane per pair; wave 1 the point checks of
//   k_pair_check, a lane per pair, with the endomorphism test.
// Then wave 0 alone runs the Miller loop and the final exponentiation with f in LDS as six Fq2 (the coefficients of
// 1, w, ..., w^5) and every Fq12 product, squaring and line product sliced over its lanes (pairing_coop.hpp: 36 or 18 Fq2
// products at once, six lanes sum).  Frobenius maps and conjugations are a lane per coefficient.  The one inversion is
// f12_inv on lane 0.
//
// Synchronisation.  Workgroup barriers separate the phases and are reached by every wave: none sits inside a role's
// branch, and a wave returns only after the last of them.  No wave waits on a flag.  Inside wave 0 the lanes exchange
// through LDS; the DS operations of one wave complete in order, so wsync() only has to keep the compiler from moving LDS
// accesses across the exchange: a workgroup fence on either side of a wave barrier.  Every sliced operation ends with one,
// so each finds its operands written.
//
// The LDS block, the sliced operations and the body of k_verify_coop are in pairing_coop_dev.hpp, which pairing_set.hip
// runs too.
#include "pairing_coop_dev.hpp"

namespace {

__global__ __launch_bounds__(VERIFY_THREADS) void k_verify_coop(uint8_t *verdict, const uint8_t *__restrict__ proofs, const Fr *__restrict__ publics,
                                                                uint32_t nPublic, const G1Affine *__restrict__ ic, const Line *__restrict__ tab,
                                                                const Fq12 *__restrict__ ml_ab, const PairConsts *__restrict__ k, Line *lines, Fq b1, Fq2 b2,
                                                                Fq beta) {
    const uint64_t i = blockIdx.x;
    verify_coop_proof(verdict + i, proofs + i * 256, publics + i * nPublic, nPublic, ic, tab, ml_ab, k, lines + i * MILLER_LINES, b1, b2, beta);
}

// ---------------------------------------------------------------- a workgroup per group of pairs
__global__ __launch_bounds__(PAIRING_THREADS) void k_pairing_coop(uint8_t *out, const G1Affine *__restrict__ g1, const G2Affine *__restrict__ g2, Line *lines,
                                                                  uint8_t *skip, uint32_t *err, uint64_t n_pairs, uint32_t group, uint32_t flags,
                                                                  const PairConsts *__restrict__ k, Fq b1, Fq2 b2) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t j = blockIdx.x, lo = j * group;
    const uint64_t hi = n_pairs - lo < group ? n_pairs : lo + group;
    if (tid == 0) L.bad_point = 0;
    __syncthreads();
    if (wave == 0) {                                  // a pair with a point at infinity contributes 1: no lines
        for (uint64_t p = lo + lane; p < hi; p += 64) {
            const G2Affine Q = load_pt(g2 + p);
            const bool none = load_pt(g1 + p).is_inf() || Q.is_inf();
            skip[p] = none ? 1 : 0;
            if (!none) line_table(lines + p * MILLER_LINES, Q, *k);
        }
    } else if (flags & COOP_CHECK) {                  // k_pair_check's three words
        for (uint64_t p = lo + lane; p < hi; p += 64) {
            const G1Affine P = load_pt(g1 + p);
            const G2Affine Q = load_pt(g2 + p);
            int bad = -1;
            if (!P.is_inf() && !nl_on_curve(P, b1)) bad = 0;
            if (bad >= 0) atomicMin(err + 0, (uint32_t)p);
            if (!Q.is_inf()) {
                if (!nl_on_curve(Q, b2)) {
                    atomicMin(err + 1, (uint32_t)p);
                    bad = 1;
                } else if (!nl_subgroup(Q, k)) {
                    atomicMin(err + 2, (uint32_t)p);
                    bad = 2;
                }
            }
            if (bad >= 0) L.bad_point = 1;
        }
    }
    __syncthreads();
    if (L.bad_point || wave) return;                  // a bad point is the host's error: nothing more is computed
    c_one(E_IN);
    int at = 0;
    for (int i = 0; i <= 64; i++) {                   // i = 64: the two Frobenius chords
        const int nl = i < 64 ? 1 + (ate_bit(i) ? 1 : 0) : 2;
        if (i < 64) c_mul(E_IN, E_IN, E_IN);
        for (uint64_t p = lo; p < hi; p++) {
            if (skip[p]) continue;                    // the same in every lane
            const Line *lp = lines + p * MILLER_LINES + at;
            for (int q = 0; q < nl; q++) c_line(E_IN, lp + q, g1 + p);
        }
        at += nl;
    }
    Fq *o = reinterpret_cast<Fq *>(out + j * sizeof(Fq12));
    const int src = (flags & COOP_FINAL) ? E_F : E_IN;
    if (flags & COOP_FINAL) c_final_exp(k);
    if (lane < 12) {                                  // Fq number `lane` of the Fq12 in pairing.hpp's layout
        const int slot = lane >> 1, kw = (slot % 3) * 2 + slot / 3;
        const Fq2 c = L.e[src][kw];
        const Fq v = (lane & 1) ? c.b : c.a;
        store_el(o + lane, (flags & COOP_FINAL) ? Fq::from_mont(v) : v);
    }
}

}   // namespace

namespace zk {

void launch_verify_coop(uint8_t *verdict, const uint8_t *proofs, const Fr *publics, uint64_t n, uint32_t nPublic, const G1Affine *ic, const Line *tab,
                        const Fq12 *ml_ab, const PairConsts *k, Line *lines, hipStream_t s) {
    if (!n) return;
    ZK_LAUNCH(k_verify_coop, dim3((uint32_t)n), dim3(VERIFY_THREADS), 0, s, verdict, proofs, publics, nPublic, ic, tab, ml_ab, k, lines, curve_b<Fq>(),
              curve_b<Fq2>(), endo_const<Fq>());
    ZK_LAUNCH_OK("cooperative verification");
}

void launch_pairing_coop(uint8_t *out, const G1Affine *g1, const G2Affine *g2, Line *lines, uint8_t *skip, uint32_t *err, uint64_t n_pairs, uint32_t group,
                         uint32_t flags, const PairConsts *k, hipStream_t s) {
    if (!n_pairs) return;
    const uint64_t jobs = (n_pairs + group - 1) / group;
    ZK_LAUNCH(k_pairing_coop, dim3((uint32_t)jobs), dim3(PAIRING_THREADS), 0, s, out, g1, g2, lines, skip, err, n_pairs, group, flags, k, curve_b<Fq>(),
              curve_b<Fq2>());
    ZK_LAUNCH_OK("cooperative pairing");
}

}   // namespace zk
