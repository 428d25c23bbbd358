// What the PLONK units share and what plonkprove.hip chains.  First the one validation of a zk_plonk_circuit_view and of the
// coset's shift, for zk_plonk_circuit_create, zk_plonk_opening_create and zk_plonk_prover_create (every message under the
// calling entry's name).  Then, unit by unit, what the prover chains (the five rounds of a PLONK proof on one stream,
// nothing per-row crossing PCIe): the device-pointer cores of frscan.hip (round 2), plonkquot.hip (round 3) and plonkopen.hip
// (rounds 4 and 5), the entries that make a circuit and an opening object from a checked view, and kzg.hip's one-lane
// pairing check, the last step of plonkverify.hip.  Each core stays in its unit with its kernels; the public entries of
// those units are thin wrappers over the same cores (check or upload, core, download).  Every core reads its unit's own knob
// (ZKHIP_SCAN_SEG, _QUOT_SEG, _OPEN_SEG).  The transcript and the scalars prover and verifier share: plonk_transcript.hpp.
#pragma once
#include "kzg_internal.hpp"

// ---------------------------------------------------------------- a checked zk_plonk_circuit_view
constexpr uint32_t PLONK_MAX_LOG_N = 25, PLONK_CIRC_VECS = 8;
struct CheckedView {
    uint32_t log_n;
    uint64_t n;
    bool lagrange;
    const uint8_t *vec[PLONK_CIRC_VECS];              // ql qr qm qo qc s1 s2 s3, the view's order: n rows below r each
    Fr k1, k2;                                        // Montgomery
};
// In two steps, since every entry checks its own arguments between them: the dimensions (log_n, basis) ..
inline CheckedView checked_view_dims(const char *who, const zk_plonk_circuit_view *v, uint32_t min_log_n) {
    if (v->log_n < min_log_n || v->log_n > PLONK_MAX_LOG_N)
        throw std::invalid_argument(std::string(who) + ": log_n " + std::to_string(v->log_n) + " is outside " + std::to_string(min_log_n) + " .. 25");
    if (v->basis != ZK_KZG_MONOMIAL && v->basis != ZK_KZG_LAGRANGE) throw std::invalid_argument(std::string(who) + ": basis " + std::to_string(v->basis) + " is unknown");
    CheckedView cv{};
    cv.log_n = v->log_n, cv.n = 1ull << v->log_n, cv.lagrange = v->basis == ZK_KZG_LAGRANGE;
    return cv;
}
// .. then the eight vectors, k1 and k2
inline void checked_view_rows(const char *who, const zk_plonk_circuit_view *v, CheckedView &cv) {
    const uint8_t *vec[PLONK_CIRC_VECS] = {v->ql, v->qr, v->qm, v->qo, v->qc, v->s1, v->s2, v->s3};
    static const char *const names[PLONK_CIRC_VECS] = {"ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3"};
    for (uint32_t j = 0; j < PLONK_CIRC_VECS; j++) {
        if (!vec[j]) throw std::invalid_argument("null argument");
        check_below_r(who, names[j], vec[j], cv.n);
        cv.vec[j] = vec[j];
    }
    cv.k1 = checked_one(who, "k1", v->k1);
    cv.k2 = checked_one(who, "k2", v->k2);
}
// the coset's shift g (a view's: NULL is 5) and g^n, Montgomery.  g^(4n) = 1: the coset is the 4n-th roots of unity themselves
// and Z_H vanishes on a quarter of it
struct CheckedShift {
    Fr g, gn;
};
inline CheckedShift checked_shift(const char *who, const uint8_t *shift, uint32_t log_n) {
    CheckedShift c;
    c.g = shift ? checked_one(who, "shift", shift) : fr_small(5);
    if (c.g.is_zero()) throw std::invalid_argument(std::string(who) + ": shift is zero");
    c.gn = c.g;
    for (uint32_t i = 0; i < log_n; i++) c.gn = Fr::sqr(c.gn);
    if (Fr::sqr(Fr::sqr(c.gn)) == Fr::one()) throw std::invalid_argument(std::string(who) + ": shift^(4n) is 1: Z_H vanishes on the coset");
    return c;
}

// ---------------------------------------------------------------- kzg.hip
// ZK_VERIFY_OK iff e(L, G2) = e(pi, [tau]G2), else ZK_VERIFY_INVALID; L, pi: points of the curve, the file's form
uint8_t kzg_pair_one(zk_kzg *k, const uint8_t L[64], const uint8_t pi[64]);

// ---------------------------------------------------------------- frscan.hip
struct PlonkPerm;                                     // the work buffers of the scan
PlonkPerm *plonk_perm_new();
void plonk_perm_free(PlonkPerm *p);
uint32_t plonk_perm_seg();
uint64_t plonk_perm_need_bytes(uint64_t n);
size_t plonk_perm_bytes(const PlonkPerm *p);
// z[0, n) and last of zk_plonk_permutation_product for three columns, all vectors on the device, standard form; beta,
// gamma: standard, host.  false: a denominator is zero and z was not written.  The stream is drained once inside
bool plonk_perm_dev(PlonkPerm *p, Fr *z, uint8_t last[32], const Fr *wires, const Fr *sigmas, const Fr *shifts, uint32_t log_n, const uint8_t beta[32],
                    const uint8_t gamma[32], hipStream_t s);

// ---------------------------------------------------------------- plonkquot.hip
constexpr uint32_t PLONK_ROWS = 5;                    // a, b, c, z, pi
uint32_t plonk_quot_seg();
// zk_plonk_circuit_create past its checks: the public entry checks its view and calls this, a prover calls it with its own
zk_plonk_circuit *plonk_circuit_make(const CheckedView &cv, const CheckedShift &shift, int32_t device);
uint64_t plonk_circuit_need_bytes(uint32_t log_n);
size_t plonk_circuit_bytes(const zk_plonk_circuit *c);
// where round 3 reads its rows: a | b | c | z (| pi) back to back, lens[] standard rows each (20n rows of room)
Fr *plonk_circuit_rows(zk_plonk_circuit *c);
// zk_plonk_quotient without the staging: t's 4n coefficients (standard, zeros from *t_len on) stay on the device, where the
// return value points, until the object's next call
const Fr *plonk_circuit_quotient_dev(zk_plonk_circuit *c, const uint64_t lens[PLONK_ROWS], uint32_t vecs, const Fr &alpha, const Fr &beta, const Fr &gamma,
                                     uint64_t *t_len, hipStream_t s);
// values at w^i -> coefficients for `batch` <= 5 vectors of n standard rows, `in` n apart, out[v] n rows each: one load, one
// batched inverse transform of size n, a store a vector.  Works in the vectors of a quotient call; `in` and out[] lie elsewhere.
// The tables of size n are made by plonk_circuit_prepare_interpolate, or by the first call
void plonk_circuit_prepare_interpolate(zk_plonk_circuit *c, hipStream_t s);
void plonk_circuit_interpolate_dev(zk_plonk_circuit *c, Fr *const out[], const Fr *in, uint32_t batch, hipStream_t s);

// ---------------------------------------------------------------- plonkopen.hip
uint32_t plonk_open_seg();
// zk_plonk_opening_create past its checks, on the kzg's device: cv.n + 6 <= the kzg's max_coeffs is the caller's check too
zk_plonk_opening *plonk_opening_make(zk_kzg *kzg, const CheckedView &cv);
uint64_t plonk_opening_need_bytes(uint64_t n, uint64_t cap, bool lagrange);
size_t plonk_opening_bytes(const zk_plonk_opening *o);
Fr *plonk_opening_wit(zk_plonk_opening *o, uint32_t j);          // a, b, c, z: max_coeffs rows each
Fr *plonk_opening_part(zk_plonk_opening *o, uint32_t j);         // t_lo, t_mid, t_hi: max_coeffs rows each
const Fr *plonk_opening_circ(const zk_plonk_opening *o, uint32_t j);   // the view's order, n coefficients each
void plonk_opening_clear(zk_plonk_opening *o, hipStream_t s);    // zeros in every row of a proof: a shorter vector reads as padded
// zk_plonk_evaluate and zk_plonk_open over the rows already in the object: len[] of a, b, c, z and tlen[] of the parts of t.
// The scalars are Montgomery.  Both multiplications of plonk_opening_open_dev run over one row more than their quotient has (as
// many rows as the polynomial divided), which the call zeroes after each division: with every len[] equal, all multiplications of
// a proof have one size
void plonk_opening_evaluate_dev(zk_plonk_opening *o, uint8_t evals[6 * 32], const uint64_t len[4], const Fr &zeta, hipStream_t s);
void plonk_opening_open_dev(zk_plonk_opening *o, uint8_t w_zeta[64], uint8_t w_zeta_omega[64], uint8_t r_zeta[32], uint8_t *f, uint64_t *f_len,
                            const uint64_t tlen[3], const Fr &pi_zeta, const Fr &alpha, const Fr &beta, const Fr &gamma, const Fr &v, hipStream_t s);
// The same without the two multiplications, for a prover that multiplies many proofs' quotients at once: the quotients are
// divided straight into the caller's rows (on the object's device, as many rows each as the polynomial divided: its
// quotient and, zeroed here, the one row above it).  The stream is drained once inside, for F(zeta)
void plonk_opening_open_rows_dev(zk_plonk_opening *o, Fr *q_zeta, Fr *q_zeta_omega, uint8_t r_zeta[32], const uint64_t tlen[3], const Fr &pi_zeta,
                                 const Fr &alpha, const Fr &beta, const Fr &gamma, const Fr &v, hipStream_t s);

// ---------------------------------------------------------------- plonkr1cs.hip
struct zk_plonk_r1cs;
struct PlonkR1csDims {
    int device;
    uint32_t log_n;
    uint64_t n, n_wires, n_public, n_witness;
    const uint8_t *k1, *k2;                           // standard, 32 bytes each, the object's
};
PlonkR1csDims plonk_r1cs_dims(const zk_plonk_r1cs *c);
// "witness has 5 values, the r1cs 7 wires"; "<who>: witness 5 is not below r"
void plonk_r1cs_check_witness(const zk_plonk_r1cs *c, const char *who, const uint8_t *wtns, uint32_t nVars);
// w: n_witness standard rows on the object's device whose first n_wires hold a circom witness; the rest is written.  The
// stream is drained once inside
void plonk_r1cs_extend_dev(zk_plonk_r1cs *c, Fr *w, hipStream_t s);
