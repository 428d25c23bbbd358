// What kzg.hip shares with plonkopen.hip (PLONK rounds 4 and 5 divide and commit on a zk_kzg's resident points): the object,
// the buffers of a division by X - z, the division's launcher and the multiplication over resident bases.  The division's
// kernels stay in kzg.hip, and with them launch_divide's body; everything else here is the text kzg.hip held.
#pragma once
#include <memory>
#include <mutex>

#include "hiputil.hpp"
#include "devmem.hpp"
#include "ptcheck.hpp"
#include "pairing.hpp"
#include "paircheck.hpp"
#include "mulglv.hpp"
#include "ptengine.hpp"
#include "pairing_internal.hpp"

constexpr uint32_t DIV_WG = 256, DIV_WAVES = DIV_WG / 64;
constexpr uint32_t KZG_DEFAULT_SEG = 16, KZG_MAX_SEG = 4096;   // the default: the best of profiles/kzg_timing.txt's sweep at 2^20
constexpr uint32_t NO_LEVEL = ZK_KZG_NO_LAGRANGE;

// The weights of one tier of the scan, Montgomery form
struct DivPows {
    Fr z;                                             // between neighbouring elements
    Fr lane[6];                                       // z^(seg 2^k): between lanes 2^k apart
    Fr wave;                                          // z^(64 seg): between waves
};

inline uint32_t kzg_seg_in_effect() {
    return (uint32_t)env_number("ZKHIP_KZG_SEG", KZG_DEFAULT_SEG, 1, KZG_MAX_SEG, "a number of coefficients per lane from 1 to 4096", ENV_LAX);
}

// the sums between the launches; grown, never shrunk
struct DivWork {
    DevBuf<Fr> wsum, gsum, behind;
    DevBuf<DivPows> pows;                             // [0]: the coefficients' tiers, [1]: the carry pass's
    DivPows h[2];                                     // their host image: it outlives the copy (every caller drains the stream before the next division)
    void size(uint64_t groups) {
        if (!pows.p) pows.alloc(2);
        if (gsum.n >= groups) return;
        wsum.alloc(groups * DIV_WAVES);
        gsum.alloc(groups);
        behind.alloc(groups);
    }
    size_t bytes() const { return wsum.bytes() + gsum.bytes() + behind.bytes() + pows.bytes(); }
    static uint64_t groups_of(uint64_t n, uint32_t seg) { return (n + (uint64_t)DIV_WG * seg - 1) / ((uint64_t)DIV_WG * seg); }
};

// q[0, n - 1) and *y from c[0, n), n >= 1, all on the device, standard form; z in Montgomery form (kzg.hip)
void launch_divide(Fr *q, Fr *y, const Fr *c, uint64_t n, const Fr &z, uint32_t seg, DivWork &w, hipStream_t s);

// kzg.hip's two kernels of the pairing check e(L_i, G2) = e(pi_i, [tau]G2) for a caller with tables of its own: the lines of Q[0]
// (the generator of G2) and Q[1] ([tau]G2) into tab[0, 2 * MILLER_LINES); verdict[i] for m openings, MALFORMED where
// status[i] is not ST_OK (such a lane reads neither L nor pi).  All pointers on the device
void launch_kzg_line_tables(Line *tab, const G2Affine *Q, const PairConsts *k, hipStream_t s);
void launch_kzg_pair(uint8_t *verdict, const uint32_t *status, const G1Affine *L, const G1Affine *pi, const Line *tab, uint64_t m, const PairConsts *k,
                     hipStream_t s);

// ---------------------------------------------------------------- host: the multiplication over resident bases
// operators.hip's msm_generic without the upload and the conversion of the bases: pts is already in the kernels' own form
inline void msm_resident(DevMsm<Fq> &e, uint8_t out[64], const G1Affine *pts, const Fr *sc, uint64_t n, hipStream_t s) {
    e.size(n);
    e.sb.run(sc, s);
    launch_msm_accum_g1(e.buckets.p, e.sb.offsets.p, e.sb.entries.p, pts, 0, 0, e.sb.total_buckets(), e.emax, e.ws.p, e.wkey.p, e.wflag.p, s);
    launch_msm_reduce_g1(e.wsum.p, e.scratch.p, e.buckets.p, 1, e.sb.plan, s);
    HIP_TRY(hipMemcpyAsync(e.w.data(), e.wsum.p, e.w.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HostTail::combine_windows_g1(e.w.data(), e.sb.plan.sets, e.sb.plan.c, e.rc, out);
}

inline size_t msm_bytes(const DevMsm<Fq> &e) {
    return e.sb.bytes() + e.buckets.bytes() + e.scratch.bytes() + e.ws.bytes() + e.wsum.bytes() + e.wkey.bytes() + e.wflag.bytes();
}

// ---------------------------------------------------------------- the object
struct zk_kzg {
    int device = 0;
    uint32_t power = 0, lag_log = NO_LEVEL;
    uint64_t max_coeffs = 0, lag_n = 0;
    std::mutex mu;                                    // calls on one object are serialised
    std::unique_ptr<Stream> st;
    Consts kc;
    DevBuf<G1Affine> tau, lag;                        // section 2's first max_coeffs points, level lag_log of section 12: the bucket kernels' form
    DevBuf<Line> tab;                                 // the G2 generator's lines, then [tau]G2's
    DevBuf<Fr> sc, quot, yv;                          // a polynomial, its quotient, its value
    DivWork div;
    DevMsm<Fq> msm;                                   // commit and open; sized for max_coeffs when the object is made
    DevMsm<Fq> bmsm;                                  // verify_batch's three sums over m points: made by the first such call
    uint8_t g1[64];                                   // the generator, the file's form
    uint8_t g2tau[128];                               // [tau]G2, the file's form: what a PLONK key names
    uint32_t last_launches = 0;
    size_t bytes() const {
        return tau.bytes() + lag.bytes() + tab.bytes() + sc.bytes() + quot.bytes() + yv.bytes() + div.bytes() + msm_bytes(msm) + msm_bytes(bmsm) +
               sizeof(PairConsts);
    }
};
