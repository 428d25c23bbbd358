// What one proof costs a batch verification by random combination in Fr (include/zkhip.h, zk_plonk_verifier_verify_batch;
// DESIGN.md section 34), as ONE __host__ __device__ function: the proof's nineteen scalars of plonk_verify_lane, each
// times the proof's 128-bit r.  k_plonk_batch_scale (plonkverify_batch.hip) runs it with a lane per proof;
// tools/plonk_batch_host_test.cpp runs the same text on the host against products made from plonk_transcript.hpp's
// lin_scalars.  With it, the arithmetic that cuts a call into chunks and a chunk into groups, for the host and that program.
//
// Nothing here indexes a register array at run time: the nineteen products are made one after the other and each goes
// straight to memory.
#pragma once
#include "plonk_verify_dev.hpp"

namespace zk {

constexpr uint32_t PB_L_TERMS = PV_WZW_U - PV_FIXED, PB_W_TERMS = 2;       // a proof's nine scalars of L and two of W

// 16 bytes little-endian -> the low half of a standard-form element
ZK_HD Fr pb_load_r(const uint8_t *r16) {
    Fr r;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 lo = *reinterpret_cast<const uint4 *>(r16);                // 16-byte aligned: rows of 16 bytes in a hipMalloc'ed buffer
    r.v[0] = lo.x, r.v[1] = lo.y, r.v[2] = lo.z, r.v[3] = lo.w;
#else
    for (int i = 0; i < 4; i++) r.v[i] = (uint32_t)r16[4 * i] | (uint32_t)r16[4 * i + 1] << 8 | (uint32_t)r16[4 * i + 2] << 16 | (uint32_t)r16[4 * i + 3] << 24;
#endif
    r.v[4] = r.v[5] = r.v[6] = r.v[7] = 0;
    return r;
}

// sc: the proof's PV_TERMS scalars `stride` apart, standard form, as plonk_verify_lane wrote them (never read when !ok);
// r16: its scalar.  Written, all in standard form:
//   fx[t fstride] = r s_t, t < PV_FIXED    what the fold sums into the group's S_t
//   lsc[j]        = r s_(9 + j), j < 9     by the proof's points a b c z t_lo t_mid t_hi W_zeta W_zeta_omega, for L
//   wsc[0], [1]   = r, r u                 by W_zeta and W_zeta_omega, for W
// ok false (a malformed proof, the empty slot of a short group): r is taken as 0 and every product is 0 by the same
// multiplication, so that the slot's points take no part in any sum
ZK_HD void plonk_batch_scale_lane(Fr *fx, uint64_t fstride, Fr *lsc, Fr *wsc, const Fr *sc, uint64_t stride, const uint8_t *r16, bool ok) {
    Fr r = pb_load_r(r16);
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = ok ? r.v[i] : 0;
    const Fr rm = Fr::to_mont(r);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint32_t t = 0; t < PV_TERMS; t++) {
        Fr s = Fr::zero();
        if (ok) s = pv_load_el<Fr>(reinterpret_cast<const uint8_t *>(sc + t * stride));
        const Fr p = pv_mul(rm, s);                    // (r R) s / R: standard
        Fr *to = t < PV_FIXED ? fx + t * fstride : t < PV_WZW_U ? lsc + (t - PV_FIXED) : wsc + 1;
        pv_store(reinterpret_cast<uint8_t *>(to), p.v);
    }
    pv_store(reinterpret_cast<uint8_t *>(wsc), r.v);
}

// ---------------------------------------------------------------- chunks and groups
// A call of m proofs under a chunk knob and a group knob: chunks of cap = min(m, chunk) proofs (the last may be short),
// groups of pb_group(cap, group) consecutive proofs inside a chunk (a chunk's last may be short): no group straddles a chunk
ZK_HD uint64_t pb_cap(uint64_t m, uint64_t chunk) { return m < chunk ? m : chunk; }
ZK_HD uint64_t pb_group(uint64_t cap, uint64_t group) { return group < cap ? group : cap; }
ZK_HD uint64_t pb_groups_in(uint64_t cnt, uint64_t g) { return (cnt + g - 1) / g; }
// the groups of the whole call (every proof well-formed)
inline uint64_t pb_groups_of_call(uint64_t m, uint64_t chunk, uint64_t group) {
    if (!m) return 0;
    const uint64_t cap = pb_cap(m, chunk), g = pb_group(cap, group);
    uint64_t n = 0;
    for (uint64_t off = 0; off < m; off += cap) n += pb_groups_in(m - off < cap ? m - off : cap, g);
    return n;
}
// where a group's scalars and points begin: a group's L side is 9 g proof slots and the nine fixed terms, its W side 2 g
ZK_HD uint64_t pb_l_stride(uint64_t g) { return PB_L_TERMS * g + PV_FIXED; }
ZK_HD uint64_t pb_w_stride(uint64_t g) { return PB_W_TERMS * g; }

}   // namespace zk
