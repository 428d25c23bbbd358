// PLONK batch verification by random combination with every proof's own verdict kept (zk_plonk_verifier_verify_batch,
// include/zkhip.h).  Every well-formed proof i asks e(L_i, G2) = e(W_i, [tau]G2) with the same two
// G2 points, L_i = sum_(t < 18) s_it B_it and W_i = W_zeta,i + s_i18 W_zeta_omega,i (plonk_verify_dev.hpp's scalars).
// Consecutive proofs of a chunk form groups; with a 128-bit scalar r_i != 0 per proof a group passes iff
//     e(L, G2) e(-W, [tau]G2) = 1,
//     L = sum_(t < 9) S_t F_t + sum_i sum_(j < 9) (r_i s_i,9+j) P_ij,   S_t = sum_i r_i s_it (mod r),
//     W = sum_i r_i W_zeta,i + (r_i s_i18) W_zeta_omega,i,
// F_t the key's eight commitments and the generator, P_ij the proof's nine points.  That is no pairing per proof, eleven
// points per proof in two bucket multiplications per group (msm_resident, the library's own), and one cooperative pairing
// product of two pairs per group.  The well-formed proofs of a failing group go through the per-proof kernels of
// plonkverify_dev.hip (launch_per_proof) from the status and scalars the transcript kernel left on the device, all failed
// groups of a chunk before the chunk's verdicts leave, so a verdict differs from zk_plonk_verifier_verify's only when an
// INVALID proof sits in a group that passes: at most one of the 2^128 - 1 values of its scalar does that.
//
// Kernels of this unit, in launch order per chunk (after k_plonk_transcript):
//   k_plonk_batch_scale   a lane per proof slot: plonk_batch_dev.hpp's twenty products, the eleven of L and W as rows of the
//                         two scalar arrays msm_resident reads, the nine fixed-term ones kept for the fold; a malformed
//                         proof and the empty slots of a short group write zeros
//   k_plonk_batch_gather  a lane per point: the proofs' points (768 bytes apart) and the nine fixed bases into the groups'
//                         contiguous arrays, in the bucket kernels' form; (0, 0) where the slot takes no part
//   k_plonk_batch_fold    a workgroup per 256 slots of one group and one term: lanes add across the wave with cross-lane
//                         moves, the four waves through LDS
//   k_plonk_batch_fold2   a wave per (group, term) over the workgroups' sums: S_t, written as the group's last nine scalars
// No atomics on field elements: every sum has a fixed shape, so the bytes do not depend on scheduling.  A workgroup never
// holds slots of two groups, so a group shorter than, equal to or longer than 256 is summed the same way.
#include "plonk_verifier_internal.hpp"
#include "plonk_batch_dev.hpp"
#include "pairing_coop.hpp"
#include "verify_batch_host.hpp"
#include "field29.hpp"

namespace {

constexpr uint32_t FOLD_WG = 256, FOLD_WAVES = FOLD_WG / 64;

// ---------------------------------------------------------------- device
// slot i = g group + k of the chunk's n_slots = ngroups group; proof i when i < cnt
__global__ __launch_bounds__(64) void k_plonk_batch_scale(Fr *fx, Fr *lsc, Fr *wsc, const uint32_t *__restrict__ status, const Fr *__restrict__ sc,
                                                           const uint8_t *__restrict__ r16, uint64_t cnt, uint64_t n_slots, uint64_t group, uint64_t stride) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    const uint64_t g = i / group, k = i - g * group;
    const bool ok = i < cnt && status[i] == PV_OK;
    const uint64_t at = ok ? i : 0;                   // a slot that takes no part reads nothing of its own
    plonk_batch_scale_lane(fx + i, n_slots, lsc + g * pb_l_stride(group) + k * PB_L_TERMS, wsc + g * pb_w_stride(group) + k * PB_W_TERMS, sc + at, stride,
                           r16 + at * 16, ok);
}

__device__ __forceinline__ void store_internal(G1Affine *to, const G1Affine &p) {
    store_el(&to->x, Fq29::store(Fq29::from_mont256(p.x)));
    store_el(&to->y, Fq29::store(Fq29::from_mont256(p.y)));
}

// lane q of group g's 11 group + 9 points: the nine points of L a slot, the nine fixed bases (already in the kernels'
// form), then W_zeta and W_zeta_omega a slot
__global__ __launch_bounds__(256) void k_plonk_batch_gather(G1Affine *lpt, G1Affine *wpt, const uint32_t *__restrict__ status, const uint8_t *__restrict__ proofs,
                                                             const G1Affine *__restrict__ fixed, uint64_t cnt, uint64_t ngroups, uint64_t group) {
    const uint64_t per = pb_l_stride(group) + pb_w_stride(group);
    const uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= ngroups * per) return;
    const uint64_t g = lane / per, q = lane - g * per;
    G1Affine *to;
    uint64_t k;
    uint32_t j;
    if (q < PB_L_TERMS * group) {
        k = q / PB_L_TERMS;
        j = (uint32_t)(q - k * PB_L_TERMS);
        to = lpt + g * pb_l_stride(group) + q;
    } else if (q < pb_l_stride(group)) {
        const uint64_t t = q - PB_L_TERMS * group;
        const G1Affine b = load_pt(fixed + t);
        to = lpt + g * pb_l_stride(group) + q;
        store_el(&to->x, b.x);
        store_el(&to->y, b.y);
        return;
    } else {
        const uint64_t w = q - pb_l_stride(group);
        k = w / PB_W_TERMS;
        j = (uint32_t)(PV_POINTS - PB_W_TERMS + (w - k * PB_W_TERMS));
        to = wpt + g * pb_w_stride(group) + w;
    }
    const uint64_t i = g * group + k;
    G1Affine p{Fq::zero(), Fq::zero()};
    if (i < cnt && status[i] == PV_OK) p = load_pt(reinterpret_cast<const G1Affine *>(proofs + i * PV_PROOF_BYTES) + j);
    store_internal(to, p);
}

// the lanes of a wave: lane 0 ends with the sum of all 64 (a lane near the top adds its own value where there is no lane
// d places up; those lanes' results are not used)
__device__ __forceinline__ Fr wave_sum(Fr acc) {
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) acc = Fr::add(acc, shfl_down_fr(acc, d));
    return acc;
}

// workgroup (g bpg + b, t): partial[t n_part + g bpg + b] = the sum of fx[t][g group + 256 b ..], as far as the group goes
__global__ __launch_bounds__(FOLD_WG) void k_plonk_batch_fold(Fr *partial, const Fr *__restrict__ fx, uint64_t n_slots, uint64_t group, uint32_t bpg,
                                                               uint64_t n_part) {
    __shared__ Fr wsum[FOLD_WAVES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, t = blockIdx.y;
    const uint64_t g = blockIdx.x / bpg, b = blockIdx.x - g * bpg;
    const uint64_t k = b * FOLD_WG + tid;
    Fr acc = Fr::zero();
    if (k < group) acc = load_el(fx + t * n_slots + g * group + k);
    acc = wave_sum(acc);
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        Fr s = wsum[0];
#pragma unroll
        for (uint32_t w = 1; w < FOLD_WAVES; w++) s = Fr::add(s, wsum[w]);
        store_el(partial + t * n_part + blockIdx.x, s);
    }
}

// wave (g, t): S_t of group g = the sum of its bpg workgroup sums, the group's scalar 9 group + t
__global__ __launch_bounds__(64) void k_plonk_batch_fold2(Fr *lsc, const Fr *__restrict__ partial, uint64_t group, uint32_t bpg, uint64_t n_part) {
    const uint32_t lane = threadIdx.x, t = blockIdx.y;
    const uint64_t g = blockIdx.x;
    Fr acc = Fr::zero();
    for (uint32_t b = lane; b < bpg; b += 64) acc = Fr::add(acc, load_el(partial + t * n_part + g * bpg + b));
    acc = wave_sum(acc);
    if (lane == 0) store_el(lsc + g * pb_l_stride(group) + PB_L_TERMS * group + t, acc);
}

// ---------------------------------------------------------------- host
const char *const WHO_BATCH = "zk_plonk_verifier_verify_batch", *const WHO_SUMS = "zk_plonk_verifier_batch_sums";

// the object's batch buffers for chunks of `cap` proofs in groups of `group`: made by the first batch call, re-made when the
// group changes or the chunk grows.  Free HBM is checked first, with what the chunk's own buffers will ask for
void batch_size(zk_plonk_verifier *v, const char *who, uint64_t cap, uint64_t group, hipStream_t s) {
    PlonkBatchBufs &b = v->batch;
    if (b.group == group && cap <= b.cap) return;
    const bool first = !b.fixed.p;
    b.cap = b.group = b.ngroups = 0;
    b.r16.release(), b.fx.release(), b.partial.release(), b.lsc.release(), b.wsc.release(), b.lpt.release(), b.wpt.release();
    need_hbm(who, PlonkBatchBufs::bytes_for(cap, group) + (cap > v->cap ? zk_plonk_verifier::chunk_bytes(cap, v->n_public) : 0));
    if (first) {                                      // what no size changes
        b.fixed.alloc(PV_FIXED);
        HIP_TRY(hipMemcpyAsync(b.fixed.p, v->fixed.p, PV_FIXED * sizeof(G1Affine), hipMemcpyDeviceToDevice, s));
        launch_fq_to_internal(reinterpret_cast<Fq *>(b.fixed.p), PV_FIXED * 2, s);
        b.p1.alloc(2 * PLONK_BATCH_SLICE);
        b.p2.alloc(2 * PLONK_BATCH_SLICE);
        b.lines.alloc(2 * PLONK_BATCH_SLICE * MILLER_LINES);
        b.skip.alloc(2 * PLONK_BATCH_SLICE);
        b.out.alloc(PLONK_BATCH_SLICE * sizeof(Fq12));
        b.err.alloc(3);
        std::vector<uint8_t> q2(PLONK_BATCH_SLICE * sizeof v->q2);
        for (uint64_t g = 0; g < PLONK_BATCH_SLICE; g++) memcpy(q2.data() + g * sizeof v->q2, v->q2, sizeof v->q2);
        HIP_TRY(hipMemcpyAsync(b.p2.p, q2.data(), q2.size(), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(b.err.p, 0xFF, 12, s));
        HIP_TRY(hipStreamSynchronize(s));             // q2 leaves scope
    }
    const uint64_t ng = pb_groups_in(cap, group);
    b.r16.alloc(cap * 16);
    b.fx.alloc(ng * group * PV_FIXED);
    b.partial.alloc(ng * PlonkBatchBufs::fold_blocks(group) * PV_FIXED);
    b.lsc.alloc(ng * pb_l_stride(group));
    b.lpt.alloc(ng * pb_l_stride(group));
    b.wsc.alloc(ng * pb_w_stride(group));
    b.wpt.alloc(ng * pb_w_stride(group));
    b.lmsm.size(pb_l_stride(group));
    b.wmsm.size(pb_w_stride(group));
    b.cap = cap, b.group = group, b.ngroups = ng;
}

// One chunk as far as the groups' sums.  On return: status (host) of the chunk's proofs, well[g] the well-formed proofs
// of group g, and sums[g] = L | W (the file's form) of every group with one; the transcript's status and scalars stay on
// the device for a recheck
struct ChunkSums {
    std::vector<uint32_t> status;
    std::vector<uint64_t> well;
    std::vector<uint8_t> sums, drawn;
    uint64_t ngroups = 0, malformed = 0;
};
void chunk_sums(zk_plonk_verifier *v, const char *who, ChunkSums &c, uint64_t cnt, const uint8_t *scalars16, hipStream_t s) {
    PlonkBatchBufs &b = v->batch;
    const uint64_t group = b.group, ng = pb_groups_in(cnt, group), n_slots = ng * group;
    c.ngroups = ng;
    c.status.resize(cnt);
    c.well.assign(ng, 0);
    c.sums.assign(ng * 128, 0);
    launch_transcript(v, cnt, true, s);
    ZK_LAUNCH_OK("plonk transcript");
    HIP_TRY(hipMemcpyAsync(c.status.data(), v->status.p, cnt * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    uint64_t well = 0;
    for (uint64_t i = 0; i < cnt; i++)
        if (c.status[i] == PV_OK) c.well[i / group]++, well++;
    c.malformed = cnt - well;
    if (!well) return;                                // nothing to combine: no launch
    if (!scalars16) {                                 // drawn now: the proofs of this call are fixed
        c.drawn.resize(cnt * 16);
        draw_scalars(c.drawn.data(), cnt, who);
        scalars16 = c.drawn.data();
    }
    HIP_TRY(hipMemcpyAsync(b.r16.p, scalars16, cnt * 16, hipMemcpyHostToDevice, s));
    const uint32_t bpg = (uint32_t)PlonkBatchBufs::fold_blocks(group);
    const uint64_t n_part = ng * bpg;
    ZK_LAUNCH(k_plonk_batch_scale, dim3(nblocks(n_slots, 64)), dim3(64), 0, s, b.fx.p, b.lsc.p, b.wsc.p, v->status.p, v->sc.p, b.r16.p, cnt, n_slots, group, v->cap);
    ZK_LAUNCH(k_plonk_batch_gather, dim3(nblocks(ng * (pb_l_stride(group) + pb_w_stride(group)), 256)), dim3(256), 0, s, b.lpt.p, b.wpt.p, v->status.p, v->proofs.p,
              b.fixed.p, cnt, ng, group);
    ZK_LAUNCH(k_plonk_batch_fold, dim3((uint32_t)n_part, PV_FIXED), dim3(FOLD_WG), 0, s, b.partial.p, b.fx.p, n_slots, group, bpg, n_part);
    ZK_LAUNCH(k_plonk_batch_fold2, dim3((uint32_t)ng, PV_FIXED), dim3(64), 0, s, b.lsc.p, b.partial.p, group, bpg, n_part);
    ZK_LAUNCH_OK("plonk batch verification: scalars and points");
    for (uint64_t g = 0; g < ng; g++) {
        if (!c.well[g]) continue;
        msm_resident(b.lmsm, c.sums.data() + g * 128, b.lpt.p + g * pb_l_stride(group), b.lsc.p + g * pb_l_stride(group), pb_l_stride(group), s);
        msm_resident(b.wmsm, c.sums.data() + g * 128 + 64, b.wpt.p + g * pb_w_stride(group), b.wsc.p + g * pb_w_stride(group), pb_w_stride(group), s);
    }
}

void group_equations(zk_plonk_verifier *v, std::vector<uint8_t> &pass, const ChunkSums &c, const std::vector<uint64_t> &at, hipStream_t s) {
    PlonkBatchBufs &b = v->batch;
    plonk_group_equations(PlonkPairBufs{b.p1.p, b.p2.p, b.lines.p, b.skip.p, b.out.p, b.err.p}, v->kc.k.p, pass, c.sums.data(), at, s);
}

// what both entries check before a device is touched; false: m = 0
bool batch_checks(zk_plonk_verifier *v, const char *who, const uint8_t *proofs, const uint8_t *publics, uint64_t m, const uint8_t *scalars16, const void *out) {
    if (!v) throw std::invalid_argument("null argument");
    if (!m) return false;
    if (m >= (1ull << 31)) throw std::invalid_argument(std::string(who) + ": m is not below 2^31");
    if (!proofs || !out || (v->n_public && !publics)) throw std::invalid_argument("null argument");
    refuse_zero_scalars(scalars16, m, who);
    return true;
}

void verify_batch(zk_plonk_verifier *v, const uint8_t *proofs, const uint8_t *publics, uint64_t m, const uint8_t *scalars16, uint8_t *verdict,
                  zk_plonk_batch_report *report) {
    const uint32_t rep_size = report_size(report);
    zk_plonk_batch_report rep;
    memset(&rep, 0, sizeof rep);
    const uint64_t knob = plonk_verify_group_in_effect();
    rep.size = rep_size;
    rep.group = (uint32_t)knob;
    auto leave = [&]() {
        if (report) memcpy(report, &rep, rep_size);
    };
    if (!batch_checks(v, WHO_BATCH, proofs, publics, m, scalars16, verdict)) {
        leave();
        return;
    }
    ChunkSums c;
    std::vector<uint64_t> at;
    std::vector<uint8_t> pass;
    over_chunks(
        v, WHO_BATCH, proofs, publics, m, verdict, verdict,
        [&](uint64_t off, uint64_t cnt, hipStream_t s) {
            const uint64_t group = v->batch.group;
            chunk_sums(v, WHO_BATCH, c, cnt, scalars16 ? scalars16 + off * 16 : nullptr, s);
            rep.malformed += c.malformed;
            for (uint64_t i = 0; i < cnt; i++) verdict[off + i] = c.status[i] == PV_OK ? ZK_VERIFY_OK : ZK_VERIFY_MALFORMED;
            at.clear();
            for (uint64_t g = 0; g < c.ngroups; g++)
                if (c.well[g]) at.push_back(g);
            rep.groups += at.size();
            if (at.empty()) return;
            group_equations(v, pass, c, at, s);
            // the failed groups of this chunk through the per-proof kernels, neighbours in one pass; a malformed proof among
            // them keeps its MALFORMED there too
            for (uint64_t q = 0; q < at.size();) {
                if (pass[q]) {
                    q++;
                    continue;
                }
                uint64_t e = q;
                while (e + 1 < at.size() && !pass[e + 1] && at[e + 1] == at[e] + 1) e++;
                const uint64_t lo = at[q] * group, hi = (at[e] + 1) * group < cnt ? (at[e] + 1) * group : cnt;
                for (uint64_t g = q; g <= e; g++) rep.proofs_rechecked += c.well[at[g]];
                rep.groups_failed += e - q + 1;
                launch_per_proof(v, lo, hi - lo, s);
                HIP_TRY(hipMemcpyAsync(verdict + off + lo, v->verdict.p + lo, hi - lo, hipMemcpyDeviceToHost, s));
                q = e + 1;
            }
            HIP_TRY(hipStreamSynchronize(s));
        },
        [&](uint64_t cap) {
            rep.group = (uint32_t)pb_group(cap, knob);
            batch_size(v, WHO_BATCH, cap, rep.group, v->st->s);
        });
    rep.launches = v->last_launches;
    rep.chunks = v->last_chunks;
    leave();
}

void batch_sums(zk_plonk_verifier *v, const uint8_t *proofs, const uint8_t *publics, uint64_t m, const uint8_t *scalars16, uint8_t *sums, uint64_t sums_cap,
                uint64_t *n_groups) {
    if (!n_groups) throw std::invalid_argument("null argument");
    *n_groups = 0;
    const uint64_t knob = plonk_verify_group_in_effect();
    if (!batch_checks(v, WHO_SUMS, proofs, publics, m, scalars16, sums)) return;
    if (!scalars16) throw std::invalid_argument("null argument");
    const uint64_t want = pb_groups_of_call(m, plonk_verify_chunk_in_effect(), knob);
    if (sums_cap < want) throw std::invalid_argument(std::string(WHO_SUMS) + ": sums_cap " + std::to_string(sums_cap) + " is below the call's " + std::to_string(want) + " groups");
    ChunkSums c;
    uint64_t written = 0;
    over_chunks(
        v, WHO_SUMS, proofs, publics, m, sums, sums,
        [&](uint64_t off, uint64_t cnt, hipStream_t s) {
            chunk_sums(v, WHO_SUMS, c, cnt, scalars16 + off * 16, s);
            memcpy(sums + written * 128, c.sums.data(), c.ngroups * 128);
            written += c.ngroups;
        },
        [&](uint64_t cap) { batch_size(v, WHO_SUMS, cap, pb_group(cap, knob), v->st->s); });
    *n_groups = written;
}

}   // namespace

// ---------------------------------------------------------------- what plonkverify_set.hip runs too (plonk_verifier_internal.hpp)
// pass[q] for the groups at[q] of sums (L | W a group): e(L, G2) e(-W, [tau]G2) = 1.  A pair with a point at infinity contributes 1
// in k_pairing_coop (its `skip`), which is the value of that pairing, so L or W at infinity needs no path of its own
void plonk_group_equations(const PlonkPairBufs &b, const PairConsts *k, std::vector<uint8_t> &pass, const uint8_t *sums, const std::vector<uint64_t> &at, hipStream_t s) {
    uint8_t one[sizeof(Fq12)] = {1};
    std::vector<uint8_t> pairs(2 * PLONK_BATCH_SLICE * 64), out(PLONK_BATCH_SLICE * sizeof(Fq12));
    pass.assign(at.size(), 0);
    for (uint64_t lo = 0; lo < at.size(); lo += PLONK_BATCH_SLICE) {
        const uint64_t n = at.size() - lo < PLONK_BATCH_SLICE ? at.size() - lo : PLONK_BATCH_SLICE;
        for (uint64_t q = 0; q < n; q++) {
            const uint8_t *lw = sums + at[lo + q] * 128;
            memcpy(pairs.data() + q * 128, lw, 64);
            memcpy(pairs.data() + q * 128 + 64, Pt<Fq>(lw + 64).neg().b, 64);
        }
        HIP_TRY(hipMemcpyAsync(b.p1, pairs.data(), n * 128, hipMemcpyHostToDevice, s));
        launch_pairing_coop(b.out, b.p1, b.p2, b.lines, b.skip, b.err, 2 * n, 2, COOP_FINAL, k, s);
        HIP_TRY(hipMemcpyAsync(out.data(), b.out, n * sizeof(Fq12), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (uint64_t q = 0; q < n; q++) pass[lo + q] = memcmp(out.data() + q * sizeof(Fq12), one, sizeof one) == 0;
    }
}

extern "C" {

int zk_plonk_verifier_verify_batch(zk_plonk_verifier *v, const uint8_t *proofs, const uint8_t *publics, uint64_t m, const uint8_t *scalars16, uint8_t *verdict,
                                   zk_plonk_batch_report *report) {
    return guarded([&] { verify_batch(v, proofs, publics, m, scalars16, verdict, report); });
}

int zk_plonk_verifier_batch_sums(zk_plonk_verifier *v, const uint8_t *proofs, const uint8_t *publics, uint64_t m, const uint8_t *scalars16, uint8_t *sums,
                                 uint64_t sums_cap, uint64_t *n_groups) {
    return guarded([&] { batch_sums(v, proofs, publics, m, scalars16, sums, sums_cap, n_groups); });
}

}   // extern "C"
