// PLONK verifier over a key set (include/zkhip.h, zk_plonk_verifier_set_*): proofs under many keys
// that share one [tau]G2, each labelled with its key, in one call.  PLONK's setup is universal, so every key of a set has the
// same two G2 points: one pair of line tables and the generator serve all keys, and a key costs its PlonkVerifyConsts
// record and its eight commitments.  A chunk's proofs are ORDERED BY KEY (keys rising, a key's proofs in the caller's
// order; plonk_set_plan.hpp) through an index array the kernels read, src[slot] = the proof's position: the proofs and the
// publics are uploaded as the caller holds them, and the lanes of a wave mostly share a key.
//
// Per-proof path, four launches a chunk whatever the keys:
//   k_plonk_set_transcript  a lane per slot: plonk_verify_dev.hpp's plonk_verify_lane as it is, over K[key[slot]] and the
//                           slot's publics at their ragged offset
//   k_plonk_set_combine     a lane per (slot, term), term-major: the base is fixed[8 key + t], the shared generator, or the
//                           proof's point
//   k_plonk_set_sum         a lane per slot: L and W, affine
//   k_kzg_pair              kzg.hip's, over the set's tables
// Batch path (one equation a group of consecutive slots, any number of keys a group), after the transcript:
//   k_plonk_set_scale       a lane per slot: plonk_batch_dev.hpp's twenty products, the scalar read at the proof's position
//   k_plonk_set_gather      a lane per point of the groups' arrays: 9 group proof points, 8 bases a segment, the generator,
//                           then (0, 0) with a zero scalar up to the stride; and the two points a slot of W
//   k_plonk_set_fold        THE SEGMENTED FOLD, first pass: a workgroup per 256 slots of one range of the plan (a segment: the
//                           eight key terms; a group: the generator's term) and one term; lanes add across the wave with
//                           cross-lane moves, the four waves through LDS
//   k_plonk_set_fold2       second pass: a wave per (range, term) over the range's workgroup sums, written where the
//                           bucket multiplication reads the range's scalars
// No atomics on field elements: the plan fixes every sum's shape, so the bytes do not depend on scheduling.  A segment of
// one proof, one of malformed proofs alone (sum 0) and one longer than a workgroup take the same two passes.
#include "plonk_verifier_internal.hpp"
#include "plonk_transcript.hpp"
#include "plonk_batch_dev.hpp"
#include "plonk_set_plan.hpp"
#include "verify_batch_host.hpp"
#include "field29.hpp"

namespace {

constexpr uint32_t MAX_KEYS = 65536;
constexpr uint32_t FOLD_WAVES = PS_FOLD_WG / 64;

// ---------------------------------------------------------------- device: the per-proof path
__global__ __launch_bounds__(64) void k_plonk_set_transcript(uint32_t *status, uint8_t *ch, Fr *sc, const uint8_t *__restrict__ proofs,
                                                              const uint8_t *__restrict__ publics, const uint32_t *__restrict__ src,
                                                              const uint32_t *__restrict__ key, const uint64_t *__restrict__ pub_at, uint64_t m, uint64_t stride,
                                                              const PlonkVerifyConsts *__restrict__ K, uint32_t want_scalars) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    status[i] = plonk_verify_lane(K[key[i]], proofs + (uint64_t)src[i] * PV_PROOF_BYTES, publics + pub_at[i], ch + i * PV_CHALLENGES * 32,
                                  want_scalars ? sc + i : nullptr, stride, nullptr);
}

// part[t stride + i] = sc[t stride + i] B: B the commitment t of the slot's key, the generator, or the proof's point
__global__ __launch_bounds__(64) void k_plonk_set_combine(G1XYZZ *part, const uint32_t *__restrict__ status, const Fr *__restrict__ sc,
                                                           const uint8_t *__restrict__ proofs, const uint32_t *__restrict__ src, const uint32_t *__restrict__ key,
                                                           const G1Affine *__restrict__ fixed, const G1Affine *__restrict__ gen, uint64_t m, uint64_t stride, Fq endo) {
    const uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= m * PV_TERMS) return;
    const uint32_t t = (uint32_t)(lane / m);
    const uint64_t i = lane - (uint64_t)t * m;
    if (status[i] != PV_OK) return;
    const uint32_t j = t == PV_WZW_U ? PV_POINTS - 1 : t - PV_FIXED;           // the proof's point, t >= PV_FIXED
    const G1Affine *base = t < PV_KEY_POINTS ? fixed + (uint64_t)key[i] * PV_KEY_POINTS + t
                           : t == PV_G       ? gen
                                             : reinterpret_cast<const G1Affine *>(proofs + (uint64_t)src[i] * PV_PROOF_BYTES) + j;
    store_pt(part + t * stride + i, mul_glv(load_pt(base), load_el(sc + t * stride + i), endo));
}

__global__ __launch_bounds__(64) void k_plonk_set_sum(G1Affine *L, G1Affine *W, const uint32_t *__restrict__ status, const G1XYZZ *__restrict__ part,
                                                       const uint8_t *__restrict__ proofs, const uint32_t *__restrict__ src, uint64_t m, uint64_t stride) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || status[i] != PV_OK) return;
    G1XYZZ acc = load_pt(part + i);
#pragma unroll 1
    for (uint32_t t = 1; t < PV_WZW_U; t++) add(acc, load_pt(part + t * stride + i));
    const G1Affine l = g1_to_affine(acc);
    acc = load_pt(part + PV_WZW_U * stride + i);
    madd(acc, load_pt(reinterpret_cast<const G1Affine *>(proofs + (uint64_t)src[i] * PV_PROOF_BYTES) + P_WZ));
    const G1Affine w = g1_to_affine(acc);
    store_el(&L[i].x, l.x);
    store_el(&L[i].y, l.y);
    store_el(&W[i].x, w.x);
    store_el(&W[i].y, w.y);
}

// ---------------------------------------------------------------- device: the batch path
// slot i = g group + k of the chunk's n_slots = ngroups group; a proof when i < cnt.  lstride: a group's L array
__global__ __launch_bounds__(64) void k_plonk_set_scale(Fr *fx, Fr *lsc, Fr *wsc, const uint32_t *__restrict__ status, const Fr *__restrict__ sc,
                                                         const uint8_t *__restrict__ r16, const uint32_t *__restrict__ src, uint64_t cnt, uint64_t n_slots,
                                                         uint64_t group, uint64_t lstride, uint64_t stride) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    const uint64_t g = i / group, k = i - g * group;
    const bool ok = i < cnt && status[i] == PV_OK;
    const uint64_t at = ok ? i : 0;                   // a slot that takes no part reads nothing of its own
    plonk_batch_scale_lane(fx + i, n_slots, lsc + g * lstride + k * PB_L_TERMS, wsc + g * pb_w_stride(group) + k * PB_W_TERMS, sc + at, stride,
                           r16 + (ok ? (uint64_t)src[i] : 0) * 16, ok);
}

__device__ __forceinline__ void store_internal(G1Affine *to, const G1Affine &p) {
    store_el(&to->x, Fq29::store(Fq29::from_mont256(p.x)));
    store_el(&to->y, Fq29::store(Fq29::from_mont256(p.y)));
}

// lane q of group g's lstride + 2 group points.  L: nine points a slot, then eight bases a segment of the group (bfixed: the
// keys' commitments and, last, the generator, already in the bucket kernels' form), the generator, and (0, 0) with a zero
// scalar up to lstride.  W: W_zeta and W_zeta_omega a slot
__global__ __launch_bounds__(256) void k_plonk_set_gather(G1Affine *lpt, G1Affine *wpt, Fr *lsc, const uint32_t *__restrict__ status,
                                                           const uint8_t *__restrict__ proofs, const uint32_t *__restrict__ src,
                                                           const G1Affine *__restrict__ bfixed, uint64_t n_keys, const uint32_t *__restrict__ group_seg0,
                                                           const uint32_t *__restrict__ seg_key, uint64_t cnt, uint64_t ngroups, uint64_t group, uint64_t lstride) {
    const uint64_t per = lstride + pb_w_stride(group);
    const uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= ngroups * per) return;
    const uint64_t g = lane / per, q = lane - g * per;
    G1Affine *to;
    uint64_t k;
    uint32_t j;
    if (q < PB_L_TERMS * group) {
        k = q / PB_L_TERMS;
        j = (uint32_t)(q - k * PB_L_TERMS);
        to = lpt + g * lstride + q;
    } else if (q < lstride) {
        const uint64_t e = q - PB_L_TERMS * group, sg = e / PS_KEY_TERMS;
        const uint32_t s0 = group_seg0[g], nseg = group_seg0[g + 1] - s0;
        to = lpt + g * lstride + q;
        if (sg < nseg || e == (uint64_t)PS_KEY_TERMS * nseg) {
            const G1Affine b = load_pt(sg < nseg ? bfixed + (uint64_t)seg_key[s0 + sg] * PS_KEY_TERMS + (e - sg * PS_KEY_TERMS) : bfixed + n_keys * PS_KEY_TERMS);
            store_el(&to->x, b.x);
            store_el(&to->y, b.y);
        } else {
            store_internal(to, G1Affine{Fq::zero(), Fq::zero()});
            store_el(lsc + g * lstride + q, Fr::zero());
        }
        return;
    } else {
        const uint64_t w = q - lstride;
        k = w / PB_W_TERMS;
        j = (uint32_t)(PV_POINTS - PB_W_TERMS + (w - k * PB_W_TERMS));
        to = wpt + g * pb_w_stride(group) + w;
    }
    const uint64_t i = g * group + k;
    G1Affine p{Fq::zero(), Fq::zero()};
    if (i < cnt && status[i] == PV_OK) p = load_pt(reinterpret_cast<const G1Affine *>(proofs + (uint64_t)src[i] * PV_PROOF_BYTES) + j);
    store_internal(to, p);
}

// the lanes of a wave: lane 0 ends with the sum of all 64 (the other lanes' results are not used)
__device__ __forceinline__ Fr wave_sum(Fr acc) {
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) acc = Fr::add(acc, shfl_down_fr(acc, d));
    return acc;
}

// workgroup (x, y): x names a range r of the plan and its workgroup b; partial[y n_blocks + x] = the sum of
// fx[r.t0 + y][r.lo + 256 b ..], as far as the range goes.  A range with fewer than eight terms leaves the other rows alone
__global__ __launch_bounds__(PS_FOLD_WG) void k_plonk_set_fold(Fr *partial, const Fr *__restrict__ fx, const PsRange *__restrict__ ranges,
                                                                const PsBlock *__restrict__ blocks, uint64_t n_slots, uint32_t n_blocks) {
    __shared__ Fr wsum[FOLD_WAVES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, y = blockIdx.y;
    const PsBlock bl = blocks[blockIdx.x];
    const PsRange r = ranges[bl.range];
    if (y >= r.nterms) return;                        // the whole workgroup
    const uint64_t k = (uint64_t)r.lo + (uint64_t)bl.b * PS_FOLD_WG + tid;
    Fr acc = Fr::zero();
    if (k < r.hi) acc = load_el(fx + (uint64_t)(r.t0 + y) * n_slots + k);
    acc = wave_sum(acc);
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        Fr s = wsum[0];
#pragma unroll
        for (uint32_t w = 1; w < FOLD_WAVES; w++) s = Fr::add(s, wsum[w]);
        store_el(partial + (uint64_t)y * n_blocks + blockIdx.x, s);
    }
}

// wave (range, y): the sum of the range's workgroup sums of term y, the scalar of the range's base y
__global__ __launch_bounds__(64) void k_plonk_set_fold2(Fr *lsc, const Fr *__restrict__ partial, const PsRange *__restrict__ ranges, uint32_t n_blocks) {
    const uint32_t lane = threadIdx.x, y = blockIdx.y;
    const PsRange r = ranges[blockIdx.x];
    if (y >= r.nterms) return;
    Fr acc = Fr::zero();
    for (uint32_t b = lane; b < r.nblk; b += 64) acc = Fr::add(acc, load_el(partial + (uint64_t)y * n_blocks + r.blk0 + b));
    acc = wave_sum(acc);
    if (lane == 0) store_el(lsc + r.out + y, acc);
}

}   // namespace

// ---------------------------------------------------------------- the object
struct PlonkSetBatchBufs {
    uint64_t cap = 0, group = 0, ngroups = 0, lstride = 0, segs = 0, ranges = 0, blocks = 0;   // what the buffers were made for
    DevBuf<G1Affine> fixed;                           // 8 n_keys commitments and the generator in the bucket kernels' form: made once
    DevBuf<uint8_t> r16;                              // cap x 16 bytes, the caller's order
    DevBuf<Fr> fx, partial;                           // PV_FIXED rows of ngroups group slots; PS_KEY_TERMS rows of the fold's workgroup sums
    DevBuf<Fr> lsc, wsc;                              // a group: lstride scalars; 2 group scalars
    DevBuf<G1Affine> lpt, wpt;                        // their points, the bucket kernels' form
    DevBuf<uint32_t> group_seg0, seg_key;             // the plan of a chunk
    DevBuf<PsRange> d_ranges;
    DevBuf<PsBlock> d_blocks;
    DevMsm<Fq> lmsm, wmsm;
    DevBuf<G1Affine> p1;                              // the pairs of a slice: L, -W a group
    DevBuf<G2Affine> p2;                              // G2, [tau]G2 a group
    DevBuf<Line> lines;
    DevBuf<uint8_t> skip, out;
    DevBuf<uint32_t> err;
    static uint64_t bytes_for(uint64_t cap_, uint64_t group_, uint64_t lstride_, uint64_t segs_, uint64_t ranges_, uint64_t blocks_, uint64_t n_keys) {
        const uint64_t ng = (cap_ + group_ - 1) / group_;
        return cap_ * 16 + ng * group_ * PV_FIXED * sizeof(Fr) + blocks_ * PS_KEY_TERMS * sizeof(Fr) +
               ng * (lstride_ + 2 * group_) * (sizeof(Fr) + sizeof(G1Affine)) + (ng + 1 + segs_) * 4 + ranges_ * sizeof(PsRange) + blocks_ * sizeof(PsBlock) +
               DevMsm<Fq>::bytes(lstride_) + DevMsm<Fq>::bytes(2 * group_) +
               PLONK_BATCH_SLICE * (2 * (sizeof(G1Affine) + sizeof(G2Affine) + MILLER_LINES * sizeof(Line) + 1) + sizeof(Fq12)) +
               (n_keys * PS_KEY_TERMS + 1) * sizeof(G1Affine) + 65536;
    }
    size_t bytes() const {
        return fixed.bytes() + r16.bytes() + fx.bytes() + partial.bytes() + lsc.bytes() + wsc.bytes() + lpt.bytes() + wpt.bytes() + group_seg0.bytes() +
               seg_key.bytes() + d_ranges.bytes() + d_blocks.bytes() + msm_bytes(lmsm) + msm_bytes(wmsm) + p1.bytes() + p2.bytes() + lines.bytes() +
               skip.bytes() + out.bytes() + err.bytes();
    }
};

struct zk_plonk_verifier_set {
    int device = 0;
    std::vector<uint64_t> n_public;                   // per key
    uint64_t max_n_public = 0;
    std::mutex mu;                                    // calls on one object are serialised
    std::unique_ptr<Stream> st;
    Consts kc;
    DevBuf<Line> tab;                                 // the G2 generator's lines, then [tau]G2's: one pair for every key
    DevBuf<G1Affine> fixed, gen;                      // eight commitments a key; the generator once: the file's form
    DevBuf<PlonkVerifyConsts> kv;                     // a record a key
    Fq endo;
    uint8_t q2[2 * sizeof(G2Affine)];                 // the generator of G2 and [tau]G2, the file's form
    // a chunk of proofs; grown, never shrunk
    uint64_t cap = 0, pub_cap = 0;
    DevBuf<uint8_t> proofs, publics, ch, verdict;
    DevBuf<uint32_t> status, src, key;
    DevBuf<uint64_t> pub_at;
    DevBuf<Fr> sc;                                    // PV_TERMS rows of cap
    DevBuf<G1XYZZ> part;
    DevBuf<G1Affine> L, W;
    PlonkSetBatchBufs batch;
    std::unique_ptr<PlonkSetChunk> plan;              // the chunk in hand
    uint32_t last_launches = 0, last_chunks = 0;
    static uint64_t chunk_bytes(uint64_t cap_, uint64_t pub_bytes) {
        return cap_ * (PV_PROOF_BYTES + PV_CHALLENGES * 32 + 1 + 4 + 4 + 4 + 8 + PV_TERMS * (sizeof(Fr) + sizeof(G1XYZZ)) + 2 * sizeof(G1Affine)) + pub_bytes + 32;
    }
    size_t bytes() const {
        return tab.bytes() + fixed.bytes() + gen.bytes() + kv.bytes() + sizeof(PairConsts) + proofs.bytes() + publics.bytes() + ch.bytes() + verdict.bytes() +
               status.bytes() + src.bytes() + key.bytes() + pub_at.bytes() + sc.bytes() + part.bytes() + L.bytes() + W.bytes() + batch.bytes();
    }
    // chunks of cap_ proofs whose publics take pub_bytes at the most
    void size(const char *who, uint64_t cap_, uint64_t pub_bytes) {
        if (cap_ <= cap && pub_bytes <= pub_cap) return;
        need_hbm(who, (cap_ > cap ? chunk_bytes(cap_, 0) : 0) + (pub_bytes > pub_cap ? pub_bytes + 32 : 0));
        if (pub_bytes > pub_cap || !publics.p) {
            pub_cap = 0;
            publics.alloc(pub_bytes + 32);            // never empty: a key without publics reads nothing of it
            pub_cap = pub_bytes;
        }
        if (cap_ <= cap) return;
        cap = 0;
        proofs.alloc(cap_ * PV_PROOF_BYTES);
        ch.alloc(cap_ * PV_CHALLENGES * 32);
        verdict.alloc(cap_);
        status.alloc(cap_);
        src.alloc(cap_);
        key.alloc(cap_);
        pub_at.alloc(cap_);
        sc.alloc(cap_ * PV_TERMS);
        part.alloc(cap_ * PV_TERMS);
        L.alloc(cap_);
        W.alloc(cap_);
        cap = cap_;
    }
};

namespace {

const char *const WHO_CREATE = "zk_plonk_verifier_set_create", *const WHO_VERIFY = "zk_plonk_verifier_set_verify",
                  *const WHO_BATCH = "zk_plonk_verifier_set_verify_batch", *const WHO_SUMS = "zk_plonk_verifier_set_batch_sums";

zk_plonk_verifier_set *set_create(const zk_plonk_vkey *const *vks, uint32_t n_keys, int32_t device) {
    if (!vks) throw std::invalid_argument("null argument");
    if (n_keys < 1 || n_keys > MAX_KEYS) throw std::invalid_argument(std::string(WHO_CREATE) + ": n_keys " + std::to_string(n_keys) + " is outside 1 .. 65536");
    std::vector<PlonkVerifyConsts> K(n_keys);
    std::vector<uint8_t> fixed((size_t)n_keys * PV_KEY_POINTS * 64);
    std::unique_ptr<zk_plonk_verifier_set> v(new zk_plonk_verifier_set);
    v->n_public.resize(n_keys);
    for (uint32_t q = 0; q < n_keys; q++) {           // every key as zk_plonk_verifier_create checks it
        const zk_plonk_vkey *vk = vks[q];
        const std::string who = std::string(WHO_CREATE) + ": key " + std::to_string(q);
        if (!vk) throw std::invalid_argument(who + " is null");
        if (vk->size != sizeof(zk_plonk_vkey)) throw std::invalid_argument(who + ": vk->size is not sizeof(zk_plonk_vkey)");
        if (vk->log_n < 3 || vk->log_n > PLONK_MAX_LOG_N) throw std::invalid_argument(who + ": log_n " + std::to_string(vk->log_n) + " is outside 3 .. 25");
        const uint64_t n = 1ull << vk->log_n;
        if (vk->n_public > n) throw std::invalid_argument(who + ": n_public " + std::to_string(vk->n_public) + " exceeds n = " + std::to_string(n));
        const Fr k1 = checked_one(who.c_str(), "k1", vk->k1), k2 = checked_one(who.c_str(), "k2", vk->k2);
        const uint8_t *vkp[PV_KEY_POINTS] = {vk->qm, vk->ql, vk->qr, vk->qo, vk->qc, vk->s1, vk->s2, vk->s3};
        for (uint32_t j = 0; j < PV_KEY_POINTS; j++) {
            if (!g1_well_formed(vkp[j])) throw std::invalid_argument(who + ": a commitment of the key is not a point of the curve");
            memcpy(fixed.data() + ((size_t)q * PV_KEY_POINTS + j) * 64, vkp[j], 64);
        }
        if (memcmp(vk->tau_g2, vks[0]->tau_g2, sizeof(G2Affine)) != 0)
            throw std::invalid_argument(std::string(WHO_CREATE) + ": key " + std::to_string(q) + "'s [tau]G2 is not key 0's");
        K[q] = plonk_verify_consts(*vk, k1, k2);
        v->n_public[q] = vk->n_public;
        v->max_n_public = std::max<uint64_t>(v->max_n_public, vk->n_public);
    }
    Pt<Fq> g1;
    Pt<Fq2> g2;
    generators(g1, g2);
    memcpy(v->q2, g2.b, sizeof(G2Affine));
    memcpy(v->q2 + sizeof(G2Affine), vks[0]->tau_g2, sizeof(G2Affine));

    v->device = resolve_device(device);
    v->endo = endo_const<Fq>();
    v->plan.reset(new PlonkSetChunk(n_keys));
    DeviceGuard g(v->device);
    need_hbm(WHO_CREATE, 2 * MILLER_LINES * sizeof(Line) + fixed.size() + 64 + sizeof v->q2 + K.size() * sizeof(PlonkVerifyConsts) + sizeof(PairConsts) + 65536);
    v->st.reset(new Stream);
    hipStream_t s = v->st->s;
    DevBuf<uint32_t> derr;
    DevBuf<G2Affine> d2;
    derr.alloc(4);
    d2.alloc(2);
    HIP_TRY(hipMemcpyAsync(d2.p, v->q2, sizeof v->q2, hipMemcpyHostToDevice, s));
    // [tau]G2, once for the set, as ptau_check.hip judges section 3's points: coordinates, the twist, the subgroup
    const PsiConsts psi = psi_consts();
    uint32_t h[4];
    enqueue_classify<Fq2>(h, derr.p, d2.p + 1, 1, true, &psi, plain_subgroup(), s);
    if (classified(h, s).kind) throw std::invalid_argument(std::string(WHO_CREATE) + ": the keys' [tau]G2 is not a point of the twist in the subgroup");
    v->kc.make(s);
    v->tab.alloc(2 * MILLER_LINES);
    launch_kzg_line_tables(v->tab.p, d2.p, v->kc.k.p, s);
    v->fixed.alloc((size_t)n_keys * PV_KEY_POINTS);
    v->gen.alloc(1);
    v->kv.alloc(n_keys);
    HIP_TRY(hipMemcpyAsync(v->fixed.p, fixed.data(), fixed.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(v->gen.p, g1.b, 64, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(v->kv.p, K.data(), K.size() * sizeof(PlonkVerifyConsts), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    return v.release();
}

// ---------------------------------------------------------------- a call
// What every call checks before a device is touched: the arguments, key_of and the ragged publics (at: plonk_set_plan.hpp's
// offsets).  false: m = 0
bool call_checks(zk_plonk_verifier_set *v, const char *who, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes, uint64_t m,
                 const void *out, std::vector<uint64_t> &at) {
    if (!v) throw std::invalid_argument("null argument");
    if (!m) return false;
    if (m >= (1ull << 31)) throw std::invalid_argument(std::string(who) + ": m is not below 2^31");
    if (!proofs || !key_of || !out) throw std::invalid_argument("null argument");
    ps_offsets(at, who, key_of, m, v->n_public, publics_bytes);
    if (at[m] && !publics) throw std::invalid_argument("null argument");
    return true;
}

// run(off, cnt, s) for every chunk, with the chunk ordered by key in v->plan and its proofs, publics, index, keys and
// offsets on the device.  group_knob: ZKHIP_PLONK_VERIFY_GROUP for a batch call, 0 otherwise; before(cap, stats): once, under
// the lock and on the set's device, before the chunk's buffers are sized
template <class Run, class Before>
void over_chunks(zk_plonk_verifier_set *v, const char *who, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, const std::vector<uint64_t> &at,
                 uint64_t m, uint64_t group_knob, Run run, Before before) {
    const uint64_t chunk = plonk_verify_chunk_in_effect(), cap = pb_cap(m, chunk);
    std::lock_guard<std::mutex> lock(v->mu);
    DeviceGuard g(v->device);
    LaunchCount lc(v->last_launches);
    v->last_chunks = 0;
    PlonkSetChunk &c = *v->plan;
    const PlonkSetCallStats stats = ps_call_stats(c, key_of, at, m, cap, group_knob ? pb_group(cap, group_knob) : 0);
    before(cap, stats);
    v->size(who, cap, stats.max_pub_bytes);
    hipStream_t s = v->st->s;
    for (uint64_t off = 0; off < m; off += cap) {
        const uint64_t cnt = m - off < cap ? m - off : cap, pub_bytes = at[off + cnt] - at[off];
        c.order(key_of + off, at.data() + off, cnt);
        HIP_TRY(hipMemcpyAsync(v->proofs.p, proofs + off * PV_PROOF_BYTES, cnt * PV_PROOF_BYTES, hipMemcpyHostToDevice, s));
        if (pub_bytes) HIP_TRY(hipMemcpyAsync(v->publics.p, publics + at[off], pub_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(v->src.p, c.src.data(), cnt * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(v->key.p, c.key.data(), cnt * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(v->pub_at.p, c.pub_at.data(), cnt * 8, hipMemcpyHostToDevice, s));
        run(off, cnt, s);                             // drains the stream: the plan's arrays are free again
        v->last_chunks++;
    }
}

void launch_transcript(zk_plonk_verifier_set *v, uint64_t cnt, hipStream_t s) {
    ZK_LAUNCH(k_plonk_set_transcript, dim3(nblocks(cnt, 64)), dim3(64), 0, s, v->status.p, v->ch.p, v->sc.p, v->proofs.p, v->publics.p, v->src.p, v->key.p,
              v->pub_at.p, cnt, v->cap, v->kv.p, 1u);
}

// the per-proof kernels for slots [lo, lo + cnt) of the chunk, from status and sc as the transcript left them
void launch_per_proof(zk_plonk_verifier_set *v, uint64_t lo, uint64_t cnt, hipStream_t s) {
    ZK_LAUNCH(k_plonk_set_combine, dim3(nblocks(cnt * PV_TERMS, 64)), dim3(64), 0, s, v->part.p + lo, v->status.p + lo, v->sc.p + lo, v->proofs.p, v->src.p + lo,
              v->key.p + lo, v->fixed.p, v->gen.p, cnt, v->cap, v->endo);
    ZK_LAUNCH(k_plonk_set_sum, dim3(nblocks(cnt, 64)), dim3(64), 0, s, v->L.p + lo, v->W.p + lo, v->status.p + lo, v->part.p + lo, v->proofs.p, v->src.p + lo, cnt,
              v->cap);
    ZK_LAUNCH_OK("plonk set verification");
    launch_kzg_pair(v->verdict.p + lo, v->status.p + lo, v->L.p + lo, v->W.p + lo, v->tab.p, cnt, v->kc.k.p, s);
}

void set_verify(zk_plonk_verifier_set *v, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes, uint64_t m,
                uint8_t *verdict) {
    std::vector<uint64_t> at;
    if (!call_checks(v, WHO_VERIFY, proofs, key_of, publics, publics_bytes, m, verdict, at)) return;
    std::vector<uint8_t> hv;
    over_chunks(
        v, WHO_VERIFY, proofs, key_of, publics, at, m, 0,
        [&](uint64_t off, uint64_t cnt, hipStream_t s) {
            hv.resize(cnt);
            launch_transcript(v, cnt, s);
            launch_per_proof(v, 0, cnt, s);
            HIP_TRY(hipMemcpyAsync(hv.data(), v->verdict.p, cnt, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            const std::vector<uint32_t> &src = v->plan->src;
            for (uint64_t i = 0; i < cnt; i++) verdict[off + src[i]] = hv[i];   // back to the caller's positions
        },
        [](uint64_t, const PlonkSetCallStats &) {});
}

// ---------------------------------------------------------------- batch
// the set's batch buffers for chunks of `cap` proofs in groups of `group` whose arrays are lstride apart: made by the first
// batch call, re-made when a size grows or the group or the stride changes.  Free HBM is checked first, with what the chunk's
// own buffers will ask for
void batch_size(zk_plonk_verifier_set *v, const char *who, uint64_t cap, uint64_t group, const PlonkSetCallStats &st, hipStream_t s) {
    PlonkSetBatchBufs &b = v->batch;
    const uint64_t lstride = ps_l_stride(group, st.max_group_segs), n_keys = v->n_public.size();
    if (b.group == group && b.lstride == lstride && cap <= b.cap && st.max_segs <= b.segs && st.max_ranges <= b.ranges && st.max_blocks <= b.blocks) return;
    const bool first = !b.fixed.p;
    b.cap = b.group = b.ngroups = b.lstride = b.segs = b.ranges = b.blocks = 0;
    b.r16.release(), b.fx.release(), b.partial.release(), b.lsc.release(), b.wsc.release(), b.lpt.release(), b.wpt.release();
    b.group_seg0.release(), b.seg_key.release(), b.d_ranges.release(), b.d_blocks.release();
    need_hbm(who, PlonkSetBatchBufs::bytes_for(cap, group, lstride, st.max_segs, st.max_ranges, st.max_blocks, n_keys) +
                      (cap > v->cap ? zk_plonk_verifier_set::chunk_bytes(cap, st.max_pub_bytes) : 0));
    if (first) {                                      // what no size changes
        b.fixed.alloc(n_keys * PS_KEY_TERMS + 1);
        HIP_TRY(hipMemcpyAsync(b.fixed.p, v->fixed.p, n_keys * PS_KEY_TERMS * sizeof(G1Affine), hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(b.fixed.p + n_keys * PS_KEY_TERMS, v->gen.p, sizeof(G1Affine), hipMemcpyDeviceToDevice, s));
        launch_fq_to_internal(reinterpret_cast<Fq *>(b.fixed.p), (n_keys * PS_KEY_TERMS + 1) * 2, s);
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
    b.partial.alloc(st.max_blocks * PS_KEY_TERMS);
    b.lsc.alloc(ng * lstride);
    b.lpt.alloc(ng * lstride);
    b.wsc.alloc(ng * pb_w_stride(group));
    b.wpt.alloc(ng * pb_w_stride(group));
    b.group_seg0.alloc(ng + 1);
    b.seg_key.alloc(st.max_segs);
    b.d_ranges.alloc(st.max_ranges);
    b.d_blocks.alloc(st.max_blocks);
    b.lmsm.size(lstride);
    b.wmsm.size(pb_w_stride(group));
    b.cap = cap, b.group = group, b.ngroups = ng, b.lstride = lstride, b.segs = st.max_segs, b.ranges = st.max_ranges, b.blocks = st.max_blocks;
}

// One chunk as far as the groups' sums.  On return: status (host, by slot) of the chunk's proofs, well[g] the well-formed
// proofs of group g, segments the segments with one, and sums[g] = L | W (the file's form) of every group with one; the
// transcript's status and scalars stay on the device for a recheck
struct ChunkSums {
    std::vector<uint32_t> status;
    std::vector<uint64_t> well;
    std::vector<uint8_t> sums, drawn;
    uint64_t ngroups = 0, malformed = 0, segments = 0;
};
void chunk_sums(zk_plonk_verifier_set *v, const char *who, ChunkSums &c, uint64_t cnt, const uint8_t *scalars16, hipStream_t s) {
    PlonkSetBatchBufs &b = v->batch;
    PlonkSetChunk &p = *v->plan;
    const uint64_t group = b.group, lstride = b.lstride;
    p.groups(group);
    p.fold(lstride);
    const uint64_t ng = p.ngroups, n_slots = ng * group;
    if (ng > b.ngroups || p.max_group_segs * PS_KEY_TERMS + PS_PROOF_TERMS * group + 1 > lstride || p.segs.size() > b.segs || p.ranges.size() > b.ranges ||
        p.blocks.size() > b.blocks)
        throw std::logic_error(std::string(who) + ": a chunk's plan exceeds the call's");
    c.ngroups = ng;
    c.status.resize(cnt);
    c.well.assign(ng, 0);
    c.sums.assign(ng * 128, 0);
    c.segments = 0;
    HIP_TRY(hipMemcpyAsync(b.group_seg0.p, p.group_seg0.data(), (ng + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b.seg_key.p, p.seg_key.data(), p.seg_key.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b.d_ranges.p, p.ranges.data(), p.ranges.size() * sizeof(PsRange), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b.d_blocks.p, p.blocks.data(), p.blocks.size() * sizeof(PsBlock), hipMemcpyHostToDevice, s));
    launch_transcript(v, cnt, s);
    ZK_LAUNCH_OK("plonk set transcript");
    HIP_TRY(hipMemcpyAsync(c.status.data(), v->status.p, cnt * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    uint64_t well = 0;
    for (const PsSeg &sg : p.segs) {
        uint64_t w = 0;
        for (uint32_t i = sg.lo; i < sg.hi; i++) w += c.status[i] == PV_OK;
        c.well[sg.group] += w;
        c.segments += w != 0;
        well += w;
    }
    c.malformed = cnt - well;
    if (!well) return;                                // nothing to combine: no launch
    if (!scalars16) {                                 // drawn now: the proofs of this call are fixed
        c.drawn.resize(cnt * 16);
        draw_scalars(c.drawn.data(), cnt, who);
        scalars16 = c.drawn.data();
    }
    HIP_TRY(hipMemcpyAsync(b.r16.p, scalars16, cnt * 16, hipMemcpyHostToDevice, s));
    const uint32_t n_blocks = (uint32_t)p.blocks.size(), n_ranges = (uint32_t)p.ranges.size();
    ZK_LAUNCH(k_plonk_set_scale, dim3(nblocks(n_slots, 64)), dim3(64), 0, s, b.fx.p, b.lsc.p, b.wsc.p, v->status.p, v->sc.p, b.r16.p, v->src.p, cnt, n_slots, group,
              lstride, v->cap);
    ZK_LAUNCH(k_plonk_set_gather, dim3(nblocks(ng * (lstride + pb_w_stride(group)), 256)), dim3(256), 0, s, b.lpt.p, b.wpt.p, b.lsc.p, v->status.p, v->proofs.p,
              v->src.p, b.fixed.p, (uint64_t)v->n_public.size(), b.group_seg0.p, b.seg_key.p, cnt, ng, group, lstride);
    ZK_LAUNCH(k_plonk_set_fold, dim3(n_blocks, PS_KEY_TERMS), dim3(PS_FOLD_WG), 0, s, b.partial.p, b.fx.p, b.d_ranges.p, b.d_blocks.p, n_slots, n_blocks);
    ZK_LAUNCH(k_plonk_set_fold2, dim3(n_ranges, PS_KEY_TERMS), dim3(64), 0, s, b.lsc.p, b.partial.p, b.d_ranges.p, n_blocks);
    ZK_LAUNCH_OK("plonk set batch verification: scalars and points");
    for (uint64_t g = 0; g < ng; g++) {
        if (!c.well[g]) continue;
        msm_resident(b.lmsm, c.sums.data() + g * 128, b.lpt.p + g * lstride, b.lsc.p + g * lstride, lstride, s);
        msm_resident(b.wmsm, c.sums.data() + g * 128 + 64, b.wpt.p + g * pb_w_stride(group), b.wsc.p + g * pb_w_stride(group), pb_w_stride(group), s);
    }
}

bool batch_checks(zk_plonk_verifier_set *v, const char *who, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes, uint64_t m,
                  const uint8_t *scalars16, const void *out, std::vector<uint64_t> &at) {
    if (!call_checks(v, who, proofs, key_of, publics, publics_bytes, m, out, at)) return false;
    refuse_zero_scalars(scalars16, m, who);
    return true;
}

void set_verify_batch(zk_plonk_verifier_set *v, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes, uint64_t m,
                      const uint8_t *scalars16, uint8_t *verdict, zk_plonk_set_batch_report *report) {
    const uint32_t rep_size = report_size(report);
    zk_plonk_set_batch_report rep;
    memset(&rep, 0, sizeof rep);
    const uint64_t knob = plonk_verify_group_in_effect();
    rep.size = rep_size;
    rep.group = (uint32_t)knob;
    auto leave = [&]() {
        if (report) memcpy(report, &rep, rep_size);
    };
    std::vector<uint64_t> at;
    if (!batch_checks(v, WHO_BATCH, proofs, key_of, publics, publics_bytes, m, scalars16, verdict, at)) {
        leave();
        return;
    }
    ChunkSums c;
    std::vector<uint64_t> eq, redo;                   // the groups whose equation is evaluated; the slot ranges rechecked, lo hi lo hi ..
    std::vector<uint8_t> pass, hv;
    over_chunks(
        v, WHO_BATCH, proofs, key_of, publics, at, m, knob,
        [&](uint64_t off, uint64_t cnt, hipStream_t s) {
            PlonkSetBatchBufs &b = v->batch;
            const uint64_t group = b.group;
            chunk_sums(v, WHO_BATCH, c, cnt, scalars16 ? scalars16 + off * 16 : nullptr, s);
            const std::vector<uint32_t> &src = v->plan->src;
            rep.malformed += c.malformed;
            rep.segments += c.segments;
            for (uint64_t i = 0; i < cnt; i++) verdict[off + src[i]] = c.status[i] == PV_OK ? ZK_VERIFY_OK : ZK_VERIFY_MALFORMED;
            eq.clear();
            for (uint64_t g = 0; g < c.ngroups; g++)
                if (c.well[g]) eq.push_back(g);
            rep.groups += eq.size();
            if (eq.empty()) return;
            plonk_group_equations(PlonkPairBufs{b.p1.p, b.p2.p, b.lines.p, b.skip.p, b.out.p, b.err.p}, v->kc.k.p, pass, c.sums.data(), eq, s);
            // the failed groups of this chunk through the per-proof kernels, neighbours in one pass; a malformed proof among
            // them keeps its MALFORMED there too
            redo.clear();
            hv.resize(cnt);
            for (uint64_t q = 0; q < eq.size();) {
                if (pass[q]) {
                    q++;
                    continue;
                }
                uint64_t e = q;
                while (e + 1 < eq.size() && !pass[e + 1] && eq[e + 1] == eq[e] + 1) e++;
                const uint64_t lo = eq[q] * group, hi = (eq[e] + 1) * group < cnt ? (eq[e] + 1) * group : cnt;
                for (uint64_t g = q; g <= e; g++) rep.proofs_rechecked += c.well[eq[g]];
                rep.groups_failed += e - q + 1;
                launch_per_proof(v, lo, hi - lo, s);
                HIP_TRY(hipMemcpyAsync(hv.data() + lo, v->verdict.p + lo, hi - lo, hipMemcpyDeviceToHost, s));
                redo.push_back(lo), redo.push_back(hi);
                q = e + 1;
            }
            HIP_TRY(hipStreamSynchronize(s));
            for (size_t q = 0; q < redo.size(); q += 2)
                for (uint64_t i = redo[q]; i < redo[q + 1]; i++) verdict[off + src[i]] = hv[i];
        },
        [&](uint64_t cap, const PlonkSetCallStats &st) {
            rep.group = (uint32_t)pb_group(cap, knob);
            batch_size(v, WHO_BATCH, cap, rep.group, st, v->st->s);
        });
    rep.launches = v->last_launches;
    rep.chunks = v->last_chunks;
    leave();
}

void set_batch_sums(zk_plonk_verifier_set *v, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes, uint64_t m,
                    const uint8_t *scalars16, uint8_t *sums, uint64_t sums_cap, uint64_t *n_groups) {
    if (!n_groups) throw std::invalid_argument("null argument");
    *n_groups = 0;
    const uint64_t knob = plonk_verify_group_in_effect();
    std::vector<uint64_t> at;
    if (!batch_checks(v, WHO_SUMS, proofs, key_of, publics, publics_bytes, m, scalars16, sums, at)) return;
    if (!scalars16) throw std::invalid_argument("null argument");
    const uint64_t want = pb_groups_of_call(m, plonk_verify_chunk_in_effect(), knob);
    if (sums_cap < want) throw std::invalid_argument(std::string(WHO_SUMS) + ": sums_cap " + std::to_string(sums_cap) + " is below the call's " + std::to_string(want) + " groups");
    ChunkSums c;
    uint64_t written = 0;
    over_chunks(
        v, WHO_SUMS, proofs, key_of, publics, at, m, knob,
        [&](uint64_t off, uint64_t cnt, hipStream_t s) {
            chunk_sums(v, WHO_SUMS, c, cnt, scalars16 + off * 16, s);
            memcpy(sums + written * 128, c.sums.data(), c.ngroups * 128);
            written += c.ngroups;
        },
        [&](uint64_t cap, const PlonkSetCallStats &st) { batch_size(v, WHO_SUMS, cap, pb_group(cap, knob), st, v->st->s); });
    *n_groups = written;
}

}   // namespace

extern "C" {

int zk_plonk_verifier_set_create(zk_plonk_verifier_set **out, const zk_plonk_vkey *const *vks, uint32_t n_keys, int32_t device) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        *out = set_create(vks, n_keys, device);
    });
}

void zk_plonk_verifier_set_destroy(zk_plonk_verifier_set *set) { destroy_on_device(set); }

int zk_plonk_verifier_set_info(zk_plonk_verifier_set *set, zk_plonk_verifier_set_plan *plan) {
    return guarded([&] {
        if (!set || !plan) throw std::invalid_argument("null argument");
        info_into("zk_plonk_verifier_set_info", plan, [&](zk_plonk_verifier_set_plan &p) {
            std::lock_guard<std::mutex> lock(set->mu);
            p.n_keys = (uint32_t)set->n_public.size();
            p.max_n_public = set->max_n_public;
            p.device_bytes = set->bytes();
            p.chunk = plonk_verify_chunk_in_effect();
            p.last_launches = set->last_launches;
            p.last_chunks = set->last_chunks;
        });
    });
}

int zk_plonk_verifier_set_verify(zk_plonk_verifier_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes, uint64_t m,
                                 uint8_t *verdict) {
    return guarded([&] { set_verify(set, proofs, key_of, publics, publics_bytes, m, verdict); });
}

int zk_plonk_verifier_set_verify_batch(zk_plonk_verifier_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes,
                                       uint64_t m, const uint8_t *scalars16, uint8_t *verdict, zk_plonk_set_batch_report *report) {
    return guarded([&] { set_verify_batch(set, proofs, key_of, publics, publics_bytes, m, scalars16, verdict, report); });
}

int zk_plonk_verifier_set_batch_sums(zk_plonk_verifier_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes, uint64_t m,
                                     const uint8_t *scalars16, uint8_t *sums, uint64_t sums_cap, uint64_t *n_groups) {
    return guarded([&] { set_batch_sums(set, proofs, key_of, publics, publics_bytes, m, scalars16, sums, sums_cap, n_groups); });
}

}   // extern "C"
