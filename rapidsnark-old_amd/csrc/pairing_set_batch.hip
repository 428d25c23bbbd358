// Batch verification across a key set: one equation for proofs under many keys (zk_vkey_set_verify_batch, include/zkhip.h;
// DESIGN.md section 25).  Inside a chunk the host orders the proofs by key (a stable counting sort over key_of, as
// pairing_set.hip's lane path does).  In that order consecutive proofs form groups: a group closes when it holds
// ZKHIP_VERIFY_GROUP proofs, or when the next proof would bring a key beyond the ZKHIP_VERIFY_GROUP_KEYS-th into it.  The
// proofs of one key inside one group are a segment.  With a 128-bit scalar r_i per proof, over the well-formed proofs of
// segment s (key k)
//     R_s = sum r_i,  S_sj = sum r_i pub_ij (mod r),  X_s = R_s IC_0 + sum_j S_sj IC_(j+1),  Cs_s = sum r_i C_i,
// and the group passes iff
//     prod_i e(r_i A_i, B_i) . prod_s [ e(-R_s alpha_k, beta_k) . e(-X_s, gamma_k) . e(-Cs_s, delta_k) ] = 1
// with one final exponentiation.  The well-formed proofs of all failing groups of a chunk go through the set's own per-proof
// pass (set_verify_locked, pairing_set.hip) in one call.
//
// Kernels, in launch order per chunk:
//   k_setb_check    a lane per proof over per-wave records (a wave's proofs have one key): k_batch_check's criteria,
//                   nPublic from the key record
//   k_setb_scale    a lane per proof: r_i A_i (made affine) and r_i C_i, as k_batch_scale
//   k_setb_miller   a lane per proof: the Miller value of (r_i A_i, B_i), as k_batch_miller
//   k_setb_fr       a wave per (segment, j), j up to the segment's own nPublic: S_sj and R_s by a fixed tree in LDS
//   k_setb_reduce   a wave per 64 values: the product of the f_i per group and the sum of the r_i C_i per segment, by a
//                   fixed tree in LDS; run again on its own output while a group has more than one value left
//   k_setb_tail     a workgroup per group: the segments in passes of TAIL_SEGS; a pass makes -R_s alpha_k, -X_s, -Cs_s and
//                   runs one squaring chain with three table-driven line evaluations per segment; then the product with
//                   the group's f and one final exponentiation, on pairing_coop_dev.hpp's sliced Fq12 operations
//   k_setb_ab       once per set, a lane per key: beta_k's lines
// Only the groups and segments with a well-formed proof reach k_setb_fr, k_setb_reduce and k_setb_tail: the host has the
// status words before it makes their records.  No atomics on points or field elements: every tree's shape is fixed by the
// indices, so verdicts and intermediate bytes do not depend on scheduling.
//
// What this unit has in common with pairing_batch.hip is written once: what a lane does in the check, scale and Miller
// kernels, the wave that sums X_s and the tail's points in verify_batch_dev.hpp; the scalars, the group switches, the
// report's size and the chunk's layout (ChunkPlan) in verify_batch_host.hpp.  The kernels here find the lane's proof, and
// the fr, reduce and tail kernels keep their own structure: ragged records where pairing_batch.hip has a stride.
#include "verify_batch_dev.hpp"
#include "pairing_set_internal.hpp"

namespace {

constexpr uint64_t DEFAULT_GROUP_KEYS = 1;            // profiles/verify_set_batch_timing.txt
constexpr uint64_t MAX_GROUP_KEYS = 65536;
constexpr uint32_t TAIL_SEGS = 16;

struct SegRec {                                       // a segment with a well-formed proof
    uint64_t pub_at;                                  // where the signals of slot `lo` begin
    uint32_t lo, hi;                                  // its slots
    uint32_t key, s_at;                               // its sums are S[s_at .. s_at + nPublic]: S_j, then R
    uint32_t c_at, reserved;                          // where its sum of r_i C_i stands after the reduction
};
struct GroupRec {                                     // a group with a well-formed proof
    uint32_t seg_lo, seg_hi;                          // its segments in the SegRec array
    uint32_t f_at, reserved;                          // where its product of Miller values stands after the reduction
};
struct Range {                                        // a level of the reduction: `len` values from in_lo become ceil(len / 64) from out_lo
    uint32_t in_lo, len, out_lo;
};
static_assert(sizeof(SegRec) == 32 && sizeof(GroupRec) == 16 && sizeof(Range) == 12, "layout");

// the last r below n with key(r) <= b; key(0) <= b.  The same in every lane.
template <class Key>
__device__ __forceinline__ uint32_t find_range(uint32_t n, uint32_t b, Key key) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (key(mid) <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------- a lane per proof: verify_batch_dev.hpp's bodies
// The check's grid is the chunk's waves exactly; w is the same in every lane.  The other two: lane i has slot i.
__global__ __launch_bounds__(64) void k_setb_check(uint32_t *status, const uint8_t *__restrict__ proofs, const Fr *__restrict__ publics,
                                                   const BWave *__restrict__ waves, const KeyRec *__restrict__ keys, const PairConsts *__restrict__ k, Fq b1,
                                                   Fq2 b2) {
    const BWave w = waves[blockIdx.x];
    if (threadIdx.x >= w.cnt) return;
    const uint32_t nPublic = keys[w.key].nPublic;
    const uint64_t i = (uint64_t)w.slot0 + threadIdx.x;
    batch_check_lane(status + i, proofs + i * 256, publics + w.pub_at + (uint64_t)threadIdx.x * nPublic, nPublic, k, b1, b2);
}

__global__ __launch_bounds__(64) void k_setb_scale(G1Affine *ra, G1XYZZ *rc, const uint32_t *__restrict__ status, const uint8_t *__restrict__ proofs,
                                                   const Scalar16 *__restrict__ scalars, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    batch_scale_lane(ra + i, rc + i, status[i], proofs + i * 256, scalars + i);
}

__global__ __launch_bounds__(64) void k_setb_miller(Fq12 *f_out, const uint32_t *__restrict__ status, const uint8_t *__restrict__ proofs,
                                                    const G1Affine *__restrict__ ra, uint64_t n, const PairConsts *k) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    batch_miller_lane(f_out + i, status[i], proofs + i * 256, ra + i, k);
}

// ---------------------------------------------------------------- the sums in Fr, ragged
// Block b belongs to the segment s with s_at <= b < s_at + nPublic(key) + 1 and makes S[b]: with j = b - s_at, the sum over
// the segment's well-formed proofs of r_i pub_ij for j < nPublic, of r_i for j = nPublic (R), standard form.
__global__ __launch_bounds__(64) void k_setb_fr(Fr *S, const uint32_t *__restrict__ status, const Fr *__restrict__ publics, const Scalar16 *__restrict__ scalars,
                                                const SegRec *__restrict__ segs, uint32_t nsegs, const KeyRec *__restrict__ keys) {
    __shared__ Fr part[64];
    const uint32_t lane = threadIdx.x;
    const SegRec sg = segs[find_range(nsegs, blockIdx.x, [&](uint32_t r) { return segs[r].s_at; })];
    const uint32_t nPublic = keys[sg.key].nPublic, j = blockIdx.x - sg.s_at;
    Fr acc = Fr::zero();
    for (uint32_t i = sg.lo + lane; i < sg.hi; i += 64) {
        if (status[i] != ST_OK) continue;
        const Fr r = scalar_of(scalars + i);
        if (j == nPublic) acc = Fr::add(acc, r);
        else acc = Fr::add(acc, Fr::mul(Fr::to_mont(r), load_el(publics + sg.pub_at + (uint64_t)(i - sg.lo) * nPublic + j)));   // (r R) pub / R
    }
    part[lane] = acc;
    for (uint32_t s = 32; s; s >>= 1) {
        __syncthreads();
        if (lane < s) part[lane] = Fr::add(part[lane], part[lane + s]);
    }
    if (lane == 0) store_el(S + blockIdx.x, part[0]);
}

// ---------------------------------------------------------------- the products per group and the sums per segment
// Blocks 0 .. f_blocks - 1 multiply Miller values, range by range of fr; the blocks after them add points, range by range
// of cr.  Block b of either kind writes value b of its output: it reads values 64 t .. 64 t + 63 of the range r with
// out_lo <= b, t = b - out_lo.
union ReduceLds {
    Fq12 f[64];
    G1XYZZ c[64];
};
static_assert(sizeof(ReduceLds) == 64 * 384, "LDS of a reduction wave");

__global__ __launch_bounds__(64) void k_setb_reduce(Fq12 *fout, G1XYZZ *cout, const Fq12 *__restrict__ fin, const G1XYZZ *__restrict__ cin,
                                                    const Range *__restrict__ fr, uint32_t nfr, uint32_t f_blocks, const Range *__restrict__ cr, uint32_t ncr) {
    __shared__ ReduceLds R;
    const uint32_t lane = threadIdx.x;
    const bool points = blockIdx.x >= f_blocks;       // the same in every lane
    const uint32_t b = points ? blockIdx.x - f_blocks : blockIdx.x;
    const Range *ranges = points ? cr : fr;
    const Range rg = ranges[find_range(points ? ncr : nfr, b, [&](uint32_t r) { return ranges[r].out_lo; })];
    const uint32_t base = (b - rg.out_lo) * 64;
    const uint32_t cnt = rg.len - base < 64 ? rg.len - base : 64;
    const uint64_t at = (uint64_t)rg.in_lo + base + lane;
    if (points) {
        if (lane < cnt) R.c[lane] = load_pt(cin + at);
        for (uint32_t s = 32; s; s >>= 1) {
            __syncthreads();
            if (lane < s && lane + s < cnt) {
                G1XYZZ p = R.c[lane];
                const G1XYZZ q = R.c[lane + s];
                nl_add(p, q);
                R.c[lane] = p;
            }
        }
        if (lane == 0) store_pt(cout + b, R.c[0]);
    } else {
        if (lane < cnt) R.f[lane] = fin[at];
        for (uint32_t s = 32; s; s >>= 1) {
            __syncthreads();
            if (lane < s && lane + s < cnt) {
                Fq12 x = R.f[lane];
                const Fq12 y = R.f[lane + s];
                f12_mul(x, x, y);
                R.f[lane] = x;
            }
        }
        if (lane == 0) fout[b] = R.f[0];
    }
}

// ---------------------------------------------------------------- the tail: a workgroup per group
__shared__ TailPts<TAIL_SEGS> T;                     // per segment of the pass: -R alpha, -X, -Cs

// pass[g] = 1 when group g's equation holds, 0 when it fails.  F, Cs: the reduction's outputs (f_at, c_at); S: k_setb_fr's;
// alpha[key], tab_beta[key][MILLER_LINES]: the set's; keys[key].tab: gamma's lines, then delta's.
// Every wave passes the same barriers: two a pass, and the number of passes is the group's.
__global__ __launch_bounds__(TAIL_THREADS) void k_setb_tail(uint8_t *pass, const GroupRec *__restrict__ groups, const SegRec *__restrict__ segs,
                                                            const Fq12 *__restrict__ F, const G1XYZZ *__restrict__ Cs, const Fr *__restrict__ S,
                                                            const KeyRec *__restrict__ keys, const G1Affine *__restrict__ alpha,
                                                            const Line *__restrict__ tab_beta, const PairConsts *__restrict__ k, Fq beta) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const GroupRec g = groups[blockIdx.x];
    if (wave == 0) {                                  // E_T0: the value so far, from the group's product of Miller values on
        if (lane < 6) L.e[E_T0][lane] = load_el(reinterpret_cast<const Fq2 *>(F + g.f_at) + coop_slot(lane));
        wsync();
    }
    for (uint32_t s0 = g.seg_lo; s0 < g.seg_hi; s0 += TAIL_SEGS) {
        const uint32_t np = g.seg_hi - s0 < TAIL_SEGS ? g.seg_hi - s0 : TAIL_SEGS;
        // side by side: -R alpha and -Cs with a lane per segment, -X with a wave per segment in turn
        if (wave == 0) {
            if (lane < np) {
                const SegRec sg = segs[s0 + lane];
                G1XYZZ t;
                nl_mul_glv(t, load_pt(alpha + sg.key), load_el(S + sg.s_at + keys[sg.key].nPublic), beta);
                put_neg(&T.pt[lane][0], &T.have[lane][0], t);
            }
        } else if (wave == 1) {
            if (lane < np) put_neg(&T.pt[lane][2], &T.have[lane][2], load_pt(Cs + segs[s0 + lane].c_at));
        } else {
            for (uint32_t q = 0; q < np; q++) {
                const SegRec sg = segs[s0 + q];
                const KeyRec key = keys[sg.key];
                wsync();                              // the tree before has been read
                x_wave(lane, key.ic, S + sg.s_at, key.nPublic, beta);
                if (lane == 0) put_neg(&T.pt[q][1], &T.have[q][1], L.part[0]);
            }
        }
        __syncthreads();
        if (wave == 0) {
            c_one(E_IN);
            int at = 0;
            auto lines = [&]() {
                for (uint32_t q = 0; q < np; q++) {
                    const uint32_t key = segs[s0 + q].key;
                    const Line *tg = keys[key].tab, *td = tg + MILLER_LINES;
                    if (T.have[q][0]) c_line(E_IN, tab_beta + (uint64_t)key * MILLER_LINES + at, &T.pt[q][0]);
                    if (T.have[q][1]) c_line(E_IN, tg + at, &T.pt[q][1]);
                    if (T.have[q][2]) c_line(E_IN, td + at, &T.pt[q][2]);
                }
                at++;
            };
            for (int s = 0; s < 64; s++) {
                c_mul(E_IN, E_IN, E_IN);
                lines();
                if (ate_bit(s)) lines();
            }
            lines();
            lines();
            c_mul(E_T0, E_T0, E_IN);
        }
        __syncthreads();                              // the next pass writes T
    }
    if (wave) return;                                 // no barrier below
    c_copy(E_IN, E_T0);
    c_final_exp(k);
    if (lane == 0) pass[blockIdx.x] = c_is_one(E_F) ? 1 : 0;
}

// tab[key][MILLER_LINES]: the lines of beta_key, a lane per key
__global__ __launch_bounds__(64) void k_setb_ab(Line *tab, const G2Affine *__restrict__ beta, uint32_t n_keys, const PairConsts *k) {
    const uint32_t key = blockIdx.x * blockDim.x + threadIdx.x;
    if (key >= n_keys) return;
    line_table(tab + (uint64_t)key * MILLER_LINES, load_pt(beta + key), *k);
}

// ---------------------------------------------------------------- host
// alpha_k on the device and beta_k's lines for every key, once per set, one launch
void batch_prepare(zk_vkey_set *set, hipStream_t s) {
    const uint32_t n_keys = (uint32_t)set->nPublic.size();
    DevBuf<G2Affine> db;
    db.alloc(n_keys);
    set->batch.alpha.alloc(n_keys);
    set->batch.tab_beta.alloc((size_t)n_keys * MILLER_LINES);
    HIP_TRY(hipMemcpyAsync(set->batch.alpha.p, set->alpha_h.data(), (size_t)n_keys * sizeof(G1Affine), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(db.p, set->beta_h.data(), (size_t)n_keys * sizeof(G2Affine), hipMemcpyHostToDevice, s));
    ZK_LAUNCH(k_setb_ab, dim3(nblocks(n_keys, 64)), dim3(64), 0, s, set->batch.tab_beta.p, db.p, n_keys, set->kc.k.p);
    ZK_LAUNCH_OK("batch verification of a key set: the lines of beta");
    HIP_TRY(hipStreamSynchronize(s));
    set->batch.ready = true;
}

uint64_t ceil64(uint64_t v) { return (v + 63) / 64; }

void set_verify_batch(zk_vkey_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes, uint64_t n,
                      const uint8_t *scalars16, uint8_t *verdict, zk_vkey_set_batch_report *report) {
    if (!set) throw std::invalid_argument("null argument");
    const uint32_t rep_size = report_size(report);
    zk_vkey_set_batch_report rep;
    memset(&rep, 0, sizeof rep);
    const uint64_t group = group_size();
    const uint64_t group_keys = env_number("ZKHIP_VERIFY_GROUP_KEYS", DEFAULT_GROUP_KEYS, 1, MAX_GROUP_KEYS, "a number of keys from 1 to 65536");
    const uint64_t chunk = chunk_jobs();
    rep.size = rep_size;
    rep.group = (uint32_t)group;
    rep.group_keys = (uint32_t)group_keys;
    auto leave = [&]() {
        if (report) memcpy(report, &rep, rep_size);
    };
    if (!n) {
        leave();
        return;
    }
    if (!proofs || !key_of || !verdict) throw std::invalid_argument("null argument");
    const uint64_t n_keys = set->nPublic.size();
    std::vector<uint64_t> at(n + 1);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (key_of[i] >= n_keys)
            throw std::invalid_argument("zk_vkey_set_verify_batch: key_of[" + std::to_string(i) + "] = " + std::to_string(key_of[i]) + ", the set holds " +
                                        std::to_string(n_keys) + " keys");
        at[i] = total;
        total += set->nPublic[key_of[i]];
    }
    at[n] = total;
    if (publics_bytes != total * 32)
        throw std::invalid_argument("zk_vkey_set_verify_batch: publics_bytes: " + std::to_string(total * 32) + " expected (" + std::to_string(total) +
                                    " signals of 32 bytes), " + std::to_string(publics_bytes) + " given");
    if (total && !publics) throw std::invalid_argument("null argument");
    refuse_zero_scalars(scalars16, n, "zk_vkey_set_verify_batch");
    std::lock_guard<std::mutex> lock(set->mu);
    DeviceGuard dg(set->device);
    const uint64_t cap = n < chunk ? n : chunk;
    ChunkPlan lay(n_keys);
    // what the largest chunk needs, whatever n: its signals, waves, segments, groups, sums and the reduction's first two levels
    uint64_t cap_pub = 0, cap_waves = 0, cap_segs = 0, cap_groups = 0, cap_S = 0, cap_f1 = 0, cap_c1 = 0;
    for (uint64_t off = 0; off < n; off += cap) {
        lay.plan(key_of + off, n - off < cap ? n - off : cap, set->nPublic, group, group_keys);
        uint64_t nS = 0, f1 = 0, c1 = 0;
        for (const Seg &sg : lay.segs) {
            nS += set->nPublic[sg.key] + 1;
            c1 += ceil64(sg.hi - sg.lo);
        }
        for (size_t g = 0; g + 1 < lay.group_seg0.size(); g++) f1 += ceil64(lay.segs[lay.group_seg0[g + 1] - 1].hi - lay.segs[lay.group_seg0[g]].lo);
        cap_pub = std::max(cap_pub, lay.npub);
        cap_waves = std::max<uint64_t>(cap_waves, lay.waves.size());
        cap_segs = std::max<uint64_t>(cap_segs, lay.segs.size());
        cap_groups = std::max<uint64_t>(cap_groups, lay.group_seg0.size() - 1);
        cap_S = std::max(cap_S, nS);
        cap_f1 = std::max(cap_f1, f1);
        cap_c1 = std::max(cap_c1, c1);
    }
    if (group == 1) cap_f1 = cap_c1 = 0;              // every range has one value: no reduction
    const uint64_t cap_ranges = 2 * (cap_groups + cap_segs);   // a level's records; the levels take turns in two halves
    uint64_t need = cap * (256 + 16 + 4 + sizeof(G1Affine) + sizeof(G1XYZZ) + sizeof(Fq12)) + cap_pub * 32 + cap_waves * sizeof(BWave) +
                    cap_segs * sizeof(SegRec) + cap_groups * (sizeof(GroupRec) + 1) + cap_S * 32 + 2 * cap_f1 * sizeof(Fq12) + 2 * cap_c1 * sizeof(G1XYZZ) +
                    cap_ranges * sizeof(Range) + 65536;
    if (!set->batch.ready) need += n_keys * (sizeof(G1Affine) + sizeof(G2Affine) + MILLER_LINES * sizeof(Line));
    need_hbm("zk_vkey_set_verify_batch", need);
    Stream st;
    hipStream_t s = st.s;
    uint32_t launches = 0;
    if (!set->batch.ready) {
        batch_prepare(set, s);
        launches++;
    }
    DevBuf<uint8_t> dp, dpass;
    DevBuf<Fr> dpub, dS;
    DevBuf<Scalar16> dsc;
    DevBuf<uint32_t> dst;
    DevBuf<G1Affine> dra;
    DevBuf<G1XYZZ> drc, dc1, dc2;
    DevBuf<Fq12> df, df1, df2;
    DevBuf<BWave> dw;
    DevBuf<SegRec> dsegs;
    DevBuf<GroupRec> dgroups;
    DevBuf<Range> dranges;
    dp.alloc(cap * 256);
    dpub.alloc(cap_pub);
    dsc.alloc(cap);
    dst.alloc(cap);
    dra.alloc(cap);
    drc.alloc(cap);
    df.alloc(cap);
    df1.alloc(cap_f1);
    df2.alloc(cap_f1);
    dc1.alloc(cap_c1);
    dc2.alloc(cap_c1);
    dw.alloc(cap_waves);
    dsegs.alloc(cap_segs);
    dgroups.alloc(cap_groups);
    dS.alloc(cap_S);
    dpass.alloc(cap_groups);
    dranges.alloc(cap_ranges);
    std::vector<uint8_t> hp(cap * 256), hpub(cap_pub * 32), hsc(cap * 16), drawn, pass(cap_groups), re_proofs, re_publics, re_verdict;
    std::vector<uint32_t> status(cap), re_key;
    std::vector<uint64_t> filled(n_keys), caller_of(cap), re_at, re_sig;
    std::vector<SegRec> hsegs;
    std::vector<GroupRec> hgroups;
    std::vector<uint32_t> live_group;                 // the plan's group of every record of hgroups
    std::vector<std::vector<Range>> levels;           // kept until the chunk's last synchronisation
    const Fq b1 = curve_b<Fq>(), beta = endo_const<Fq>();
    const Fq2 b2 = curve_b<Fq2>();
    set->plan.last_waves_padded = 0;
    for (uint64_t off = 0; off < n; off += cap) {
        const uint64_t cnt = n - off < cap ? n - off : cap;
        lay.plan(key_of + off, cnt, set->nPublic, group, group_keys);
        const uint8_t *sc = scalars16 ? scalars16 + off * 16 : nullptr;
        if (!sc) {                                    // drawn now: the proofs of this call are fixed
            drawn.resize(cnt * 16);
            draw_scalars(drawn.data(), cnt, "zk_vkey_set_verify_batch");
            sc = drawn.data();
        }
        for (uint32_t k : lay.present) filled[k] = 0;
        for (uint64_t i = 0; i < cnt; i++) {
            const uint32_t k = key_of[off + i];
            const uint64_t pos = filled[k]++, slot = lay.slot0[k] + pos, pb = (uint64_t)set->nPublic[k] * 32;
            caller_of[slot] = off + i;
            memcpy(hp.data() + slot * 256, proofs + (off + i) * 256, 256);
            memcpy(hsc.data() + slot * 16, sc + i * 16, 16);
            if (pb) memcpy(hpub.data() + lay.pub0[k] * 32 + pos * pb, publics + at[off + i] * 32, pb);
        }
        const uint64_t nw = lay.waves.size();
        const dim3 block(64);
        HIP_TRY(hipMemcpyAsync(dp.p, hp.data(), cnt * 256, hipMemcpyHostToDevice, s));
        if (lay.npub) HIP_TRY(hipMemcpyAsync(dpub.p, hpub.data(), lay.npub * 32, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(dsc.p, hsc.data(), cnt * 16, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(dw.p, lay.waves.data(), nw * sizeof(BWave), hipMemcpyHostToDevice, s));
        ZK_LAUNCH(k_setb_check, dim3((uint32_t)nw), block, 0, s, dst.p, dp.p, dpub.p, dw.p, set->recs.p, set->kc.k.p, b1, b2);
        ZK_LAUNCH_OK("batch verification of a key set: checks");
        launches++;
        HIP_TRY(hipMemcpyAsync(status.data(), dst.p, cnt * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        uint64_t well = 0;
        for (uint64_t i = 0; i < cnt; i++) {
            well += status[i] == ST_OK;
            verdict[caller_of[i]] = status[i] == ST_OK ? ZK_VERIFY_OK : ZK_VERIFY_MALFORMED;
        }
        rep.malformed += cnt - well;
        if (!well) continue;                          // nothing to combine: no launch
        // the records of the groups and segments with a well-formed proof
        hsegs.clear();
        hgroups.clear();
        live_group.clear();
        uint32_t s_at = 0;
        for (size_t g = 0; g + 1 < lay.group_seg0.size(); g++) {
            const uint32_t first = (uint32_t)hsegs.size();
            for (uint32_t q = lay.group_seg0[g]; q < lay.group_seg0[g + 1]; q++) {
                const Seg &sg = lay.segs[q];
                bool any = false;
                for (uint32_t i = sg.lo; i < sg.hi && !any; i++) any = status[i] == ST_OK;
                if (!any) continue;
                hsegs.push_back(SegRec{sg.pub_at, sg.lo, sg.hi, sg.key, s_at, sg.lo, 0});
                s_at += set->nPublic[sg.key] + 1;
            }
            if (hsegs.size() == first) continue;
            hgroups.push_back(GroupRec{first, (uint32_t)hsegs.size(), lay.segs[lay.group_seg0[g]].lo, 0});
            live_group.push_back((uint32_t)g);
        }
        const uint32_t nsegs = (uint32_t)hsegs.size(), ngroups = (uint32_t)hgroups.size();
        rep.groups += ngroups;
        rep.segments += nsegs;
        // the reduction's levels: the groups' ranges of Miller values and the segments' ranges of points, until every group has one value
        levels.clear();
        std::vector<Range> cur(ngroups + nsegs);      // the groups' ranges, then the segments'
        uint32_t longest = 0;
        for (uint32_t g = 0; g < ngroups; g++) {
            const uint32_t lo = lay.segs[lay.group_seg0[live_group[g]]].lo, hi = lay.segs[lay.group_seg0[live_group[g] + 1] - 1].hi;
            cur[g] = Range{lo, hi - lo, 0};
            longest = std::max(longest, hi - lo);
        }
        for (uint32_t q = 0; q < nsegs; q++) cur[ngroups + q] = Range{hsegs[q].lo, hsegs[q].hi - hsegs[q].lo, 0};
        std::vector<uint32_t> f_blocks, c_blocks;
        for (; longest > 1; longest = (uint32_t)ceil64(longest)) {
            uint32_t out = 0;
            for (uint32_t r = 0; r < ngroups + nsegs; r++) {
                if (r == ngroups) {
                    f_blocks.push_back(out);
                    out = 0;
                }
                cur[r].out_lo = out;
                out += (uint32_t)ceil64(cur[r].len);
            }
            c_blocks.push_back(out);
            levels.push_back(cur);
            for (Range &r : cur) r = Range{r.out_lo, (uint32_t)ceil64(r.len), 0};
        }
        for (uint32_t g = 0; g < ngroups; g++) hgroups[g].f_at = cur[g].in_lo;
        for (uint32_t q = 0; q < nsegs; q++) hsegs[q].c_at = cur[ngroups + q].in_lo;
        HIP_TRY(hipMemcpyAsync(dsegs.p, hsegs.data(), nsegs * sizeof(SegRec), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(dgroups.p, hgroups.data(), ngroups * sizeof(GroupRec), hipMemcpyHostToDevice, s));
        const dim3 grid(nblocks(cnt, 64));
        ZK_LAUNCH(k_setb_scale, grid, block, 0, s, dra.p, drc.p, dst.p, dp.p, dsc.p, cnt);
        ZK_LAUNCH(k_setb_miller, grid, block, 0, s, df.p, dst.p, dp.p, dra.p, cnt, set->kc.k.p);
        ZK_LAUNCH(k_setb_fr, dim3(s_at), block, 0, s, dS.p, dst.p, dpub.p, dsc.p, dsegs.p, nsegs, set->recs.p);
        launches += 3;
        const Fq12 *fin = df.p;
        const G1XYZZ *cin = drc.p;
        for (size_t level = 0; level < levels.size(); level++) {
            Fq12 *fo = level & 1 ? df2.p : df1.p;
            G1XYZZ *co = level & 1 ? dc2.p : dc1.p;
            Range *dr = dranges.p + (level & 1) * (cap_groups + cap_segs);   // level + 2 writes here after level has run: one stream
            HIP_TRY(hipMemcpyAsync(dr, levels[level].data(), (ngroups + nsegs) * sizeof(Range), hipMemcpyHostToDevice, s));
            ZK_LAUNCH(k_setb_reduce, dim3(f_blocks[level] + c_blocks[level]), block, 0, s, fo, co, fin, cin, dr, ngroups, f_blocks[level], dr + ngroups, nsegs);
            launches++;
            fin = fo;
            cin = co;
        }
        ZK_LAUNCH(k_setb_tail, dim3(ngroups), dim3(TAIL_THREADS), 0, s, dpass.p, dgroups.p, dsegs.p, fin, cin, dS.p, set->recs.p, set->batch.alpha.p,
                  set->batch.tab_beta.p, set->kc.k.p, beta);
        ZK_LAUNCH_OK("batch verification of a key set");
        launches++;
        HIP_TRY(hipMemcpyAsync(pass.data(), dpass.p, ngroups, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        // the well-formed proofs of every failed group of this chunk, in the caller's order: one pass of the set's per-proof code
        re_at.clear();
        for (uint32_t g = 0; g < ngroups; g++) {
            if (pass[g]) continue;
            rep.groups_failed++;
            for (uint32_t q = hgroups[g].seg_lo; q < hgroups[g].seg_hi; q++)
                for (uint32_t i = hsegs[q].lo; i < hsegs[q].hi; i++)
                    if (status[i] == ST_OK) re_at.push_back(caller_of[i]);
        }
        if (re_at.empty()) continue;
        std::sort(re_at.begin(), re_at.end());
        const uint64_t m = re_at.size();
        re_proofs.resize(m * 256);
        re_publics.clear();
        re_key.resize(m);
        re_sig.assign(m + 1, 0);
        re_verdict.assign(m, 0);
        for (uint64_t q = 0; q < m; q++) {
            const uint64_t i = re_at[q];
            memcpy(re_proofs.data() + q * 256, proofs + i * 256, 256);
            re_key[q] = key_of[i];
            re_sig[q] = re_publics.size() / 32;
            if (at[i + 1] > at[i]) re_publics.insert(re_publics.end(), publics + at[i] * 32, publics + at[i + 1] * 32);
        }
        re_sig[m] = re_publics.size() / 32;
        set_verify_locked(set, re_proofs.data(), re_key.data(), re_publics.data(), re_sig, m, re_verdict.data());
        launches += set->plan.last_launches;
        for (uint64_t q = 0; q < m; q++) verdict[re_at[q]] = re_verdict[q];
        rep.proofs_rechecked += m;
    }
    set->plan.last_path = ZK_VERIFY_PATH_BATCH;
    set->plan.last_launches = launches;
    set->plan.last_waves_padded = 0;
    rep.launches = launches;
    leave();
}

}   // namespace

extern "C" int zk_vkey_set_verify_batch(zk_vkey_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes,
                                        uint64_t n, const uint8_t *scalars16, uint8_t *verdict, zk_vkey_set_batch_report *report) {
    return guarded([&] { set_verify_batch(set, proofs, key_of, publics, publics_bytes, n, scalars16, verdict, report); });
}
