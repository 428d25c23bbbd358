// Batch verification by random linear combination with every proof's own verdict kept (zk_vkey_verify_batch,
// include/zkhip.h).  Consecutive proofs of a chunk form groups; with a 128-bit scalar r_i per proof
// a group passes iff
//     prod_i e(r_i A_i, B_i) . e(-R alpha, beta) . e(-X, gamma) . e(-Cs, delta) = 1,
//     R = sum r_i,  S_j = sum r_i pub_ij (mod r),  X = R IC_0 + sum_j S_j IC_j,  Cs = sum r_i C_i,
// which costs one variable-Q Miller loop and two short G1 multiplications per proof and everything else once per group.
// The well-formed proofs of a failing group go through the per-proof pass of pairing.hip (vkey_verify_locked), all failed
// groups of a chunk in one pass, so a verdict differs from zk_vkey_verify's only when an INVALID proof sits in a group that
// passes: at most one of the 2^128 - 1 values of its scalar does that.
//
// Kernels, in launch order per chunk:
//   k_batch_check    a lane per proof: the format and curve tests of k_verify_check, B's subgroup by the endomorphism
//   k_batch_scale    a lane per proof: r_i A_i (made affine) and r_i C_i by one double-and-add over the scalar's bits
//   k_batch_miller   a lane per proof: the Miller value of (r_i A_i, B_i); 1 for a malformed proof
//   k_batch_fr       a wave per (group, j): S_j, R and the count of well-formed proofs, summed by a fixed tree in LDS
//   k_batch_reduce   a wave per 64 values: the product of the f_i and the sum of the r_i C_i, by a fixed tree in LDS; run
//                    again on its own output until one value a group is left (groups above 64 proofs)
//   k_batch_tail     a workgroup per group: X and R alpha with mul_glv, the three table-driven pairs under one squaring
//                    chain, the product with the group's f and the final exponentiation, on pairing_coop_dev.hpp's LDS
//                    block and sliced Fq12 operations
// No atomics on points or field elements: every sum has a fixed shape, so the bytes do not depend on scheduling.
//
// What this unit has in common with pairing_set_batch.hip is written once: what a lane does in the check, scale and Miller
// kernels, the wave that sums X and the tail's points in verify_batch_dev.hpp; the scalars, the group switch and the
// report's size in verify_batch_host.hpp.  The kernels here only find the lane's proof.
#include "verify_batch_dev.hpp"
#include "pairing_internal.hpp"

namespace {

// ---------------------------------------------------------------- a lane per proof: verify_batch_dev.hpp's bodies, lane i has proof i
__global__ __launch_bounds__(64) void k_batch_check(uint32_t *status, const uint8_t *__restrict__ proofs, const Fr *__restrict__ publics, uint64_t n,
                                                    uint32_t nPublic, const PairConsts *__restrict__ k, Fq b1, Fq2 b2) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    batch_check_lane(status + i, proofs + i * 256, publics + i * nPublic, nPublic, k, b1, b2);
}

__global__ __launch_bounds__(64) void k_batch_scale(G1Affine *ra, G1XYZZ *rc, const uint32_t *__restrict__ status, const uint8_t *__restrict__ proofs,
                                                    const Scalar16 *__restrict__ scalars, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    batch_scale_lane(ra + i, rc + i, status[i], proofs + i * 256, scalars + i);
}

__global__ __launch_bounds__(64) void k_batch_miller(Fq12 *f_out, const uint32_t *__restrict__ status, const uint8_t *__restrict__ proofs,
                                                     const G1Affine *__restrict__ ra, uint64_t n, const PairConsts *k) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    batch_miller_lane(f_out + i, status[i], proofs + i * 256, ra + i, k);
}

// ---------------------------------------------------------------- the sums in Fr
// Block g (nPublic + 1) + j: S[g (nPublic + 1) + j] = sum over the well-formed proofs i of group g of r_i pub_ij for
// j < nPublic, and of r_i for j = nPublic (R), standard form; that block also counts the well-formed proofs into wf[g].
__global__ __launch_bounds__(64) void k_batch_fr(Fr *S, uint32_t *wf, const uint32_t *__restrict__ status, const Fr *__restrict__ publics,
                                                 const Scalar16 *__restrict__ scalars, uint64_t n, uint32_t nPublic, uint32_t group) {
    __shared__ Fr part[64];
    __shared__ uint32_t cnt[64];
    const uint32_t lane = threadIdx.x, terms = nPublic + 1;
    const uint64_t g = blockIdx.x / terms;
    const uint32_t j = blockIdx.x % terms;
    const uint64_t lo = g * group, hi = n - lo < group ? n : lo + group;
    Fr acc = Fr::zero();
    uint32_t c = 0;
    for (uint64_t i = lo + lane; i < hi; i += 64) {
        if (status[i] != ST_OK) continue;
        const Fr r = scalar_of(scalars + i);
        c++;
        if (j == nPublic) acc = Fr::add(acc, r);
        else acc = Fr::add(acc, Fr::mul(Fr::to_mont(r), load_el(publics + i * nPublic + j)));   // (r R) pub / R
    }
    part[lane] = acc;
    cnt[lane] = c;
    for (uint32_t s = 32; s; s >>= 1) {
        __syncthreads();
        if (lane < s) {
            part[lane] = Fr::add(part[lane], part[lane + s]);
            cnt[lane] += cnt[lane + s];
        }
    }
    if (lane == 0) {
        store_el(S + blockIdx.x, part[0]);
        if (j == nPublic) wf[g] = cnt[0];
    }
}

// ---------------------------------------------------------------- the product of the f_i and the sum of the r_i C_i
// Group g holds `stride_in` consecutive values (the last group `len_last`); block g stride_out + b multiplies values
// 64 b .. 64 b + 63 of it into fout / cout[g stride_out + b].  stride_out = ceil(stride_in / 64).
struct ReduceLds {
    Fq12 f[64];
    G1XYZZ c[64];
};
static_assert(sizeof(ReduceLds) == 64 * (384 + 128), "LDS of a reduction wave");

__global__ __launch_bounds__(64) void k_batch_reduce(Fq12 *fout, G1XYZZ *cout, const Fq12 *__restrict__ fin, const G1XYZZ *__restrict__ cin,
                                                     uint32_t stride_in, uint32_t len_last, uint32_t ngroups, uint32_t stride_out) {
    __shared__ ReduceLds R;
    const uint32_t lane = threadIdx.x;
    const uint32_t g = blockIdx.x / stride_out, b = blockIdx.x % stride_out;
    const uint32_t len = g == ngroups - 1 ? len_last : stride_in;
    const uint32_t base = b * 64;
    if (base >= len) return;                          // the same in every lane, before any barrier
    const uint32_t cnt = len - base < 64 ? len - base : 64;
    const uint64_t at = (uint64_t)g * stride_in + base + lane;
    if (lane < cnt) {
        R.f[lane] = fin[at];
        R.c[lane] = load_pt(cin + at);
    }
    for (uint32_t s = 32; s; s >>= 1) {
        __syncthreads();
        if (lane < s && lane + s < cnt) {
            Fq12 x = R.f[lane];
            const Fq12 y = R.f[lane + s];
            f12_mul(x, x, y);
            R.f[lane] = x;
            G1XYZZ p = R.c[lane];
            const G1XYZZ q = R.c[lane + s];
            nl_add(p, q);
            R.c[lane] = p;
        }
    }
    if (lane == 0) {
        const uint64_t to = (uint64_t)g * stride_out + b;
        fout[to] = R.f[0];
        store_pt(cout + to, R.c[0]);
    }
}

// ---------------------------------------------------------------- the tail: a workgroup per group
__shared__ TailPts<1> T;                             // -R alpha, -X, -Cs

// pass[g] = 1 when group g's equation holds, 0 when it fails; a group without a well-formed proof is left alone.
// F, Cs: the group's product and sum at index g stride; S, wf: k_batch_fr's; tab: gamma's lines, then delta's
__global__ __launch_bounds__(TAIL_THREADS) void k_batch_tail(uint8_t *pass, const Fq12 *__restrict__ F, const G1XYZZ *__restrict__ Cs, uint32_t stride,
                                                             const Fr *__restrict__ S, const uint32_t *__restrict__ wf, uint32_t nPublic,
                                                             const G1Affine *__restrict__ alpha, const G1Affine *__restrict__ ic,
                                                             const Line *__restrict__ tab_beta, const Line *__restrict__ tab,
                                                             const PairConsts *__restrict__ k, Fq beta) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t g = blockIdx.x;
    if (wf[g] == 0) return;                           // the same in every lane, before any barrier
    const Fr *Sg = S + g * (nPublic + 1);
    // side by side: -R alpha, -Cs, -X
    if (wave == 0) {
        if (lane == 0) {
            G1XYZZ t;
            nl_mul_glv(t, load_pt(alpha), load_el(Sg + nPublic), beta);
            put_neg(&T.pt[0][0], &T.have[0][0], t);
        }
    } else if (wave == 1) {
        if (lane == 0) put_neg(&T.pt[0][2], &T.have[0][2], load_pt(Cs + g * stride));
    } else {
        x_wave(lane, ic, Sg, nPublic, beta);
        if (lane == 0) put_neg(&T.pt[0][1], &T.have[0][1], L.part[0]);
    }
    __syncthreads();
    if (wave) return;                                 // no barrier below
    // E_T0: the group's product of Miller values, until the final exponentiation takes the slot
    if (lane < 6) L.e[E_T0][lane] = load_el(reinterpret_cast<const Fq2 *>(F + g * stride) + coop_slot(lane));
    c_one(E_IN);
    const bool have_x = T.have[0][1] != 0, have_c = T.have[0][2] != 0;
    const Line *tg = tab, *td = tab + MILLER_LINES;
    int at = 0;
    auto lines3 = [&]() {
        c_line(E_IN, tab_beta + at, &T.pt[0][0]);
        if (have_x) c_line(E_IN, tg + at, &T.pt[0][1]);
        if (have_c) c_line(E_IN, td + at, &T.pt[0][2]);
        at++;
    };
    for (int s = 0; s < 64; s++) {
        c_mul(E_IN, E_IN, E_IN);
        lines3();
        if (ate_bit(s)) lines3();
    }
    lines3();
    lines3();
    c_mul(E_IN, E_IN, E_T0);
    c_final_exp(k);
    if (lane == 0) pass[g] = c_is_one(E_F) ? 1 : 0;
}

__global__ void k_batch_beta_lines(Line *tab, const G2Affine *Q, const PairConsts *k) {
    if (blockIdx.x == 0 && threadIdx.x == 0) line_table(tab, load_pt(Q), *k);
}

// ---------------------------------------------------------------- host
// alpha on the device and beta's lines, once per key
void batch_prepare(zk_vkey *vk, hipStream_t s) {
    if (vk->batch.ready) return;
    DevBuf<G2Affine> db;
    db.alloc(1);
    vk->batch.alpha.alloc(1);
    vk->batch.tab_beta.alloc(MILLER_LINES);
    HIP_TRY(hipMemcpyAsync(vk->batch.alpha.p, vk->alpha_h, sizeof(G1Affine), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(db.p, vk->beta_h, sizeof(G2Affine), hipMemcpyHostToDevice, s));
    ZK_LAUNCH(k_batch_beta_lines, dim3(1), dim3(64), 0, s, vk->batch.tab_beta.p, db.p, vk->kc.k.p);
    ZK_LAUNCH_OK("batch verification: the lines of beta");
    HIP_TRY(hipStreamSynchronize(s));
    vk->batch.ready = true;
}

void verify_batch(zk_vkey *vk, const uint8_t *proofs, const uint8_t *publics, uint64_t n, const uint8_t *scalars16, uint8_t *verdict,
                  zk_vkey_batch_report *report) {
    if (!vk) throw std::invalid_argument("null argument");
    const uint32_t rep_size = report_size(report);
    zk_vkey_batch_report rep;
    memset(&rep, 0, sizeof rep);
    const uint64_t group = group_size(), chunk = chunk_jobs();
    rep.size = rep_size;
    rep.group = (uint32_t)group;
    auto leave = [&]() {
        if (report) memcpy(report, &rep, rep_size);
    };
    if (!n) {
        leave();
        return;
    }
    if (!proofs || !verdict || (vk->nPublic && !publics)) throw std::invalid_argument("null argument");
    refuse_zero_scalars(scalars16, n, "zk_vkey_verify_batch");
    std::lock_guard<std::mutex> lock(vk->mu);
    const uint64_t cap = n < chunk ? n : chunk, pub_bytes = (uint64_t)vk->nPublic * 32, terms = (uint64_t)vk->nPublic + 1;
    const uint64_t cap_groups = (cap + group - 1) / group;
    // the reduction's levels for a chunk of `cap` proofs: level 0 reads the lanes' values, each level writes ceil(stride / 64) a group
    const uint64_t stride1 = (group + 63) / 64, stride2 = (stride1 + 63) / 64;
    const uint64_t n1 = group > 1 ? cap_groups * stride1 : 0, n2 = stride1 > 1 ? cap_groups * stride2 : 0;
    DeviceGuard dg(vk->device);
    need_hbm("zk_vkey_verify_batch", cap * (256 + pub_bytes + 16 + 4 + sizeof(G1Affine) + sizeof(G1XYZZ) + sizeof(Fq12)) +
                                         (n1 + n2) * (sizeof(Fq12) + sizeof(G1XYZZ)) + cap_groups * (terms * 32 + 5) + 65536);
    Stream st;
    hipStream_t s = st.s;
    uint32_t launches = 0;
    if (!vk->batch.ready) {
        batch_prepare(vk, s);
        launches++;
    }
    DevBuf<uint8_t> dp, dpass;
    DevBuf<Fr> dpub, dS;
    DevBuf<Scalar16> dsc;
    DevBuf<uint32_t> dst, dwf;
    DevBuf<G1Affine> dra;
    DevBuf<G1XYZZ> drc, dc1, dc2;
    DevBuf<Fq12> df, df1, df2;
    dp.alloc(cap * 256);
    dpub.alloc(cap * vk->nPublic);
    dsc.alloc(cap);
    dst.alloc(cap);
    dra.alloc(cap);
    drc.alloc(cap);
    df.alloc(cap);
    df1.alloc(n1);
    dc1.alloc(n1);
    df2.alloc(n2);
    dc2.alloc(n2);
    dS.alloc(cap_groups * terms);
    dwf.alloc(cap_groups);
    dpass.alloc(cap_groups);
    std::vector<uint8_t> drawn, pass(cap_groups), re_proofs, re_publics, re_verdict;
    std::vector<uint32_t> status(cap);
    std::vector<uint64_t> re_at;
    const Fq b1 = curve_b<Fq>(), beta = endo_const<Fq>();
    const Fq2 b2 = curve_b<Fq2>();
    for (uint64_t off = 0; off < n; off += cap) {
        const uint64_t cnt = n - off < cap ? n - off : cap;
        const uint64_t ngroups = (cnt + group - 1) / group;
        const dim3 grid(nblocks(cnt, 64)), block(64);
        const uint8_t *sc = scalars16 ? scalars16 + off * 16 : nullptr;
        if (!sc) {                                    // drawn now: the proofs of this call are fixed
            drawn.resize(cnt * 16);
            draw_scalars(drawn.data(), cnt, "zk_vkey_verify_batch");
            sc = drawn.data();
        }
        HIP_TRY(hipMemcpyAsync(dp.p, proofs + off * 256, cnt * 256, hipMemcpyHostToDevice, s));
        if (pub_bytes) HIP_TRY(hipMemcpyAsync(dpub.p, publics + off * pub_bytes, cnt * pub_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(dsc.p, sc, cnt * 16, hipMemcpyHostToDevice, s));
        ZK_LAUNCH(k_batch_check, grid, block, 0, s, dst.p, dp.p, dpub.p, cnt, vk->nPublic, vk->kc.k.p, b1, b2);
        ZK_LAUNCH_OK("batch verification: checks");
        launches++;
        HIP_TRY(hipMemcpyAsync(status.data(), dst.p, cnt * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        uint64_t well = 0;
        for (uint64_t i = 0; i < cnt; i++) well += status[i] == ST_OK;
        rep.malformed += cnt - well;
        for (uint64_t i = 0; i < cnt; i++) verdict[off + i] = status[i] == ST_OK ? ZK_VERIFY_OK : ZK_VERIFY_MALFORMED;
        for (uint64_t g = 0; g < ngroups; g++) {
            bool any = false;
            for (uint64_t i = g * group; i < cnt && i < (g + 1) * group && !any; i++) any = status[i] == ST_OK;
            rep.groups += any;
        }
        if (!well) continue;                          // nothing to combine: no launch
        ZK_LAUNCH(k_batch_scale, grid, block, 0, s, dra.p, drc.p, dst.p, dp.p, dsc.p, cnt);
        ZK_LAUNCH(k_batch_miller, grid, block, 0, s, df.p, dst.p, dp.p, dra.p, cnt, vk->kc.k.p);
        ZK_LAUNCH(k_batch_fr, dim3((uint32_t)(ngroups * terms)), block, 0, s, dS.p, dwf.p, dst.p, dpub.p, dsc.p, cnt, vk->nPublic, (uint32_t)group);
        launches += 3;
        const Fq12 *fin = df.p;
        const G1XYZZ *cin = drc.p;
        uint64_t stride = group, len_last = cnt - (ngroups - 1) * group;
        for (int level = 0; stride > 1; level++) {
            const uint64_t so = (stride + 63) / 64;
            Fq12 *fo = level & 1 ? df2.p : df1.p;
            G1XYZZ *co = level & 1 ? dc2.p : dc1.p;
            ZK_LAUNCH(k_batch_reduce, dim3((uint32_t)(ngroups * so)), block, 0, s, fo, co, fin, cin, (uint32_t)stride, (uint32_t)len_last, (uint32_t)ngroups,
                      (uint32_t)so);
            launches++;
            fin = fo;
            cin = co;
            stride = so;
            len_last = (len_last + 63) / 64;
        }
        HIP_TRY(hipMemsetAsync(dpass.p, 1, ngroups, s));
        ZK_LAUNCH(k_batch_tail, dim3((uint32_t)ngroups), dim3(TAIL_THREADS), 0, s, dpass.p, fin, cin, 1u, dS.p, dwf.p, vk->nPublic, vk->batch.alpha.p, vk->ic.p,
                  vk->batch.tab_beta.p, vk->tab.p, vk->kc.k.p, beta);
        ZK_LAUNCH_OK("batch verification");
        launches++;
        HIP_TRY(hipMemcpyAsync(pass.data(), dpass.p, ngroups, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        // the well-formed proofs of every failed group of this chunk: one pass of the per-proof path
        re_at.clear();
        for (uint64_t g = 0; g < ngroups; g++) {
            if (pass[g]) continue;
            rep.groups_failed++;
            for (uint64_t i = g * group; i < cnt && i < (g + 1) * group; i++)
                if (status[i] == ST_OK) re_at.push_back(off + i);
        }
        if (re_at.empty()) continue;
        const uint64_t m = re_at.size();
        re_proofs.resize(m * 256);
        re_publics.resize(m * pub_bytes);
        re_verdict.assign(m, 0);
        for (uint64_t q = 0; q < m; q++) {
            memcpy(re_proofs.data() + q * 256, proofs + re_at[q] * 256, 256);
            if (pub_bytes) memcpy(re_publics.data() + q * pub_bytes, publics + re_at[q] * pub_bytes, pub_bytes);
        }
        vkey_verify_locked(vk, re_proofs.data(), re_publics.data(), m, re_verdict.data());
        launches += vk->plan.last_launches;
        for (uint64_t q = 0; q < m; q++) verdict[re_at[q]] = re_verdict[q];
        rep.proofs_rechecked += m;
    }
    vk->plan.last_path = ZK_VERIFY_PATH_BATCH;
    vk->plan.last_launches = launches;
    rep.launches = launches;
    leave();
}

}   // namespace

extern "C" int zk_vkey_verify_batch(zk_vkey *vk, const uint8_t *proofs, const uint8_t *publics, uint64_t n, const uint8_t *scalars16, uint8_t *verdict,
                                    zk_vkey_batch_report *report) {
    return guarded([&] { verify_batch(vk, proofs, publics, n, scalars16, verdict, report); });
}
