// Is this .zkey the key of this circuit over this Powers of Tau file?  (include/zkhip.h, section "Is this .zkey the key
// of this circuit".)  Nothing in the reference corresponds to it: its prover reads a finished .zkey and trusts it
// (src/main_prover.cpp:57-72); the counterpart is the arithmetic half of snarkjs `zkey verify` (section 10 of the key,
// the contribution transcript, is NOT read: DESIGN.md section 19 says why).
//
// The obvious way is to make the key again (setup.hip) and compare bytes: a few hundred doublings per non-zero.  This
// unit never makes a second key.  With one scalar s drawn AFTER the three files are mapped, p_w = s^w over the wires and
//     a = A'.p,  b = B.p,  c = C.p       (row sums over the domain; A' = A plus the public-input rows of setup.hip)
// the sum over the wires of s^w (key point of wire w) is, by linearity, a multi-scalar multiplication of a Lagrange level
// of the .ptau (T12 .. T15 = level k of sections 12 .. 15, T12' = level k + 1 of section 12) by one of these vectors:
//   A    sum s^w A_w  = MSM(T12, a)                 B1   sum s^w B1_w = MSM(T12, b)            B2   sum s^w B2_w = MSM(T13, b)
//   IC   sum_(w <= nPublic) s^w IC_w = MSM(T15, a_pub) + MSM(T14, b_pub) + MSM(T12, c_pub)
//   C    e(sum_(w > nPublic) s^w C_w, delta2) = e(MSM(T15, a_priv) + MSM(T14, b_priv) + MSM(T12, c_priv), G2)
//   H    e(sum s^i H_i, delta2) = e(sum s^i T12'[2i + 1], G2)
//   delta  e(delta1, G2) = e(G1, delta2)
// with a_pub / a_priv the row sums of p with the private / the public wires zeroed (a = a_pub + a_priv).  Every item is a
// polynomial identity in s of degree < 2^29 (nVars < 2^29): a wrong key passes one with probability < 2^29 / r.  The G1
// and G2 equalities are compared after normalisation; the three pairing products are one zk_pairing(group = 2) call.
// The items stay separate, so that the report says which section is wrong.
//
// What runs where.  The row sums are r1cs.hip's segmented sum (r1cs_internal.hpp) with x = p_pub and x = p_priv; the
// kernels below make those two vectors from the table of squarings of s, turn the sums from the 2^261 form into the
// standard form the sort of a multiplication reads (appending the public-input rows s^i to a_pub), add two vectors and
// gather the odd points of T12'.  Section 4 is compared by zk_r1cs_match_zkey.  The multiplications, the pass over the
// key's points (coordinates, curve, subgroup) and the powers of s are ptengine.hpp's, the code of zk_ptau_check: key
// sections go through the engines in chunks of ZKHIP_ZKEY_VERIFY_CHUNK points (2^22 otherwise) and chunk sums are added
// on the host; the .ptau's levels stay on the device while they are used and are copied into the engine's chunk buffer
// for every multiplication (the engine rewrites its points in place).
//
// Fields: field.hpp's 8 x 32-bit Montgomery forms in the kernels here; the multiplications keep their 29-bit form.
#include "ptengine.hpp"
#include "r1cs_section.hpp"
#include "r1cs_internal.hpp"

namespace {

constexpr uint64_t DEFAULT_CHUNK = 1ull << 22;
constexpr uint32_t MAX_LOG_DOMAIN = 27;              // the prover's limit, as setup.hip

// ---------------------------------------------------------------- device
// pub[w] = s^w for w <= nPublic, else 0; priv[w] = s^w for w > nPublic, else 0.  Standard form (what the row sum reads)
__global__ __launch_bounds__(256) void k_zv_masked_powers(Fr *pub, Fr *priv, const Fr *__restrict__ tab, uint64_t nVars, uint64_t nPublic) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nVars) return;
    const Fr p = Fr::from_mont(pow_tab(tab, w)), z = Fr::zero();
    const bool is_pub = w <= nPublic;
    store_el(pub + w, is_pub ? p : z);
    store_el(priv + w, is_pub ? z : p);
}

// out[i], i < n: the row sum rows[i] (value * 2^261 mod r, canonical words) in standard form for i < m; s^(i - m) for
// m <= i < m + nP1 (the public-input rows: constraint m + i, wire i, value 1; nP1 = 0 for a vector that has none); 0 after.
// inv32 = 2^-5 mod r as plain words: a Montgomery product by it is a division by 2^261.
__global__ __launch_bounds__(256) void k_zv_rows(Fr *out, const Fr *__restrict__ rows, const Fr *__restrict__ tab, uint64_t m, uint64_t nP1, uint64_t n,
                                                 Fr inv32) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr v = Fr::zero();
    if (i < m) v = Fr::mul(load_el(rows + i), inv32);
    else if (i - m < nP1) v = Fr::from_mont(pow_tab(tab, i - m));
    store_el(out + i, v);
}

// a[i] += b[i] mod r
__global__ __launch_bounds__(256) void k_zv_add(Fr *a, const Fr *__restrict__ b, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_el(a + i, Fr::add(load_el(a + i), load_el(b + i)));
}

// out[i] = lvl[2 i + 1], i < cnt: G1 points as four 16-byte words
__global__ __launch_bounds__(256) void k_zv_gather_odd(uint4 *out, const uint4 *__restrict__ lvl, uint64_t cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
#pragma unroll
    for (int q = 0; q < 4; q++) out[4 * i + q] = lvl[4 * (2 * i + 1) + q];
}

// ---------------------------------------------------------------- host: the three files against each other
uint64_t chunk_points() { return env_number("ZKHIP_ZKEY_VERIFY_CHUNK", DEFAULT_CHUNK, 1, 1ull << 28, "a number of points from 1 to 2^28", ENV_LAX); }

struct Plan {
    uint32_t k = 0, m = 0, nWires = 0, nPublic = 0, shape = 0;
    uint64_t nnz = 0, nCoefs = 0, cap = 0, device_bytes = 0;
    uint64_t n() const { return 1ull << k; }
    uint64_t nP1() const { return (uint64_t)nPublic + 1; }
};

void need_section(const char *name, const void *p, uint64_t have, uint64_t need) {
    if (need && !p) throw std::invalid_argument(std::string("zkey has no ") + name);
    if (have < need) throw std::invalid_argument(std::string("zkey ") + name + " is short: " + std::to_string(have) + " bytes, the header implies " + std::to_string(need));
}

void make_plan(const zk_r1cs_view *r, const zk_ptau_view *p, const zk_zkey_verify_view *zv, Plan &pl) {
    if (!r || !p || !zv) throw std::invalid_argument("null argument");
    const zk_zkey_view &z = zv->key;
    pl.m = r->nConstraints;
    pl.nWires = r->nWires;
    const uint64_t npub = (uint64_t)r->nPubOut + r->nPubIn;
    if (npub + 1 > r->nWires)
        throw std::invalid_argument("r1cs has " + std::to_string(r->nWires) + " wires: fewer than the constant wire and " + std::to_string(npub) + " public signals");
    pl.nPublic = (uint32_t)npub;
    if (r->nConstraints && !r->constraints) throw std::invalid_argument("null constraints section");
    std::vector<uint64_t> lc_off, rowptr;
    walk_constraints(r, lc_off, rowptr);
    pl.nnz = rowptr.back();
    if (pl.nnz + pl.nP1() >= (1ull << 32)) throw std::invalid_argument("r1cs has 2^32 terms or more: not supported");
    const uint64_t need = (uint64_t)pl.m + npub + 1;
    uint32_t k = 1;
    while ((1ull << k) < need) k++;
    // the key's own domain when it can hold the circuit (snarkjs writes the smallest; a larger power of two is a key too)
    const uint64_t dom = zv->key.domainSize;
    const bool dom_ok = dom >= need && dom >= 2 && (dom & (dom - 1)) == 0;
    if (dom_ok) k = ilog2_exact(dom);
    pl.k = k;
    if (k > MAX_LOG_DOMAIN)
        throw std::invalid_argument("the circuit needs a domain of 2^" + std::to_string(k) + ": more than 2^27, the prover's limit");
    if (!z.vk_alpha1 || !z.vk_beta1 || !z.vk_beta2 || !z.vk_delta1 || !z.vk_delta2 || !zv->vk_gamma2) throw std::invalid_argument("null zkey point");
    if (!p->alpha1 || !p->beta1 || !p->beta2) throw std::invalid_argument("null ptau point");

    // ---- shapes of well-formed files that disagree: a finding, not an error
    if (z.nVars != r->nWires) pl.shape |= 1u << ZK_ZV_SHAPE_NVARS;
    if (z.nPublic != pl.nPublic) pl.shape |= 1u << ZK_ZV_SHAPE_NPUBLIC;
    if (!dom_ok) pl.shape |= 1u << ZK_ZV_SHAPE_DOMAIN;
    const bool prepared = p->lagrange_g1 && p->lagrange_g2 && p->lagrange_alpha_g1 && p->lagrange_beta_g1;
    if (!prepared) pl.shape |= 1u << ZK_ZV_SHAPE_PTAU_UNPREPARED;
    if (p->power < k) pl.shape |= 1u << ZK_ZV_SHAPE_PTAU_POWER;
    if (p->power > 32) throw std::invalid_argument("ptau power " + std::to_string(p->power) + " is not supported");

    if (!pl.shape) {
        const uint64_t nv = z.nVars, n = pl.n();
        if (z.nCoefs >= (1ull << 32)) throw std::invalid_argument("nCoefs >= 2^32 is not supported");
        need_section("section 3 (IC)", zv->pointsIC, zv->pointsIC_bytes, pl.nP1() * 64);
        need_section("section 4 (coefficients)", z.coefs, z.coefs_bytes, 4 + z.nCoefs * 44);
        need_section("section 5 (A)", z.pointsA, z.pointsA_bytes, nv * 64);
        need_section("section 6 (B1)", z.pointsB1, z.pointsB1_bytes, nv * 64);
        need_section("section 7 (B2)", z.pointsB2, z.pointsB2_bytes, nv * 128);
        need_section("section 8 (C)", z.pointsC, z.pointsC_bytes, (nv - pl.nP1()) * 64);
        need_section("section 9 (H)", z.pointsH, z.pointsH_bytes, n * 64);
        const uint64_t pts1 = (1ull << (p->power + 1)) - 1;       // levels 0 .. power
        const struct {
            int id;
            uint64_t have, need;
        } sec[4] = {{12, p->lagrange_g1_bytes, (2 * pts1 + 1) * 64}, {13, p->lagrange_g2_bytes, pts1 * 128},
                    {14, p->lagrange_alpha_g1_bytes, pts1 * 64}, {15, p->lagrange_beta_g1_bytes, pts1 * 64}};
        for (const auto &s : sec)
            if (s.have < s.need)
                throw std::invalid_argument("ptau section " + std::to_string(s.id) + " is short: " + std::to_string(s.have) + " bytes, power " +
                                            std::to_string(p->power) + " needs " + std::to_string(s.need));
    }
    pl.nCoefs = pl.shape ? pl.nnz + pl.nP1() : z.nCoefs;

    // ---- an upper estimate of the HBM, from the circuit's own numbers
    const uint64_t n = pl.n(), nw = pl.nWires, m = pl.m, chunk = chunk_points(), most = nw > n ? nw : n;
    pl.cap = most < chunk ? most : chunk;
    const uint64_t segs = 3 * m + pl.nnz / 8 + 16;
    const uint64_t circuit = r->constraints_bytes + 8 * (6 * m + 2)                // the section and its offsets while it is decoded
                             + pl.nnz * 36 + 3 * m * 32 + nw * 32                   // wire ids, coefficients, row sums, x
                             + 16 * segs + 32 * (pl.nnz / 8 + 2);                   // the passes' bounds and partials
    const uint64_t match = pl.nCoefs * (44 + 36) + n * (16 + 96) + 4096;            // zk_r1cs_match_zkey: records, CSR, a | b | c
    const uint64_t vectors = 2 * nw * 32 + 6 * n * 32;                              // p_pub, p_priv; a, b, c (pub and priv)
    const uint64_t levels = n * (64 + 128 + 64 + 64) + 2 * n * 64;                  // level k of 12 .. 15, level k + 1 of 12
    pl.device_bytes = circuit + match + vectors + levels + EnginePair::bytes(pl.cap) + POW_BITS * sizeof(Fr) + 65536;
}

// ---------------------------------------------------------------- the check
struct R1csHandle {
    zk_r1cs *r = nullptr;
    ~R1csHandle() { zk_r1cs_destroy(r); }
};

struct Verifier : EnginePair {
    const Plan &pl;
    zk_zkey_verify_report &rep;
    hipStream_t st;
    PowTable stab;
    Verifier(const Plan &pl_, zk_zkey_verify_report &rep_, const Fr &s, hipStream_t st_) : EnginePair(st_, pl_.cap), pl(pl_), rep(rep_), st(st_) {
        stab.build(s, st);
    }

    // The pass of zk_ptau_check over the cnt points the engine holds; false: the report names a malformed point of `sec`,
    // index0 + its place
    template <class F>
    bool checked(int sec, uint64_t index0, uint64_t cnt, bool inf_bad, bool subgroup) {
        const BadPoint bad = classify<F>(cnt, inf_bad, subgroup);
        if (!bad.kind) return true;
        rep.verdict = 2;
        rep.bad_section = (uint32_t)sec;
        rep.bad_kind = bad.kind;
        rep.bad_index = index0 + bad.index;
        return false;
    }

    // sum = sum_(i < cnt) s^(e0 + i) P_i over the cnt points of key section `sec`, checked chunk by chunk; false: malformed
    template <class F>
    bool key_row(int sec, const void *points, uint64_t cnt_all, uint64_t e0, Pt<F> &sum) {
        sum = Pt<F>();
        return power_sum(engine<F>(), sum, cnt_all, stab, e0, [&](uint64_t off, uint64_t cnt) {
            engine<F>().load(static_cast<const uint8_t *>(points) + off * sizeof(Affine<F>), cnt);
            return checked<F>(sec, off, cnt, false, sec == 7);
        });
    }

    // sum_(i < n) vec[i] lvl[i]: a level that is on the device by a vector that is (standard form)
    template <class F>
    Pt<F> level_msm(const DevBuf<uint8_t> &lvl, const Fr *vec, uint64_t n) {
        Engine<F> &e = engine<F>();
        Pt<F> sum;
        for (uint64_t off = 0; off < n; off += e.cap) {
            const uint64_t cnt = n - off < e.cap ? n - off : e.cap;
            HIP_TRY(hipMemcpyAsync(e.pts.p, lvl.p + off * sizeof(Affine<F>), cnt * sizeof(Affine<F>), hipMemcpyDeviceToDevice, st));
            Pt<F> part;
            e.msm.run(part.b, e.pts.p, vec + off, cnt, st);
            sum = sum + part;
        }
        return sum;
    }
};

void write_report(zk_zkey_verify_report *out, zk_zkey_verify_report &r, uint32_t size) {
    r.size = size;
    memcpy(out, &r, size);
}

void zkey_verify(const zk_r1cs_view *rv, const zk_ptau_view *p, const zk_zkey_verify_view *zv, const uint8_t *s32_in, int32_t device,
                 zk_zkey_verify_report *out) {
    if (!out) throw std::invalid_argument("null argument");
    const uint32_t size = out->size && out->size < sizeof *out ? out->size : (uint32_t)sizeof *out;
    zk_zkey_verify_report rep;
    memset(&rep, 0, sizeof rep);
    rep.coef_first_row = NONE;
    Plan pl;
    make_plan(rv, p, zv, pl);                         // the files are checked before the device is touched
    uint8_t s32[32];
    if (s32_in) {
        memcpy(s32, s32_in, 32);
        if (is_0_or_1(s32) || !below(s32, FrParams::P)) throw std::invalid_argument("zk_zkey_verify: the check scalar must be at least 2 and below r");
    } else {
        draw_scalar(s32, "zk_zkey_verify");            // after the files are mapped: their maker did not know s
    }
    if (pl.shape) {
        rep.verdict = 1;
        rep.shape_failed = pl.shape;
        write_report(out, rep, size);
        return;
    }
    const zk_zkey_view &z = zv->key;
    const Fr s = fr_from_std(s32);
    Pt<Fq> g1;
    Pt<Fq2> g2;
    generators(g1, g2);
    const Pt<Fq> alpha1(z.vk_alpha1), beta1(z.vk_beta1), delta1(z.vk_delta1);
    const Pt<Fq2> beta2(z.vk_beta2), gamma2(zv->vk_gamma2), delta2(z.vk_delta2);
    uint32_t failed = 0;
    if (!(alpha1 == Pt<Fq>(p->alpha1))) failed |= 1u << ZK_ZV_ALPHA1;
    if (!(beta1 == Pt<Fq>(p->beta1))) failed |= 1u << ZK_ZV_BETA1;
    if (!(beta2 == Pt<Fq2>(p->beta2))) failed |= 1u << ZK_ZV_BETA2;
    if (!(gamma2 == g2)) failed |= 1u << ZK_ZV_GAMMA2;
    rep.delta_is_generator = delta2 == g2 ? 1 : 0;

    const int dev = resolve_device(device);
    DeviceGuard g(dev);
    need_hbm("zk_zkey_verify", pl.device_bytes);
    R1csHandle rh;
    if (zk_r1cs_create(&rh.r, rv, dev) != 0) throw std::runtime_error(std::string("zk_zkey_verify: ") + get_error());
    const R1csDev rd = r1cs_dev(rh.r);
    const hipStream_t st = rd.stream;                 // one stream: the row sums and what reads them stay in order
    Verifier v(pl, rep, s, st);
    const uint64_t n = pl.n(), nw = pl.nWires, nP1 = pl.nP1(), m = pl.m;

    // ---- every point of the key: section 2 point by point in the file's order, then sections 3 and 5 to 9, whose sums
    // sum s^w P_w are made as their chunks pass
    auto bad = [&] { write_report(out, rep, size); };
    {
        const struct {
            const uint8_t *b;
            bool g2;
        } sec2[6] = {{alpha1.b, false}, {beta1.b, false}, {beta2.b, true}, {gamma2.b, true}, {delta1.b, false}, {delta2.b, true}};
        for (uint64_t i = 0; i < 6; i++) {
            bool ok;
            if (sec2[i].g2) {
                HIP_TRY(hipMemcpyAsync(v.e2.pts.p, sec2[i].b, 128, hipMemcpyHostToDevice, st));
                ok = v.checked<Fq2>(2, i, 1, true, true);
            } else {
                HIP_TRY(hipMemcpyAsync(v.e1.pts.p, sec2[i].b, 64, hipMemcpyHostToDevice, st));
                ok = v.checked<Fq>(2, i, 1, true, false);
            }
            if (!ok) return bad();
        }
    }
    Pt<Fq> sIC, sA, sB1, sC, sH;
    Pt<Fq2> sB2;
    if (!v.key_row<Fq>(3, zv->pointsIC, nP1, 0, sIC) || !v.key_row<Fq>(5, z.pointsA, nw, 0, sA) || !v.key_row<Fq>(6, z.pointsB1, nw, 0, sB1) ||
        !v.key_row<Fq2>(7, z.pointsB2, nw, 0, sB2) || !v.key_row<Fq>(8, z.pointsC, nw - nP1, nP1, sC) || !v.key_row<Fq>(9, z.pointsH, n, 0, sH))
        return bad();

    // ---- section 4 against the circuit
    {
        uint64_t rows = 0;
        uint32_t first = NONE;
        if (zk_r1cs_match_zkey(rh.r, &z, &rows, &first) != 0) throw std::runtime_error(std::string("zk_zkey_verify: ") + get_error());
        rep.coef_rows_differing = rows;
        rep.coef_first_row = first;
        if (rows) failed |= 1u << ZK_ZV_COEFS;
    }

    // ---- a, b, c with the public and with the private wires: six vectors over the domain, standard form
    DevBuf<Fr> vec[6];                                // a_pub, b_pub, c_pub, a_priv, b_priv, c_priv
    {
        DevBuf<Fr> ppub, ppriv;
        ppub.alloc(nw);
        ppriv.alloc(nw);
        ZK_LAUNCH(k_zv_masked_powers, dim3(nblocks(nw, 256)), dim3(256), 0, st, ppub.p, ppriv.p, v.stab.d.p, nw, (uint64_t)pl.nPublic);
        ZK_LAUNCH_OK("zkey verify masked powers");
        const Fr inv32 = Fr::from_mont(Fr::inv(fr_small(32)));
        for (int half = 0; half < 2; half++) {
            r1cs_spmv(rh.r, half ? ppriv.p : ppub.p);
            for (int mat = 0; mat < 3; mat++) {
                DevBuf<Fr> &d = vec[3 * half + mat];
                d.alloc(n);
                ZK_LAUNCH(k_zv_rows, dim3(nblocks(n, 256)), dim3(256), 0, st, d.p, rd.rows + (uint64_t)mat * m, v.stab.d.p, (uint64_t)m,
                          half == 0 && mat == 0 ? nP1 : (uint64_t)0, n, inv32);
            }
            ZK_LAUNCH_OK("zkey verify rows");
        }
        HIP_TRY(hipStreamSynchronize(st));            // ppub, ppriv leave scope
    }

    // ---- the multiplications of the .ptau's levels
    Pt<Fq> mA, mB1, mIC, mK, mH;
    Pt<Fq2> mB2;
    {
        DevBuf<uint8_t> t12, t14, t15;
        upload_level(t12, p->lagrange_g1, pl.k, 64, st);
        upload_level(t14, p->lagrange_alpha_g1, pl.k, 64, st);
        upload_level(t15, p->lagrange_beta_g1, pl.k, 64, st);
        mIC = v.level_msm<Fq>(t15, vec[0].p, n) + v.level_msm<Fq>(t14, vec[1].p, n) + v.level_msm<Fq>(t12, vec[2].p, n);
        mK = v.level_msm<Fq>(t15, vec[3].p, n) + v.level_msm<Fq>(t14, vec[4].p, n) + v.level_msm<Fq>(t12, vec[5].p, n);
        t14.release();
        t15.release();
        ZK_LAUNCH(k_zv_add, dim3(nblocks(n, 256)), dim3(256), 0, st, vec[0].p, vec[3].p, n);      // a = a_pub + a_priv
        ZK_LAUNCH(k_zv_add, dim3(nblocks(n, 256)), dim3(256), 0, st, vec[1].p, vec[4].p, n);      // b
        ZK_LAUNCH_OK("zkey verify add");
        mA = v.level_msm<Fq>(t12, vec[0].p, n);
        mB1 = v.level_msm<Fq>(t12, vec[1].p, n);
    }
    {
        DevBuf<uint8_t> t13;
        upload_level(t13, p->lagrange_g2, pl.k, 128, st);
        mB2 = v.level_msm<Fq2>(t13, vec[1].p, n);
    }
    for (auto &d : vec) d.release();
    {
        // sum s^i T12'[2 i + 1]: the odd points of level k + 1, gathered chunk by chunk into the engine's buffer
        DevBuf<uint8_t> top;
        upload_level(top, p->lagrange_g1, pl.k + 1, 64, st);
        Engine<Fq> &e = v.e1;
        for (uint64_t off = 0; off < n; off += e.cap) {
            const uint64_t cnt = n - off < e.cap ? n - off : e.cap;
            ZK_LAUNCH(k_zv_gather_odd, dim3(nblocks(cnt, 256)), dim3(256), 0, st, reinterpret_cast<uint4 *>(e.pts.p),
                      reinterpret_cast<const uint4 *>(top.p + 2 * off * 64), cnt);
            ZK_LAUNCH(k_fr_powers, dim3(nblocks(cnt, 256)), dim3(256), 0, st, e.sc.p, v.stab.d.p, off, cnt);
            ZK_LAUNCH_OK("zkey verify H");
            e.accumulate(mH, cnt);
        }
    }

    // ---- the equalities, and the three pairing products in one call
    if (!(sA == mA)) failed |= 1u << ZK_ZV_A;
    if (!(sB1 == mB1)) failed |= 1u << ZK_ZV_B1;
    if (!(sB2 == mB2)) failed |= 1u << ZK_ZV_B2;
    if (!(sIC == mIC)) failed |= 1u << ZK_ZV_IC;
    const Pt<Fq> p1[6] = {delta1, g1.neg(), sC, mK.neg(), sH, mH.neg()};
    const Pt<Fq2> p2[6] = {g2, delta2, delta2, g2, delta2, g2};
    uint8_t b1[6 * 64], b2[6 * 128], gt[3 * 384];
    for (int i = 0; i < 6; i++) {
        memcpy(b1 + 64 * i, p1[i].b, 64);
        memcpy(b2 + 128 * i, p2[i].b, 128);
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (zk_pairing(gt, b1, b2, 6, 2, dev) != 0) throw std::runtime_error(std::string("zk_zkey_verify: ") + get_error());
    bool one[3];
    for (int e = 0; e < 3; e++) {
        const uint8_t *o = gt + 384 * e;
        one[e] = o[0] == 1;
        for (int i = 1; i < 384 && one[e]; i++) one[e] = o[i] == 0;
    }
    if (!one[0]) {
        failed |= 1u << ZK_ZV_DELTA;
        rep.not_checked = (1u << ZK_ZV_C) | (1u << ZK_ZV_H);      // e(., delta2) says nothing when delta1 and delta2 disagree
    } else {
        if (!one[1]) failed |= 1u << ZK_ZV_C;
        if (!one[2]) failed |= 1u << ZK_ZV_H;
    }
    rep.failed = failed;
    rep.verdict = failed ? 1 : 0;
    write_report(out, rep, size);
}

}   // namespace

extern "C" {

int zk_zkey_verify_sizes(const zk_r1cs_view *r1cs, const zk_ptau_view *ptau, const zk_zkey_verify_view *zkey, zk_zkey_verify_sizes_t *sizes) {
    return guarded([&] {
        if (!sizes) throw std::invalid_argument("null argument");
        Plan pl;
        make_plan(r1cs, ptau, zkey, pl);
        sizes->log_domain = pl.k;
        sizes->shape_failed = pl.shape;
        sizes->chunk_points = pl.cap;
        sizes->device_bytes = pl.device_bytes;
    });
}

int zk_zkey_verify(const zk_r1cs_view *r1cs, const zk_ptau_view *ptau, const zk_zkey_verify_view *zkey, const uint8_t *s32, int32_t device,
                   zk_zkey_verify_report *report) {
    return guarded([&] { zkey_verify(r1cs, ptau, zkey, s32, device, report); });
}

}   // extern "C"
