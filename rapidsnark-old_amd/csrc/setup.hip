// Groth16 setup on the device (include/zkhip.h, section "Groth16 setup"): the phase-2 starting key that snarkjs
// `groth16 setup circuit.r1cs pot.ptau circuit_0000.zkey` writes (gamma = delta = 1), from circom's .r1cs and the
// Lagrange-basis sections of a prepared Powers of Tau file.  Nothing in the reference corresponds to it: its prover reads
// a finished .zkey (src/main_prover.cpp:57-72).
//
// What is computed.  With T12, T13, T14, T15 = level k (the circuit's domain 2^k) of .ptau sections 12 (tau G1),
// 13 (tau G2), 14 (alpha tau G1), 15 (beta tau G1), every table entry of the key is a sparse linear combination of
// given points, one term per R1CS term:
//   A_s  = sum over the A terms (c, s, v) of v T12[c]          (the A terms include snarkjs's public-input rows:
//   B1_s = sum over the B terms of v T12[c]                     constraint m + i, wire i, value 1, i = 0 .. nPublic)
//   B2_s = sum over the B terms of v T13[c]                     G2
//   K_s  = sum_A v T15[c] + sum_B v T14[c] + sum_C v T12[c]     IC = K_0 .. K_nPublic, C = the rest
// and H_i = T12'[2i + 1] (level k + 1 of section 12), a strided gather.
//
// Layout.  The constraints section is uploaded as it is in the file and decoded on the device through
// r1cs_section.hpp (walk_constraints: one host pass over the term counts; term_at: a lane's term), as the witness check
// of r1cs.hip does, into one term list: the A terms, then the nPublic + 1 public-input rows, then the B terms, then the C terms, each (wire, constraint, coefficient in standard form).  Every
// output table is a contiguous range of that list; its base table is chosen per term by two split points.
//
// One table.  (1) k_setup_count: terms per wire and per signed bit length.  (2) The host turns the wire counts into row
// offsets (one pass over the wires, as many as the key has points) and plans the segmented sum.  (3) k_setup_scatter:
// a counting sort by bit length (the order the per-term lanes run in) that also hands every term its slot in the
// wire-grouped order (a counting sort by wire).  (4) k_setup_term: one lane per term, v T[c] by devmem.hpp's double-and-add over
// the bit length of the SIGNED coefficient (v > (r-1)/2 is taken as -(r - v): circom writes -1 as r - 1), so a wave of
// +-1 and +-2^i terms does one or a few steps and never waits for a 254-bit term.  (5) k_setup_pass: the
// cut-into-segments sum (r1cs_section.hpp's plan_segments, as r1cs.hip) over the wire groups (at most 16 inputs per lane, pass after pass, no atomics on
// points), so the constant wire's column of ~m terms is m / 16 lanes, then m / 256, ...  (6) The batched affine
// normalisation of synth.hip.  Integer atomics place terms; point sums do not depend on the order they come in.
//
// Fields: curve.hpp's 8 x 32-bit Montgomery forms (R = 2^256), the .ptau's and the .zkey's own byte form, so points go
// in and come out without a conversion and the result is the fixed-base kernels' (synth.hip) form bit for bit.
#include "r1cs_section.hpp"
#include "devmem.hpp"

namespace {

constexpr uint32_t MAX_LOG_DOMAIN = 27;              // the prover's limit (prover_create.hip)
constexpr uint32_t BL_BINS = 256;                    // signed bit lengths 0 .. 254

// (r - 1) / 2 for BN254's r, little-endian words
__device__ constexpr uint32_t HALF_R[8] = {0xf8000000u, 0xa1f0fac9u, 0x3cdcb848u, 0x9419f424u, 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u};

// v (standard form, < r) -> |v| in w as a signed residue (v > (r-1)/2: r - v, neg) and its bit length
__device__ __forceinline__ int signed_mag(uint32_t w[8], bool &neg) {
    neg = false;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        if (w[i] != HALF_R[i]) {
            neg = w[i] > HALF_R[i];
            break;
        }
    }
    if (neg) {
        uint32_t bw = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint64_t d = (uint64_t)FrParams::P[i] - w[i] - bw;
            w[i] = (uint32_t)d;
            bw = (uint32_t)(d >> 63);
        }
    }
    int bl = 0;
#pragma unroll
    for (int i = 7; i >= 0; i--)
        if (bl == 0 && w[i]) bl = 32 * i + 32 - __clz(w[i]);
    return bl;
}

// The term list: A terms [0, nnzA), public-input rows [nnzA, nnzA + nP1), B terms, C terms.  rows = 3m rows of the
// file (A, B, C); one lane per term of the section (term_at: r1cs_section.hpp) and per public-input row.
__global__ __launch_bounds__(256) void k_setup_decode(uint32_t *wire, uint32_t *cons, Fr *coef, uint32_t *err, const uint32_t *sec,
                                                      const uint64_t *lc_off, const uint64_t *rowptr, uint32_t rows, uint32_t m, uint32_t nWires,
                                                      uint64_t nnz, uint64_t nnzA, uint32_t nP1) {
    const uint64_t st = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nnz + nP1; t += st) {
        Fr w;
        uint64_t g;
        uint32_t wi, ci;
        if (t < nnz) {
            uint32_t row;
            const uint32_t *p = term_at(t, sec, lc_off, rowptr, rows, row);
            wi = p[0];
            ci = row % m;
#pragma unroll
            for (int j = 0; j < 8; j++) w.v[j] = p[1 + j];
            if (wi >= nWires) atomicMin(&err[0], ci);
            if (ge_r(w.v)) atomicMin(&err[1], ci);
            if (wi >= nWires) wi = 0;
            g = t < nnzA ? t : t + nP1;
        } else {                                    // public-input row i: A, constraint m + i, wire i, value 1
            const uint32_t i = (uint32_t)(t - nnz);
            wi = i;
            ci = m + i;
            w.v[0] = 1;
#pragma unroll
            for (int j = 1; j < 8; j++) w.v[j] = 0;
            g = nnzA + i;
        }
        wire[g] = wi;
        cons[g] = ci;
        store_el(coef + g, w);
    }
}

// Section 4: one 44-byte record (matrix, constraint, wire, value * R^2 mod r) per A / B term, words after the count
__global__ __launch_bounds__(256) void k_setup_coefs(uint32_t *rec, const uint32_t *wire, const uint32_t *cons, const Fr *coef, uint64_t nA,
                                                     uint64_t nRec, Fr r3) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g == 0) rec[0] = (uint32_t)nRec;
    if (g >= nRec) return;
    const Fr v = Fr::mul(load_el(coef + g), r3);                             // v R^3 / R
    uint32_t *o = rec + 1 + 11 * g;
    o[0] = g < nA ? 0u : 1u;
    o[1] = cons[g];
    o[2] = wire[g];
#pragma unroll
    for (int j = 0; j < 8; j++) o[3 + j] = v.v[j];
}

// terms per wire and per signed bit length of the table's range [t0, t1)
__global__ __launch_bounds__(256) void k_setup_count(uint32_t *cntW, uint32_t *cntB, const uint32_t *wire, const Fr *coef, uint64_t t0, uint64_t t1) {
    __shared__ uint32_t h[BL_BINS];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t g = t0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < t1) {
        Fr w = load_el(coef + g);
        bool neg;
        atomicAdd(&h[signed_mag(w.v, neg)], 1u);
        atomicAdd(&cntW[wire[g]], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&cntB[threadIdx.x], h[threadIdx.x]);
}

// Counting sorts: order[j] = the term lane j computes (ascending bit length), slot[j] = its place among the terms
// grouped by wire.  curB / curW start at the exclusive offsets of the counts.
__global__ __launch_bounds__(256) void k_setup_scatter(uint32_t *order, uint64_t *slot, uint32_t *curB, unsigned long long *curW, const uint32_t *wire,
                                                       const Fr *coef, uint64_t t0, uint64_t t1) {
    __shared__ uint32_t h[BL_BINS], base[BL_BINS];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t g = t0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bl = 0, rank = 0;
    if (g < t1) {
        Fr w = load_el(coef + g);
        bool neg;
        bl = (uint32_t)signed_mag(w.v, neg);
        rank = atomicAdd(&h[bl], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) base[threadIdx.x] = atomicAdd(&curB[threadIdx.x], h[threadIdx.x]);
    __syncthreads();
    if (g < t1) {
        const uint32_t j = base[bl] + rank;
        order[j] = (uint32_t)g;
        slot[j] = atomicAdd(&curW[wire[g]], 1ull);
    }
}

// base table of term g: t[0] below split[0], t[1] below split[1], t[2] after
template <class F>
struct Bases {
    const Affine<F> *t[3];
    uint64_t split[2];
};

// One lane per term: v T[c] by devmem.hpp's double-and-add over the bit length of the signed coefficient (-|v| P is
// |v| (-P): the base's y is negated, so -1 costs what 1 costs).
template <class F>
__global__ __launch_bounds__(64) void k_setup_term(XYZZ<F> *tmp, const uint32_t *order, const uint64_t *slot, uint64_t cnt, const uint32_t *cons,
                                                   const Fr *coef, Bases<F> b) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt) return;
    const uint32_t g = order[j];
    Fr k = load_el(coef + g);
    bool neg;
    signed_mag(k.v, neg);
    const Affine<F> *tab = g < b.split[0] ? b.t[0] : (g < b.split[1] ? b.t[1] : b.t[2]);
    Affine<F> P = load_pt(tab + cons[g]);
    if (neg) P.y = F::neg(P.y);
    store_pt(tmp + slot[j], scalar_mul_affine(P, k));
}

// One lane per segment [lo[j], lo[j+1]) of this pass's input (pass 0: the terms grouped by wire; later passes: the
// previous pass's partials); dest & SEG_FINAL: the wire's sum, else a partial for the next pass.
template <class F>
__global__ __launch_bounds__(64) void k_setup_pass(XYZZ<F> *sums, XYZZ<F> *next, const uint64_t *lo, const uint64_t *dest, uint64_t nseg,
                                                   const XYZZ<F> *in) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nseg) return;
    const uint64_t a = lo[j], e = lo[j + 1];
    XYZZ<F> acc = XYZZ<F>::inf();
    for (uint64_t t = a; t < e; t++) add(acc, load_pt(in + t));
    const uint64_t d = dest[j];
    store_pt((d & SEG_FINAL) ? sums + (d & ~SEG_FINAL) : next + d, acc);
}

// H_i = T12'[2i + 1]
__global__ __launch_bounds__(256) void k_setup_h(uint4 *out, const uint4 *lvl, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int q = 0; q < 4; q++) out[4 * i + q] = lvl[4 * (2 * i + 1) + q];
}

struct Sizes {                                      // what zk_groth16_setup_sizes decides, and the walk of the file
    uint32_t k = 0, m = 0, nWires = 0, nPublic = 0;
    uint64_t nnzA = 0, nnzB = 0, nnz = 0;
    std::vector<uint64_t> lc_off, rowptr;
    uint64_t n() const { return 1ull << k; }
    uint64_t nP1() const { return (uint64_t)nPublic + 1; }
    uint64_t nCoefs() const { return nnzA + nP1() + nnzB; }
};

void check_views(const zk_r1cs_view *r, const zk_ptau_view *p, Sizes &z) {
    if (!r || !p) throw std::invalid_argument("null argument");
    z.m = r->nConstraints;
    z.nWires = r->nWires;
    const uint64_t npub = (uint64_t)r->nPubOut + r->nPubIn;
    if (npub + 1 > r->nWires)
        throw std::invalid_argument("r1cs has " + std::to_string(r->nWires) + " wires: fewer than the constant wire and " + std::to_string(npub) +
                                    " public signals");
    z.nPublic = (uint32_t)npub;
    if (!p->lagrange_g1 || !p->lagrange_g2 || !p->lagrange_alpha_g1 || !p->lagrange_beta_g1)
        throw std::invalid_argument("the ptau file is not prepared for phase 2 (no Lagrange sections 12 to 15; "
                                    "`snarkjs powersoftau prepare phase2` writes them)");
    if (!p->alpha1 || !p->beta1 || !p->beta2) throw std::invalid_argument("null ptau point");
    const uint64_t need = (uint64_t)r->nConstraints + npub + 1;
    uint32_t k = 1;
    while ((1ull << k) < need) k++;
    z.k = k;
    if (k > MAX_LOG_DOMAIN)
        throw std::invalid_argument("the circuit needs a domain of 2^" + std::to_string(k) + " (" + std::to_string(r->nConstraints) + " constraints + " +
                                    std::to_string(npub) + " + 1 public-input rows): more than 2^27, the prover's limit");
    if (k > p->power)
        throw std::invalid_argument("the circuit needs 2^" + std::to_string(k) + " and the ptau file holds 2^" + std::to_string(p->power) +
                                    ": it needs a ptau of power " + std::to_string(k) + " or more");
    if (p->power > 32) throw std::invalid_argument("ptau power " + std::to_string(p->power) + " is not supported");
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
    if (r->nConstraints && !r->constraints) throw std::invalid_argument("null constraints section");
    walk_constraints(r, z.lc_off, z.rowptr);
    z.nnz = z.rowptr.back();
    z.nnzA = z.rowptr[z.m];
    z.nnzB = z.rowptr[2ull * z.m] - z.nnzA;
    if (z.nnz + z.nP1() >= (1ull << 32)) throw std::invalid_argument("r1cs has 2^32 terms or more: not supported");
}

// One output table: the points of every wire for the terms [t0, t1), affine in `out` (nWires points)
template <class F>
void run_table(Affine<F> *out, const Sizes &z, uint64_t t0, uint64_t t1, const Bases<F> &b, const DevBuf<uint32_t> &wire,
               const DevBuf<uint32_t> &cons, const DevBuf<Fr> &coef, hipStream_t s) {
    const uint64_t cnt = t1 - t0, nw = z.nWires;
    DevBuf<uint32_t> cntW, cntB, order;
    DevBuf<unsigned long long> curW;
    DevBuf<uint64_t> slot;
    cntW.alloc(nw);
    cntB.alloc(BL_BINS);
    HIP_TRY(hipMemsetAsync(cntW.p, 0, nw * 4, s));
    HIP_TRY(hipMemsetAsync(cntB.p, 0, BL_BINS * 4, s));
    if (cnt) ZK_LAUNCH(k_setup_count, dim3(nblocks(cnt, 256)), dim3(256), 0, s, cntW.p, cntB.p, wire.p, coef.p, t0, t1);
    ZK_LAUNCH_OK("setup count");
    std::vector<uint32_t> hw(nw), hb(BL_BINS);
    HIP_TRY(hipMemcpyAsync(hw.data(), cntW.p, nw * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(hb.data(), cntB.p, BL_BINS * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<uint64_t> rowptr(nw + 1, 0);              // the terms of wire w: [rowptr[w], rowptr[w + 1]) in slot order
    for (uint64_t w = 0; w < nw; w++) rowptr[w + 1] = rowptr[w] + hw[w];
    std::vector<uint32_t> boff(BL_BINS, 0);
    for (uint32_t i = 1; i < BL_BINS; i++) boff[i] = boff[i - 1] + hb[i - 1];
    cntW.release();
    curW.alloc(nw);
    HIP_TRY(hipMemcpyAsync(curW.p, rowptr.data(), nw * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(cntB.p, boff.data(), BL_BINS * 4, hipMemcpyHostToDevice, s));
    DevBuf<XYZZ<F>> tmp, sums, part[2];
    if (cnt) {
        order.alloc(cnt);
        slot.alloc(cnt);
        tmp.alloc(cnt);
        ZK_LAUNCH(k_setup_scatter, dim3(nblocks(cnt, 256)), dim3(256), 0, s, order.p, slot.p, cntB.p, curW.p, wire.p, coef.p, t0, t1);
        ZK_LAUNCH(k_setup_term<F>, dim3(nblocks(cnt, 64)), dim3(64), 0, s, tmp.p, order.p, slot.p, cnt, cons.p, coef.p, b);
        ZK_LAUNCH_OK("setup terms");
    }
    std::vector<std::unique_ptr<SegPass>> passes;
    uint64_t max_part[2];
    HIP_TRY(hipStreamSynchronize(s));                     // plan_segments uploads with blocking copies
    plan_segments(rowptr, passes, max_part);
    order.release();
    slot.release();
    curW.release();
    sums.alloc(nw);
    for (int q = 0; q < 2; q++) part[q].alloc(max_part[q] ? max_part[q] : 1);
    for (size_t l = 0; l < passes.size(); l++) {
        const SegPass &p = *passes[l];
        const XYZZ<F> *in = l ? part[(l - 1) & 1].p : tmp.p;
        ZK_LAUNCH(k_setup_pass<F>, dim3(nblocks(p.nseg, 64)), dim3(64), 0, s, sums.p, part[l & 1].p, p.lo.p, p.dest.p, p.nseg, in);
    }
    ZK_LAUNCH_OK("setup segmented sum");
    DevBuf<F> pref;
    pref.alloc(nw);
    normalize(out, sums.p, pref.p, nw, s);
    HIP_TRY(hipStreamSynchronize(s));
}

// HBM the setup holds at its peak (bounded from above: G2 sizes for every table)
uint64_t hbm_need(const Sizes &z, const zk_r1cs_view *r) {
    const uint64_t n = z.n(), N = z.nnz + z.nP1(), nw = z.nWires;
    const uint64_t table_terms = N;                                       // the K table holds every term
    return r->constraints_bytes + 8 * (z.lc_off.size() + z.rowptr.size())  // decode inputs
           + N * (4 + 4 + 32) + 4 + 44 * z.nCoefs()                          // the term list, section 4
           + n * (64 + 64 + 64 + 128)                                        // level k of sections 12 .. 15
           + table_terms * (4 + 8 + 256 + 16 * 2)                            // order, slot, per-term points, partials
           + nw * (4 + 8 + 256 + 64 + 128);                                  // counts, cursors, sums, prefix, affine
}

void groth16_setup(const zk_r1cs_view *r, const zk_ptau_view *p, int32_t device, zk_setup_out *out) {
    if (!out) throw std::invalid_argument("null argument");
    Sizes z;
    check_views(r, p, z);                                 // both files are checked before the device is touched
    const uint64_t n = z.n(), nw = z.nWires, nP1 = z.nP1(), nC = nw - nP1, nRec = z.nCoefs();
    if (!out->coefs || !out->pointsIC || !out->pointsA || !out->pointsB1 || !out->pointsB2 || !out->pointsH || (nC && !out->pointsC))
        throw std::invalid_argument("null output buffer");
    DeviceGuard g(resolve_device(device));
    need_hbm("zk_groth16_setup", hbm_need(z, r));
    Stream st;
    const hipStream_t s = st.s;

    // ---- the term list
    const uint64_t N = z.nnz + nP1;
    DevBuf<uint32_t> wire, cons;
    DevBuf<Fr> coef;
    wire.alloc(N);
    cons.alloc(N);
    coef.alloc(N);
    {
        SectionOnDevice sec;
        sec.upload(r, z.lc_off, z.rowptr, s);
        const uint64_t gsz = N < 256ull * 4096 ? (N + 255) / 256 : 4096;
        ZK_LAUNCH(k_setup_decode, dim3((uint32_t)gsz), dim3(256), 0, s, wire.p, cons.p, coef.p, sec.err.p, sec.sec(), sec.d_off.p, sec.d_ptr.p, sec.rows(),
                  z.m, z.nWires, z.nnz, z.nnzA, (uint32_t)nP1);
        ZK_LAUNCH_OK("setup decode");
        sec.check(s);
    }

    // ---- section 4
    {
        DevBuf<uint32_t> rec;
        rec.alloc(1 + 11 * nRec);
        Fr r3 = Fr::r2();                                 // R^3 mod r = R^2 * R^2 / R
        r3 = Fr::mul(r3, Fr::r2());
        ZK_LAUNCH(k_setup_coefs, dim3(nblocks(nRec + 1, 256)), dim3(256), 0, s, rec.p, wire.p, cons.p, coef.p, z.nnzA + nP1, nRec, r3);
        ZK_LAUNCH_OK("setup coefficients");
        HIP_TRY(hipMemcpyAsync(out->coefs, rec.p, 4 + 44 * nRec, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }

    // ---- G1 tables: A, B1, K = IC | C
    const uint64_t endA = z.nnzA + nP1, endB = endA + z.nnzB;
    {
        DevBuf<uint8_t> t12, t14, t15;
        DevBuf<G1Affine> aff;
        upload_level(t12, p->lagrange_g1, z.k, 64, s);
        upload_level(t14, p->lagrange_alpha_g1, z.k, 64, s);
        upload_level(t15, p->lagrange_beta_g1, z.k, 64, s);
        const G1Affine *T12 = (const G1Affine *)t12.p, *T14 = (const G1Affine *)t14.p, *T15 = (const G1Affine *)t15.p;
        aff.alloc(nw);
        run_table<Fq>(aff.p, z, 0, endA, Bases<Fq>{{T12, T12, T12}, {endA, endA}}, wire, cons, coef, s);
        HIP_TRY(hipMemcpy(out->pointsA, aff.p, nw * 64, hipMemcpyDeviceToHost));
        run_table<Fq>(aff.p, z, endA, endB, Bases<Fq>{{T12, T12, T12}, {endB, endB}}, wire, cons, coef, s);
        HIP_TRY(hipMemcpy(out->pointsB1, aff.p, nw * 64, hipMemcpyDeviceToHost));
        run_table<Fq>(aff.p, z, 0, N, Bases<Fq>{{T15, T14, T12}, {endA, endB}}, wire, cons, coef, s);
        HIP_TRY(hipMemcpy(out->pointsIC, aff.p, nP1 * 64, hipMemcpyDeviceToHost));
        if (nC) HIP_TRY(hipMemcpy(out->pointsC, aff.p + nP1, nC * 64, hipMemcpyDeviceToHost));
    }
    // ---- G2 table B2
    {
        DevBuf<uint8_t> t13;
        DevBuf<G2Affine> aff;
        upload_level(t13, p->lagrange_g2, z.k, 128, s);
        const G2Affine *T13 = (const G2Affine *)t13.p;
        aff.alloc(nw);
        run_table<Fq2>(aff.p, z, endA, endB, Bases<Fq2>{{T13, T13, T13}, {endB, endB}}, wire, cons, coef, s);
        HIP_TRY(hipMemcpy(out->pointsB2, aff.p, nw * 128, hipMemcpyDeviceToHost));
    }
    wire.release();
    cons.release();
    coef.release();
    // ---- H: the odd points of level k + 1 of section 12
    {
        DevBuf<uint8_t> lvl, h;
        upload_level(lvl, p->lagrange_g1, z.k + 1, 64, s);
        h.alloc(n * 64);
        ZK_LAUNCH(k_setup_h, dim3(nblocks(n, 256)), dim3(256), 0, s, (uint4 *)h.p, (const uint4 *)lvl.p, n);
        ZK_LAUNCH_OK("setup H");
        HIP_TRY(hipMemcpyAsync(out->pointsH, h.p, n * 64, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
}

}   // namespace

extern "C" {

int zk_groth16_setup_sizes(const zk_r1cs_view *r1cs, const zk_ptau_view *ptau, zk_setup_sizes *sizes) {
    return guarded([&] {
        if (!sizes) throw std::invalid_argument("null argument");
        Sizes z;
        check_views(r1cs, ptau, z);
        sizes->nVars = z.nWires;
        sizes->nPublic = z.nPublic;
        sizes->domainSize = (uint32_t)z.n();
        sizes->log_domain = z.k;
        sizes->nCoefs = z.nCoefs();
    });
}

int zk_groth16_setup(const zk_r1cs_view *r1cs, const zk_ptau_view *ptau, int32_t device, zk_setup_out *out) {
    return guarded([&] { groth16_setup(r1cs, ptau, device, out); });
}

}   // extern "C"
