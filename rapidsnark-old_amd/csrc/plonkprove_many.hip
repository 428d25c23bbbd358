// PLONK prover, many witnesses a call (include/zkhip.h, section "PLONK prover and verifier"): m witnesses of
// one circuit, the proofs of a chunk of B advancing through the five rounds in lock-step, and every round's commitments for
// the whole chunk in ONE multiplication.  A chunk makes four multiplications whatever it holds, against nine a proof.
//
// The multiplication is the one zk_prove_batch_submit has (MsmPlan::batch: vector v gets bucket set v over the same table rows,
// through launch_msm_sort, launch_msm_accum_g1 and launch_msm_reduce_g1, none of which changes here).  It needs tables with a
// row per window, which a zk_kzg has not: the prover makes one over the kzg's first n + 6 points, lazily, for ONE window width,
// so that every k from 1 to 3 B reads the same table.  Its buffers are sized once for 3 B vectors.
//
// A slot is one proof's state across the rounds; plonk_many_plan.hpp states where it lies.  The committed rows are n + 6 long,
// cleared when the slots are made, and every round writes only its own length (section 31's invariant).  What is looped a proof
// at a time are the existing cores (the inverse transforms, the scan, the quotient, the evaluation, the linearisation and the
// divisions), each with the drain it has; zk_plonk_prover_many_info counts them.
//
// New kernels, all memory-bound and in STANDARD form (a move or one subtraction an element, no product, no LDS, no atomics):
// k_wire_gather_many, k_plonk_blind_many and k_plonk_split_many are the lane maps of plonkprove.hip's k_wire_gather,
// k_plonk_blind and k_plonk_split with a proof dimension in the grid.  A proof's base is a stride from one pointer; the maps
// are shared by all proofs; the witness row an index names is the only access that is not a neighbour's.  No byte depends on seg.
#include <sys/random.h>

#include "plonk_prover_internal.hpp"
#include "tail_pool.hpp"

namespace {

constexpr uint32_t PV_WG = 256, BLINDS = ZK_PLONK_BLINDS, POINTS = PLONK_POINTS;
static_assert(PM_BLINDS == ZK_PLONK_BLINDS && PM_MAX_WIDTH == ZK_PLONK_MANY_MAX_BATCH, "plonk_many_plan.hpp and zkhip.h");
static_assert(PM_MADE == ZK_PLONK_MANY_MADE && PM_ZERO_DENOMINATOR == ZK_PLONK_MANY_ZERO_DENOMINATOR && PM_COPIES == ZK_PLONK_MANY_COPIES &&
                  PM_GATES == ZK_PLONK_MANY_GATES && PM_NOT_BELOW_R == ZK_PLONK_MANY_NOT_BELOW_R,
              "plonk_many_plan.hpp and zkhip.h");

// ---------------------------------------------------------------- device
// proof q: out[q][v][i] = wit[q][map[v][i]] for v < 3; out[q][3][i] = -pub[q][i] for i < n_public, else 0
struct GatherManyArgs {
    const uint32_t *map;                              // 3 x n, every index below the witness's length
    const Fr *wit, *pub;                              // wit_stride and pub_stride rows a proof
    Fr *out;                                          // 4 x n a proof
    uint64_t n, n_public, wit_stride, pub_stride;
    uint32_t seg;
};
__global__ __launch_bounds__(PV_WG) void k_wire_gather_many(GatherManyArgs A) {
    const uint64_t T = (uint64_t)gridDim.x * PV_WG, l = (uint64_t)blockIdx.x * PV_WG + threadIdx.x;
    const uint32_t v = blockIdx.y, q = blockIdx.z;
    const uint32_t *map = A.map + v * A.n;
    const Fr *wit = A.wit + q * A.wit_stride, *pub = A.pub + q * A.pub_stride;
    Fr *out = A.out + ((uint64_t)q * 4 + v) * A.n;
#pragma unroll 1
    for (uint32_t k = 0; k < A.seg; k++) {
        const uint64_t i = l + k * T;
        if (i >= A.n) break;
        if (v < 3) store_el(out + i, load_el(wit + map[i]));
        else store_el(out + i, i < A.n_public ? Fr::sub(Fr::zero(), load_el(pub + i)) : Fr::zero());
    }
}

// proof q, row y of its `vecs` rows of len: row += (r_0 + .. + r_(cnt-1) X^(cnt-1)) (X^n - 1), r_j = b[q][first[y] + cnt - 1 - j]
struct BlindManyArgs {
    Fr *rows;                                         // vecs x len a proof
    const Fr *b;                                      // BLINDS a proof
    uint64_t n, len;
    uint32_t vecs, cnt;
    uint32_t first[3];
};
__global__ __launch_bounds__(64) void k_plonk_blind_many(BlindManyArgs A) {
    const uint32_t j = threadIdx.x, y = blockIdx.x, q = blockIdx.y;
    if (j >= A.cnt) return;
    const Fr r = load_el(A.b + (uint64_t)q * BLINDS + A.first[y] + A.cnt - 1 - j);
    Fr *row = A.rows + ((uint64_t)q * A.vecs + y) * A.len;
    store_el(row + j, Fr::sub(load_el(row + j), r));
    store_el(row + A.n + j, r);
}

// proof q: k_plonk_split from t[q] (3n + 6 rows) into its three rows of len, with its b10, b11
struct SplitManyArgs {
    const Fr *t;                                      // 3n + 6 a proof
    Fr *parts;                                        // 3 x len a proof
    const Fr *b;                                      // BLINDS a proof
    uint64_t n;
    uint32_t seg;
};
__global__ __launch_bounds__(PV_WG) void k_plonk_split_many(SplitManyArgs A) {
    const uint64_t T = (uint64_t)gridDim.x * PV_WG, l = (uint64_t)blockIdx.x * PV_WG + threadIdx.x, n = A.n, len = n + 6;
    const uint32_t q = blockIdx.y;
    const Fr *t = A.t + (uint64_t)q * (3 * n + 6), *b = A.b + (uint64_t)q * BLINDS + 9;
    Fr *lo = A.parts + (uint64_t)q * 3 * len, *mid = lo + len, *hip = mid + len;
#pragma unroll 1
    for (uint32_t k = 0; k < A.seg; k++) {
        const uint64_t i = l + k * T;
        if (i >= n + 6) break;
        Fr hi = load_el(t + 2 * n + i);               // 2n + i < 3n + 6
        if (i == 0) hi = Fr::sub(hi, load_el(b + 1));
        store_el(hip + i, hi);
        if (i < n) {
            Fr md = load_el(t + n + i);
            if (i == 0) md = Fr::sub(md, load_el(b));
            store_el(lo + i, load_el(t + i));
            store_el(mid + i, md);
        } else if (i == n) {
            store_el(lo + n, load_el(b));
            store_el(mid + n, load_el(b + 1));
        }
    }
}

uint32_t blocks_of(uint64_t n, uint32_t seg) { return nblocks(n, PV_WG * seg); }

}   // namespace

// ---------------------------------------------------------------- the table, the slots, the multiplication's buffers
struct PlonkMany {
    uint32_t B = 0, K = 0, c = 0, W = 0, rows = 0;      // K = 3 B vectors at most; c window bits, W windows, rows of the table
    uint64_t len = 0;
    PmLayout L;
    DevBuf<G1Affine> table;                           // rows x len: row j holds 2^(c j) P_i
    DevBuf<Fr> slab;                                  // the slots
    SortBufs sb;
    DevBuf<G1Acc> buckets, scratch, ws;
    DevBuf<G1XYZZ> wsum;
    DevBuf<uint32_t> wkey, wflag;
    std::vector<uint8_t> w;                           // the window sums on the host
    size_t msm_bytes() const { return sb.bytes() + buckets.bytes() + scratch.bytes() + ws.bytes() + wsum.bytes() + wkey.bytes() + wflag.bytes(); }
    size_t bytes() const { return table.bytes() + slab.bytes() + msm_bytes(); }
    Fr *at(uint64_t rows_from_first) { return slab.p + rows_from_first; }
};
void plonk_many_free(PlonkMany *m) { delete m; }
size_t plonk_many_bytes(const PlonkMany *m) { return m ? m->bytes() : 0; }

namespace {

// what k = 1 .. K vectors of len scalars need at most, every k over ONE window width: the plan's for a batch of K
struct ManySizes {
    uint32_t c, W, rows;
    MsmSortSizes z;
    uint64_t buckets, scratch, slots, wsum;
    uint64_t bytes(uint64_t len) const {
        const uint64_t sort = 2 * z.lo_u16 + 4 * (z.counts_u32 + z.starts_u32 + z.offsets_u32 + z.entries_u32 + z.codes_u32 + z.val_u32 + z.bin_counts_u32 + z.bin_starts_u32);
        return sort + (buckets + scratch + slots) * sizeof(G1Acc) + slots * 8 + wsum * sizeof(G1XYZZ) + (uint64_t)rows * len * sizeof(G1Affine);
    }
    uint64_t transient(uint64_t len) const { return (uint64_t)(rows - 1) * len * (sizeof(G1XYZZ) + sizeof(Fq)); }      // the doubling walks' scratch
};
uint32_t many_window_bits(uint64_t len, uint32_t K) { return make_msm_plan(len, 0, 1, K > 1 ? K : 2).c; }
ManySizes many_sizes(uint64_t len, uint32_t K, uint32_t c) {
    ManySizes m{};
    m.c = c;
    auto up = [](uint64_t &a, uint64_t b) { a = b > a ? b : a; };
    for (uint32_t k = 1; k <= K; k++) {
        const MsmPlan p = make_msm_plan(len, c, 1, k);
        const MsmSortSizes z = msm_sort_sizes((uint64_t)k * len, p);
        up(m.z.counts_u32, z.counts_u32), up(m.z.starts_u32, z.starts_u32), up(m.z.offsets_u32, z.offsets_u32), up(m.z.entries_u32, z.entries_u32);
        up(m.z.codes_u32, z.codes_u32), up(m.z.lo_u16, z.lo_u16), up(m.z.val_u32, z.val_u32), up(m.z.bin_counts_u32, z.bin_counts_u32);
        up(m.z.bin_starts_u32, z.bin_starts_u32);
        up(m.scratch, msm_reduce_scratch_points(1, p));
        up(m.wsum, (uint64_t)k * msm_wsum_rc(p));
        up(m.buckets, (uint64_t)p.sets * p.nbuckets);
        m.W = p.W, m.rows = msm_table_rows(p);
    }
    m.slots = msm_accum_workspace_slots((uint64_t)K * len * m.W);
    return m;
}

// The object's table, slots and buffers for a chunk width of B, made once and kept (remade only when the width changes).
// Every limit is checked before anything is allocated
PlonkMany *many_of(zk_plonk_prover *p, const char *who, uint32_t B) {
    if (p->many && p->many->B == B) return p->many;
    const uint64_t len = p->n + 6;
    const uint32_t K = PM_MAX_VECS * B, c = many_window_bits(len, K);
    pm_check_limits(who, B, len, make_msm_plan(len, c, 1, 1).W);
    const ManySizes z = many_sizes(len, K, c);
    const PmLayout L = pm_layout(B, p->n, p->n_witness, p->n_public);
    if (p->many) plonk_many_free(p->many), p->many = nullptr;          // another width: its buffers go first
    size_t fr = 0, tot = 0;
    HIP_TRY(hipMemGetInfo(&fr, &tot));
    auto need_of = [&](uint32_t b, const ManySizes &zs) { return zs.bytes(len) + zs.transient(len) + pm_layout(b, p->n, p->n_witness, p->n_public).bytes() + 65536; };
    const uint64_t need = need_of(B, z);
    if (!pm_hbm_fits(need, fr)) {
        uint32_t fit = B - 1;
        for (; fit > 1; fit--) {
            const uint32_t kf = PM_MAX_VECS * fit;
            if (pm_hbm_fits(need_of(fit, many_sizes(len, kf, many_window_bits(len, kf))), fr)) break;
        }
        throw HipError(pm_hbm_message(who, B, need, fr, fit));
    }
    std::unique_ptr<PlonkMany> M(new PlonkMany());
    M->B = B, M->K = K, M->c = c, M->W = z.W, M->rows = z.rows, M->len = len, M->L = L;
    hipStream_t s = p->st->s;
    M->table.alloc((uint64_t)z.rows * len);
    M->slab.alloc(L.rows);
    M->sb.lo.alloc(z.z.lo_u16), M->sb.counts.alloc(z.z.counts_u32), M->sb.starts.alloc(z.z.starts_u32), M->sb.offsets.alloc(z.z.offsets_u32);
    M->sb.entries.alloc(z.z.entries_u32), M->sb.codes.alloc(z.z.codes_u32), M->sb.val.alloc(z.z.val_u32), M->sb.bin_counts.alloc(z.z.bin_counts_u32);
    M->sb.bin_starts.alloc(z.z.bin_starts_u32);
    M->buckets.alloc(z.buckets), M->scratch.alloc(z.scratch), M->ws.alloc(z.slots), M->wkey.alloc(z.slots), M->wflag.alloc(z.slots);
    M->wsum.alloc(z.wsum);
    M->w.resize(z.wsum * sizeof(G1XYZZ));
    {
        // row 0: the kzg's points, already in the kernels' form; the other rows by the doubling walks (scratch freed on return)
        zk_kzg *k = p->kzg;
        std::lock_guard<std::mutex> kl(k->mu);
        HIP_TRY(hipMemcpyAsync(M->table.p, k->tau.p, len * sizeof(G1Affine), hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (z.rows > 1) {
        DevBuf<G1XYZZ> tmp;
        DevBuf<Fq> pref;
        tmp.alloc((uint64_t)(z.rows - 1) * len);
        pref.alloc((uint64_t)(z.rows - 1) * len);
        launch_msm_precomp_g1(M->table.p, tmp.p, pref.p, len, make_msm_plan(len, c, 1, 1), s);
        HIP_TRY(hipStreamSynchronize(s));
    }
    HIP_TRY(hipMemsetAsync(M->at(L.committed_at()), 0, L.committed_rows() * sizeof(Fr), s));
    HIP_TRY(hipStreamSynchronize(s));
    p->many = M.release();
    return p->many;
}

// out[v] = [vector v] for k <= K vectors of len standard rows back to back on the device: one sort over k len scalars, one
// accumulation, one reduction, ONE drain; the k host combinations on the pool's threads.  A vector of zeros has no entry and
// gives infinity
void many_multiply(PlonkMany *M, uint8_t *out, const Fr *sc, uint32_t k, hipStream_t s) {
    const MsmPlan plan = make_msm_plan(M->len, M->c, 1, k);
    M->sb.plan = plan, M->sb.n = (uint64_t)k * M->len;
    M->sb.run(sc, s);
    launch_msm_accum_g1(M->buckets.p, M->sb.offsets.p, M->sb.entries.p, M->table.p, 0, 0, M->sb.total_buckets(), M->sb.max_entries(), M->ws.p, M->wkey.p,
                        M->wflag.p, s);
    launch_msm_reduce_g1(M->wsum.p, M->scratch.p, M->buckets.p, 1, plan, s);
    const uint32_t rc = msm_wsum_rc(plan);
    const size_t rec = (size_t)rc * sizeof(G1XYZZ);
    HIP_TRY(hipMemcpyAsync(M->w.data(), M->wsum.p, k * rec, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint8_t *w = M->w.data();
    const uint32_t c = plan.c;
    zk::tail_pool().for_each(k, [&](uint32_t v) { HostTail::combine_windows_g1(w + v * rec, 1, c, rc, out + (size_t)v * 64); });
}

struct WipeBytes {                                    // drawn blinds are secrets: gone from the host however the call leaves
    std::vector<uint8_t> &v;
    ~WipeBytes() {
        volatile uint8_t *q = v.data();
        for (size_t i = 0; i < v.size(); i++) q[i] = 0;
    }
};

// What a many-call is given.  r1cs: the witnesses are circom's, n_vars values each, extended on the slot, publics inside them
struct ManyCall {
    const char *who;
    uint64_t m;
    uint8_t *proofs;
    uint32_t *status;
    const uint8_t *witnesses, *publics, *blinds;      // blinds: m x BLINDS scalars, given or drawn
    bool r1cs;
    uint64_t up;                                      // values of a witness that go up
    const uint8_t *witness(uint64_t i) const { return witnesses + i * up * 32; }
    const uint8_t *publics_of(uint64_t i, uint64_t n_public) const { return r1cs ? witness(i) + 32 : (n_public ? publics + i * n_public * 32 : nullptr); }
    const uint8_t *blind(uint64_t i) const { return blinds + i * BLINDS * 32; }
};

struct ManyRun {                                      // what the call counts, and its first refusal
    uint32_t chunks = 0, multiplications = 0, drains = 0, refused = 0;
    uint64_t first_bad = ~0ull;
    std::string text;
    void refuse(const ManyCall &C, uint64_t i, uint32_t status, const std::string &what) {
        C.status[i] = status;
        refused++;
        if (i < first_bad) first_bad = i, text = pm_refusal(C.who, i, what);
    }
};

// One chunk of `count` proofs from proof `first` on, in lock-step.  The caller holds p->mu and the device
void prove_chunk(zk_plonk_prover *p, PlonkMany *M, const ManyCall &C, ManyRun &R, uint64_t first, uint32_t count, uint32_t seg) {
    hipStream_t s = p->st->s;
    const PmLayout &L = M->L;
    const uint64_t n = p->n, len = L.len, n_public = p->n_public;
    const uint32_t log_n = p->log_n, vecs = n_public ? 4u : 3u;
    std::vector<uint8_t> out((size_t)count * ZK_PLONK_PROOF_BYTES);
    std::vector<Challenges> ch(count);
    std::vector<uint8_t> live(count), pts;
    uint32_t alive = 0;
    for (uint32_t q = 0; q < count; q++) alive += live[q] = C.status[first + q] == PM_MADE;
    auto proof_of = [&](uint32_t q) { return out.data() + (size_t)q * ZK_PLONK_PROOF_BYTES; };
    // a round's rows of the chunk: round r, proof q, vector y
    auto row = [&](int r, uint32_t q, uint32_t y) { return M->at(L.round[r]) + ((uint64_t)q * PM_ROUND_VECS[r] + y) * len; };
    // the round's ONE multiplication: the rows of a proof that is refused (or never began) are zeros, its points are not read
    auto multiply = [&](int r, uint32_t point) {
        const uint32_t v = PM_ROUND_VECS[r];
        for (uint32_t q = 0; q < count; q++)
            if (!live[q]) HIP_TRY(hipMemsetAsync(row(r, q, 0), 0, v * len * sizeof(Fr), s));
        pts.resize((size_t)count * v * 64);
        many_multiply(M, pts.data(), row(r, 0, 0), count * v, s);
        R.multiplications++, R.drains++;
        for (uint32_t q = 0; q < count; q++)
            if (live[q]) memcpy(proof_of(q) + point * 64, pts.data() + (size_t)q * v * 64, v * 64);
    };
    auto refuse = [&](uint32_t q, uint32_t status) {
        live[q] = 0, alive--;
        R.refuse(C, first + q, status, pm_status_text(status));
    };

    // round 1: the witnesses up, the wires by values (one launch), their coefficients, the blinding (one launch), [a] [b] [c]
    for (uint32_t q = 0; q < count; q++) {
        if (!live[q]) continue;
        HIP_TRY(hipMemcpyAsync(M->at(L.wit) + q * L.n_witness, C.witness(first + q), C.up * sizeof(Fr), hipMemcpyHostToDevice, s));
        if (n_public) HIP_TRY(hipMemcpyAsync(M->at(L.pub) + q * L.pub_stride, C.publics_of(first + q, n_public), n_public * sizeof(Fr), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(M->at(L.blind) + q * BLINDS, C.blind(first + q), BLINDS * sizeof(Fr), hipMemcpyHostToDevice, s));
        if (C.r1cs) plonk_r1cs_extend_dev(p->r1cs, M->at(L.wit) + q * L.n_witness, s), R.drains++;
    }
    if (alive) {
        GatherManyArgs G{p->maps.p, M->at(L.wit), M->at(L.pub), M->at(L.vals), n, n_public, L.n_witness, L.pub_stride, seg};
        ZK_LAUNCH(k_wire_gather_many, dim3(blocks_of(n, seg), vecs, count), dim3(PV_WG), 0, s, G);
        ZK_LAUNCH_OK("wire gather of a chunk");
        for (uint32_t q = 0; q < count; q++) {
            if (!live[q]) continue;
            Fr *const out1[4] = {row(0, q, 0), row(0, q, 1), row(0, q, 2), M->at(L.pic) + q * n};
            plonk_circuit_interpolate_dev(p->circ, out1, M->at(L.vals) + (uint64_t)q * 4 * n, vecs, s);
        }
        BlindManyArgs Bl{M->at(L.round[0]), M->at(L.blind), n, len, 3, 2, {0, 2, 4}};
        ZK_LAUNCH(k_plonk_blind_many, dim3(3, count), dim3(64), 0, s, Bl);
        ZK_LAUNCH_OK("blinding of a chunk");
    }
    multiply(0, P_A);
    for (uint32_t q = 0; q < count; q++)
        if (live[q]) round1_challenges(ch[q], p->vk, C.publics_of(first + q, n_public), proof_of(q));

    // round 2: z by values a proof at a time (the scan drains once), its coefficients, the blinding (one launch), [z]
    for (uint32_t q = 0; q < count; q++) {
        if (!live[q]) continue;
        uint8_t beta[32], gamma[32], last[32];
        fr_to_std(beta, ch[q].beta);
        fr_to_std(gamma, ch[q].gamma);
        const bool ok = plonk_perm_dev(p->perm, M->at(L.zval) + q * n, last, M->at(L.vals) + (uint64_t)q * 4 * n, p->sig.p, p->shifts.p, log_n, beta, gamma, s);
        R.drains++;
        if (!ok) refuse(q, PM_ZERO_DENOMINATOR);
        else if (!(fr_from_std(last) == Fr::one())) refuse(q, PM_COPIES);
        else {
            Fr *const out2[1] = {row(1, q, 0)};
            plonk_circuit_interpolate_dev(p->circ, out2, M->at(L.zval) + q * n, 1, s);
        }
    }
    if (alive) {
        BlindManyArgs Bz{M->at(L.round[1]), M->at(L.blind), n, len, 1, 3, {6, 0, 0}};
        ZK_LAUNCH(k_plonk_blind_many, dim3(1, count), dim3(64), 0, s, Bz);
        ZK_LAUNCH_OK("blinding of a chunk");
    }
    multiply(1, P_Z);
    for (uint32_t q = 0; q < count; q++)
        if (live[q]) round2_challenge(ch[q], proof_of(q));

    // round 3: a proof at a time the rows to the quotient's input and t (t's length drains); the split (one launch);
    // [t_lo] [t_mid] [t_hi]
    const uint64_t lens[PLONK_ROWS] = {n + 2, n + 2, n + 2, n + 3, n};
    for (uint32_t q = 0; q < count; q++) {
        if (!live[q]) continue;
        Fr *in = plonk_circuit_rows(p->circ);
        const Fr *src[PLONK_ROWS] = {row(0, q, 0), row(0, q, 1), row(0, q, 2), row(1, q, 0), M->at(L.pic) + q * n};
        uint64_t at = 0;
        for (uint32_t j = 0; j < vecs + 1; j++) {
            HIP_TRY(hipMemcpyAsync(in + at, src[j], lens[j] * sizeof(Fr), hipMemcpyDeviceToDevice, s));
            at += lens[j];
        }
        uint64_t t_len = 0;
        const Fr *t = plonk_circuit_quotient_dev(p->circ, lens, vecs + 1, ch[q].alpha, ch[q].beta, ch[q].gamma, &t_len, s);
        R.drains++;
        if (t_len > 3 * n + 6) refuse(q, PM_GATES);
        else HIP_TRY(hipMemcpyAsync(M->at(L.t) + (uint64_t)q * (3 * n + 6), t, (3 * n + 6) * sizeof(Fr), hipMemcpyDeviceToDevice, s));
    }
    if (alive) {
        SplitManyArgs S{M->at(L.t), M->at(L.round[2]), M->at(L.blind), n, seg};
        ZK_LAUNCH(k_plonk_split_many, dim3(blocks_of(n + 6, seg), count), dim3(PV_WG), 0, s, S);
        ZK_LAUNCH_OK("split of a chunk's t");
    }
    multiply(2, P_TLO);
    for (uint32_t q = 0; q < count; q++)
        if (live[q]) round3_challenge(ch[q], proof_of(q));

    // rounds 4 and 5 a proof at a time: its seven rows into the opening object (as round 3 copies its five), the six values, the
    // linearisation and the two divisions straight into the slot's rows; then [W_zeta] [W_zeta_omega] of the chunk
    const uint64_t wlen[4] = {len, len, len, len}, tlen[3] = {n + 1, n + 1, n + 6};
    static const uint8_t zero[32] = {0};
    for (uint32_t q = 0; q < count; q++) {
        if (!live[q]) continue;
        for (uint32_t j = 0; j < 4; j++)
            HIP_TRY(hipMemcpyAsync(plonk_opening_wit(p->open, j), j < 3 ? row(0, q, j) : row(1, q, 0), len * sizeof(Fr), hipMemcpyDeviceToDevice, s));
        for (uint32_t j = 0; j < 3; j++) HIP_TRY(hipMemcpyAsync(plonk_opening_part(p->open, j), row(2, q, j), len * sizeof(Fr), hipMemcpyDeviceToDevice, s));
        uint8_t *evals = proof_of(q) + POINTS * 64;
        plonk_opening_evaluate_dev(p->open, evals, wlen, ch[q].zeta, s);
        R.drains++;
        round4_challenge(ch[q], evals);
        const AtZeta z = at_zeta(log_n, ch[q].zeta, C.publics_of(first + q, n_public), n_public);
        uint8_t r_zeta[32];
        plonk_opening_open_rows_dev(p->open, row(3, q, 0), row(3, q, 1), r_zeta, tlen, z.pi, ch[q].alpha, ch[q].beta, ch[q].gamma, ch[q].v, s);
        R.drains++;
        if (memcmp(r_zeta, zero, 32) != 0) refuse(q, PM_GATES);
    }
    multiply(3, P_WZ);
    for (uint32_t q = 0; q < count; q++)
        if (live[q]) memcpy(C.proofs + (first + q) * ZK_PLONK_PROOF_BYTES, proof_of(q), ZK_PLONK_PROOF_BYTES);
}

void prove_many(zk_plonk_prover *p, ManyCall C, uint32_t n_vars) {
    const char *who = C.who;
    if (!p) throw std::invalid_argument("null argument");
    if (C.r1cs && !p->r1cs) throw std::invalid_argument(std::string(who) + ": the prover was not made from an r1cs (zk_plonk_prover_create_r1cs)");
    if (C.m && (!C.proofs || !C.status || !C.witnesses || (!C.r1cs && p->n_public && !C.publics))) throw std::invalid_argument("null argument");
    // a bad knob is an error of the call before any work
    const uint32_t B = pm_width(p->log_n), seg = plonk_quot_seg();
    (void)plonk_perm_seg(), (void)plonk_open_seg(), (void)kzg_seg_in_effect();
    if (C.r1cs) {
        const PlonkR1csDims d = plonk_r1cs_dims(p->r1cs);
        if (n_vars != d.n_wires) throw std::invalid_argument("witness has " + std::to_string(n_vars) + " values, the r1cs " + std::to_string(d.n_wires) + " wires");
        C.up = n_vars;
    } else {
        C.up = p->n_witness;
    }
    ManyRun R;
    if (!C.m) {
        std::lock_guard<std::mutex> lock(p->mu);
        p->many_last.chunks = p->many_last.multiplications = p->many_last.launches = p->many_last.drains = p->many_last.refused = 0;
        return;
    }
    if (C.m >= (1ull << 31)) throw std::invalid_argument(std::string(who) + ": m is not below 2^31");
    std::vector<uint8_t> drawn;
    WipeBytes wipe{drawn};
    if (!C.blinds) {
        drawn.resize((size_t)C.m * BLINDS * 32);
        for (uint64_t j = 0; j < C.m * BLINDS; j++) draw_scalar(drawn.data() + j * 32, who);
        C.blinds = drawn.data();
    }
    // a value that is not below r refuses its proof alone
    static const char *const names[3] = {"witness", "publics", "blind"};
    for (uint64_t i = 0; i < C.m; i++) {
        C.status[i] = PM_MADE;
        const uint8_t *v[3] = {C.witness(i), C.r1cs ? nullptr : C.publics_of(i, p->n_public), C.blind(i)};
        const uint64_t cnt[3] = {C.up, p->n_public, BLINDS};
        for (int j = 0; j < 3; j++) {
            if (!v[j]) continue;
            const uint64_t bad = first_not_below_r(v[j], cnt[j]);
            if (bad < cnt[j]) {
                R.refuse(C, i, PM_NOT_BELOW_R, std::string(names[j]) + " " + std::to_string(bad) + " is not below r");
                break;
            }
        }
    }
    std::lock_guard<std::mutex> lock(p->mu);
    DeviceGuard dg(p->device);
    hipStream_t s = p->st->s;
    const uint64_t at = launches_now();
    R.chunks = (uint32_t)pm_chunks(C.m, B);
    if (B == 1) {
        // the loop: plonkprove.hip's core a proof, nine multiplications each over the kzg's own buffers; no table, no slots
        for (uint64_t i = 0; i < C.m; i++) {
            if (C.status[i] != PM_MADE) continue;
            HIP_TRY(hipMemcpyAsync(p->wit.p, C.witness(i), C.up * sizeof(Fr), hipMemcpyHostToDevice, s));
            if (p->n_public) HIP_TRY(hipMemcpyAsync(p->pub.p, C.publics_of(i, p->n_public), p->n_public * sizeof(Fr), hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(p->blind.p, C.blind(i), BLINDS * sizeof(Fr), hipMemcpyHostToDevice, s));
            if (C.r1cs) plonk_r1cs_extend_dev(p->r1cs, p->wit.p, s), R.drains++;
            try {
                plonk_prover_core(p, who, C.proofs + i * ZK_PLONK_PROOF_BYTES, C.publics_of(i, p->n_public), seg, launches_now());
                R.multiplications += 9, R.drains += 9 + 3 + 1;      // the nine, then the scan, t's length and the six values, and the core's last
            } catch (const PlonkRefusal &e) {
                R.refuse(C, i, e.status, pm_status_text(e.status));
                HIP_TRY(hipMemsetAsync(p->blind.p, 0, p->blind.bytes(), s));
                HIP_TRY(hipStreamSynchronize(s));
            }
        }
    } else {
        PlonkMany *M = many_of(p, who, B);
        struct WipeDev {                              // and from the device, as a lone proof wipes its own
            PlonkMany *M;
            hipStream_t s;
            ~WipeDev() {
                (void)hipMemsetAsync(M->at(M->L.blind), 0, (size_t)M->L.B * BLINDS * sizeof(Fr), s);
                (void)hipStreamSynchronize(s);
            }
        } wipe_dev{M, s};
        for (uint64_t g = 0; g < R.chunks; g++) prove_chunk(p, M, C, R, pm_chunk_first(g, B), pm_chunk_count(C.m, g, B), seg);
    }
    p->many_last.chunks = R.chunks, p->many_last.multiplications = R.multiplications, p->many_last.drains = R.drains, p->many_last.refused = R.refused;
    p->many_last.launches = (uint32_t)(launches_now() - at);
    if (R.refused) set_error(R.text);                  // the call succeeds: the text is for whoever asks why a status is not 0
}

// k polynomials of n + 6 coefficients -> k commitments over the table, 3 B vectors a multiplication
void commit_many(zk_plonk_prover *p, uint8_t *out, const uint8_t *coeffs, uint64_t k) {
    const char *who = "zk_plonk_prover_commit_many";
    if (!p || !out || !coeffs) throw std::invalid_argument("null argument");
    if (!k) throw std::invalid_argument(std::string(who) + ": k is 0");
    const uint32_t B = pm_width(p->log_n);
    const uint64_t len = p->n + 6;
    for (uint64_t v = 0; v < k; v++) {
        const uint64_t bad = first_not_below_r(coeffs + v * len * 32, len);
        if (bad < len) throw std::invalid_argument(std::string(who) + ": vector " + std::to_string(v) + " coefficient " + std::to_string(bad) + " is not below r");
    }
    std::lock_guard<std::mutex> lock(p->mu);
    DeviceGuard dg(p->device);
    hipStream_t s = p->st->s;
    const uint64_t at = launches_now();
    PlonkMany *M = many_of(p, who, B);
    ManyRun R;
    Fr *rows = M->at(M->L.round[0]);                  // the chunk's a b c rows: 3 B vectors of len, zero between calls
    for (uint64_t v = 0; v < k; v += M->K) {
        const uint32_t cnt = (uint32_t)(k - v < M->K ? k - v : M->K);
        HIP_TRY(hipMemcpyAsync(rows, coeffs + v * len * 32, cnt * len * sizeof(Fr), hipMemcpyHostToDevice, s));
        many_multiply(M, out + v * 64, rows, cnt, s);
        R.chunks++, R.multiplications++, R.drains++;
        HIP_TRY(hipMemsetAsync(rows, 0, cnt * len * sizeof(Fr), s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    p->many_last.chunks = R.chunks, p->many_last.multiplications = R.multiplications, p->many_last.drains = R.drains + 1, p->many_last.refused = 0;
    p->many_last.launches = (uint32_t)(launches_now() - at);
}

}   // namespace

extern "C" {

int zk_plonk_prove_many(zk_plonk_prover *p, uint64_t m, uint8_t *proofs, uint32_t *status, const uint8_t *witnesses, const uint8_t *publics,
                        const uint8_t *blinds) {
    return guarded([&] { prove_many(p, ManyCall{"zk_plonk_prove_many", m, proofs, status, witnesses, publics, blinds, false, 0}, 0); });
}

int zk_plonk_prove_r1cs_many(zk_plonk_prover *p, uint64_t m, uint8_t *proofs, uint32_t *status, const uint8_t *wtns, uint32_t nVars, const uint8_t *blinds) {
    return guarded([&] { prove_many(p, ManyCall{"zk_plonk_prove_r1cs_many", m, proofs, status, wtns, nullptr, blinds, true, 0}, nVars); });
}

int zk_plonk_prover_commit_many(zk_plonk_prover *p, uint8_t *out, const uint8_t *coeffs, uint64_t k) {
    return guarded([&] { commit_many(p, out, coeffs, k); });
}

int zk_plonk_prover_many_info(zk_plonk_prover *p, zk_plonk_prover_many_plan *plan) {
    return guarded([&] {
        if (!p || !plan) throw std::invalid_argument("null argument");
        info_into("zk_plonk_prover_many_info", plan, [&](zk_plonk_prover_many_plan &q) {
            q.batch = pm_width(p->log_n);
            std::lock_guard<std::mutex> lock(p->mu);
            if (const PlonkMany *M = p->many) {
                q.table_batch = M->B, q.window_bits = M->c, q.table_rows = M->rows;
                q.table_bytes = M->table.bytes(), q.slot_bytes = M->slab.bytes(), q.msm_bytes = M->msm_bytes();
            }
            q.last_chunks = p->many_last.chunks, q.last_multiplications = p->many_last.multiplications, q.last_launches = p->many_last.launches;
            q.last_drains = p->many_last.drains, q.last_refused = p->many_last.refused;
        });
    });
}

}   // extern "C"
