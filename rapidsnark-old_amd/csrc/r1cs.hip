// R1CS witness check on the device (include/zkhip.h, section "R1CS"): A.w, B.w, C.w of a circom .r1cs and the
// pointwise test a.b = c per constraint, plus the test that a .zkey was made from the same circuit.  Nothing in the
// reference corresponds to it: its prover never looks at C (src/groth16.cpp:48-254; the .zkey does not even hold it).
//
// Layout.  The constraints section is uploaded as it is in the file together with the word offset of every linear
// combination (one host pass over the term counts, zk_r1cs_create).  k_r1cs_decode turns it into one row-major
// structure over 3m rows — rows [0, m) are A, [m, 2m) B, [2m, 3m) C — with 64-bit term offsets (nnz passes 2^32 at
// 2^27 constraints), the wire id of every term and its coefficient pre-scaled to value * 2^522 (as the zkey CSR,
// fieldops.hip k_spmv_abc): one Fr29 Montgomery product with the standard-form witness value lands in the 2^261 form.
//
// Sparse product whose cost does not depend on row lengths.  Every row is cut into segments of at most SEG terms at
// fixed boundaries chosen at create time; one lane sums one segment.  A row with one segment writes its value; a row
// with several writes one partial per segment into a contiguous run, and the next pass applies the same cut to those
// runs, until one value per row is left (10^5 terms: 6250 -> 391 -> 25 -> 2 -> 1, five passes).  Field addition is
// exact, so the result does not depend on how a row is cut, and no pass needs an atomic on a field value.
//
// Lazy-sum bound.  Fr29 operands may lie anywhere in (-16r, 16r) (field29.hpp); a product of two such operands lands in
// (-r, 2r), reduce_near_zero returns (-r, r), and a canonical partial is in [0, r).  A lane starts at 0 and reduces
// after every LAZY = 7 additions, so its running sum stays in (-r, r) + 7 (-r, 2r) = (-8r, 15r): inside the operand
// range of add / reduce_near_zero / canonical with one r to spare on either side.  (k_spmv_abc reduces every 8
// products, which touches the bound; a row of r - 1 coefficients times r - 1 witness values is the extreme case, and
// tests/test_gpu_r1cs.py runs it at every row length around the cut points.)  A witness value >= r is a 256-bit word
// below 2^256 < 6r: still a valid operand, so the sums stay exact and such values are reported, not mis-summed.
#include <sys/random.h>
#include <mutex>
#include "r1cs_section.hpp"
#include "r1cs_internal.hpp"
#include "csr_long.hpp"
#include "field29.hpp"
#include "devmem.hpp"

namespace {

constexpr uint32_t SEG = SEG_TERMS;          // terms (or partials) one lane sums
constexpr uint32_t LAZY = 7;                 // additions between two reductions (bound above)
constexpr uint64_t FINAL = SEG_FINAL;        // segment destination: a row value, not a partial of the next pass
constexpr uint32_t NONE = 0xFFFFFFFFu;

// per-lane hit counts and lowest indices -> one pair of integer atomics per wave (the kernels below stride over their
// rows with a bounded grid, so a check in which every constraint fails still issues only a few thousand atomics)
__device__ __forceinline__ void wave_flush(uint32_t cnt, uint32_t low, unsigned long long *count, uint32_t *lowest) {
    for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_xor(cnt, off);
        const uint32_t o = __shfl_xor(low, off);
        low = o < low ? o : low;
    }
    if ((threadIdx.x & 63) == 0 && cnt) {
        if (count) atomicAdd(count, (unsigned long long)cnt);
        atomicMin(lowest, low);
    }
}
#define R1CS_FOR(i, n) for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += gridDim.x * blockDim.x)

// one lane per term of the section (term_at: r1cs_section.hpp) -> its wire id and its coefficient as value * 2^522
__global__ __launch_bounds__(256) void k_r1cs_decode(uint32_t *col, Fr *val, uint32_t *err, const uint32_t *sec, const uint64_t *lc_off,
                                                     const uint64_t *rowptr, uint32_t rows, uint32_t m, uint32_t nWires, uint64_t nnz, Fr k783) {
    const uint64_t st = (uint64_t)gridDim.x * blockDim.x;
    const Fr29 k = Fr29::load(k783);
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nnz; t += st) {
        uint32_t row;
        const uint32_t *p = term_at(t, sec, lc_off, rowptr, rows, row);
        const uint32_t wire = p[0], cons = row % m;
        Fr c;
#pragma unroll
        for (int j = 0; j < 8; j++) c.v[j] = p[1 + j];
        if (wire >= nWires) atomicMin(&err[0], cons);
        if (ge_r(c.v)) atomicMin(&err[1], cons);
        col[t] = wire < nWires ? wire : 0;
        store_el(val + t, Fr29::store(Fr29::mul(Fr29::load(c), k)));      // value * 2^522
    }
}

// One lane per segment [lo[j], lo[j+1]) of this pass's input: the terms (pass 0: coefficient x witness value) or the
// previous pass's partials.  dest[j] & FINAL: the row value (index into rows), else a partial for the next pass.
template <bool TERMS>
__global__ __launch_bounds__(256) void k_r1cs_pass(Fr *rows, Fr *next, const uint64_t *lo, const uint64_t *dest, uint64_t nseg,
                                                   const Fr *in, const uint32_t *col, const Fr *val, const Fr *w) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nseg) return;
    const uint64_t a = lo[j], b = lo[j + 1];
    Fr29 sum = Fr29::zero();
    uint32_t pending = 0;
    for (uint64_t t = a; t < b; t++) {
        const Fr29 x = TERMS ? Fr29::mul(Fr29::load(load_el(w + col[t])), Fr29::load(load_el(val + t))) : Fr29::load(load_el(in + t));
        sum = Fr29::add(sum, x);
        if (++pending == LAZY) {
            sum = Fr29::reduce_near_zero(sum);
            pending = 0;
        }
    }
    const uint64_t d = dest[j];
    store_el((d & FINAL) ? rows + (d & ~FINAL) : next + d, Fr29::store(sum));
}

struct DevReport {                            // zk_r1cs_report's device half
    unsigned long long failed;
    uint32_t first_failed, first_unreduced, one_ok, pad[3];
    Fr abc[3];                                // A.w, B.w, C.w of first_failed, standard form
};

__global__ void k_r1cs_report_init(DevReport *rep) {
    rep->failed = 0;
    rep->first_failed = NONE;
    rep->first_unreduced = NONE;
    rep->one_ok = 0;
}

// a.b - c per constraint (rows hold the 2^261 form: a.b.2^-261 is ab in it, like c)
__global__ __launch_bounds__(256) void k_r1cs_check(DevReport *rep, const Fr *rows, uint32_t m) {
    uint32_t cnt = 0, low = NONE;
    R1CS_FOR(i, m) {
        const Fr29 a = Fr29::load(load_el(rows + i)), b = Fr29::load(load_el(rows + (uint64_t)m + i)), c = Fr29::load(load_el(rows + 2ull * m + i));
        if (!Fr29::sub(Fr29::mul(a, b), c).is_zero()) {
            cnt++;
            low = low < i ? low : i;
        }
    }
    wave_flush(cnt, low, &rep->failed, &rep->first_failed);
}

// w[0] == 1 and the lowest index of a value >= r
__global__ __launch_bounds__(256) void k_r1cs_witness(DevReport *rep, const Fr *w, uint32_t n) {
    uint32_t cnt = 0, low = NONE;
    R1CS_FOR(i, n) {
        const Fr x = load_el(w + i);
        if (ge_r(x.v)) {
            cnt++;
            low = low < i ? low : i;
        }
        if (i == 0) {
            uint32_t o = x.v[0] ^ 1u;
#pragma unroll
            for (int j = 1; j < 8; j++) o |= x.v[j];
            rep->one_ok = o == 0;
        }
    }
    wave_flush(cnt, low, nullptr, &rep->first_unreduced);
}

// A.w, B.w, C.w of the lowest failing constraint in standard form
__global__ void k_r1cs_report_rows(DevReport *rep, const Fr *rows, uint32_t m) {
    const uint32_t f = rep->first_failed, k = threadIdx.x;
    Fr v;
    for (int j = 0; j < 8; j++) v.v[j] = 0;
    if (f != NONE && k < 3) v = Fr29::store(Fr29::from_mont(Fr29::load(load_el(rows + (uint64_t)k * m + f))));
    if (k < 3) store_el(rep->abc + k, v);
}

// zkey rows against the r1cs: row i < m: A.x and B.x equal; m <= i <= m + nPublic: A = x[i - m] (snarkjs's public-input
// rows), B = 0; later rows: both 0.  zab = k_spmv_abc's a | b over the domain, rows = this file's A.x | B.x | C.x.
__global__ __launch_bounds__(256) void k_r1cs_match(unsigned long long *differ, uint32_t *first, const Fr *zab, const Fr *rows, const Fr *x,
                                                    uint32_t n, uint32_t m, uint32_t nPublic, Fr k522) {
    uint32_t cnt = 0, low = NONE;
    R1CS_FOR(i, n) {
        Fr wa, wb;
        for (int j = 0; j < 8; j++) wa.v[j] = wb.v[j] = 0;
        if (i < m) {
            wa = load_el(rows + i);
            wb = load_el(rows + (uint64_t)m + i);
        } else if (i - m <= nPublic) {
            wa = Fr29::store(Fr29::mul(Fr29::load(load_el(x + (i - m))), Fr29::load(k522)));      // x * 2^261
        }
        const Fr za = load_el(zab + i), zb = load_el(zab + (uint64_t)n + i);
        uint32_t o = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) o |= (za.v[j] ^ wa.v[j]) | (zb.v[j] ^ wb.v[j]);
        if (o) {
            cnt++;
            low = low < i ? low : i;
        }
    }
    wave_flush(cnt, low, differ, first);
}

inline uint32_t blocks(uint64_t n) { return (uint32_t)((n + 255) / 256); }
inline uint32_t strided(uint64_t n) { return n < 256ull * 1024 ? blocks(n) : 1024; }     // the three reporting kernels

typedef SegPass Pass;                          // one pass of the segmented sum

}   // namespace

struct zk_r1cs {
    int device = 0;
    uint32_t nWires = 0, nPublic = 0, m = 0;
    uint64_t nnz = 0;
    hipStream_t stream = nullptr;
    std::mutex mtx;                            // one check / match at a time per checker
    DevBuf<uint32_t> col;
    DevBuf<Fr> val, rows, w, part[2];
    std::vector<std::unique_ptr<Pass>> passes;
    DevBuf<DevReport> rep;
    DevReport *host_rep = nullptr;             // pinned
    Fr k522, k783;
    ~zk_r1cs() {
        if (stream) (void)hipStreamSynchronize(stream);
        if (host_rep) (void)hipHostFree(host_rep);
        if (stream) (void)hipStreamDestroy(stream);
    }

    // rows = A.x | B.x | C.x for a witness x resident on the device
    void spmv(const Fr *x) {
        for (size_t l = 0; l < passes.size(); l++) {
            const Pass &p = *passes[l];
            Fr *next = part[l & 1].p;
            const Fr *in = l ? part[(l - 1) & 1].p : nullptr;
            if (l == 0) ZK_LAUNCH(k_r1cs_pass<true>, dim3(blocks(p.nseg)), dim3(256), 0, stream, rows.p, next, p.lo.p, p.dest.p, p.nseg, in, col.p, val.p, x);
            else ZK_LAUNCH(k_r1cs_pass<false>, dim3(blocks(p.nseg)), dim3(256), 0, stream, rows.p, next, p.lo.p, p.dest.p, p.nseg, in, col.p, val.p, x);
        }
        ZK_LAUNCH_OK("r1cs segmented sum");
    }

    void check(const Fr *x, zk_r1cs_report *out) {
        ZK_LAUNCH(k_r1cs_report_init, dim3(1), dim3(1), 0, stream, rep.p);
        if (m) {
            spmv(x);
            ZK_LAUNCH(k_r1cs_check, dim3(strided(m)), dim3(256), 0, stream, rep.p, rows.p, m);
        }
        if (nWires) ZK_LAUNCH(k_r1cs_witness, dim3(strided(nWires)), dim3(256), 0, stream, rep.p, x, nWires);
        if (m) ZK_LAUNCH(k_r1cs_report_rows, dim3(1), dim3(64), 0, stream, rep.p, rows.p, m);
        ZK_LAUNCH_OK("r1cs check");
        HIP_TRY(hipMemcpyAsync(host_rep, rep.p, sizeof(DevReport), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        zk_r1cs_report r;
        memset(&r, 0, sizeof r);
        r.failed = host_rep->failed;
        r.first_failed = host_rep->first_failed;
        memcpy(r.a, host_rep->abc[0].v, 32);
        memcpy(r.b, host_rep->abc[1].v, 32);
        memcpy(r.c, host_rep->abc[2].v, 32);
        r.one_ok = host_rep->one_ok;
        r.first_unreduced = host_rep->first_unreduced;
        const uint32_t size = out->size ? (out->size < sizeof r ? out->size : (uint32_t)sizeof r) : (uint32_t)sizeof r;
        r.size = size;
        memcpy(out, &r, size);
    }
};

namespace zkp {

// The one host pass over section 2: word offset and term count of every linear combination, checked against the section size
void walk_constraints(const zk_r1cs_view *v, std::vector<uint64_t> &lc_off, std::vector<uint64_t> &rowptr) {
    const uint8_t *s = static_cast<const uint8_t *>(v->constraints);
    const uint64_t size = v->constraints_bytes, m = v->nConstraints;
    if (size % 4) throw std::invalid_argument("r1cs constraints section size is not a multiple of 4");
    lc_off.resize(3 * m);
    std::vector<uint32_t> len(3 * m);
    uint64_t pos = 0;
    for (uint64_t i = 0; i < m; i++)
        for (uint64_t mat = 0; mat < 3; mat++) {
            if (pos + 4 > size) throw std::invalid_argument("r1cs constraints section is truncated (constraint " + std::to_string(i) + ")");
            uint32_t cnt;
            memcpy(&cnt, s + pos, 4);
            lc_off[mat * m + i] = pos / 4;
            len[mat * m + i] = cnt;
            pos += 4 + 36ull * cnt;
            if (pos > size) throw std::invalid_argument("r1cs constraints section is truncated (constraint " + std::to_string(i) + ")");
        }
    if (pos != size) throw std::invalid_argument("r1cs constraints section is longer than its constraints");
    rowptr.assign(3 * m + 1, 0);
    for (uint64_t r = 0; r < 3 * m; r++) rowptr[r + 1] = rowptr[r] + len[r];
}

R1csDev r1cs_dev(zk_r1cs *r) { return R1csDev{r->device, r->stream, r->nWires, r->nPublic, r->m, r->nnz, r->rows.p}; }
void r1cs_spmv(zk_r1cs *r, const Fr *x) {
    if (r->m) r->spmv(x);
}

// Segments of every pass (host, create time).  Pass 0's input is the terms of all rows in order; a row of L inputs
// gets max(1, ceil(L / SEG)) segments; the rows with several go on to the next pass with one input per segment.
void plan_segments(const std::vector<uint64_t> &rowptr, std::vector<std::unique_ptr<SegPass>> &passes, uint64_t max_part[2]) {
    struct Open {
        uint32_t row;
        uint64_t base, len;
    };
    std::vector<Open> cur, nxt;
    max_part[0] = max_part[1] = 0;
    for (int level = 0;; level++) {
        std::vector<uint64_t> lo, dest;
        uint64_t npos = 0, end = 0;
        nxt.clear();
        auto add_row = [&](uint32_t row, uint64_t base, uint64_t len) {
            const uint64_t nseg = len <= SEG ? 1 : (len + SEG - 1) / SEG;
            if (nseg == 1) {
                lo.push_back(base);
                dest.push_back(FINAL | row);
            } else {
                nxt.push_back(Open{row, npos, nseg});
                for (uint64_t k = 0; k < nseg; k++) {
                    lo.push_back(base + k * SEG);
                    dest.push_back(npos++);
                }
            }
            end = base + len;
        };
        if (level == 0) {
            const uint32_t rows = (uint32_t)(rowptr.size() - 1);
            for (uint32_t row = 0; row < rows; row++) add_row(row, rowptr[row], rowptr[row + 1] - rowptr[row]);
        } else {
            for (const Open &o : cur) add_row(o.row, o.base, o.len);
        }
        if (lo.empty()) break;
        lo.push_back(end);
        auto p = std::make_unique<Pass>();
        p->nseg = dest.size();
        p->lo.alloc(lo.size());
        p->dest.alloc(dest.size());
        HIP_TRY(hipMemcpy(p->lo.p, lo.data(), lo.size() * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(p->dest.p, dest.data(), dest.size() * 8, hipMemcpyHostToDevice));
        passes.push_back(std::move(p));
        if (npos > max_part[level & 1]) max_part[level & 1] = npos;
        if (nxt.empty()) break;
        cur.swap(nxt);
    }
}

}   // namespace zkp

namespace {

void plan_passes(zk_r1cs *r, const std::vector<uint64_t> &rowptr) {
    uint64_t max_part[2];
    plan_segments(rowptr, r->passes, max_part);
    for (int k = 0; k < 2; k++) r->part[k].alloc(max_part[k] ? max_part[k] : 1);
}

void r1cs_create(zk_r1cs **out, const zk_r1cs_view *v, int32_t device) {
    if (!out || !v) throw std::invalid_argument("null argument");
    *out = nullptr;
    if (v->nConstraints && !v->constraints) throw std::invalid_argument("null constraints section");
    std::vector<uint64_t> lc_off, rowptr;
    walk_constraints(v, lc_off, rowptr);                  // the file is checked before the device is touched
    const int dev = resolve_device(device);
    DeviceGuard g(dev);
    std::unique_ptr<zk_r1cs> r(new zk_r1cs());
    r->device = dev;
    r->nWires = v->nWires;
    r->nPublic = v->nPubOut + v->nPubIn;
    r->m = v->nConstraints;
    r->nnz = rowptr.back();
    if (3ull * r->m >= (1ull << 31)) throw std::invalid_argument("r1cs has too many constraints");
    HIP_TRY(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
    HIP_TRY(hipHostMalloc((void **)&r->host_rep, sizeof(DevReport), hipHostMallocDefault));
    // 2^522 and 2^783 mod r: 261 doublings of the internal one (2^261), then one Montgomery square
    Fr29 k = Fr29::one();
    for (int i = 0; i < 261; i++) k = Fr29::reduce_near_zero(Fr29::dbl(k));
    r->k522 = Fr29::store(k);
    r->k783 = Fr29::store(Fr29::mul(k, k));
    r->rep.alloc(1);
    r->w.alloc(r->nWires ? r->nWires : 1);
    r->rows.alloc(r->m ? 3ull * r->m : 1);
    r->col.alloc(r->nnz ? r->nnz : 1);
    r->val.alloc(r->nnz ? r->nnz : 1);
    if (r->nnz) {
        SectionOnDevice sec;
        sec.upload(v, lc_off, rowptr, r->stream);
        const uint64_t g = r->nnz < 256ull * 4096 ? (r->nnz + 255) / 256 : 4096;
        ZK_LAUNCH(k_r1cs_decode, dim3((uint32_t)g), dim3(256), 0, r->stream, r->col.p, r->val.p, sec.err.p, sec.sec(), sec.d_off.p, sec.d_ptr.p, sec.rows(),
                  r->m, r->nWires, r->nnz, r->k783);
        ZK_LAUNCH_OK("r1cs decode");
        sec.check(r->stream);
    }
    plan_passes(r.get(), rowptr);
    *out = r.release();
}

void r1cs_match(zk_r1cs *r, const zk_zkey_view *z, uint64_t *rows_differing, uint32_t *first_row) {
    if (!r || !z || !rows_differing || !first_row) throw std::invalid_argument("null argument");
    if (z->nVars != r->nWires)
        throw std::invalid_argument("r1cs does not match the zkey: nWires " + std::to_string(r->nWires) + ", zkey nVars " + std::to_string(z->nVars));
    if (z->nPublic != r->nPublic)
        throw std::invalid_argument("r1cs does not match the zkey: nPubOut + nPubIn " + std::to_string(r->nPublic) + ", zkey nPublic " + std::to_string(z->nPublic));
    const uint32_t n = z->domainSize;
    if ((uint64_t)n < (uint64_t)r->m + r->nPublic + 1)
        throw std::invalid_argument("r1cs does not match the zkey: " + std::to_string(r->m) + " constraints + " + std::to_string(r->nPublic) +
                                    " + 1 public-input rows exceed the domain " + std::to_string(n));
    const uint64_t nCoefs = z->nCoefs;
    if (nCoefs >= (1ull << 32)) throw std::invalid_argument("nCoefs >= 2^32 is not supported");
    if (nCoefs && !z->coefs) throw std::invalid_argument("null coefficient section");
    if (z->coefs_bytes && z->coefs_bytes < 4 + nCoefs * 44) throw std::invalid_argument("zkey coefficient section is shorter than nCoefs records");
    DeviceGuard g(r->device);
    std::lock_guard<std::mutex> lk(r->mtx);
    // x: random, below r (the top three bits cleared: x < 2^253 < r); a difference survives with probability ~ 1 / r
    std::vector<uint8_t> x((size_t)r->nWires * 32);
    for (size_t off = 0; off < x.size();) {
        const ssize_t got = getrandom(x.data() + off, x.size() - off, 0);
        if (got <= 0) throw std::runtime_error("getrandom failed");
        off += (size_t)got;
    }
    for (uint32_t i = 0; i < r->nWires; i++) x[(size_t)i * 32 + 31] &= 0x1F;
    DevBuf<uint8_t> raw;
    DevBuf<uint32_t> cursor, err, rowptr, col, cnt;
    DevBuf<Fr> val, ab;
    const uint32_t rows = 2 * n;
    raw.alloc(nCoefs ? nCoefs * 44 : 4);
    cursor.alloc(rows);
    err.alloc(4);
    rowptr.alloc((size_t)rows + 1 + msm_scan_extra_words(rows));
    col.alloc(nCoefs ? nCoefs : 1);
    val.alloc(nCoefs ? nCoefs : 1);
    ab.alloc(3 * (size_t)n);
    cnt.alloc(3);
    StreamUploader up(r->stream);
    if (nCoefs) up.copy(raw.p, (const uint8_t *)z->coefs + 4, nCoefs * 44);
    HIP_TRY(hipMemcpyAsync(r->w.p, x.data(), x.size(), hipMemcpyHostToDevice, r->stream));
    const uint32_t row_cut = spmv_row_cut();
    launch_csr_build(rowptr.p, col.p, val.p, cursor.p, err.p, raw.p, nCoefs, n, r->nWires, 0, n, row_cut, r->stream);
    launch_fr_to_internal(val.p, nCoefs, 2, r->stream);
    uint32_t bad[4] = {0, 0, 0, 0};       // the record check, and the key's long rows (fieldops.hip)
    HIP_TRY(hipMemcpyAsync(bad, err.p, 16, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (bad[0]) throw std::invalid_argument("zkey coefficient record out of range");
    CsrLong lr;
    DevBuf<Fr> part;
    lr.build(rowptr.p, rows, row_cut, bad, r->stream);
    if (lr.chunks) part.alloc(lr.chunks);
    const CsrDev csr = lr.view(rowptr.p, col.p, val.p);
    launch_spmv_abc(ab.p, ab.p + n, ab.p + 2 * (size_t)n, csr, r->w.p, n, r->stream, 1, 0, 0, part.p);
    if (r->m) r->spmv(r->w.p);
    HIP_TRY(hipMemsetAsync(cnt.p, 0, 8, r->stream));
    HIP_TRY(hipMemsetAsync(cnt.p + 2, 0xFF, 4, r->stream));
    ZK_LAUNCH(k_r1cs_match, dim3(strided(n)), dim3(256), 0, r->stream, (unsigned long long *)cnt.p, cnt.p + 2, ab.p, r->rows.p, r->w.p, n, r->m,
              r->nPublic, r->k522);
    ZK_LAUNCH_OK("r1cs match");
    uint32_t res[3];
    HIP_TRY(hipMemcpyAsync(res, cnt.p, 12, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    *rows_differing = (uint64_t)res[0] | ((uint64_t)res[1] << 32);
    *first_row = res[2];
}

}   // namespace

extern "C" {

int zk_r1cs_create(zk_r1cs **out, const zk_r1cs_view *v, int32_t device) {
    return guarded([&] { r1cs_create(out, v, device); });
}

void zk_r1cs_destroy(zk_r1cs *r) {
    if (!r) return;
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(r->device);
    delete r;
    if (prev >= 0) (void)hipSetDevice(prev);
}

int zk_r1cs_check(zk_r1cs *r, const uint8_t *wtns, uint32_t nVars, zk_r1cs_report *rep) {
    return guarded([&] {
        if (!r || !rep || (nVars && !wtns)) throw std::invalid_argument("null argument");
        if (nVars != r->nWires) throw std::invalid_argument("witness has " + std::to_string(nVars) + " values, the r1cs " + std::to_string(r->nWires) + " wires");
        DeviceGuard g(r->device);
        std::lock_guard<std::mutex> lk(r->mtx);
        StreamUploader up(r->stream);
        up.copy(r->w.p, wtns, (size_t)nVars * 32);
        r->check(r->w.p, rep);
    });
}

int zk_r1cs_check_dev(zk_r1cs *r, const void *d_wtns, uint32_t nVars, zk_r1cs_report *rep) {
    return guarded([&] {
        if (!r || !rep || (nVars && !d_wtns)) throw std::invalid_argument("null argument");
        if (nVars != r->nWires) throw std::invalid_argument("witness has " + std::to_string(nVars) + " values, the r1cs " + std::to_string(r->nWires) + " wires");
        DeviceGuard g(r->device);
        std::lock_guard<std::mutex> lk(r->mtx);
        r->check(static_cast<const Fr *>(d_wtns), rep);
    });
}

int zk_r1cs_match_zkey(zk_r1cs *r, const zk_zkey_view *zkey, uint64_t *rows_differing, uint32_t *first_row) {
    return guarded([&] { r1cs_match(r, zkey, rows_differing, first_row); });
}

}   // extern "C"
