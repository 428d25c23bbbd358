// PLONK from a circom .r1cs (include/zkhip.h, section "PLONK from an R1CS"): the gates, the wire maps and the permutation of
// a three-column circuit compiled on the device from section 2 of the file, and the per-proof extension of a circom witness
// by the wires the compile introduced.  Nothing in the reference corresponds to it (it proves Groth16 only); the counterpart
// is snarkjs's `plonk setup`, whose layout this follows in spirit only (the header states this project's own).  DESIGN.md
// section 32 states the steps, the launches and what was measured.
//
// Every step is flat in the row lengths: nothing loops over the terms of a linear combination (LC).
//   k_r1cs_flags        a lane a term (term_at: r1cs_section.hpp): "kept and not on wire 0", the LC's wire-0 term and their count
//   k_u32_scan_*        reduce - carry - apply, exclusive sums of 32-bit counts: a lane takes `seg` consecutive elements
//                       (ZKHIP_R1CS_SEG), a workgroup 256 lanes; the carry is one workgroup over the workgroups' sums.  Integer
//                       sums are exact, so no byte depends on seg.  Used over the terms (rank inside the LC, t_L), the
//                       constraints (first addition gate), and every digit pass of the sort (the tiles' histograms)
//   k_r1cs_additions    a lane a constraint: its number of addition gates
//   k_r1cs_emit_terms   a lane a term: the term of rank r >= 1 writes addition gate r - 1 of its LC (b, c, qr, qo, and a, ql for
//                       r >= 2) and its row of the extension tables; the term of rank 0 writes a and ql of gate 0, and its own
//                       index where the final gate finds it
//   k_r1cs_emit_final   a lane a constraint: the final gate
//   k_cell_*            the stable LSD radix sort of the 3n (wire, cell) pairs by wire, 8 bits a pass, a tile of 2048 pairs a
//                       workgroup.  Inside a tile a pair's place among EARLIER pairs of the same digit comes from wave ballots and
//                       per-wave counts, never from an atomic cursor: the order, and so sigma, is the same in every run
//   k_sigma_heads/_write  a lane a sorted position: sigma at its cell points to the right neighbour of the same wire, else to
//                       the head of its group (kept by wire by the first kernel); w^row' by pow_tab over the table of squarings
//   k_ext_*             the extension: a segmented inclusive sum in Fr over the addition gates in row order, reduce - carry -
//                       apply like the integer scan, the element of gate q being c.w[wire] of its term (plus the LC's first
//                       term where a chain starts).  Field addition is exact: no byte depends on seg
// Atomics: integer counts and minima only (the wire-0 count, the error words, a tile's histogram in LDS); every one of them
// has the same result in any order.
#include "plonk_internal.hpp"
#include "r1cs_section.hpp"

namespace {

constexpr uint32_t WG = 256, WAVES = WG / 64;
constexpr uint32_t DEFAULT_SEG = 8, MAX_SEG = 4096;
constexpr uint32_t RADIX_BITS = 8, RADIX = 1u << RADIX_BITS, TILE_ITEMS = 8, TILE = WG * TILE_ITEMS;
constexpr uint32_t MIN_LOG_N = 3, MAX_LOG_N = 25;
constexpr uint32_t NONE = 0xFFFFFFFFu;
static_assert(RADIX == WG, "a lane a digit in the tile kernels");

uint32_t seg_in_effect() { return (uint32_t)env_number("ZKHIP_R1CS_SEG", DEFAULT_SEG, 1, MAX_SEG, "a number of elements per lane from 1 to 4096", ENV_LAX); }

// ---------------------------------------------------------------- device: the integer scan
// exclusive sum of v across the workgroup's 256 lanes and their total; lds: WAVES words, free again on return
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t &total, uint32_t *lds) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off);
        if ((int)lane >= off) inc += o;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; w++) {
        if (w < wave) before += lds[w];
        total += lds[w];
    }
    __syncthreads();
    return before + inc - v;
}

// sums[b] = the sum of workgroup b's WG * seg elements of x[0, len)
__global__ __launch_bounds__(WG) void k_u32_scan_reduce(uint32_t *sums, const uint32_t *x, uint64_t len, uint32_t seg) {
    __shared__ uint32_t lds[WAVES];
    const uint64_t at = ((uint64_t)blockIdx.x * WG + threadIdx.x) * seg;
    uint32_t sum = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < seg && at + k < len; k++) sum += x[at + k];
    uint32_t total;
    (void)block_scan(sum, total, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[0, nb) -> their exclusive sums, *total = their sum
__global__ __launch_bounds__(WG) void k_u32_scan_carry(uint32_t *sums, uint64_t nb, uint32_t *total_out) {
    __shared__ uint32_t lds[WAVES];
    const uint64_t chunk = (nb + WG - 1) / WG, lo = threadIdx.x * chunk, hi = lo + chunk < nb ? lo + chunk : nb;
    uint32_t sum = 0;
    for (uint64_t i = lo; i < hi; i++) sum += sums[i];
    uint32_t total;
    uint32_t run = block_scan(sum, total, lds);
    for (uint64_t i = lo; i < hi; i++) {
        const uint32_t v = sums[i];
        sums[i] = run;
        run += v;
    }
    if (threadIdx.x == 0) *total_out = total;
}

// x[i] <- the sum of x[0, i), in place
__global__ __launch_bounds__(WG) void k_u32_scan_apply(uint32_t *x, const uint32_t *sums, uint64_t len, uint32_t seg) {
    __shared__ uint32_t lds[WAVES];
    const uint64_t at = ((uint64_t)blockIdx.x * WG + threadIdx.x) * seg;
    uint32_t sum = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < seg && at + k < len; k++) sum += x[at + k];
    uint32_t total;
    uint32_t run = sums[blockIdx.x] + block_scan(sum, total, lds);
#pragma unroll 1
    for (uint32_t k = 0; k < seg && at + k < len; k++) {
        const uint32_t v = x[at + k];
        x[at + k] = run;
        run += v;
    }
}

// ---------------------------------------------------------------- device: the terms
struct Section {
    const uint32_t *sec;
    const uint64_t *lc_off, *rowptr;
    uint32_t rows, m, nWires, nPublic;                // rows = 3m: [0, m) A, [m, 2m) B, [2m, 3m) C
    uint64_t nnz;
};

__device__ __forceinline__ Fr coef_of(const uint32_t *p) {
    Fr c;
#pragma unroll
    for (int j = 0; j < 8; j++) c.v[j] = p[1 + j];
    return c;
}

// pos[t] = 1 for a term that is kept (coefficient not 0) and not on wire 0.  A kept term on wire 0 is its LC's constant:
// w0cnt[row] counts them, w0term[row] names one (the only one of an LC that is not refused).  err[0], err[1]: the section's
// range checks (SectionOnDevice); err[2]: the lowest 3 * constraint + matrix of an LC with two kept terms on wire 0
__global__ __launch_bounds__(WG) void k_r1cs_flags(uint32_t *pos, uint32_t *w0cnt, uint32_t *w0term, uint32_t *err, uint32_t *err2, Section S) {
    const uint64_t st = (uint64_t)gridDim.x * WG;
    for (uint64_t t = (uint64_t)blockIdx.x * WG + threadIdx.x; t < S.nnz; t += st) {
        uint32_t row;
        const uint32_t *p = term_at(t, S.sec, S.lc_off, S.rowptr, S.rows, row);
        const uint32_t wire = p[0], cons = row % S.m, mat = row / S.m;
        const Fr c = coef_of(p);
        if (wire >= S.nWires) atomicMin(&err[0], cons);
        if (ge_r(c.v)) atomicMin(&err[1], cons);
        const bool kept = !c.is_zero();
        pos[t] = kept && wire != 0;
        if (kept && wire == 0) {
            if (atomicAdd(&w0cnt[row], 1u)) atomicMin(err2, cons * 3 + mat);
            w0term[row] = (uint32_t)t;
        }
    }
}

// t_L of a row from the scanned flags
__device__ __forceinline__ uint32_t terms_of(const uint32_t *pos, const uint64_t *rowptr, uint32_t row) { return pos[rowptr[row + 1]] - pos[rowptr[row]]; }
__device__ __forceinline__ uint32_t adds_of(uint32_t t) { return t ? t - 1 : 0; }

__global__ __launch_bounds__(WG) void k_r1cs_additions(uint32_t *adds, const uint32_t *pos, const uint64_t *rowptr, uint32_t m) {
    const uint32_t j = blockIdx.x * WG + threadIdx.x;
    if (j >= m) return;
    adds[j] = adds_of(terms_of(pos, rowptr, j)) + adds_of(terms_of(pos, rowptr, m + j)) + adds_of(terms_of(pos, rowptr, 2 * m + j));
}

struct Circuit {                                      // what the emit kernels write
    Fr *ql, *qr, *qm, *qo, *qc;                       // n rows each, standard form, zeroed
    uint32_t *a, *b, *c;                              // n rows each, zeroed: wire 0
    uint32_t *xw, *hw;                                // the extension tables, a row an addition gate: its term's wire, and the
    Fr *xc, *hc;                                      // wire of the LC's first term where a chain starts; the coefficients, Montgomery
    uint8_t *xstart;
};

__global__ __launch_bounds__(WG) void k_r1cs_public(Circuit C, uint32_t nPublic) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= nPublic) return;
    C.a[i] = 1 + i;
    store_el(C.ql + i, Fr::from_mont(Fr::one()));
}

// the first addition gate of LC `mat` of constraint j
__device__ __forceinline__ uint32_t first_gate(const uint32_t *pos, const uint32_t *addfirst, const Section &S, uint32_t j, uint32_t mat) {
    uint32_t q = addfirst[j];
    if (mat >= 1) q += adds_of(terms_of(pos, S.rowptr, j));
    if (mat == 2) q += adds_of(terms_of(pos, S.rowptr, S.m + j));
    return q;
}

__global__ __launch_bounds__(WG) void k_r1cs_emit_terms(Circuit C, uint32_t *first, const uint32_t *pos, const uint32_t *addfirst, Section S) {
    const uint64_t st = (uint64_t)gridDim.x * WG;
    const Fr one = Fr::from_mont(Fr::one()), minus_one = Fr::sub(Fr::zero(), one);
    for (uint64_t t = (uint64_t)blockIdx.x * WG + threadIdx.x; t < S.nnz; t += st) {
        if (pos[t + 1] == pos[t]) continue;
        uint32_t row;
        const uint32_t *p = term_at(t, S.sec, S.lc_off, S.rowptr, S.rows, row);
        const uint32_t j = row % S.m, mat = row / S.m, base = pos[S.rowptr[row]];
        const uint32_t r = pos[t] - base, cnt = pos[S.rowptr[row + 1]] - base;
        if (r == 0) first[row] = (uint32_t)t;
        if (cnt < 2) continue;
        const uint32_t wire = p[0];
        const Fr c = coef_of(p);
        const uint32_t q = first_gate(pos, addfirst, S, j, mat) + (r ? r - 1 : 0);
        const uint64_t g = (uint64_t)S.nPublic + q + j;          // the rows before it: the publics, q additions, j final gates
        if (r == 0) {
            C.a[g] = wire;
            store_el(C.ql + g, c);
            C.hw[q] = wire;
            store_el(C.hc + q, Fr::to_mont(c));
            continue;
        }
        C.b[g] = wire;
        C.c[g] = S.nWires + q;
        store_el(C.qr + g, c);
        store_el(C.qo + g, minus_one);
        C.xw[q] = wire;
        store_el(C.xc + q, Fr::to_mont(c));
        C.xstart[q] = r == 1;
        if (r >= 2) {
            C.a[g] = S.nWires + q - 1;
            store_el(C.ql + g, one);
        }
    }
}

__global__ __launch_bounds__(WG) void k_r1cs_emit_final(Circuit C, const uint32_t *first, const uint32_t *w0cnt, const uint32_t *w0term, const uint32_t *pos,
                                                       const uint32_t *addfirst, Section S) {
    const uint32_t j = blockIdx.x * WG + threadIdx.x;
    if (j >= S.m) return;
    uint32_t s[3];
    Fr c[3], k[3];                                     // standard form
    uint32_t q = addfirst[j];
#pragma unroll
    for (uint32_t mat = 0; mat < 3; mat++) {
        const uint32_t row = mat * S.m + j, cnt = terms_of(pos, S.rowptr, row);
        const uint32_t *lc = S.sec + S.lc_off[row] + 1;
        k[mat] = w0cnt[row] ? coef_of(lc + 9 * (w0term[row] - S.rowptr[row])) : Fr::zero();
        if (cnt == 0) {
            s[mat] = 0;
            c[mat] = Fr::zero();
        } else if (cnt == 1) {
            const uint32_t *p = lc + 9 * (first[row] - S.rowptr[row]);
            s[mat] = p[0];
            c[mat] = coef_of(p);
        } else {
            q += cnt - 1;
            s[mat] = S.nWires + q - 1;
            c[mat] = Fr::from_mont(Fr::one());
        }
    }
    const uint64_t g = (uint64_t)S.nPublic + addfirst[j + 1] + j;
    C.a[g] = s[0], C.b[g] = s[1], C.c[g] = s[2];
    const Fr ca = Fr::to_mont(c[0]), ka = Fr::to_mont(k[0]);
    store_el(C.qm + g, Fr::mul(ca, c[1]));
    store_el(C.ql + g, Fr::mul(ca, k[1]));
    store_el(C.qr + g, Fr::mul(ka, c[1]));
    store_el(C.qo + g, Fr::sub(Fr::zero(), c[2]));
    store_el(C.qc + g, Fr::sub(Fr::mul(ka, k[1]), k[2]));
}

// ---------------------------------------------------------------- device: the sort of the cells by wire
__global__ __launch_bounds__(WG) void k_cell_init(uint32_t *cells, uint64_t total) {
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (i < total) cells[i] = (uint32_t)i;
}

// hist[d * tiles + tile] = the pairs of the tile whose digit is d
__global__ __launch_bounds__(WG) void k_cell_hist(uint32_t *hist, const uint32_t *keys, uint64_t total, uint32_t shift, uint32_t tiles) {
    __shared__ uint32_t h[RADIX];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * TILE;
#pragma unroll 1
    for (uint32_t k = 0; k < TILE_ITEMS; k++) {
        const uint64_t i = base + k * WG + threadIdx.x;
        if (i < total) atomicAdd(&h[(keys[i] >> shift) & (RADIX - 1)], 1u);
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

// A pair goes to hist[digit][tile] (scanned) + the number of pairs of its digit EARLIER in the tile.  The tile is taken in
// TILE_ITEMS rounds of 256 neighbouring pairs; in a round a lane's place among its wave's lanes of the same digit comes
// from eight ballots, the waves before it from cnt[], the rounds before it from running[]
__global__ __launch_bounds__(WG) void k_cell_scatter(uint32_t *keys_out, uint32_t *cells_out, const uint32_t *keys, const uint32_t *cells, const uint32_t *hist,
                                                    uint64_t total, uint32_t shift, uint32_t tiles) {
    __shared__ uint32_t running[RADIX], cnt[WAVES][RADIX];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    running[threadIdx.x] = 0;
    const uint64_t base = (uint64_t)blockIdx.x * TILE;
#pragma unroll 1
    for (uint32_t k = 0; k < TILE_ITEMS; k++) {
#pragma unroll
        for (uint32_t w = 0; w < WAVES; w++) cnt[w][threadIdx.x] = 0;
        __syncthreads();
        const uint64_t i = base + k * WG + threadIdx.x;
        const bool valid = i < total;
        const uint32_t key = valid ? keys[i] : 0, cell = valid ? cells[i] : 0, d = (key >> shift) & (RADIX - 1);
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (uint32_t b = 0; b < RADIX_BITS; b++) {
            const bool bit = (d >> b) & 1;
            const unsigned long long vote = __ballot(valid && bit);
            peers &= bit ? vote : ~vote;
        }
        const uint32_t rank = __popcll(peers & ((1ull << lane) - 1));
        if (valid && rank == 0) cnt[wave][d] = __popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t before = running[d];
            for (uint32_t w = 0; w < wave; w++) before += cnt[w][d];
            const uint64_t at = (uint64_t)hist[(uint64_t)d * tiles + blockIdx.x] + before + rank;
            keys_out[at] = key;
            cells_out[at] = cell;
        }
        __syncthreads();
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t w = 0; w < WAVES; w++) sum += cnt[w][threadIdx.x];
        running[threadIdx.x] += sum;
        __syncthreads();
    }
}

// headcell[wire] = the first cell of the wire's group
__global__ __launch_bounds__(WG) void k_sigma_heads(uint32_t *headcell, const uint32_t *keys, const uint32_t *cells, uint64_t total) {
    const uint64_t p = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (p >= total) return;
    const uint32_t wire = keys[p];
    if (p == 0 || keys[p - 1] != wire) headcell[wire] = cells[p];
}

// sigma (3n rows: s1 | s2 | s3) at a sorted position's cell = K[col'] w^row' of the cell it points to.  tab: w^(2^i), then
// at POW_BITS the three shifts, all Montgomery
__global__ __launch_bounds__(WG) void k_sigma_write(Fr *sigma, const uint32_t *headcell, const uint32_t *keys, const uint32_t *cells, uint64_t total, uint32_t log_n,
                                                   const Fr *tab) {
    const uint64_t p = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (p >= total) return;
    const uint32_t wire = keys[p];
    const uint32_t to = (p + 1 < total && keys[p + 1] == wire) ? cells[p + 1] : headcell[wire];
    const uint32_t col = to >> log_n, row = to & ((1u << log_n) - 1);
    store_el(sigma + cells[p], Fr::from_mont(Fr::mul(load_el(tab + POW_BITS + col), pow_tab(tab, row))));
}

// ---------------------------------------------------------------- device: the extension
struct Seg {
    uint32_t f;                                       // a chain starts in what the value sums
    Fr v;
};
__device__ __forceinline__ Seg seg_join(const Seg &a, const Seg &b) { return Seg{a.f | b.f, b.f ? b.v : Fr::add(a.v, b.v)}; }   // a, then b

struct Ext {
    const uint32_t *xw, *hw;
    const Fr *xc, *hc;
    const uint8_t *xstart;
    uint64_t n_add;
    uint32_t nWires, seg;
};
// gate q's element: its term's c w[wire], and with it the LC's first term where the chain starts.  Coefficients are
// Montgomery and the witness standard, so a product is standard
__device__ __forceinline__ Seg ext_element(const Ext &E, const Fr *w, uint64_t q) {
    Seg e{E.xstart[q], Fr::mul(load_el(E.xc + q), load_el(w + E.xw[q]))};
    if (e.f) e.v = Fr::add(e.v, Fr::mul(load_el(E.hc + q), load_el(w + E.hw[q])));
    return e;
}
// a lane's `seg` consecutive gates joined
__device__ __forceinline__ Seg ext_lane(const Ext &E, const Fr *w, uint64_t at) {
    Seg acc{0, Fr::zero()};
#pragma unroll 1
    for (uint32_t k = 0; k < E.seg && at + k < E.n_add; k++) acc = seg_join(acc, ext_element(E, w, at + k));
    return acc;
}
// what lies before the lane in the workgroup, joined (nothing for lane 0), and the workgroup's total
__device__ __forceinline__ Seg block_seg_scan(Seg mine, Seg &total, uint32_t *lf, Fr *lv) {
    const uint32_t tid = threadIdx.x;
    lf[tid] = mine.f;
    lv[tid] = mine.v;
    __syncthreads();
#pragma unroll 1
    for (uint32_t off = 1; off < WG; off <<= 1) {
        Seg o{0, Fr::zero()};
        const bool has = tid >= off;
        if (has) o = Seg{lf[tid - off], lv[tid - off]};
        __syncthreads();
        if (has) {
            mine = seg_join(o, mine);
            lf[tid] = mine.f;
            lv[tid] = mine.v;
        }
        __syncthreads();
    }
    total = Seg{lf[WG - 1], lv[WG - 1]};
    const Seg ex = tid ? Seg{lf[tid - 1], lv[tid - 1]} : Seg{0, Fr::zero()};
    __syncthreads();
    return ex;
}

__global__ __launch_bounds__(WG) void k_ext_reduce(uint32_t *agg_f, Fr *agg_v, Ext E, const Fr *w) {
    __shared__ uint32_t lf[WG];
    __shared__ Fr lv[WG];
    Seg total;
    (void)block_seg_scan(ext_lane(E, w, ((uint64_t)blockIdx.x * WG + threadIdx.x) * E.seg), total, lf, lv);
    if (threadIdx.x == 0) {
        agg_f[blockIdx.x] = total.f;
        store_el(agg_v + blockIdx.x, total.v);
    }
}

// one workgroup: the workgroups' totals -> what lies before each of them, joined
__global__ __launch_bounds__(WG) void k_ext_carry(uint32_t *agg_f, Fr *agg_v, uint64_t nb) {
    __shared__ uint32_t lf[WG];
    __shared__ Fr lv[WG];
    const uint64_t chunk = (nb + WG - 1) / WG, lo = threadIdx.x * chunk, hi = lo + chunk < nb ? lo + chunk : nb;
    Seg acc{0, Fr::zero()};
    for (uint64_t i = lo; i < hi; i++) acc = seg_join(acc, Seg{agg_f[i], load_el(agg_v + i)});
    Seg total;
    Seg run = block_seg_scan(acc, total, lf, lv);
    for (uint64_t i = lo; i < hi; i++) {
        const Seg v{agg_f[i], load_el(agg_v + i)};
        agg_f[i] = run.f;
        store_el(agg_v + i, run.v);
        run = seg_join(run, v);
    }
}

// w[nWires + q] = the sum of gate q's chain up to q
__global__ __launch_bounds__(WG) void k_ext_apply(Fr *w, const uint32_t *agg_f, const Fr *agg_v, Ext E) {
    __shared__ uint32_t lf[WG];
    __shared__ Fr lv[WG];
    const uint64_t at = ((uint64_t)blockIdx.x * WG + threadIdx.x) * E.seg;
    Seg total;
    const Seg ex = block_seg_scan(ext_lane(E, w, at), total, lf, lv);
    Seg run = seg_join(Seg{agg_f[blockIdx.x], load_el(agg_v + blockIdx.x)}, ex);
#pragma unroll 1
    for (uint32_t k = 0; k < E.seg && at + k < E.n_add; k++) {
        run = seg_join(run, ext_element(E, w, at + k));
        store_el(w + E.nWires + at + k, run.v);
    }
}

// ---------------------------------------------------------------- host
uint64_t scan_blocks(uint64_t len, uint32_t seg) { return (len + (uint64_t)WG * seg - 1) / ((uint64_t)WG * seg); }

// x[0, len] <- the exclusive sums of x[0, len) and, at x[len], their total: three launches
void scan_u32(uint32_t *x, uint64_t len, uint32_t seg, DevBuf<uint32_t> &sums, hipStream_t s) {
    if (!len) {
        HIP_TRY(hipMemsetAsync(x, 0, 4, s));
        return;
    }
    const uint64_t nb = scan_blocks(len, seg);
    if (nb >= (1ull << 31)) throw std::invalid_argument("zk_plonk_r1cs: too many elements for ZKHIP_R1CS_SEG");
    if (sums.n < nb) sums.alloc(nb);
    ZK_LAUNCH(k_u32_scan_reduce, dim3((uint32_t)nb), dim3(WG), 0, s, sums.p, x, len, seg);
    ZK_LAUNCH(k_u32_scan_carry, dim3(1), dim3(WG), 0, s, sums.p, nb, x + len);
    ZK_LAUNCH(k_u32_scan_apply, dim3((uint32_t)nb), dim3(WG), 0, s, x, sums.p, len, seg);
    ZK_LAUNCH_OK("r1cs integer scan");
}

uint32_t bits_of(uint64_t count) {                    // of the largest index below count
    uint32_t b = 0;
    while (b < 64 && (count - 1) >> b) b++;
    return count <= 1 ? 0 : b;
}

}   // namespace

// ---------------------------------------------------------------- the object
struct zk_plonk_r1cs {
    int device = 0;
    uint32_t log_n = 0, nWires = 0, nPublic = 0, m = 0, passes = 0, last_launches = 0;
    uint64_t n = 0, rows = 0, n_add = 0, n_witness = 0, terms = 0;
    uint8_t k1[32], k2[32];
    std::mutex mu;                                    // calls on one object are serialised
    std::unique_ptr<Stream> st;
    DevBuf<Fr> vec;                                   // ql qr qm qo qc s1 s2 s3 by values, n rows each
    DevBuf<uint32_t> maps;                            // a | b | c, n rows each
    DevBuf<uint32_t> xw, hw, agg_f;
    DevBuf<Fr> xc, hc, agg_v, wit;                    // wit: zk_plonk_r1cs_extend's own witness, made by its first call
    DevBuf<uint8_t> xstart;
    size_t bytes() const {
        return vec.bytes() + maps.bytes() + xw.bytes() + hw.bytes() + agg_f.bytes() + xc.bytes() + hc.bytes() + agg_v.bytes() + wit.bytes() + xstart.bytes();
    }
    Ext ext(uint32_t seg) const { return Ext{xw.p, hw.p, xc.p, hc.p, xstart.p, n_add, nWires, seg}; }
};

namespace {

// t_L of every LC on the host, for the circuits whose upper bound from the term counts passes a limit
uint64_t exact_additions(const zk_r1cs_view *v, const std::vector<uint64_t> &lc_off) {
    const uint32_t *sec = static_cast<const uint32_t *>(v->constraints);
    uint64_t adds = 0;
    for (uint64_t row = 0; row < lc_off.size(); row++) {
        const uint32_t *lc = sec + lc_off[row];
        uint64_t t = 0;
        for (uint32_t i = 0; i < lc[0]; i++) {
            const uint32_t *p = lc + 1 + 9 * (uint64_t)i;
            bool kept = false;
            for (int j = 1; j <= 8; j++) kept |= p[j] != 0;
            t += kept && p[0] != 0;
        }
        adds += t ? t - 1 : 0;
    }
    return adds;
}

zk_plonk_r1cs *r1cs_compile(const zk_r1cs_view *v, const uint8_t *k1, const uint8_t *k2, int32_t device) {
    const char *who = "zk_plonk_r1cs_create";
    if (!v || !k1 || !k2) throw std::invalid_argument("null argument");
    if (v->nConstraints && !v->constraints) throw std::invalid_argument("null constraints section");
    const Fr K1 = checked_scalar(k1, std::string(who) + ": k1"), K2 = checked_scalar(k2, std::string(who) + ": k2");
    const uint32_t seg = seg_in_effect();
    std::vector<uint64_t> lc_off, rowptr;
    walk_constraints(v, lc_off, rowptr);
    const uint64_t m = v->nConstraints, nnz = rowptr.back(), nPublic = (uint64_t)v->nPubOut + v->nPubIn;
    if (3 * m >= (1ull << 31)) throw std::invalid_argument(std::string(who) + ": the r1cs has too many constraints");
    if (nnz >= (1ull << 32) - 1) throw std::invalid_argument(std::string(who) + ": the r1cs has 2^32 - 1 terms or more");
    if (!v->nWires) throw std::invalid_argument(std::string(who) + ": nWires is 0: wire 0 is the constant");
    if (nPublic >= v->nWires) throw std::invalid_argument(std::string(who) + ": nPublic " + std::to_string(nPublic) + " is not below nWires = " + std::to_string(v->nWires));
    // the limits: an upper bound from the term counts first, the exact count on the host only where that passes a limit
    uint64_t bound = 0;
    for (uint64_t row = 0; row < 3 * m; row++) bound += rowptr[row + 1] - rowptr[row] ? rowptr[row + 1] - rowptr[row] - 1 : 0;
    constexpr uint64_t MAX_ROWS = 1ull << MAX_LOG_N;
    if (nPublic + m + bound > MAX_ROWS || v->nWires + bound >= (1ull << 32)) bound = exact_additions(v, lc_off);
    if (nPublic + m + bound > MAX_ROWS)
        throw std::invalid_argument(std::string(who) + ": N = " + std::to_string(nPublic + m + bound) + " rows exceed 2^25");
    if (v->nWires + bound >= (1ull << 32)) throw std::invalid_argument(std::string(who) + ": n_witness = " + std::to_string(v->nWires + bound) + " is not below 2^32");
    // 1, k1, k2 in three cosets of the n-th roots, for every n the bound allows (k^n = 1 for a smaller n gives 1 for a larger)
    {
        uint32_t lg = MIN_LOG_N;
        while ((1ull << lg) < nPublic + m + bound) lg++;
        if (K1.is_zero() || K2.is_zero()) throw std::invalid_argument(std::string(who) + ": k1 or k2 is zero");
        Fr a = K1, b = K2, c = Fr::mul(K1, Fr::inv(K2));
        for (uint32_t i = 0; i < lg; i++) a = Fr::sqr(a), b = Fr::sqr(b), c = Fr::sqr(c);
        if (a == Fr::one() || b == Fr::one() || c == Fr::one())
            throw std::invalid_argument(std::string(who) + ": 1, k1 and k2 do not name three different cosets of the n-th roots of unity");
    }

    const int dev = resolve_device(device);
    DeviceGuard dg(dev);
    std::unique_ptr<zk_plonk_r1cs> c(new zk_plonk_r1cs());
    c->device = dev, c->nWires = v->nWires, c->nPublic = (uint32_t)nPublic, c->m = (uint32_t)m, c->terms = nnz;
    memcpy(c->k1, k1, 32);
    memcpy(c->k2, k2, 32);
    need_hbm(who, v->constraints_bytes + (6 * m + 1) * 8 + (nnz + 1 + 10 * m) * 4 + (nPublic + m + bound) * 2 * (8 * 32 + 3 * 4 + 4 * 4) + bound * 80 +
                      (uint64_t)v->nWires * 4);
    c->st.reset(new Stream());
    hipStream_t s = c->st->s;
    const uint64_t at = launches_now();

    SectionOnDevice sec;
    DevBuf<uint32_t> pos, w0cnt, w0term, first, adds, err2, sums;
    sec.upload(v, lc_off, rowptr, s);
    pos.alloc(nnz + 1);
    w0cnt.alloc(3 * m + 1), w0term.alloc(3 * m + 1), first.alloc(3 * m + 1), adds.alloc(m + 1), err2.alloc(1);
    HIP_TRY(hipMemsetAsync(w0cnt.p, 0, w0cnt.bytes(), s));
    HIP_TRY(hipMemsetAsync(err2.p, 0xFF, 4, s));
    Section S{sec.sec(), sec.d_off.p, sec.d_ptr.p, (uint32_t)(3 * m), (uint32_t)m, v->nWires, (uint32_t)nPublic, nnz};
    const uint32_t term_grid = nnz < (uint64_t)WG * 8192 ? nblocks(nnz, WG) : 8192;
    if (nnz) {
        ZK_LAUNCH(k_r1cs_flags, dim3(term_grid), dim3(WG), 0, s, pos.p, w0cnt.p, w0term.p, sec.err.p, err2.p, S);
        ZK_LAUNCH_OK("r1cs flags");
    }
    scan_u32(pos.p, nnz, seg, sums, s);
    if (m) {
        ZK_LAUNCH(k_r1cs_additions, dim3(nblocks(m, WG)), dim3(WG), 0, s, adds.p, pos.p, sec.d_ptr.p, (uint32_t)m);
        ZK_LAUNCH_OK("r1cs additions");
    }
    scan_u32(adds.p, m, seg, sums, s);
    uint32_t n_add = 0, twice = NONE;
    HIP_TRY(hipMemcpyAsync(&n_add, adds.p + m, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&twice, err2.p, 4, hipMemcpyDeviceToHost, s));
    sec.check(s);                                      // drains the stream; a wire id or a coefficient out of range
    if (twice != NONE)
        throw std::invalid_argument(std::string(who) + ": constraint " + std::to_string(twice / 3) + ": " + "ABC"[twice % 3] + " names wire 0 twice");

    const uint64_t N = nPublic + m + n_add;
    uint32_t log_n = MIN_LOG_N;
    while ((1ull << log_n) < N) log_n++;
    const uint64_t n = 1ull << log_n, cells = 3 * n;
    c->rows = N, c->log_n = log_n, c->n = n, c->n_add = n_add, c->n_witness = (uint64_t)v->nWires + n_add;
    c->vec.alloc(8 * n);
    c->maps.alloc(3 * n);
    const uint64_t ext_rows = n_add ? n_add : 1;
    c->xw.alloc(ext_rows), c->hw.alloc(ext_rows), c->xc.alloc(ext_rows), c->hc.alloc(ext_rows), c->xstart.alloc(ext_rows);
    HIP_TRY(hipMemsetAsync(c->vec.p, 0, 5 * n * sizeof(Fr), s));
    HIP_TRY(hipMemsetAsync(c->maps.p, 0, c->maps.bytes(), s));
    HIP_TRY(hipMemsetAsync(c->hw.p, 0, c->hw.bytes(), s));
    HIP_TRY(hipMemsetAsync(c->hc.p, 0, c->hc.bytes(), s));
    Fr *q = c->vec.p;
    Circuit C{q, q + n, q + 2 * n, q + 3 * n, q + 4 * n, c->maps.p, c->maps.p + n, c->maps.p + 2 * n, c->xw.p, c->hw.p, c->xc.p, c->hc.p, c->xstart.p};
    if (nPublic) ZK_LAUNCH(k_r1cs_public, dim3(nblocks(nPublic, WG)), dim3(WG), 0, s, C, (uint32_t)nPublic);
    if (nnz) ZK_LAUNCH(k_r1cs_emit_terms, dim3(term_grid), dim3(WG), 0, s, C, first.p, pos.p, adds.p, S);
    if (m) ZK_LAUNCH(k_r1cs_emit_final, dim3(nblocks(m, WG)), dim3(WG), 0, s, C, first.p, w0cnt.p, w0term.p, pos.p, adds.p, S);
    ZK_LAUNCH_OK("r1cs gates");

    // the cells by wire: keys of pass 0 are the maps themselves (cell = col n + row is their index)
    const uint32_t passes = (bits_of(c->n_witness) + RADIX_BITS - 1) / RADIX_BITS, tiles = nblocks(cells, TILE);
    c->passes = passes;
    DevBuf<uint32_t> key[2], cell[2], hist, headcell;
    cell[0].alloc(cells);
    if (passes) key[1].alloc(cells), cell[1].alloc(cells), hist.alloc((uint64_t)RADIX * tiles + 1);
    if (passes > 1) key[0].alloc(cells);
    headcell.alloc(c->n_witness);
    ZK_LAUNCH(k_cell_init, dim3(nblocks(cells, WG)), dim3(WG), 0, s, cell[0].p, cells);
    const uint32_t *keys = c->maps.p;
    uint32_t cur = 0;
    for (uint32_t pass = 0; pass < passes; pass++, cur ^= 1) {
        const uint32_t shift = pass * RADIX_BITS;
        ZK_LAUNCH(k_cell_hist, dim3(tiles), dim3(WG), 0, s, hist.p, keys, cells, shift, tiles);
        scan_u32(hist.p, (uint64_t)RADIX * tiles, seg, sums, s);
        ZK_LAUNCH(k_cell_scatter, dim3(tiles), dim3(WG), 0, s, key[cur ^ 1].p, cell[cur ^ 1].p, keys, cell[cur].p, hist.p, cells, shift, tiles);
        ZK_LAUNCH_OK("cell sort");
        keys = key[cur ^ 1].p;
    }
    // w^(2^i) and the shifts
    DevBuf<Fr> tab;
    tab.alloc(POW_BITS + 3);
    std::vector<Fr> h(POW_BITS + 3);
    h[0] = root_of_unity(log_n);
    for (uint32_t i = 1; i < POW_BITS; i++) h[i] = Fr::sqr(h[i - 1]);
    h[POW_BITS] = Fr::one(), h[POW_BITS + 1] = K1, h[POW_BITS + 2] = K2;
    HIP_TRY(hipMemcpyAsync(tab.p, h.data(), h.size() * sizeof(Fr), hipMemcpyHostToDevice, s));
    ZK_LAUNCH(k_sigma_heads, dim3(nblocks(cells, WG)), dim3(WG), 0, s, headcell.p, keys, cell[cur].p, cells);
    ZK_LAUNCH(k_sigma_write, dim3(nblocks(cells, WG)), dim3(WG), 0, s, c->vec.p + 5 * n, headcell.p, keys, cell[cur].p, cells, log_n, tab.p);
    ZK_LAUNCH_OK("sigma");
    HIP_TRY(hipStreamSynchronize(s));
    c->last_launches = (uint32_t)(launches_now() - at);
    return c.release();
}

}   // namespace

// ---------------------------------------------------------------- what plonkprove.hip takes (plonk_internal.hpp)
PlonkR1csDims plonk_r1cs_dims(const zk_plonk_r1cs *c) {
    return PlonkR1csDims{c->device, c->log_n, c->n, c->nWires, c->nPublic, c->n_witness, c->k1, c->k2};
}

// the caller holds c->mu
static void extend_locked(zk_plonk_r1cs *c, Fr *w, hipStream_t s, uint32_t seg) {
    const uint64_t at = launches_now();
    if (c->n_add) {
        const uint64_t nb = scan_blocks(c->n_add, seg);
        if (c->agg_f.n < nb) c->agg_f.alloc(nb), c->agg_v.alloc(nb);
        const Ext E = c->ext(seg);
        ZK_LAUNCH(k_ext_reduce, dim3((uint32_t)nb), dim3(WG), 0, s, c->agg_f.p, c->agg_v.p, E, (const Fr *)w);
        ZK_LAUNCH(k_ext_carry, dim3(1), dim3(WG), 0, s, c->agg_f.p, c->agg_v.p, nb);
        ZK_LAUNCH(k_ext_apply, dim3((uint32_t)nb), dim3(WG), 0, s, w, c->agg_f.p, c->agg_v.p, E);
        ZK_LAUNCH_OK("witness extension");
    }
    c->last_launches = (uint32_t)(launches_now() - at);
}

void plonk_r1cs_extend_dev(zk_plonk_r1cs *c, Fr *w, hipStream_t s) {
    const uint32_t seg = seg_in_effect();
    std::lock_guard<std::mutex> lock(c->mu);
    extend_locked(c, w, s, seg);
    HIP_TRY(hipStreamSynchronize(s));                  // the work buffers are the object's: free for its next caller
}

void plonk_r1cs_check_witness(const zk_plonk_r1cs *c, const char *who, const uint8_t *wtns, uint32_t nVars) {
    if (nVars != c->nWires) throw std::invalid_argument("witness has " + std::to_string(nVars) + " values, the r1cs " + std::to_string(c->nWires) + " wires");
    const uint64_t bad = first_not_below_r(wtns, nVars);
    if (bad < nVars) throw std::invalid_argument(std::string(who) + ": witness " + std::to_string(bad) + " is not below r");
}

extern "C" {

int zk_plonk_r1cs_create(zk_plonk_r1cs **out, const zk_r1cs_view *view, const uint8_t k1[32], const uint8_t k2[32], int32_t device) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        *out = r1cs_compile(view, k1, k2, device);
    });
}

void zk_plonk_r1cs_destroy(zk_plonk_r1cs *c) { destroy_on_device(c); }

int zk_plonk_r1cs_info(zk_plonk_r1cs *c, zk_plonk_r1cs_plan *plan) {
    return guarded([&] {
        if (!c || !plan) throw std::invalid_argument("null argument");
        info_into("zk_plonk_r1cs_info", plan, [&](zk_plonk_r1cs_plan &q) {
            q.seg = seg_in_effect();
            std::lock_guard<std::mutex> lock(c->mu);
            q.log_n = c->log_n, q.rows = c->rows, q.n_public = c->nPublic, q.n_wires = c->nWires, q.n_additions = c->n_add, q.n_witness = c->n_witness;
            q.terms = c->terms, q.device_bytes = c->bytes(), q.sort_passes = c->passes, q.last_launches = c->last_launches;
        });
    });
}

int zk_plonk_r1cs_circuit(zk_plonk_r1cs *c, uint8_t *vectors, uint32_t *a_map, uint32_t *b_map, uint32_t *c_map) {
    return guarded([&] {
        if (!c || !vectors || !a_map || !b_map || !c_map) throw std::invalid_argument("null argument");
        std::lock_guard<std::mutex> lock(c->mu);
        DeviceGuard dg(c->device);
        hipStream_t s = c->st->s;
        uint32_t *maps[3] = {a_map, b_map, c_map};
        HIP_TRY(hipMemcpyAsync(vectors, c->vec.p, c->vec.bytes(), hipMemcpyDeviceToHost, s));
        for (int j = 0; j < 3; j++) HIP_TRY(hipMemcpyAsync(maps[j], c->maps.p + j * c->n, c->n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    });
}

int zk_plonk_r1cs_extend(zk_plonk_r1cs *c, uint8_t *out, const uint8_t *wtns, uint32_t nVars) {
    return guarded([&] {
        if (!c || !out || (nVars && !wtns)) throw std::invalid_argument("null argument");
        plonk_r1cs_check_witness(c, "zk_plonk_r1cs_extend", wtns, nVars);
        const uint32_t seg = seg_in_effect();
        std::lock_guard<std::mutex> lock(c->mu);
        DeviceGuard dg(c->device);
        hipStream_t s = c->st->s;
        if (!c->wit.p) c->wit.alloc(c->n_witness);
        HIP_TRY(hipMemcpyAsync(c->wit.p, wtns, (size_t)nVars * sizeof(Fr), hipMemcpyHostToDevice, s));
        extend_locked(c, c->wit.p, s, seg);
        HIP_TRY(hipMemcpyAsync(out, c->wit.p, c->n_witness * sizeof(Fr), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    });
}

}   // extern "C"
