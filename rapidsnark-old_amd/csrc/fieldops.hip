// Pointwise Fr/Fq kernels and the sparse A.w / B.w accumulation (src/groth16.cpp:56-96).
#include "common.hpp"
#include "kernels.hpp"
#include "hipcheck.hpp"
#include "field29.hpp"
#include "devmem.hpp"

namespace zk {

template <class F>
__global__ __launch_bounds__(256) void k_mul_vec(F *out, const F *a, const F *b, uint64_t n) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        store_el(out + i, F::mul(load_el(a + i), load_el(b + i)));
}

static inline uint32_t grid_for(uint64_t n, uint32_t block, uint32_t cap = 256 * 8) {
    uint64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    return (uint32_t)(g > cap ? cap : g);
}

void launch_fr_mul_vec(Fr *out, const Fr *a, const Fr *b, uint64_t n, hipStream_t s) {
    ZK_LAUNCH(k_mul_vec<Fr>, dim3(grid_for(n, 256)), dim3(256), 0, s, out, a, b, n);
    ZK_LAUNCH_OK("fr_mul_vec");
}
void launch_fq_mul_vec(Fq *out, const Fq *a, const Fq *b, uint64_t n, hipStream_t s) {
    ZK_LAUNCH(k_mul_vec<Fq>, dim3(grid_for(n, 256)), dim3(256), 0, s, out, a, b, n);
    ZK_LAUNCH_OK("fq_mul_vec");
}

// the sum of one CSR row's terms [lo, hi) on one lane, in (-r, r): the loop k_spmv_abc and k_spmv_abc_long share
__device__ __forceinline__ Fr29 spmv_row(const CsrDev &csr, const Fr *wtns, uint32_t lo, uint32_t hi) {
    Fr29 sum = Fr29::zero();
    uint32_t pending = 0;
    for (uint32_t k = lo; k < hi; k++) {
        Fr29 w = Fr29::load(load_el(wtns + csr.col[k]));       // standard form, < r for well-formed files
        Fr29 v = Fr29::load(load_el(csr.val + k));             // value * 2^522 (pre-scaled at create)
        sum = Fr29::add(sum, Fr29::mul(w, v));                 // += w*value * 2^261
        if (++pending == 8) {                                  // long rows: keep the lazy sum small
            sum = Fr29::reduce_near_zero(sum);
            pending = 0;
        }
    }
    return Fr29::reduce_near_zero(sum);
}

// One lane per domain row i: a[i] = sum_A coef*w[s], b[i] = sum_B coef*w[s], c[i] = a[i]*b[i].
// The reference does this with 1024 striped omp locks (src/groth16.cpp:63-84); a row-sorted
// CSR built once at create time needs neither locks nor atomics.  The zkey stores
// value*2^512; create rescales it to value*2^522 so that one 2^-261 Montgomery product with
// the standard-form witness gives w*value in this library's 2^261 form (field29.hpp).
// blockIdx.y = vector of a batched submission: its witness at wtns + y * wtns_stride, its a|b|c at + y * abc_stride
// A lane runs as long as its row: right for the rows of at most a few terms that most constraints have, and the only
// kernel of a key without a row above the cut (csr.chunks == 0).  A key WITH such rows goes through k_spmv_chunks,
// k_spmv_long_rows and k_spmv_abc_long below instead; this kernel is not part of that path.
__global__ __launch_bounds__(256) void k_spmv_abc(Fr *a, Fr *b, Fr *c, CsrDev csr, const Fr *wtns, uint32_t n, uint64_t abc_stride, uint64_t wtns_stride) {
    ZK_CHAIN_PRIO();
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    a += (uint64_t)blockIdx.y * abc_stride;
    b += (uint64_t)blockIdx.y * abc_stride;
    c += (uint64_t)blockIdx.y * abc_stride;
    wtns += (uint64_t)blockIdx.y * wtns_stride;
    Fr29 acc[2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
        uint32_t row = i + (m ? n : 0);
        acc[m] = spmv_row(csr, wtns, csr.rowptr[row], csr.rowptr[row + 1]);
    }
    store_el(a + i, Fr29::store(acc[0]));
    store_el(b + i, Fr29::store(acc[1]));
    store_el(c + i, Fr29::store(Fr29::mul(acc[0], acc[1])));
}

// ---- Rows of more than csr.cut terms.  Such a row is cut into chunks of at most SPMV_CHUNK
// terms at create time (k_csr_long_*: below); a wave sums a chunk, a wave sums a row's partials, and the lane that owns
// the row in k_spmv_abc_long picks the finished value up.  Time grows with the number of terms, not with the longest row;
// field addition is exact, so the values are those of k_spmv_abc whatever the cut, and no step needs an atomic.
//
// Operand ranges (field29.hpp: an operand may lie anywhere in (-16r, 16r); a product lands in (-r, 2r),
// reduce_near_zero returns (-r, r), a stored partial is canonical, [0, r)).  A lane starts at 0 and reduces after every
// SPMV_LAZY = 7 additions: its running sum stays in (-r, r) + 7 (-r, 2r) = (-8r, 15r) (csrc/r1cs.hip has the same
// derivation), and it leaves the loop through one more reduce_near_zero: (-r, r).  The wave sum is six exchange-and-add
// steps, each of which doubles the bound: (-2r, 2r), (-4r, 4r), (-8r, 8r) after the third - a fourth would only touch
// (-16r, 16r), a fifth leave it - so the sum is reduced to (-r, r) there and the last three steps end in (-8r, 8r),
// which canonical() (Fr29::store) accepts.
constexpr uint32_t SPMV_LAZY = 7;
constexpr uint32_t SPMV_CHUNK = 64 * SPMV_LANE_TERMS;      // terms of one chunk: a wave, SPMV_LANE_TERMS per lane

// the sum of the wave's 64 values, each in (-r, r), in every lane: in (-8r, 8r)
__device__ __forceinline__ Fr29 spmv_wave_sum(Fr29 x) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        Fr29 o;
#pragma unroll
        for (int j = 0; j < 9; j++) o.l[j] = __shfl_xor(x.l[j], off);
        x = Fr29::add(x, o);
        if (off == 4) x = Fr29::reduce_near_zero(x);
    }
    return x;
}
// lane l of the wave sums inputs first + l, first + l + 64, ... below first + count (adjacent lanes read adjacent
// col / val / partial entries): the terms' products, or partials
template <bool TERMS>
__device__ __forceinline__ Fr29 spmv_lane_sum(const CsrDev &csr, const Fr *in, uint32_t first, uint32_t count) {
    Fr29 sum = Fr29::zero();
    uint32_t pending = 0;
    for (uint32_t t = threadIdx.x & 63; t < count; t += 64) {
        const uint32_t k = first + t;
        const Fr29 x = TERMS ? Fr29::mul(Fr29::load(load_el(in + csr.col[k])), Fr29::load(load_el(csr.val + k))) : Fr29::load(load_el(in + k));
        sum = Fr29::add(sum, x);
        if (++pending == SPMV_LAZY) {
            sum = Fr29::reduce_near_zero(sum);
            pending = 0;
        }
    }
    return Fr29::reduce_near_zero(sum);
}
// stage 1, one wave per chunk descriptor {row, first term, terms, partial slot}: part[slot] = the chunk's sum, canonical.
// blockIdx.y = vector of a batch: its own witness and its own csr.chunks partials.
__global__ __launch_bounds__(256) void k_spmv_chunks(Fr *part, CsrDev csr, const Fr *wtns, uint64_t wtns_stride) {
    ZK_CHAIN_PRIO();
    const uint32_t ch = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ch >= csr.chunks) return;
    const uint4 d = csr.chunk_desc[ch];
    const Fr29 sum = spmv_wave_sum(spmv_lane_sum<true>(csr, wtns + (uint64_t)blockIdx.y * wtns_stride, d.y, d.z));
    if ((threadIdx.x & 63) == 0) store_el(part + (uint64_t)blockIdx.y * csr.chunks + d.w, Fr29::store(sum));
}
// stage 2, one wave per long row {row, first partial slot, partials, -}: the row's value into a[i] (row < n) or b[i - n]
__global__ __launch_bounds__(256) void k_spmv_long_rows(Fr *a, Fr *b, const Fr *part, CsrDev csr, uint32_t n, uint64_t abc_stride) {
    ZK_CHAIN_PRIO();
    const uint32_t lr = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (lr >= csr.long_rows) return;
    const uint4 d = csr.long_desc[lr];
    const Fr29 sum = spmv_wave_sum(spmv_lane_sum<false>(csr, part + (uint64_t)blockIdx.y * csr.chunks, d.y, d.z));
    Fr *out = (d.x < n ? a + d.x : b + (d.x - n)) + (uint64_t)blockIdx.y * abc_stride;
    if ((threadIdx.x & 63) == 0) store_el(out, Fr29::store(sum));
}
// k_spmv_abc for a key with long rows: a row above the cut is not walked, its value is what stage 2 left in a[i] / b[i]
__global__ __launch_bounds__(256) void k_spmv_abc_long(Fr *a, Fr *b, Fr *c, CsrDev csr, const Fr *wtns, uint32_t n, uint64_t abc_stride, uint64_t wtns_stride) {
    ZK_CHAIN_PRIO();
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    a += (uint64_t)blockIdx.y * abc_stride;
    b += (uint64_t)blockIdx.y * abc_stride;
    c += (uint64_t)blockIdx.y * abc_stride;
    wtns += (uint64_t)blockIdx.y * wtns_stride;
    Fr29 acc[2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
        uint32_t row = i + (m ? n : 0);
        uint32_t lo = csr.rowptr[row], hi = csr.rowptr[row + 1];
        acc[m] = hi - lo > csr.cut ? Fr29::load(load_el((m ? b : a) + i)) : spmv_row(csr, wtns, lo, hi);
    }
    store_el(a + i, Fr29::store(acc[0]));
    store_el(b + i, Fr29::store(acc[1]));
    store_el(c + i, Fr29::store(Fr29::mul(acc[0], acc[1])));
}

void launch_spmv_abc(Fr *a, Fr *b, Fr *c, CsrDev csr, const Fr *wtns, uint32_t n, hipStream_t s, uint32_t vectors, uint64_t abc_stride, uint64_t wtns_stride,
                     Fr *partials) {
    const uint32_t v = vectors ? vectors : 1;
    if (!csr.chunks) {
        ZK_LAUNCH(k_spmv_abc, dim3((n + 255) / 256, v), dim3(256), 0, s, a, b, c, csr, wtns, n, abc_stride, wtns_stride);
        ZK_LAUNCH_OK("spmv_abc");
        return;
    }
    if (!partials) throw std::invalid_argument("spmv: a key with long rows needs a partial buffer");
    ZK_LAUNCH(k_spmv_chunks, dim3((csr.chunks + 3) / 4, v), dim3(256), 0, s, partials, csr, wtns, wtns_stride);
    ZK_LAUNCH(k_spmv_long_rows, dim3((csr.long_rows + 3) / 4, v), dim3(256), 0, s, a, b, partials, csr, n, abc_stride);
    ZK_LAUNCH(k_spmv_abc_long, dim3((n + 255) / 256, v), dim3(256), 0, s, a, b, c, csr, wtns, n, abc_stride, wtns_stride);
    ZK_LAUNCH_OK("spmv_abc (long rows)");
}

// ---- CSR build on the device (the reference has no such step: it walks the records under 1024
// striped locks on every proof, src/groth16.cpp:63-84).  Records are 44-byte packed, 4-byte aligned.
// Rows outside [row_lo, row_hi) are skipped (a prover that holds one block of a partitioned chain keeps
// only its rows); the range check covers every record either way.  Local row = c - row_lo, rows of
// matrix B follow the nl = row_hi - row_lo rows of matrix A.
__global__ __launch_bounds__(256) void k_csr_count(uint32_t *rowcount, uint32_t *err, const uint32_t *rec, uint64_t nCoefs, uint32_t n,
                                                   uint32_t nVars, uint32_t row_lo, uint32_t row_hi) {
    uint64_t st = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t nl = row_hi - row_lo;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nCoefs; i += st) {
        const uint32_t *r = rec + i * 11;
        const uint32_t m = r[0] ? 1u : 0u, c = r[1], sg = r[2];      // the reference: (coefs[i].m == 0) ? a : b  (groth16.cpp:69)
        if (c >= n || sg >= nVars) {
            atomicOr(err, 1u);
            continue;
        }
        if (c < row_lo || c >= row_hi) continue;
        atomicAdd(&rowcount[(uint64_t)m * nl + (c - row_lo)], 1u);
    }
}
// The order of a row's terms depends on atomic arbitration; their (exact, modular) sum does not.
__global__ __launch_bounds__(256) void k_csr_fill(uint32_t *col, Fr *val, uint32_t *cursor, const uint32_t *rec, uint64_t nCoefs, uint32_t n,
                                                  uint32_t nVars, uint32_t row_lo, uint32_t row_hi) {
    uint64_t st = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t nl = row_hi - row_lo;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nCoefs; i += st) {
        const uint32_t *r = rec + i * 11;
        const uint32_t m = r[0] ? 1u : 0u, c = r[1], sg = r[2];
        if (c >= n || sg >= nVars || c < row_lo || c >= row_hi) continue;
        uint32_t pos = atomicAdd(&cursor[(uint64_t)m * nl + (c - row_lo)], 1u);
        col[pos] = sg;
        Fr v;
#pragma unroll
        for (int j = 0; j < 8; j++) v.v[j] = r[3 + j];
        store_el(val + pos, v);
    }
}

// Rows above the cut: how many, the chunks they need, and the longest row of all (one pass over rowptr; a wave adds its
// counts up before its one lane touches the three words)
__global__ __launch_bounds__(256) void k_csr_long_stats(uint32_t *stats, const uint32_t *rowptr, uint32_t rows, uint32_t cut) {
    uint32_t nlong = 0, nch = 0, longest = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) {
        const uint32_t len = rowptr[r + 1] - rowptr[r];
        longest = len > longest ? len : longest;
        if (cut && len > cut) {
            nlong++;
            nch += (len + SPMV_CHUNK - 1) / SPMV_CHUNK;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        nlong += __shfl_xor(nlong, off);
        nch += __shfl_xor(nch, off);
        const uint32_t o = __shfl_xor(longest, off);
        longest = o > longest ? o : longest;
    }
    if ((threadIdx.x & 63) == 0) {
        if (nlong) {
            atomicAdd(&stats[0], nlong);
            atomicAdd(&stats[1], nch);
        }
        if (longest) atomicMax(&stats[2], longest);
    }
}
// one lane per row; a long row takes a run of partial slots and an entry of the long-row list (which run and which entry
// depends on atomic arbitration; the sums do not)
__global__ __launch_bounds__(256) void k_csr_long_list(uint4 *long_desc, uint32_t *counters, const uint32_t *rowptr, uint32_t rows, uint32_t cut,
                                                       uint32_t long_rows, uint32_t chunks) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) {
        const uint32_t lo = rowptr[r], len = rowptr[r + 1] - lo;
        if (len <= cut) continue;
        const uint32_t nch = (len + SPMV_CHUNK - 1) / SPMV_CHUNK;
        const uint32_t slot = atomicAdd(&counters[0], nch), at = atomicAdd(&counters[1], 1u);
        if (at < long_rows && slot + nch <= chunks) long_desc[at] = make_uint4(r, slot, nch, lo);
    }
}
// one workgroup per long row: its chunk descriptors {row, first term, terms, partial slot}
__global__ __launch_bounds__(256) void k_csr_long_chunks(uint4 *chunk_desc, const uint4 *long_desc, const uint32_t *rowptr) {
    const uint4 d = long_desc[blockIdx.x];
    const uint32_t hi = rowptr[d.x + 1];
    for (uint32_t j = threadIdx.x; j < d.z; j += blockDim.x) {
        const uint32_t first = d.w + j * SPMV_CHUNK;
        chunk_desc[d.y + j] = make_uint4(d.x, first, hi - first < SPMV_CHUNK ? hi - first : SPMV_CHUNK, d.y + j);
    }
}

void launch_csr_build(uint32_t *rowptr, uint32_t *col, Fr *val, uint32_t *cursor, uint32_t *err, const uint8_t *records,
                      uint64_t nCoefs, uint32_t n, uint32_t nVars, uint32_t row_lo, uint32_t row_hi, uint32_t row_cut, hipStream_t s) {
    const uint32_t rows = 2 * (row_hi - row_lo);
    ZK_HIP(hipMemsetAsync(cursor, 0, (size_t)rows * 4, s));
    ZK_HIP(hipMemsetAsync(err, 0, 16, s));
    const uint32_t g = grid_for(nCoefs ? nCoefs : 1, 256, 256 * 16);
    ZK_LAUNCH(k_csr_count, dim3(g), dim3(256), 0, s, cursor, err, (const uint32_t *)records, nCoefs, n, nVars, row_lo, row_hi);
    launch_exclusive_scan_u32(rowptr, cursor, rows, s);
    ZK_HIP(hipMemcpyAsync(cursor, rowptr, (size_t)rows * 4, hipMemcpyDeviceToDevice, s));
    ZK_LAUNCH(k_csr_fill, dim3(g), dim3(256), 0, s, col, val, cursor, (const uint32_t *)records, nCoefs, n, nVars, row_lo, row_hi);
    ZK_LAUNCH(k_csr_long_stats, dim3(grid_for(rows, 256)), dim3(256), 0, s, err + 1, rowptr, rows, row_cut);
    ZK_LAUNCH_OK("csr build");
}

void launch_csr_long_rows(uint4 *long_desc, uint4 *chunk_desc, uint32_t *counters, const uint32_t *rowptr, uint32_t rows, uint32_t row_cut,
                          uint32_t long_rows, uint32_t chunks, hipStream_t s) {
    ZK_HIP(hipMemsetAsync(counters, 0, 8, s));
    ZK_LAUNCH(k_csr_long_list, dim3(grid_for(rows, 256)), dim3(256), 0, s, long_desc, counters, rowptr, rows, row_cut, long_rows, chunks);
    ZK_LAUNCH(k_csr_long_chunks, dim3(long_rows), dim3(256), 0, s, chunk_desc, long_desc, rowptr);
    ZK_LAUNCH_OK("csr long rows");
}

// ZKHIP_SPMV_ROW_CUT, read at every call: 0 = no row is long, n >= 1 = rows of more than n terms
uint32_t spmv_row_cut() {
    const char *e = getenv("ZKHIP_SPMV_ROW_CUT");
    if (!e || !*e) return SPMV_ROW_CUT;
    const long long v = atoll(e);
    return v <= 0 ? 0u : v > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)v;
}

}   // namespace zk
