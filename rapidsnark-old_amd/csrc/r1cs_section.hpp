// The constraints section of a circom .r1cs on the device, shared by r1cs.hip (witness check) and setup.hip (Groth16
// setup).  The section is uploaded as it is in the file together with the word offset of every linear combination and
// the row offsets of their terms (walk_constraints: one host pass over the term counts); each file's own decode kernel
// then runs one lane per term through term_at() and writes what it needs.  Also here: the segment plan of the
// cut-into-segments sums both files run over rows of any length (r1cs.hip defines the walk and the plan).
#pragma once
#include <memory>
#include <vector>
#include "hiputil.hpp"

namespace zkp {

// w >= r (BN254 scalar field), 256-bit words little-endian
__device__ __forceinline__ bool ge_r(const uint32_t *w) {
#pragma unroll
    for (int i = 7; i >= 0; i--)
        if (w[i] != FrParams::P[i]) return w[i] > FrParams::P[i];
    return true;
}

// Term t of the section -> its row and the pointer to its 9 words (wire id, 8 coefficient words).  rowptr is ascending
// with rowptr[0] = 0 and rowptr[rows] = nnz; the row of t is the LAST r with rowptr[r] <= t (empty rows share their
// start with the next row and are skipped by that rule).  Rows [0, m) are A, [m, 2m) B, [2m, 3m) C.
__device__ __forceinline__ const uint32_t *term_at(uint64_t t, const uint32_t *sec, const uint64_t *lc_off, const uint64_t *rowptr, uint32_t rows,
                                                   uint32_t &row) {
    uint32_t lo = 0, hi = rows;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rowptr[mid] <= t) lo = mid;
        else hi = mid;
    }
    row = lo;
    return sec + lc_off[lo] + 1 + 9 * (t - rowptr[lo]);
}

// The decode kernels' inputs in HBM and their error words: err[0] / err[1] = the lowest constraint with a wire id >=
// nWires / a coefficient >= r (atomicMin by the kernel), 0xFFFFFFFF = none.
struct SectionOnDevice {
    DevBuf<uint8_t> raw;                            // the section's bytes
    DevBuf<uint64_t> d_off, d_ptr;                  // lc_off (3m), rowptr (3m + 1)
    DevBuf<uint32_t> err;
    const uint32_t *sec() const { return (const uint32_t *)raw.p; }
    uint32_t rows() const { return (uint32_t)(d_ptr.n - 1); }
    void upload(const zk_r1cs_view *v, const std::vector<uint64_t> &lc_off, const std::vector<uint64_t> &rowptr, hipStream_t s) {
        raw.alloc(v->constraints_bytes ? v->constraints_bytes : 4);
        d_off.alloc(lc_off.size() ? lc_off.size() : 1);
        d_ptr.alloc(rowptr.size());
        err.alloc(2);
        {
            StreamUploader up(s);
            up.copy(raw.p, v->constraints, v->constraints_bytes);
        }
        d_off.upload(lc_off.data(), lc_off.size(), s);
        d_ptr.upload(rowptr.data(), rowptr.size(), s);
        HIP_TRY(hipMemsetAsync(err.p, 0xFF, 8, s));
    }
    // after the caller's decode kernel on s: waits for it and reports the first bad term
    void check(hipStream_t s) {
        uint32_t bad[2];
        HIP_TRY(hipMemcpyAsync(bad, err.p, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (bad[0] != 0xFFFFFFFFu) throw std::invalid_argument("r1cs constraint " + std::to_string(bad[0]) + ": wire id >= nWires");
        if (bad[1] != 0xFFFFFFFFu) throw std::invalid_argument("r1cs constraint " + std::to_string(bad[1]) + ": coefficient >= r");
    }
};

// ---- defined in r1cs.hip: the one host pass over the section and the segment plan of the cut-into-segments sums
// (rows of any length -> segments of at most SEG_TERMS inputs, one lane each, pass after pass)
constexpr uint32_t SEG_TERMS = 16;
constexpr uint64_t SEG_FINAL = 1ull << 63;          // segment destination: a row value, not a partial of the next pass
struct SegPass {
    DevBuf<uint64_t> lo, dest;                      // nseg + 1 bounds into this pass's input, nseg destinations
    uint64_t nseg = 0;
};
// word offset of every linear combination (3m: A rows, then B, then C) and the row offsets of their terms (3m + 1)
void walk_constraints(const zk_r1cs_view *v, std::vector<uint64_t> &lc_off, std::vector<uint64_t> &rowptr);
// the passes over rows with the given offsets; max_part: partials the even / odd passes write
void plan_segments(const std::vector<uint64_t> &rowptr, std::vector<std::unique_ptr<SegPass>> &passes, uint64_t max_part[2]);

}   // namespace zkp
