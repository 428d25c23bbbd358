// MSM steps 1 and 2 (overview: msm_lanes.hpp): the plan, signed digits, the two-level LDS counting sort and the scan.
// Integer kernels only: none of the 29-bit-limb field or curve code is used here.
#include "kernels.hpp"
#include "hipcheck.hpp"
#include "common.hpp"
#include "devmem.hpp"
#include <string.h>

namespace zk {

MsmPlan make_msm_plan(uint64_t n, uint32_t window_bits, uint32_t precomp, uint32_t batch) {
    if (precomp > 2) throw std::invalid_argument("table mode: 0 (as in the zkey), 1 (a row per window) or 2 (a row per second window)");
    MsmPlan p;
    uint32_t lg = 0;
    while ((1ull << (lg + 1)) <= n) lg++;
    uint32_t c = window_bits;
    if (precomp) {
        // all windows share one bucket set (tables hold 2^(c*j) P): the reduction is paid once, so
        // the window can grow until ~100 entries per bucket remain.  c = 17 buys nothing (W = 16).
        if (c == 0) {
            c = lg > 2 ? lg - 2 : 2;
            if (lg == 20) c = 19;     // 14 windows instead of 15 pay for four times the buckets only here (2^20: 9.40 -> 9.16 ms per proof;
                                      // 2^16 .. 2^19 measured neutral or worse with a wider window)
            if (lg == 21) c = 20;     // 13 instead of 14: pays since the split bucket reduction (17.0 -> 16.55 ms, profiles/r05ze_window_sweep.txt)
            if (batch > 1) c++;       // a batch shares the fixed costs of a set of launches: one window fewer pays (2^16 x 8: 0.76 -> 0.69 ms per proof)
            if (c > 20) c = 20;       // the size-based choice stops at 2^19 buckets per set: a 22-bit window (12 additions per point) was measured at
                                      // 2^24, where the reductions are cheapest — see the cap below
        }
        if (c > 22) c = 22;           // an explicit width may go to 22 (2^21 buckets per set: 8192-bucket bins in the sort's second level, 64-bucket
                                      // lanes in the split reduction; parity-tested) — it does not pay: profiles/r06t_ab_window_22_at_2p24.txt
    } else {
        if (c == 0) c = lg > 6 ? lg - 6 : 2;     // ~128 points per bucket on random scalars
        if (c > 16) c = 16;                      // one window's histogram must fit one CU's LDS
    }
    if (c < 2) c = 2;
    p.c = c;
    p.W = (256 + c - 1) / c;        // W*c >= 256: the top digit is never negative
    {
        // Scalars are reduced below r < 2^254 first (k_msm_digits), so 255 bits (254 + the carry of the signed recoding) are
        // enough — IF the top window's largest value, r >> ((W-1)*c), plus a carry still stays below 2^(c-1) (then its digit is
        // never negative).  That saves a window exactly when c divides 255: c = 15 (W 18 -> 17) and c = 17 (16 -> 15); for
        // c = 3 the check fails (r >> 252 = 3) and the 256-bit rule stays.
        const uint32_t W255 = (255 + c - 1) / c;
        if (W255 < p.W) {
            const uint32_t sh = (W255 - 1) * c;                   // < 256
            uint64_t top = 0;                                     // r >> sh (fits: 254 - sh <= c - 1 <= 19 bits)
            for (int k = 7; k >= 0; k--) {
                const int lo_bit = 32 * k;
                if (lo_bit + 32 <= (int)sh) break;
                const uint64_t w = FrParams::P[k];
                top |= lo_bit >= (int)sh ? w << (lo_bit - sh) : w >> (sh - lo_bit);
            }
            if (top + 1 < (1ull << (c - 1))) p.W = W255;
        }
    }
    p.nbuckets = 1u << (c - 1);
    p.precomp = precomp;
    p.sets = precomp ? precomp : p.W;
    p.batch = 1;
    p.batch_n = 0;
    if (batch > 1) {
        if (precomp != 1) throw std::invalid_argument("batched MSMs need window-precomputed tables with a row per window");
        p.batch = batch;
        p.batch_n = (uint32_t)n;
        p.sets = batch;
    }
    return p;
}

// ---------------------------------------------------------------- digits + two-level LDS counting sort
// Signed c-bit digits d in [-2^(c-1), 2^(c-1) - 1] (a window value >= 2^(c-1) becomes negative
// and carries into the next window; +2^(c-1) never occurs).  Every non-zero digit becomes one
// entry (table row | sign) keyed by its bucket; the sort brings the entries into bucket order.
//
// The key space (sets * 2^(c-1) buckets, 2^19 at 2^22) is sorted in two LDS-only levels:
//   1. k_bin_count / k_bin_scatter partition the codes by their high key bits into <= 256 bins,
//      staged through LDS so that the partitioned copy is written in coalesced runs;
//   2. k_bin_count_lds / k_bin_scatter_lds counting-sort every bin (<= 2^15 buckets, normally
//      2^11) with its histogram in LDS, `slices` workgroups per bin.
// No global atomics at all (the first version spent 83 % of its cycles waiting on them).  The
// order of entries inside a bucket depends on LDS arbitration; the sum does not.
#define CODE32_ZERO 0x7FFFFFFFu
#ifndef SORT_THREADS
#define SORT_THREADS 1024u      // (512 / 256 in measurement builds: workgroups that fit beside a level-1 launch's waves)
#endif

// 32-bit codes, window-major: bit 31 = sign, bits 0..30 = bucket key, 0x7FFFFFFF = zero digit.
// key = (|d| - 1) + w * nbuckets with per-window bucket sets, |d| - 1 with window-precomputed
// tables (one shared set).
__global__ __launch_bounds__(256) void k_msm_digits(uint32_t *digits, const Fr *scalars, uint64_t n, MsmPlan p) {
    ZK_CHAIN_PRIO();
    uint64_t st = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t c = p.c, W = p.W;
    const uint32_t mask = (1u << c) - 1u, half = 1u << (c - 1);
    // bucket set of window w: its own with plain tables, the one shared set with a row per window, set w & 1 with a row per second window
    const uint32_t set_stride = p.precomp == 1 ? 0u : p.nbuckets, set_mask = p.precomp == 2 ? 1u : 0xffffffffu;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += st) {
        Fr s = load_el(scalars + i);
        const uint32_t vec_base = p.batch > 1 ? (uint32_t)(i / p.batch_n) * p.nbuckets : 0u;      // bucket set of this scalar's vector
        // any 256-bit value is < 6r: bring it below r (never loops for well-formed inputs)
        for (int k = 0; k < 6; k++) {
            Fr d;
            u32 bw = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) d.v[j] = subb(s.v[j], FrParams::P[j], bw);
            if (bw) break;
            s = d;
        }
        uint64_t buf = 0;
        uint32_t nb = 0, w = 0, carry = 0;
        auto emit = [&](uint32_t raw) {
            uint32_t d = raw + carry;
            const bool neg = d >= half;                  // digits in [-2^(c-1), 2^(c-1) - 1]
            carry = neg ? 1u : 0u;
            uint32_t mag = neg ? (1u << c) - d : d;      // 0 when raw = 2^c - 1 and carry = 1
            uint32_t code = mag ? ((mag - 1u + (w & set_mask) * set_stride + vec_base) | (neg ? 0x80000000u : 0u)) : CODE32_ZERO;
            digits[(uint64_t)w * n + i] = code;
            w++;
        };
#pragma unroll
        for (int k = 0; k < 8; k++) {
            buf |= (uint64_t)s.v[k] << nb;
            nb += 32;
            while (nb >= c && w + 1 < W) {
                emit((uint32_t)buf & mask);
                buf >>= c;
                nb -= c;
            }
        }
        emit((uint32_t)buf & mask);   // top window: value < 2^254 and W*c >= 256 => never negative
    }
}

// offsets[k] = start of bucket k = starts[k * slices]; offsets[total] = grand total
__global__ __launch_bounds__(256) void k_msm_compact_offsets(uint32_t *offsets, const uint32_t *starts, uint32_t total, uint32_t slices) {
    ZK_CHAIN_PRIO();
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= total) offsets[k] = starts[(uint64_t)k * slices];
}

// The bins are SMALL (2^11 buckets) on purpose: the second-level scatter writes 4-byte entries
// at random inside its bin's output range, and only when the ranges being written at one time
// fit the XCD's 4 MiB L2 do those writes leave the L2 as whole lines (measured at 2^22: 1.76 ms
// with 2^15-bucket bins, 0.48 ms with 2^11).  The workgroups of one bin therefore run on one XCD
// (block id -> XCD is round-robin) and each XCD walks its bins in order, `slices` workgroups at
// a time.
#define BIN_MAX 256u

__global__ __launch_bounds__(SORT_THREADS) void k_bin_count(uint32_t *bin_counts, const uint32_t *codes, uint64_t total, uint32_t nbins,
                                                            uint32_t nblocks, uint32_t shift, uint32_t span) {
    ZK_CHAIN_PRIO();
    __shared__ uint32_t hist[BIN_MAX];
    if (threadIdx.x < BIN_MAX) hist[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * span;
    for (uint32_t k = threadIdx.x; k < span; k += SORT_THREADS) {
        uint64_t i = base + k;
        if (i < total) {
            uint32_t code = codes[i];
            if ((code & 0x7FFFFFFFu) != CODE32_ZERO) atomicAdd(&hist[(code & 0x7FFFFFFFu) >> shift], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < nbins) bin_counts[(uint64_t)threadIdx.x * nblocks + blockIdx.x] = hist[threadIdx.x];
}

// First-level partition, staged through LDS: a workgroup ranks its `span` items per bin with LDS
// atomics, lays them out bin-major in LDS, and writes them out so that consecutive lanes hit
// consecutive addresses.  (Scattering straight from registers costs one cache-line request per
// lane per store — 109 M line requests per sort at 2^22 — and was the larger half of the sort.)
#define BIN_ITEMS 8u           // items per thread; span = BIN_ITEMS * SORT_THREADS
__global__ __launch_bounds__(SORT_THREADS) void k_bin_scatter(uint16_t *lo, uint32_t *val, const uint32_t *bin_starts, const uint32_t *codes,
                                                              uint64_t total, uint32_t nbins, uint32_t nblocks, uint32_t shift, uint32_t span, uint64_t n,
                                                              uint32_t set_shift, uint32_t batch_n, uint32_t tstride) {
    ZK_CHAIN_PRIO();
    extern __shared__ uint32_t smem[];
    uint32_t *cnt = smem;                         // [BIN_MAX] per-bin count, then LDS start
    uint32_t *gdelta = smem + BIN_MAX;            // [BIN_MAX] global start - LDS start
    uint32_t *st_dst = smem + 2 * BIN_MAX;        // [span]
    uint32_t *st_val = st_dst + span;             // [span]
    uint16_t *st_lo = (uint16_t *)(st_val + span);   // [span]
    const uint32_t tid = threadIdx.x;
    if (tid < BIN_MAX) cnt[tid] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * span;
    const uint32_t lomask = (1u << shift) - 1u;
    // tables with a row per `tstride` windows: item w * n + i reads row (w / tstride) * n + i.  The block's first window by one
    // (uniform) division, the items' by comparison.
    const uint64_t w_base = tstride > 1 && n ? base / n : 0, r_base = tstride > 1 && n ? base - w_base * n : 0;      // (n = 0: an empty shard — no item is used)
    uint32_t code[BIN_ITEMS], rank[BIN_ITEMS];
#pragma unroll
    for (uint32_t k = 0; k < BIN_ITEMS; k++) {
        uint64_t i = base + (uint64_t)k * SORT_THREADS + tid;
        code[k] = i < total ? codes[i] : CODE32_ZERO;
    }
#pragma unroll
    for (uint32_t k = 0; k < BIN_ITEMS; k++) {
        uint32_t mag = code[k] & 0x7FFFFFFFu;
        rank[k] = mag != CODE32_ZERO ? atomicAdd(&cnt[mag >> shift], 1u) : 0u;
    }
    __syncthreads();
    // exclusive scan of the (<= 256) bin counts by wave 0: four bins per lane
    if (tid < 64) {
        uint32_t c0 = cnt[4 * tid], c1 = cnt[4 * tid + 1], c2 = cnt[4 * tid + 2], c3 = cnt[4 * tid + 3];
        uint32_t sum = c0 + c1 + c2 + c3, x = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            uint32_t y = __shfl_up(x, d);
            if (tid >= (uint32_t)d) x += y;
        }
        uint32_t off = x - sum;
        uint32_t o[4] = {off, off + c0, off + c0 + c1, off + c0 + c1 + c2};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint32_t bin = 4 * tid + q;
            cnt[bin] = o[q];
            gdelta[bin] = bin < nbins ? bin_starts[(uint64_t)bin * nblocks + blockIdx.x] - o[q] : 0u;
        }
        if (tid == 63) smem[2 * BIN_MAX + 2 * span + span / 2] = x;      // total kept past st_lo
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < BIN_ITEMS; k++) {
        uint32_t mag = code[k] & 0x7FFFFFFFu;
        if (mag != CODE32_ZERO) {
            uint32_t bin = mag >> shift, slot = cnt[bin] + rank[k];
            // table row: the flattened index j*n + i itself with window-precomputed tables
            // (set_shift = 32), the point index i otherwise (key >> set_shift = window j)
            uint64_t i = base + (uint64_t)k * SORT_THREADS + tid - (uint64_t)(set_shift < 32 ? mag >> set_shift : 0u) * n;
            if (tstride > 1) {
                uint64_t w = w_base, r = r_base + (uint64_t)k * SORT_THREADS + tid;
                while (n && r >= n) { r -= n; w++; }
                i = (w / tstride) * n + r;
            }
            if (batch_n) {          // batched vectors share the table: flattened j * n + (v * batch_n + r)  ->  row j * batch_n + r
                const uint64_t j = i / n, r = (i % n) % batch_n;
                i = j * batch_n + r;
            }
            st_dst[slot] = slot + gdelta[bin];
            st_val[slot] = (uint32_t)i | (code[k] & 0x80000000u);
            st_lo[slot] = (uint16_t)(mag & lomask);
        }
    }
    __syncthreads();
    const uint32_t kept = smem[2 * BIN_MAX + 2 * span + span / 2];
    for (uint32_t sidx = tid; sidx < kept; sidx += SORT_THREADS) {
        uint32_t d = st_dst[sidx];
        val[d] = st_val[sidx];
        lo[d] = st_lo[sidx];
    }
}

// 1-D grid -> (bin, slice): XCD x (= block id mod 8) owns bins x, x+8, x+16, ... and walks them
// in dispatch order, `slices` consecutive workgroups per bin.
__device__ __forceinline__ bool bin_slice_of_block(uint32_t nbins, uint32_t slices, uint32_t &bin, uint32_t &slice) {
    const uint32_t xcd = blockIdx.x & 7u, k = blockIdx.x >> 3;
    bin = (k / slices) * 8u + xcd;
    slice = k % slices;
    return bin < nbins;
}

// bin b occupies items [bin_starts[b*nblocks], bin_starts[(b+1)*nblocks]) (the scan array ends with the total)
__global__ __launch_bounds__(SORT_THREADS) void k_bin_count_lds(uint32_t *counts, const uint16_t *lo, const uint32_t *bin_starts,
                                                                uint32_t nblocks, uint32_t buckets_per_bin, uint32_t nbins, uint32_t slices,
                                                                uint32_t total_buckets) {
    ZK_CHAIN_PRIO();
    extern __shared__ uint32_t hist[];
    uint32_t b, slice;
    if (!bin_slice_of_block(nbins, slices, b, slice)) return;
    const uint32_t first = b * buckets_per_bin, nb = total_buckets - first < buckets_per_bin ? total_buckets - first : buckets_per_bin;
    for (uint32_t k = threadIdx.x; k < nb; k += SORT_THREADS) hist[k] = 0;
    __syncthreads();
    const uint64_t bs = bin_starts[(uint64_t)b * nblocks], be = bin_starts[(uint64_t)(b + 1) * nblocks];
    const uint64_t len = be - bs, s0 = bs + len * slice / slices, s1 = bs + len * (slice + 1) / slices;
    for (uint64_t i = s0 + threadIdx.x; i < s1; i += SORT_THREADS) atomicAdd(&hist[lo[i]], 1u);
    __syncthreads();
    uint32_t *out = counts + (uint64_t)first * slices + slice;
    for (uint32_t k = threadIdx.x; k < nb; k += SORT_THREADS) out[(uint64_t)k * slices] = hist[k];
}

__global__ __launch_bounds__(SORT_THREADS) void k_bin_scatter_lds(uint32_t *entries, const uint32_t *starts, const uint16_t *lo,
                                                                  const uint32_t *val, const uint32_t *bin_starts, uint32_t nblocks,
                                                                  uint32_t buckets_per_bin, uint32_t nbins, uint32_t slices, uint32_t total_buckets) {
    ZK_CHAIN_PRIO();
    extern __shared__ uint32_t cursor[];
    uint32_t b, slice;
    if (!bin_slice_of_block(nbins, slices, b, slice)) return;
    const uint32_t first = b * buckets_per_bin, nb = total_buckets - first < buckets_per_bin ? total_buckets - first : buckets_per_bin;
    const uint32_t *in = starts + (uint64_t)first * slices + slice;
    for (uint32_t k = threadIdx.x; k < nb; k += SORT_THREADS) cursor[k] = in[(uint64_t)k * slices];
    __syncthreads();
    const uint64_t bs = bin_starts[(uint64_t)b * nblocks], be = bin_starts[(uint64_t)(b + 1) * nblocks];
    const uint64_t len = be - bs, s0 = bs + len * slice / slices, s1 = bs + len * (slice + 1) / slices;
    uint64_t i = s0 + threadIdx.x;
    for (; i + 3 * SORT_THREADS < s1; i += 4 * SORT_THREADS) {      // four independent loads in flight
        uint32_t k0 = lo[i], k1 = lo[i + SORT_THREADS], k2 = lo[i + 2 * SORT_THREADS], k3 = lo[i + 3 * SORT_THREADS];
        uint32_t v0 = val[i], v1 = val[i + SORT_THREADS], v2 = val[i + 2 * SORT_THREADS], v3 = val[i + 3 * SORT_THREADS];
        entries[atomicAdd(&cursor[k0], 1u)] = v0;
        entries[atomicAdd(&cursor[k1], 1u)] = v1;
        entries[atomicAdd(&cursor[k2], 1u)] = v2;
        entries[atomicAdd(&cursor[k3], 1u)] = v3;
    }
    for (; i < s1; i += SORT_THREADS) entries[atomicAdd(&cursor[lo[i]], 1u)] = val[i];
}

// Exclusive scan in three coalesced launches: per-block (4096 elements) local scan + block
// sums, scan of the block sums (one block), add-back.  offsets[total] = grand total.
#define SCAN_BLOCK 1024u
#define SCAN_ELEMS 4096u
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *lds, uint32_t &block_total) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t y = __shfl_up(x, d);
        if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    if (wave == 0) {
        uint32_t s = lane < (SCAN_BLOCK / 64) ? lds[lane] : 0;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            uint32_t y = __shfl_up(s, d);
            if (lane >= (uint32_t)d) s += y;
        }
        if (lane < (SCAN_BLOCK / 64)) lds[lane] = s;      // inclusive wave totals
    }
    __syncthreads();
    uint32_t wave_off = wave ? lds[wave - 1] : 0;
    block_total = lds[SCAN_BLOCK / 64 - 1];
    return wave_off + x - v;
}
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_local(uint32_t *offsets, uint32_t *block_sums, const uint32_t *counts, uint32_t total) {
    ZK_CHAIN_PRIO();
    __shared__ uint32_t lds[SCAN_BLOCK / 64];
    const uint32_t base = blockIdx.x * SCAN_ELEMS + threadIdx.x * 4;
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = base + j < total ? counts[base + j] : 0;
    uint32_t sum = v[0] + v[1] + v[2] + v[3], bt;
    uint32_t ex = block_exclusive_scan(sum, lds, bt);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (base + j < total) offsets[base + j] = ex;
        ex += v[j];
    }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = bt;
}
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_sums(uint32_t *block_sums, uint32_t nblocks, uint32_t *grand_total) {
    ZK_CHAIN_PRIO();
    __shared__ uint32_t lds[SCAN_BLOCK / 64];
    __shared__ uint32_t carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nblocks; base += SCAN_BLOCK) {
        uint32_t i = base + threadIdx.x;
        uint32_t v = i < nblocks ? block_sums[i] : 0, bt;
        uint32_t ex = block_exclusive_scan(v, lds, bt) + carry_s;
        if (i < nblocks) block_sums[i] = ex;
        __syncthreads();
        if (threadIdx.x == 0) carry_s += bt;
        __syncthreads();
    }
    if (threadIdx.x == 0) *grand_total = carry_s;
}
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_add(uint32_t *offsets, const uint32_t *block_sums, uint32_t total) {
    ZK_CHAIN_PRIO();
    const uint32_t base = blockIdx.x * SCAN_ELEMS + threadIdx.x * 4;
    const uint32_t add = block_sums[blockIdx.x];
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (base + j < total) offsets[base + j] += add;
}

// Second-level scatter, STAGED: the direct version above sends every entry to L2 as a 4-byte request of its own (54.5 M requests per
// sort at 2^22: 55 % of its wave cycles stalled at issue, profiles/r05u_sort_kernel_counters.txt).  Here a workgroup takes its slice of
// the bin in tiles of STAGE_CAP entries, counting-sorts a tile INSIDE LDS (rank by LDS atomic, exclusive scan of the 2^11 bucket counts,
// placement), and writes it out in bucket order: the entries of one bucket go to consecutive addresses, so consecutive lanes store
// consecutive dwords and the address path merges them — about one request per (tile, bucket) run instead of one per entry.  The global
// position of a run is the slice's cursor of that bucket (from the scan over (bucket, slice) counts, as before), advanced tile by tile.
// For bins of at most 2^11 buckets and SORT_THREADS = 1024 (= SCAN_BLOCK); other plans keep the direct kernel.
#ifndef STAGE_CAP
#define STAGE_CAP 8192u
#endif
// The kernel's LDS layout (2048 bucket counters as two words per thread: loc[tid], loc[tid + SCAN_BLOCK]; a 16-entry area of
// wave totals; PER = STAGE_CAP / SCAN_BLOCK entries per thread; positions in a tile as u16) is written for exactly these values:
static_assert(SCAN_BLOCK == 1024u && STAGE_CAP % SCAN_BLOCK == 0 && STAGE_CAP <= 65536u, "k_bin_scatter_staged: retune its LDS layout with SCAN_BLOCK / STAGE_CAP");
__global__ __launch_bounds__(SCAN_BLOCK) void k_bin_scatter_staged(uint32_t *entries, const uint32_t *starts, const uint16_t *lo, const uint32_t *val,
                                                                   const uint32_t *bin_starts, uint32_t nblocks, uint32_t buckets_per_bin, uint32_t nbins,
                                                                   uint32_t slices, uint32_t total_buckets) {
    ZK_CHAIN_PRIO();
    extern __shared__ uint32_t sm[];
    uint32_t b, slice;
    if (!bin_slice_of_block(nbins, slices, b, slice)) return;
    const uint32_t first = b * buckets_per_bin, nb = total_buckets - first < buckets_per_bin ? total_buckets - first : buckets_per_bin;
    uint32_t *loc = sm;                               // [2048] rank counters of the tile, then its exclusive bucket offsets
    uint32_t *gcur = sm + 2048;                       // [2048] this slice's global cursor per bucket
    uint32_t *scan_lds = sm + 4096;                   // [16]
    uint32_t *sval = sm + 4096 + 16;                  // [STAGE_CAP]
    uint16_t *slo = (uint16_t *)(sval + STAGE_CAP);   // [STAGE_CAP]
    const uint32_t tid = threadIdx.x;
    const uint32_t *in = starts + (uint64_t)first * slices + slice;
    for (uint32_t k = tid; k < 2048u; k += SCAN_BLOCK) gcur[k] = k < nb ? in[(uint64_t)k * slices] : 0u;
    const uint64_t bs = bin_starts[(uint64_t)b * nblocks], be = bin_starts[(uint64_t)(b + 1) * nblocks];
    const uint64_t len = be - bs, s0 = bs + len * slice / slices, s1 = bs + len * (slice + 1) / slices;
    constexpr uint32_t PER = STAGE_CAP / SCAN_BLOCK;  // entries per thread and tile
    for (uint64_t t0 = s0; t0 < s1; t0 += STAGE_CAP) {
        const uint32_t cnt = (uint32_t)(s1 - t0 < STAGE_CAP ? s1 - t0 : STAGE_CAP);
        loc[tid] = 0;
        loc[tid + SCAN_BLOCK] = 0;
        __syncthreads();                              // (also: the previous tile's write-out has read loc / sval)
        uint32_t key[PER], v[PER], rank[PER];
#pragma unroll
        for (uint32_t k = 0; k < PER; k++) {
            const uint32_t p = k * SCAN_BLOCK + tid;
            key[k] = p < cnt ? lo[t0 + p] : 0xFFFFFFFFu;
            v[k] = p < cnt ? val[t0 + p] : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < PER; k++) rank[k] = key[k] != 0xFFFFFFFFu ? atomicAdd(&loc[key[k]], 1u) : 0u;
        __syncthreads();
        // exclusive scan of the 2048 counts: two per thread
        const uint32_t c0 = loc[2 * tid], c1 = loc[2 * tid + 1];
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(c0 + c1, scan_lds, total);
        __syncthreads();
        loc[2 * tid] = ex;
        loc[2 * tid + 1] = ex + c0;
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < PER; k++) {
            if (key[k] != 0xFFFFFFFFu) {
                const uint32_t pos = loc[key[k]] + rank[k];
                sval[pos] = v[k];
                slo[pos] = (uint16_t)key[k];
            }
        }
        __syncthreads();
        for (uint32_t p = tid; p < cnt; p += SCAN_BLOCK) {
            const uint32_t kk = slo[p];
            entries[gcur[kk] + (p - loc[kk])] = sval[p];
        }
        __syncthreads();
        // advance the cursors by the tile's counts: count of bucket k = loc[k + 1] - loc[k] (cnt - loc[k] for the last one)
        const uint32_t a0 = loc[2 * tid], a1 = loc[2 * tid + 1], a2 = 2 * tid + 2 < 2048u ? loc[2 * tid + 2] : cnt;
        gcur[2 * tid] += a1 - a0;
        gcur[2 * tid + 1] += a2 - a1;
        __syncthreads();                              // the next tile zeroes loc in another thread-to-word pattern
    }
}

// exclusive scan of counts[0..total) -> out[0..total], out[total] = grand total;
// out must hold total + 1 + msm_scan_extra_words(total) words (block sums live past the end)
static void launch_scan(uint32_t *out, const uint32_t *counts, uint32_t total, hipStream_t s) {
    uint32_t nblocks = (total + SCAN_ELEMS - 1) / SCAN_ELEMS;
    uint32_t *block_sums = out + total + 1;
    ZK_LAUNCH(k_scan_local, dim3(nblocks), dim3(SCAN_BLOCK), 0, s, out, block_sums, counts, total);
    ZK_LAUNCH(k_scan_sums, dim3(1), dim3(SCAN_BLOCK), 0, s, block_sums, nblocks, out + total);
    ZK_LAUNCH(k_scan_add, dim3(nblocks), dim3(SCAN_BLOCK), 0, s, out, (const uint32_t *)block_sums, total);
}
uint32_t msm_scan_extra_words(uint32_t total) { return (total + SCAN_ELEMS - 1) / SCAN_ELEMS; }
void launch_exclusive_scan_u32(uint32_t *out, const uint32_t *counts, uint32_t total, hipStream_t s) { launch_scan(out, counts, total, s); }

// geometry of the two sort levels
#define BIN_SHIFT 11u          // buckets per bin = 2^11 (see above)
#define BIN_SLICES 32u         // second-level workgroups per bin
static inline uint32_t plan_total_buckets(MsmPlan p) { return p.sets * p.nbuckets; }
static inline uint32_t plan_bin_shift(MsmPlan p) {      // at most BIN_MAX bins; the low key bits travel as 16 bits
    uint32_t sh = BIN_SHIFT;
    while (((plan_total_buckets(p) + (1u << sh) - 1) >> sh) > BIN_MAX) sh++;
    return sh;
}
static inline uint32_t plan_nbins(MsmPlan p) { uint32_t sh = plan_bin_shift(p); return (plan_total_buckets(p) + (1u << sh) - 1) >> sh; }
static inline uint32_t bin_span() { return BIN_ITEMS * SORT_THREADS; }       // items per first-level workgroup
static inline uint32_t plan_bin_blocks(uint64_t n, MsmPlan p) { return (uint32_t)(((n ? n : 1) * p.W + bin_span() - 1) / bin_span()); }

MsmSortSizes msm_sort_sizes(uint64_t n, MsmPlan p) {
    MsmSortSizes z;
    memset(&z, 0, sizeof z);
    const uint64_t tb = plan_total_buckets(p), items = (n ? n : 1) * p.W;
    const uint64_t bb = (uint64_t)plan_nbins(p) * plan_bin_blocks(n, p);
    z.counts_u32 = tb * BIN_SLICES;
    z.starts_u32 = tb * BIN_SLICES + 1 + msm_scan_extra_words((uint32_t)(tb * BIN_SLICES));
    z.offsets_u32 = tb + 1;
    z.entries_u32 = items;
    z.codes_u32 = items;
    z.lo_u16 = items;
    z.val_u32 = items;
    z.bin_counts_u32 = bb;
    z.bin_starts_u32 = bb + 1 + msm_scan_extra_words((uint32_t)bb);
    return z;
}

static inline size_t bin_scatter_lds_bytes() { return (size_t)(2 * BIN_MAX + 2 * bin_span() + bin_span() / 2 + 1) * 4; }
static void sort_lds_attr() {
    static PerDeviceOnce attr;
    if (!attr.need()) return;   // > 64 KiB of dynamic LDS needs the opt-in (160 KiB per CU on gfx950), on every device
    ZK_HIP(hipFuncSetAttribute((const void *)k_bin_count_lds, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    ZK_HIP(hipFuncSetAttribute((const void *)k_bin_scatter_lds, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    ZK_HIP(hipFuncSetAttribute((const void *)k_bin_scatter, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    ZK_HIP(hipFuncSetAttribute((const void *)k_bin_scatter_staged, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr.done();
}

// digits -> bin partition -> per-bin LDS histograms -> scan -> LDS-ranked scatter -> compact bucket offsets
void launch_msm_sort(const MsmSortBufs &b, const Fr *scalars, uint64_t n, MsmPlan p, hipStream_t s) {
    const uint32_t tb = plan_total_buckets(p);
    sort_lds_attr();
    uint64_t g = (n + 255) / 256;
    if (g > 8192) g = 8192;
    const uint32_t sh = plan_bin_shift(p), nbins = plan_nbins(p), nblocks = plan_bin_blocks(n, p);
    // second-level workgroups per bin: about one staging tile of entries each (longer runs per bucket = fewer, wider stores), at most
    // BIN_SLICES (what the count / start arrays are sized for), at least 4
    uint32_t slices = BIN_SLICES;
    {
        const uint64_t per_bin = (n * p.W) / (nbins ? nbins : 1);
        while (slices > 4u && per_bin / slices < STAGE_CAP * 3u / 4u) slices >>= 1;
    }
    const uint32_t bpb = tb < (1u << sh) ? tb : (1u << sh);
    const uint64_t total = n * p.W;
    const size_t lds = (size_t)bpb * 4;
    const uint32_t grid2 = ((nbins + 7u) / 8u) * 8u * slices;
    const uint32_t set_shift = p.precomp ? 32u : p.c - 1u;
    if (n) ZK_LAUNCH(k_msm_digits, dim3((uint32_t)g), dim3(256), 0, s, b.codes, scalars, n, p);
    ZK_LAUNCH(k_bin_count, dim3(nblocks), dim3(SORT_THREADS), 0, s, b.bin_counts, (const uint32_t *)b.codes, total, nbins, nblocks, sh, bin_span());
    launch_scan(b.bin_starts, b.bin_counts, nbins * nblocks, s);
    ZK_LAUNCH(k_bin_scatter, dim3(nblocks), dim3(SORT_THREADS), bin_scatter_lds_bytes(), s, b.lo, b.val, (const uint32_t *)b.bin_starts,
                       (const uint32_t *)b.codes, total, nbins, nblocks, sh, bin_span(), n, set_shift, p.batch > 1 ? p.batch_n : 0u, p.precomp);
    ZK_LAUNCH(k_bin_count_lds, dim3(grid2), dim3(SORT_THREADS), lds, s, b.counts, (const uint16_t *)b.lo,
                       (const uint32_t *)b.bin_starts, nblocks, bpb, nbins, slices, tb);
    launch_scan(b.starts, b.counts, tb * slices, s);
    static const bool direct = probe_env("ZKHIP_SORT_DIRECT") != nullptr;      // (-DZK_PROBES builds: the unstaged second-level scatter, for A/Bs)
    if (bpb <= 2048u && SORT_THREADS == SCAN_BLOCK && !direct)
        ZK_LAUNCH(k_bin_scatter_staged, dim3(grid2), dim3(SCAN_BLOCK), (size_t)(4096 + 16 + STAGE_CAP) * 4 + (size_t)STAGE_CAP * 2, s, b.entries,
                           (const uint32_t *)b.starts, (const uint16_t *)b.lo, (const uint32_t *)b.val, (const uint32_t *)b.bin_starts, nblocks, bpb, nbins,
                           slices, tb);
    else
        ZK_LAUNCH(k_bin_scatter_lds, dim3(grid2), dim3(SORT_THREADS), lds, s, b.entries, (const uint32_t *)b.starts,
                           (const uint16_t *)b.lo, (const uint32_t *)b.val, (const uint32_t *)b.bin_starts, nblocks, bpb, nbins, slices, tb);
    ZK_LAUNCH(k_msm_compact_offsets, dim3((tb + 256) / 256), dim3(256), 0, s, b.offsets, (const uint32_t *)b.starts, tb, slices);
    ZK_LAUNCH_OK("msm sort");
}

}   // namespace zk
