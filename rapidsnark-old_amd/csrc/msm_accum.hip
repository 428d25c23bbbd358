// MSM step 3 (overview: msm_lanes.hpp): level-1 bucket accumulation, the merges of cut runs, lane and round planning.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "hipcheck.hpp"
#include "msm_lanes.hpp"

namespace zk {

// ---------------------------------------------------------------- load-balanced accumulation
// A lane-per-bucket walk is hopeless on real data: the top window of uniformly random
// scalars has only a handful of non-empty buckets (r ~ 2^253.6), and real witnesses pile
// half their entries into bucket "1" of window 0.  Instead EVERY lane adds exactly
// ACC_CHUNK consecutive entries of the bucket-sorted list, whatever buckets they span:
//   * a bucket run that starts and ends inside the chunk is complete -> buckets[b];
//   * a run cut by the chunk's left edge goes to the lane's HEAD slot, one cut by the right
//     edge to its TAIL slot (at most one of each), tagged with its bucket and STARTS/ENDS flags;
//   * the slot list (2 per lane, still bucket-sorted) is reduced by wave-parallel segmented scans over
//     XYZZ partials (k_msm_accum_wave), shrinking 32x (G2: 16x) per level until one wave is left.
// Work per lane is constant, so the kernel time is flat in the scalar distribution.  Because it is constant,
// the grid runs in lock-step "rounds" of as many workgroups as fit on the chip at once (G1: 3 waves/SIMD =
// 768 workgroups, G2: 2 waves/SIMD = 512), and a last round that is only partly full costs a whole round:
// at 2^22 a fixed chunk of 128 gave 1664 workgroups = 2.17 rounds, i.e. the kernel ran at 72% of its own
// rate.  So the host launches a WHOLE number of rounds of lanes (accum_lanes_for) and the chunk is whatever
// divides the entries evenly among them (32..160 entries; below 32 fewer lanes are launched instead).  That is a LONE proof's
// plan; one submitted beside others takes 128..1280 entries per lane (AccumTail::chunk_min / chunk_max, set in prover_pipeline.hip):
// the chip is shared anyway, and fewer lanes leave fewer cut runs to merge.
#define ACC_CHUNK_MAX 160u  // affine points per lane, level 1: more than this and another round of lanes is launched
#define ACC_CHUNK_MIN 32u   // fewer than this and fewer lanes are launched (small or sharded MSMs)
// Every lane takes the same share of the E entries actually present (E <= max_entries is known on the device
// only): the host fixes the number of lanes, the chunk follows.
__device__ __forceinline__ uint32_t accum_chunk_dev(uint32_t E, uint32_t nlanes, uint32_t chunk_min) {
    const uint32_t c = (uint32_t)(((uint64_t)E + nlanes - 1) / nlanes);
    return c < chunk_min ? chunk_min : c;
}
#ifdef ZK_PROBES
#define ZK_GATHER_ROW(i) ((i) & batch.gather_mask)
#else
#define ZK_GATHER_ROW(i) (i)
#endif
#define ACC_CHUNK_N 32u     // slots per unit at levels >= 2 used to SIZE the workspace (a G2 wave takes 32, a G1 wave 64)
// Threads per workgroup of the level-1 kernels.  They use no LDS and no barrier, so the workgroup is only the unit in which the
// dispatcher hands waves to a CU (ZK_L1_BLOCK=64 in a measurement build: one wave per workgroup).
#ifndef ZK_L1_BLOCK
#define ZK_L1_BLOCK 256
#endif
#ifndef ZK_L1_PREFETCH
#define ZK_L1_PREFETCH 1      // raw points in flight per lane in the G1 level-1 kernel
#endif
#define SLOT_EMPTY 0xffffffffu
#define FLAG_STARTS 1u
#define FLAG_ENDS 2u

// Occupancy is what the compiler picks: G1 154 VGPRs, 74 SGPRs, no scratch (3 waves/SIMD); the G2 kernel (Fq2 split over lane pairs, below) 212 VGPRs
// (2 waves/SIMD).  Forcing 4 G1 waves (128 VGPRs, 20 B scratch) was measured slower for the whole proof.
// blockIdx.y selects one of up to three MSMs over the SAME sorted entry list (A, B1, C share sort(w)):
// small circuits launch them together — a level-1 launch there is latency-bound (a lane's chain of 32
// adds, a grid that does not fill the chip) and three of them cost what one costs.
#ifdef ZK_G1_FOUR_WAVES
#define ZK_G1_L1_WAVES __attribute__((amdgpu_waves_per_eu(4, 4)))
#else
#define ZK_G1_L1_WAVES
#endif
template <class F>
__global__ __launch_bounds__(ZK_L1_BLOCK) ZK_G1_L1_WAVES void k_msm_accum_l1(G1Acc *buckets0, const uint32_t *offsets, const uint32_t *entries,
                                                      AccumBatch batch, uint32_t nbuckets_total, G1Acc *out_part0, uint32_t *out_key0,
                                                      uint32_t *out_flag0, uint32_t nlanes, uint32_t chunk_min) {
    static_assert(sizeof(F) == sizeof(Fq), "G1 only: the G2 level-1 kernel is k_msm_accum_l1_g2s");
    const uint32_t m = blockIdx.y;
    G1Acc *buckets = buckets0 + (uint64_t)m * batch.bucket_stride;
    G1Acc *out_part = out_part0 + (uint64_t)m * batch.ws_stride;
    uint32_t *out_key = out_key0 + (uint64_t)m * batch.ws_stride, *out_flag = out_flag0 + (uint64_t)m * batch.ws_stride;
    const Affine<F> *points = reinterpret_cast<const Affine<F> *>(batch.points[m]);
    const uint32_t idx_min = batch.idx_min[m], idx_sub = batch.idx_sub[m];
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nlanes) return;
    const uint32_t E = offsets[nbuckets_total];
    const uint32_t ACC_CHUNK = accum_chunk_dev(E, nlanes, chunk_min);
    const uint64_t lo64 = (uint64_t)t * ACC_CHUNK;
    uint32_t hkey = SLOT_EMPTY, tkey = SLOT_EMPTY, hflag = 0, tflag = 0;
    if (lo64 < E) {
        const uint32_t lo = (uint32_t)lo64;
        const uint32_t hi = (E - lo > ACC_CHUNK) ? lo + ACC_CHUNK : E;
        // last b with offsets[b] <= lo  (skips empty buckets that share the same offset)
        uint32_t bl = 0, br = nbuckets_total - 1;
        while (bl < br) {
            uint32_t mid = (bl + br + 1) >> 1;
            if (offsets[mid] <= lo) bl = mid; else br = mid - 1;
        }
        uint32_t b = bl;
        uint32_t bend = offsets[b + 1];
        // The end of the bucket AFTER the current one, re-loaded at the top of every iteration (one cached dword next to
        // the prefetch): a dependent load at the run's end — a run ends in ~46 % of a wave's iterations — cost a memory
        // latency every time, and so does a load issued AT the run's end (the loop-top wait for the next entry is
        // in-order: it would wait for that load too).
        uint32_t bend2 = 0;
        bool started_before = offsets[b] < lo;
        typedef REGF FR;
        XYZZ<FR> acc = XYZZ<FR>::inf();
        Affine<F> nextP;                 // raw words: the next point is in flight while this one is added
        bool nextNeg = false, nextSkip = false;
        // two loads deep: the ENTRY of position e+2 is in flight while the POINT of e+1 is, so the address of a point
        // load never waits for its entry (a wave's three resident siblings run in phase with it — same work, same
        // start — and do not cover that wait)
        // The loads are UNCONDITIONAL (positions past the chunk's end are clamped to its last entry and the result is
        // never used): a load under `if (e < hi)` makes the compiler merge its result with the old value right behind
        // the branch — an s_waitcnt vmcnt(0) straight after the issue, i.e. no prefetch at all.
        uint32_t entNext = entries[lo];
        auto fetch = [&](uint32_t pos) {          // point of position pos (its entry is in entNext), entry of pos + 1
            const uint32_t ent = entNext;
            const uint32_t idx = ent & 0x7fffffffu;
            nextNeg = (ent >> 31) != 0;
            nextSkip = idx < idx_min;
            bend2 = offsets[b + 2 < nbuckets_total ? b + 2 : nbuckets_total];
            const Affine<F> *src = points + (nextSkip ? 0 : ZK_GATHER_ROW(idx - idx_sub));
            nextP.x = load_row_el(&src->x);
            nextP.y = load_row_el(&src->y);
            entNext = entries[pos + 1 < hi ? pos + 1 : hi - 1];
        };
        uint32_t e = lo;
        fetch(e);
#if ZK_L1_PREFETCH >= 2
        // TWO points in flight: the table rows are random 64-byte gathers from a 3 GiB table, and with the rows confined to an
        // L2-resident range (probe: ZKHIP_GATHER_MASK) the launch is 10 % shorter — more than the 8 % the s_waitcnt counters
        // showed: one addition (~4.5 us) is not always enough to cover a gather under this load.  The kernel has 36 VGPRs to
        // spare below the three-waves-per-SIMD limit; the second raw point costs 16 of them and 18 moves per addition.
        Affine<F> curP = nextP;
        bool curNeg = nextNeg, curSkip = nextSkip;
        fetch(lo + 1 < hi ? lo + 1 : hi - 1);
#endif
        while (e < hi) {
#if ZK_L1_PREFETCH >= 2
            Affine<F> Pw = curP;
            bool ng = curNeg, skip = curSkip;
            curP = nextP; curNeg = nextNeg; curSkip = nextSkip;      // the point of position e + 1 (still on its way, normally)
            e++;
            fetch(e + 1 < hi ? e + 1 : hi - 1);                        // point of e + 1 (entry prefetched), entry of e + 2
#else
            Affine<F> Pw = nextP;
            bool ng = nextNeg, skip = nextSkip;
            e++;
            fetch(e < hi ? e : hi - 1);
#endif
            if (!skip) {
                Affine<FR> P = to_reg_affine<F>(Pw);
                if (ng) negate_y(P);
                madd(acc, P);          // curve29.hpp: bound-tracked specialisation
            }
            if (e == bend || e == hi) {              // the run of bucket b ends here (or is cut)
                const bool ends = (e == bend);
                // ONE store sequence whatever the case (a wave's lanes are in different ones): complete run -> its bucket,
                // run cut on the left -> HEAD slot, cut on the right only -> TAIL slot
                G1Acc *dst = (!started_before && ends) ? buckets + b : out_part + 2 * (uint64_t)t + (started_before ? 0u : 1u);
                if (started_before) {
                    hkey = b;
                    hflag = ends ? FLAG_ENDS : 0u;
                } else if (!ends) {
                    tkey = b;
                    tflag = FLAG_STARTS;
                }
                LaneModel<Fq>::store(dst, acc);
                if (e < hi) {                        // next non-empty bucket
                    b++;
                    bend = bend2;
                    while (bend == e) { b++; bend = offsets[b + 1]; }        // empty buckets: rare on uniform scalars
                    started_before = false;
                    acc = XYZZ<FR>::inf();
                }
            }
        }
    }
    out_key[2 * (uint64_t)t] = hkey;
    out_flag[2 * (uint64_t)t] = hflag;
    out_key[2 * (uint64_t)t + 1] = tkey;
    out_flag[2 * (uint64_t)t + 1] = tflag;
}

// G2 level 1 with the accumulator split across lane pairs (curve29.hpp, Fq2s): two lanes per chunk,
// lane parity = Fq2 component.  Both lanes of a pair walk the same entries, so the loop and every
// branch are uniform inside the pair (the DPP exchanges need both lanes active).
#ifdef ZK_G2_THREE_WAVES
#define ZK_G2_L1_WAVES __attribute__((amdgpu_waves_per_eu(3, 3)))
#else
#define ZK_G2_L1_WAVES
#endif
__global__ __launch_bounds__(ZK_L1_BLOCK) ZK_G2_L1_WAVES void k_msm_accum_l1_g2s(G2Acc *buckets, const uint32_t *offsets, const uint32_t *entries,
                                                          const G2Affine *points, uint32_t idx_min, uint32_t idx_sub,
                                                          uint32_t nbuckets_total, G2Acc *out_part, uint32_t *out_key,
                                                          uint32_t *out_flag, uint32_t nlanes, uint32_t chunk_min) {
    const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t t = gt >> 1, comp = gt & 1u;          // chunk, component (blockDim is even: comp == threadIdx.x & 1)
    if (t >= nlanes) return;
    const uint32_t E = offsets[nbuckets_total];
    const uint32_t ACC_CHUNK = accum_chunk_dev(E, nlanes, chunk_min);
    const uint64_t lo64 = (uint64_t)t * ACC_CHUNK;
    uint32_t hkey = SLOT_EMPTY, tkey = SLOT_EMPTY, hflag = 0, tflag = 0;
    auto store_comp = [&](G2Acc *dst, const XYZZ<Fq2s> &v) { LaneModel<Fq2>::store(dst, v); };   // this lane's component (comp == threadIdx.x & 1)
    if (lo64 < E) {
        const uint32_t lo = (uint32_t)lo64;
        const uint32_t hi = (E - lo > ACC_CHUNK) ? lo + ACC_CHUNK : E;
        uint32_t bl = 0, br = nbuckets_total - 1;
        while (bl < br) {
            uint32_t mid = (bl + br + 1) >> 1;
            if (offsets[mid] <= lo) bl = mid; else br = mid - 1;
        }
        uint32_t b = bl;
        uint32_t bend = offsets[b + 1];
        uint32_t bend2 = 0;              // end of the bucket after the current one, as in the G1 kernel
        bool started_before = offsets[b] < lo;
        XYZZ<Fq2s> acc = XYZZ<Fq2s>::inf();
        Fq nextX, nextY;                 // raw words of this lane's component of the next point
        bool nextNeg = false, nextSkip = false;
        uint32_t entNext = entries[lo];               // two loads deep and unconditional, as in the G1 kernel
        auto fetch = [&](uint32_t pos) {
            const uint32_t ent = entNext;
            const uint32_t idx = ent & 0x7fffffffu;
            nextNeg = (ent >> 31) != 0;
            nextSkip = idx < idx_min;
            bend2 = offsets[b + 2 < nbuckets_total ? b + 2 : nbuckets_total];
            const Fq *src = reinterpret_cast<const Fq *>(points + (nextSkip ? 0 : idx - idx_sub)) + comp;
            nextX = load_row_el(src);
            nextY = load_row_el(src + 2);
            entNext = entries[pos + 1 < hi ? pos + 1 : hi - 1];
        };
        uint32_t e = lo;
        fetch(e);
        while (e < hi) {
            Fq Xw = nextX, Yw = nextY;
            bool ng = nextNeg, skip = nextSkip;
            e++;
            fetch(e < hi ? e : hi - 1);
            if (!skip) {
                Affine<Fq2s> P{Fq2s{Fq29::load(Xw)}, Fq2s{Fq29::load(Yw)}};
                if (ng) P.y.v = Fq29::neg_lazy(P.y.v);
                madd(acc, P);
            }
            if (e == bend || e == hi) {
                const bool ends = (e == bend);
                G2Acc *dst = (!started_before && ends) ? buckets + b : out_part + 2 * (uint64_t)t + (started_before ? 0u : 1u);
                if (started_before) {
                    hkey = b;
                    hflag = ends ? FLAG_ENDS : 0u;
                } else if (!ends) {
                    tkey = b;
                    tflag = FLAG_STARTS;
                }
                store_comp(dst, acc);
                if (e < hi) {
                    b++;
                    bend = bend2;
                    while (bend == e) { b++; bend = offsets[b + 1]; }
                    started_before = false;
                    acc = XYZZ<Fq2s>::inf();
                }
            }
        }
    }
    if (comp == 0) {
        out_key[2 * (uint64_t)t] = hkey;
        out_flag[2 * (uint64_t)t] = hflag;
        out_key[2 * (uint64_t)t + 1] = tkey;
        out_flag[2 * (uint64_t)t + 1] = tflag;
    }
}

// Pairwise merge between level 1 and the generic levels: a bucket cut by exactly ONE chunk edge
// (the overwhelmingly common case — mean run length ~ chunk length) is the TAIL slot of lane t
// plus the HEAD slot of lane t+1 that also ENDS.  One general add per lane, full occupancy,
// and both slots are retired; what is left for the serial-ish generic levels is only the
// buckets spanning three or more chunks (top window, skewed witnesses).
template <class F>
__global__ __launch_bounds__(256) void k_msm_accum_pair(ACCMEM *buckets, const ACCMEM *part, uint32_t *key, const uint32_t *flag,
                                                        uint32_t nlanes, uint64_t bucket_stride, uint64_t ws_stride) {
    ZK_TAIL_PRIO();
    typedef LaneModel<F> LM;
    buckets += (uint64_t)blockIdx.y * bucket_stride;      // blockIdx.y: MSM of a batch (see k_msm_accum_l1)
    part += (uint64_t)blockIdx.y * ws_stride;
    key += (uint64_t)blockIdx.y * ws_stride;
    flag += (uint64_t)blockIdx.y * ws_stride;
    const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t t = gt / LM::LPE;
    if (t + 1 >= nlanes) return;
    const uint32_t kt = key[2 * (uint64_t)t + 1], kh = key[2 * (uint64_t)t + 2];
    if (kt == SLOT_EMPTY || kt != kh) return;
    if (!(flag[2 * (uint64_t)t + 2] & FLAG_ENDS)) return;       // continues further: generic levels
    XYZZ<typename LM::R> a = LM::load(part + 2 * (uint64_t)t + 1);
    add(a, LM::load(part + 2 * (uint64_t)t + 2));
    LM::store(buckets + kt, a);
    // (both lanes of a G2 pair have read the keys before either of them retires the slots: the pair
    // is in one wave and the loads above precede these stores in program order)
    if (gt % LM::LPE == 0) {
        key[2 * (uint64_t)t + 1] = SLOT_EMPTY;
        key[2 * (uint64_t)t + 2] = SLOT_EMPTY;
    }
}

// Levels >= 2, wave-parallel: a WAVE takes 64 consecutive slots (32 for G2: a lane pair per element),
// compacts the non-empty ones to its low lanes (ds_permute), and runs a segmented inclusive scan by
// bucket key — log2(64) steps of one general add per lane instead of up to ACC_CHUNK_N sequential adds
// in one lane.  What made the sequential version slow is exactly the data that reaches these levels: a
// bucket spread over thousands of level-1 chunks (the top window of uniform scalars has ~12 non-empty
// buckets of n/12 points each; bucket "1" of real witnesses) is a run of thousands of partials, i.e.
// serial chains of 32 general adds per level (measured 1.3-1.7 ms per level at 2^22, exposed after the
// last MSM of a proof).  A wave that finds all its slots empty (the common case after the pairwise
// merge) leaves at once; the scan stops at the first distance no lane has a partner at.  Every wave
// emits at most two partials (its first run if that does not START there, its last run if it does not
// END there), so a level shrinks the list 32x (16x for G2).
template <class R> __device__ __forceinline__ R wave_up(const R &v, uint32_t d);
template <> __device__ __forceinline__ Fq29 wave_up<Fq29>(const Fq29 &v, uint32_t d) {
    Fq29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = __shfl_up(v.l[i], d);
    return r;
}
template <> __device__ __forceinline__ Fq2s wave_up<Fq2s>(const Fq2s &v, uint32_t d) { return Fq2s{wave_up<Fq29>(v.v, d)}; }
template <class R> __device__ __forceinline__ R wave_push(const R &v, uint32_t dst_lane);       // lane L's value -> lane dst_lane (a permutation)
template <> __device__ __forceinline__ Fq29 wave_push<Fq29>(const Fq29 &v, uint32_t dst) {
    Fq29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = __builtin_amdgcn_ds_permute((int)(dst << 2), v.l[i]);
    return r;
}
template <> __device__ __forceinline__ Fq2s wave_push<Fq2s>(const Fq2s &v, uint32_t dst) { return Fq2s{wave_push<Fq29>(v.v, dst)}; }

template <class F>
__global__ __launch_bounds__(256) void k_msm_accum_wave(ACCMEM *buckets, const ACCMEM *in_part, const uint32_t *in_key,
                                                        const uint32_t *in_flag, uint32_t nitems, ACCMEM *out_part,
                                                        uint32_t *out_key, uint32_t *out_flag, uint32_t nwaves,
                                                        uint64_t bucket_stride, uint64_t ws_stride) {
    ZK_TAIL_PRIO();
    typedef LaneModel<F> LM;
    typedef typename LM::R FR;
    {
        const uint64_t bo = (uint64_t)blockIdx.y * bucket_stride, wo = (uint64_t)blockIdx.y * ws_stride;   // MSM of a batch
        buckets += bo;
        in_part += wo; in_key += wo; in_flag += wo;
        out_part += wo; out_key += wo; out_flag += wo;
    }
    constexpr uint32_t LPE = LM::LPE, EPW = 64u / LPE;          // lanes per element, elements per wave
    const uint32_t lane = threadIdx.x & 63u, w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (w >= nwaves) return;                                    // wave-uniform
    const uint32_t e = lane / LPE, comp = lane % LPE;           // this lane's element slot, component
    const uint32_t i = w * EPW + e;
    uint32_t key = i < nitems ? in_key[i] : SLOT_EMPTY;
    uint32_t flag = key != SLOT_EMPTY ? in_flag[i] : 0u;
    if (lane == 0) {                                            // ordered before the partial stores below (same wave)
        out_key[2 * (uint64_t)w] = SLOT_EMPTY;
        out_key[2 * (uint64_t)w + 1] = SLOT_EMPTY;
        out_flag[2 * (uint64_t)w] = 0;
        out_flag[2 * (uint64_t)w + 1] = 0;
    }
    const uint64_t vmask = __ballot(key != SLOT_EMPTY);
    if (vmask == 0) return;
    XYZZ<FR> v = XYZZ<FR>::inf();
    if (key != SLOT_EMPTY) v = LM::load(in_part + i);
    // compaction: valid element with `rank` valid elements before it -> element slot rank; the invalid ones fill the rest
    const uint64_t below = vmask & ((1ull << (e * LPE)) - 1ull);
    const uint32_t rank = (uint32_t)__popcll(below) / LPE, cnt = (uint32_t)__popcll(vmask) / LPE;
    const uint32_t dst_e = key != SLOT_EMPTY ? rank : cnt + (e - rank);
    const uint32_t dst = dst_e * LPE + comp;
    key = (uint32_t)__builtin_amdgcn_ds_permute((int)(dst << 2), (int)key);
    flag = (uint32_t)__builtin_amdgcn_ds_permute((int)(dst << 2), (int)flag);
    v.x = wave_push(v.x, dst); v.y = wave_push(v.y, dst); v.zz = wave_push(v.zz, dst); v.zzz = wave_push(v.zzz, dst);
    // segmented inclusive scan over the equal-key runs of elements 0 .. cnt-1
    for (uint32_t d = 1; d < EPW; d <<= 1) {
        const uint32_t kprev = __shfl_up(key, d * LPE);
        const bool take = e >= d && e < cnt && kprev == key;
        if (!__any(take)) break;                                // runs are contiguous: nothing at 2d either
        XYZZ<FR> o{wave_up(v.x, d * LPE), wave_up(v.y, d * LPE), wave_up(v.zz, d * LPE), wave_up(v.zzz, d * LPE)};
        if (take) add(v, o);
    }
    if (e >= cnt) return;
    const uint32_t knext = __shfl_down(key, LPE);
    const uint32_t kbefore = __shfl_up(key, LPE);
    const bool last = e + 1 == cnt || knext != key;
    const bool first = e == 0 || kbefore != key;
    // STARTS comes from the first element of the run, ENDS from the last one (this lane when `last`)
    const uint64_t fmask = __ballot(first);
    const uint32_t start_lane = 63u - (uint32_t)__clzll(fmask & ((2ull << lane) - 1ull));     // highest run start at or below this lane (same comp parity not needed: flags are replicated)
    const uint32_t sflag = (uint32_t)__shfl((int)flag, (int)start_lane);
    if (!last) return;
    const bool starts = (sflag & FLAG_STARTS) != 0, ends = (flag & FLAG_ENDS) != 0;
    if (starts && ends) {
        LM::store(buckets + key, v);
    } else if (!starts) {
        LM::store(out_part + 2 * (uint64_t)w, v);
        if (comp == 0) {
            out_key[2 * (uint64_t)w] = key;
            out_flag[2 * (uint64_t)w] = ends ? FLAG_ENDS : 0u;
        }
    } else {
        LM::store(out_part + 2 * (uint64_t)w + 1, v);
        if (comp == 0) {
            out_key[2 * (uint64_t)w + 1] = key;
            out_flag[2 * (uint64_t)w + 1] = FLAG_STARTS;
        }
    }
}

// workspace: level-1 slots (2 per lane) + level-2 slots + ... (geometric: < 2.2x level 1)
static inline uint32_t accum_chunk_min() {
    static const uint32_t cmin = [] { const char *e = probe_env("ZKHIP_ACC_CHUNK_MIN"); uint32_t v = e ? (uint32_t)atoi(e) : ACC_CHUNK_MIN; return v < 4u ? 4u : v; }();
    return cmin;
}
static inline uint32_t accum_chunk_max() {
    static const uint32_t cmax = [] { const char *e = probe_env("ZKHIP_ACC_CHUNK_MAX"); uint32_t v = e ? (uint32_t)atoi(e) : ACC_CHUNK_MAX; return v < 8u ? 8u : v; }();
    return cmax;
}
// chunks one round holds: what the occupancy calculator says fits on the device at once (per MSM of a batch)
template <class F>
static uint64_t accum_round_lanes(uint32_t n_msm) {
    static const uint64_t threads = [] {
        int dev = 0, cus = 256, wgs = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e == hipSuccess) {
            if constexpr (sizeof(F) == sizeof(Fq2)) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&wgs, k_msm_accum_l1_g2s, ZK_L1_BLOCK, 0);
            else e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&wgs, k_msm_accum_l1<F>, ZK_L1_BLOCK, 0);
        }
        if (e != hipSuccess || wgs < 1) { (void)hipGetLastError(); wgs = (sizeof(F) == sizeof(Fq2) ? 2 : 3) * (256 / ZK_L1_BLOCK); }
        if (const char *o = probe_env("ZKHIP_ACC_ROUND_WGS")) wgs = atoi(o) > 0 ? atoi(o) : wgs;   // workgroups per CU (probe)
        return (uint64_t)wgs * (uint64_t)ZK_L1_BLOCK * (uint64_t)cus;
    }();
    uint64_t lanes = threads / LaneModel<F>::LPE / (n_msm ? n_msm : 1);
    return lanes ? lanes : 1;
}
template <class F>
static inline uint64_t accum_lanes_for(uint64_t max_entries, uint32_t n_msm, uint32_t chunk_min = 0, uint32_t chunk_max = 0) {
    if (!max_entries) max_entries = 1;
    const uint64_t R = accum_round_lanes<F>(n_msm), cmin = chunk_min ? chunk_min : accum_chunk_min(), cmax = chunk_max ? chunk_max : accum_chunk_max();
    if (max_entries <= R * cmin) return (max_entries + cmin - 1) / cmin;       // one partial round of minimum chunks
    const uint64_t rounds = (max_entries + R * cmax - 1) / (R * cmax);
    return rounds * R;
}
uint64_t msm_accum_workspace_slots(uint64_t max_entries) {
    // one size for whichever MSM uses the workspace: single G1, one of a G1 batch, G2
    uint64_t lanes = accum_lanes_for<Fq>(max_entries, 1);
    for (uint32_t nb = 2; nb <= 3; nb++) lanes = std::max(lanes, accum_lanes_for<Fq>(max_entries, nb));
    lanes = std::max(lanes, accum_lanes_for<Fq2>(max_entries, 1));
    uint64_t total = 0;
    for (;;) {
        uint64_t slots = 2 * lanes;
        total += slots;
        if (lanes == 1) break;
        lanes = (slots + ACC_CHUNK_N - 1) / ACC_CHUNK_N;
    }
    return total;
}

template <class F>
static void launch_accum(ACCMEM *buckets, const uint32_t *offsets, const uint32_t *entries, AccumBatch batch,
                         uint32_t total_buckets, uint64_t max_entries,
                         ACCMEM *ws_part, uint32_t *ws_key, uint32_t *ws_flag, hipStream_t s, hipEvent_t *ev, AccumTail tail) {
    const uint32_t nb = batch.n ? batch.n : 1;
    // empty buckets are never written by the kernels: infinity is the all-zero pattern
    if (!tail.buckets_zeroed) ZK_HIP(hipMemsetAsync(buckets, 0, ((size_t)(nb - 1) * batch.bucket_stride + total_buckets) * sizeof(ACCMEM), s));
    const uint32_t cmin = tail.chunk_min > accum_chunk_min() ? tail.chunk_min : accum_chunk_min();      // (never more lanes than the workspace was sized for)
    uint64_t lanes = accum_lanes_for<F>(max_entries, nb, cmin, tail.chunk_max > accum_chunk_max() ? tail.chunk_max : 0u);
    if (ev) ZK_HIP(hipEventRecord(ev[0], s));          // tight bracket around the level-1 kernel (roofline timing)
    if constexpr (sizeof(F) == sizeof(Fq2)) {
        ZK_LAUNCH(k_msm_accum_l1_g2s, dim3((uint32_t)((2 * lanes + ZK_L1_BLOCK - 1) / ZK_L1_BLOCK)), dim3(ZK_L1_BLOCK), 0, s, buckets, offsets, entries,
                           reinterpret_cast<const G2Affine *>(batch.points[0]), batch.idx_min[0], batch.idx_sub[0], total_buckets, ws_part, ws_key, ws_flag,
                           (uint32_t)lanes, cmin);
    } else {
        ZK_LAUNCH(k_msm_accum_l1<F>, dim3((uint32_t)((lanes + ZK_L1_BLOCK - 1) / ZK_L1_BLOCK), nb), dim3(ZK_L1_BLOCK), 0, s, buckets, offsets, entries,
                           batch, total_buckets, ws_part, ws_key, ws_flag, (uint32_t)lanes, cmin);
    }
    if (ev) ZK_HIP(hipEventRecord(ev[1], s));
    if (skip_followups_probe()) return;
    if (tail.stream && tail.stream != s) {            // partial merges continue on the caller's follow-up stream
        ZK_HIP(hipEventRecord(tail.l1_done, s));
        ZK_HIP(hipStreamWaitEvent(tail.stream, tail.l1_done, 0));
        s = tail.stream;
    }
    if (lanes > 1)
        ZK_LAUNCH(k_msm_accum_pair<F>, dim3((uint32_t)((lanes * LaneModel<F>::LPE + 255) / 256), nb), dim3(256), 0, s, buckets,
                           (const ACCMEM *)ws_part, ws_key, (const uint32_t *)ws_flag, (uint32_t)lanes, batch.bucket_stride, batch.ws_stride);
    uint64_t off = 0;
    while (lanes > 1) {          // a single unit has no cut runs: everything it saw was complete
        uint64_t items = 2 * lanes;
        uint64_t noff = off + items;
        const uint64_t epw = 64u / LaneModel<F>::LPE;
        const uint64_t nl = (items + epw - 1) / epw;             // waves; each emits two slots
        ZK_LAUNCH(k_msm_accum_wave<F>, dim3((uint32_t)((nl + 3) / 4), nb), dim3(256), 0, s, buckets, ws_part + off,
                           ws_key + off, ws_flag + off, (uint32_t)items, ws_part + noff, ws_key + noff, ws_flag + noff, (uint32_t)nl,
                           batch.bucket_stride, batch.ws_stride);
        off = noff;
        lanes = nl;
    }
    ZK_LAUNCH_OK("msm bucket accumulation");
}

static uint32_t gather_mask_env() {      // ZKHIP_GATHER_MASK (-DZK_PROBES builds only, WRONG results): confine the G1 table gathers to the low rows
    static const uint32_t m = [] { const char *e = probe_env("ZKHIP_GATHER_MASK"); return e ? (uint32_t)strtoul(e, nullptr, 0) : 0xffffffffu; }();
    return m;
}
static AccumBatch single(const void *points, uint32_t idx_min, uint32_t idx_sub) {
    AccumBatch b;
    memset(&b, 0, sizeof b);
    b.n = 1;
    b.gather_mask = gather_mask_env();
    b.points[0] = points;
    b.idx_min[0] = idx_min;
    b.idx_sub[0] = idx_sub;
    return b;
}

void launch_msm_accum_g1(G1Acc *buckets, const uint32_t *offsets, const uint32_t *entries, const G1Affine *points,
                         uint32_t idx_min, uint32_t idx_sub, uint32_t total, uint64_t max_entries, G1Acc *ws_part,
                         uint32_t *ws_key, uint32_t *ws_flag, hipStream_t s, hipEvent_t *ev, AccumTail tail) {
    launch_accum<Fq>(buckets, offsets, entries, single(points, idx_min, idx_sub), total, max_entries, ws_part, ws_key, ws_flag, s, ev, tail);
}
void launch_msm_accum_g1_batch(G1Acc *buckets, const uint32_t *offsets, const uint32_t *entries, const AccumBatch &batch, uint32_t total,
                               uint64_t max_entries, G1Acc *ws_part, uint32_t *ws_key, uint32_t *ws_flag, hipStream_t s, hipEvent_t *ev,
                               AccumTail tail) {
    AccumBatch b = batch;
    b.gather_mask = gather_mask_env();
    launch_accum<Fq>(buckets, offsets, entries, b, total, max_entries, ws_part, ws_key, ws_flag, s, ev, tail);
}
void launch_msm_accum_g2(G2Acc *buckets, const uint32_t *offsets, const uint32_t *entries, const G2Affine *points,
                         uint32_t idx_min, uint32_t idx_sub, uint32_t total, uint64_t max_entries, G2Acc *ws_part,
                         uint32_t *ws_key, uint32_t *ws_flag, hipStream_t s, hipEvent_t *ev, AccumTail tail) {
    launch_accum<Fq2>(buckets, offsets, entries, single(points, idx_min, idx_sub), total, max_entries, ws_part, ws_key, ws_flag, s, ev, tail);
}

}   // namespace zk
