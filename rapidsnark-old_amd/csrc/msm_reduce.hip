// MSM step 4 (overview: msm_lanes.hpp): bucket reductions (chunked + tree, split, bit sums), their choosers and scratch sizing.
#include <stdlib.h>
#include "hipcheck.hpp"
#include "msm_lanes.hpp"

namespace zk {

#define REDUCE_CHUNK 16u
#define REDUCE_THREADS 256u

// Large bucket sets, first level: lane t of a set takes the buckets t*chunk .. t*chunk + chunk - 1, so that
// (k+1) = t*chunk + (j+1) splits  sum_k (k+1) B_k  =  chunk * sum_t t*T_t  +  sum_t A_t   with T_t = sum_j B[t*chunk+j] and
// A_t = sum_j (j+1)*B[t*chunk+j]: two additions per bucket and NO per-lane scalar multiplication (the chunked form below
// pays ~28 point operations per lane for lo*T on top of its 32).  sum_t t*T_t is the same problem on the L - 1 points
// T_1 .. T_(L-1) (stored shifted by one; the chunked form finishes it), the A_t are a plain tree sum.
template <class F>
__global__ __launch_bounds__(128) void k_msm_reduce_split(ACCMEM *A, uint32_t a_stride, ACCMEM *T, const ACCMEM *buckets, uint32_t nbuckets, uint32_t chunk, uint32_t L) {
    ZK_TAIL_PRIO();
    typedef LaneModel<F> LM;
    typedef typename LM::R FR;
    const uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) / LM::LPE;
    if (t >= L) return;
    const ACCMEM *B = buckets + (uint64_t)blockIdx.y * nbuckets + (uint64_t)t * chunk;
    XYZZ<FR> run = XYZZ<FR>::inf(), sum = XYZZ<FR>::inf();
    for (int j = (int)chunk - 1; j >= 0; j--) {
        add(run, LM::load(B + j));
        add(sum, run);
    }
    LM::store(A + (uint64_t)blockIdx.y * a_stride + t, sum);
    if (t == 0) run = XYZZ<FR>::inf();                                     // weight 0; its slot is the (empty) last one
    LM::store(T + (uint64_t)blockIdx.y * L + (t ? t - 1 : L - 1), run);
}

// Lane per chunk of REDUCE_CHUNK buckets: running sums give A = sum (j+1)*B[lo+j], T = sum B;
// X = A + lo*T is the chunk's share of sum_k (k+1)*B_k.
template <class F>
__global__ __launch_bounds__(128) void k_msm_reduce_chunks(ACCMEM *scratch, uint32_t out_stride, const ACCMEM *buckets, uint32_t nbuckets,
                                                           uint32_t chunk, uint32_t total_chunks) {
    ZK_TAIL_PRIO();
    typedef LaneModel<F> LM;
    typedef typename LM::R FR;
    uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) / LM::LPE;
    if (t >= total_chunks) return;
    const uint32_t chunks_per_window = nbuckets / chunk;
    const uint32_t cw = t % chunks_per_window;          // chunk index inside its window
    const ACCMEM *B = buckets + (uint64_t)t * chunk;    // windows (and MSMs) are laid back to back
    XYZZ<FR> run = XYZZ<FR>::inf(), sum = XYZZ<FR>::inf();
    for (int j = (int)chunk - 1; j >= 0; j--) {
        add(run, LM::load(B + j));
        add(sum, run);
    }
    // sum += (cw*chunk) * run   — double-and-add, MSB first
    uint32_t k = cw * chunk;
    if (k) {
        XYZZ<FR> m = XYZZ<FR>::inf();
        for (int bit = 31 - __clz(k); bit >= 0; bit--) {
            m = dbl(m);
            if ((k >> bit) & 1u) add(m, run);
        }
        add(sum, m);
    }
    LM::store(scratch + (uint64_t)(t / chunks_per_window) * out_stride + cw, sum);      // (out_stride = chunks per set: back to back)
}

// Tree sum of `count` consecutive points per group, 2 inputs per lane + an LDS tree per workgroup:
// grid (blocks_per_group, groups) -> one point per workgroup.  Launched repeatedly until one point
// per (msm, window) is left; the last launch stores in the zkey's 2^256 Montgomery form.
template <class F>
static constexpr uint32_t tree_in() { return 2u * REDUCE_THREADS / LaneModel<F>::LPE; }    // inputs per workgroup
#define TREE_IN_MIN REDUCE_THREADS      // the smaller fan-in (G2): sizes the shared scratch formula
template <class F>
__global__ __launch_bounds__(REDUCE_THREADS) void k_msm_reduce_tree(ACCMEM *out, XYZZ<F> *out_final, const ACCMEM *in, uint32_t count, uint32_t last) {
    ZK_TAIL_PRIO();
    extern __shared__ uint32_t lds_raw[];
    typedef LaneModel<F> LM;
    typedef typename LM::R FR;
    constexpr uint32_t NE = REDUCE_THREADS / LM::LPE;           // elements per workgroup pass
    XYZZ<FR> *lds = reinterpret_cast<XYZZ<FR> *>(lds_raw);      // one entry per lane (its component(s))
    const ACCMEM *X = in + (uint64_t)blockIdx.y * count;
    const uint32_t e = threadIdx.x / LM::LPE;
    const uint32_t i0 = blockIdx.x * (2u * NE) + e, i1 = i0 + NE;
    XYZZ<FR> acc = XYZZ<FR>::inf();
    if (i0 < count) acc = LM::load(X + i0);
    if (i1 < count) add(acc, LM::load(X + i1));
    lds[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t s = NE / 2; s > 0; s >>= 1) {
        if (e < s) {
            XYZZ<FR> o = lds[threadIdx.x + s * LM::LPE];
            add(acc, o);
            lds[threadIdx.x] = acc;
        }
        __syncthreads();
    }
    if (e == 0) {
        const uint64_t at = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
        if (last) LM::store256(out_final + at, acc);    // window sums: canonical words, back in the zkey's 2^256 form
        else LM::store(out + at, acc);
    }
}

// Last launch of the split form: per set, the partial sums of the shares X (cnt_x points at P) and of the A level (cnt_a
// points behind them) are summed in the two halves of ONE LDS tree;  window sum = 2^scale_log * sum X + sum A.
template <class F>
__global__ __launch_bounds__(REDUCE_THREADS) void k_msm_reduce_final2(XYZZ<F> *out_final, const ACCMEM *P, uint32_t cnt_x, uint32_t cnt_a, uint32_t scale_log) {
    ZK_TAIL_PRIO();
    extern __shared__ uint32_t lds_raw[];
    typedef LaneModel<F> LM;
    typedef typename LM::R FR;
    constexpr uint32_t H = REDUCE_THREADS / LM::LPE / 2;        // elements per half: 2H inputs each
    XYZZ<FR> *lds = reinterpret_cast<XYZZ<FR> *>(lds_raw);
    const uint32_t e = threadIdx.x / LM::LPE;
    const bool xs = e >= H;                                      // upper half: the shares X;  lower half: A
    const uint32_t eh = xs ? e - H : e, cnt = xs ? cnt_x : cnt_a;
    const ACCMEM *in = P + (uint64_t)blockIdx.x * (cnt_x + cnt_a) + (xs ? 0u : cnt_x);
    XYZZ<FR> acc = XYZZ<FR>::inf();
    if (eh < cnt) acc = LM::load(in + eh);
    if (eh + H < cnt) add(acc, LM::load(in + eh + H));
    lds[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t s = H / 2; s > 0; s >>= 1) {
        if (eh < s) {
            XYZZ<FR> o = lds[threadIdx.x + s * LM::LPE];
            add(acc, o);
            lds[threadIdx.x] = acc;
        }
        __syncthreads();
    }
    if (xs && eh == 0) {
        for (uint32_t i = 0; i < scale_log; i++) acc = dbl(acc);
        lds[threadIdx.x] = acc;
    }
    __syncthreads();
    if (e == 0) {
        XYZZ<FR> o = lds[threadIdx.x + H * LM::LPE];
        add(acc, o);
        LM::store256(out_final + blockIdx.x, acc);
    }
}

// ---- bit-sum reduction: small bucket sets ---------------------------------------------------------------
// sum_k (k+1) B_k = T + sum_j 2^j S_j with T = sum_k B_k and S_j = sum of the buckets whose index has bit j
// set.  The c sums (T, S_0 .. S_{c-2}) come out of ONE binary tree: a block of 2^m buckets carries m+1 sums;
// joining siblings L (bit m clear) and R (bit m set) is  T = T_L + T_R,  S_j = S_j^L + S_j^R (j < m),
// S_m = T_R  — m+1 INDEPENDENT additions per join, so every level is one addition deep and the whole
// reduction is c-1 additions deep (≈ 0.1 ms), where the chunked form above is a serial chain of 2*chunk
// additions plus a ~c-step double-and-add per lane and then an LDS tree (0.35-0.5 ms per launch pair, a third
// of a small proof's kernel time).  The c sums go to the host, whose serial Horner over c-1 bits costs
// microseconds.  Used while a launch reduces at most 2^16 buckets (circuits up to 2^18 constraints); the chunked
// form stays for the large sets, where work, not depth, is what counts.  In place: a block of size 2^m keeps T in its slot 0 and S_j in slot 1+j.
#define BITS_RS 18u         // slots per block record in global memory (>= c)
template <class F>
__global__ __launch_bounds__(REDUCE_THREADS) void k_msm_reduce_bits_block(ACCMEM *rec, XYZZ<F> *final_out, const ACCMEM *buckets,
                                                                         uint32_t nbuckets, uint32_t c, uint32_t nblk) {
    ZK_TAIL_PRIO();
    extern __shared__ uint32_t lds_raw[];
    typedef LaneModel<F> LM;
    typedef typename LM::R FR;
    constexpr uint32_t NE = REDUCE_THREADS / LM::LPE;           // buckets per workgroup: 256 (G1), 128 (G2)
    constexpr uint32_t LB = LM::LPE == 1 ? 8u : 7u;
    XYZZ<FR> *lds = reinterpret_cast<XYZZ<FR> *>(lds_raw);      // slot s of the block: lds[s * LPE + component]
    const uint32_t e = threadIdx.x / LM::LPE, comp = threadIdx.x % LM::LPE;
    const uint32_t group = blockIdx.y, blk = blockIdx.x;
    const uint32_t k = blk * NE + e;
    lds[threadIdx.x] = k < nbuckets ? LM::load(buckets + (uint64_t)group * nbuckets + k) : XYZZ<FR>::inf();
    __syncthreads();
#pragma unroll 1
    for (uint32_t m = 0; m < LB; m++) {
        const uint32_t per = m + 2, ng = NE >> (m + 1);
        const uint32_t g = e / per, i = e % per;
        if (g < ng) {
            const uint32_t L = g << (m + 1), R = L + (1u << m);
            if (i <= m) {                                   // i = 0: T; i = 1 + j: S_j
                XYZZ<FR> a = lds[(L + i) * LM::LPE + comp];
                add(a, lds[(R + i) * LM::LPE + comp]);
                lds[(L + i) * LM::LPE + comp] = a;
            } else if (m >= 2) {                            // S_m = T_R (for m < 2 that slot IS R's slot 0)
                lds[(L + m + 1) * LM::LPE + comp] = lds[R * LM::LPE + comp];
            }
        }
        __syncthreads();
    }
    if (e <= LB && e < c) {
        const XYZZ<FR> v = lds[threadIdx.x];
        if (nblk == 1) LM::store256(final_out + (uint64_t)group * c + e, v);
        else LM::store(rec + ((uint64_t)group * nblk + blk) * BITS_RS + e, v);
    }
}
// the levels above the blocks, one workgroup per bucket set, on the block records in global memory
template <class F>
__global__ __launch_bounds__(REDUCE_THREADS) void k_msm_reduce_bits_top(XYZZ<F> *final_out, ACCMEM *rec, uint32_t nblk, uint32_t c) {
    ZK_TAIL_PRIO();
    typedef LaneModel<F> LM;
    typedef typename LM::R FR;
    constexpr uint32_t NE = REDUCE_THREADS / LM::LPE;
    constexpr uint32_t LB = LM::LPE == 1 ? 8u : 7u;
    const uint32_t e = threadIdx.x / LM::LPE;
    ACCMEM *R0 = rec + (uint64_t)blockIdx.x * nblk * BITS_RS;
#pragma unroll 1
    for (uint32_t m = LB; m + 1 < c; m++) {
        const uint32_t span = 1u << (m - LB), per = m + 2, ntasks = (nblk >> (m - LB + 1)) * per;
#pragma unroll 1
        for (uint32_t t = e; t < ntasks; t += NE) {
            const uint32_t g = t / per, i = t % per;
            ACCMEM *L = R0 + (uint64_t)g * 2u * span * BITS_RS, *R = L + (uint64_t)span * BITS_RS;
            if (i <= m) {
                XYZZ<FR> a = LM::load(L + i);
                add(a, LM::load(R + i));
                LM::store(L + i, a);
            } else {
                LM::store(L + m + 1, LM::load(R));
            }
        }
        __threadfence_block();
        __syncthreads();
    }
    if (e < c) LM::store256(final_out + (uint64_t)blockIdx.x * c + e, LM::load(R0 + e));
}
static inline bool reduce_bits_for(MsmPlan p) {
    static const int forced = [] { const char *e = probe_env("ZKHIP_REDUCE_BITS"); return e ? atoi(e) : -1; }();
    if (p.c > BITS_RS || (uint64_t)p.sets * p.nbuckets > (1u << 16)) return false;      // large sets: work, not depth, counts (2^22 with plain tables: +0.6 %)
    return forced < 0 ? true : forced != 0;
}
uint32_t msm_wsum_rc(MsmPlan p) { return reduce_bits_for(p) ? p.c : 1u; }

// Buckets per lane of k_msm_reduce_chunks.  16 is the cheapest in total work (2 adds per bucket + one ~20-op
// scalar multiplication per chunk); but a lane's chain is serial (32 + ~20 general adds of ~7 us each), and
// with few buckets (small circuits, shards) the launch is a handful of waves whose latency — not work — is
// what the proof waits for (2^16: 321 us per launch, the largest single item of a proof): smaller chunks
// there (ZKHIP_REDUCE_CHUNK overrides, tuning aid).
static inline uint32_t reduce_chunk_for(MsmPlan p) {
    static const uint32_t forced = [] { const char *e = probe_env("ZKHIP_REDUCE_CHUNK"); return e ? (uint32_t)atoi(e) : 0u; }();
    uint32_t chunk = REDUCE_CHUNK;
    if (forced) chunk = forced;
    else if ((uint64_t)p.sets * p.nbuckets <= (1u << 16)) chunk = 4;
    return p.nbuckets < chunk ? p.nbuckets : chunk;
}

// Buckets per lane of k_msm_reduce_split (0: the chunked form alone).  Sets of 2^14 buckets and more: below that a launch is
// a handful of waves and the chunked form's depth is what counts.  ZKHIP_REDUCE_SPLIT overrides (tuning aid; 0 = off).
#define REDUCE_SPLIT 16u
// chunk of the chunked form on the T level (L points per set): 8 where that leaves whole tree workgroups of shares, else 4
// (2^22 / 2^20, periods with 8 against 4: -0.6 % / -0.5 %, profiles/r05zd_split_parameters.txt)
static inline uint32_t reduce_split_top(uint32_t L) {
    static const uint32_t forced = [] { const char *e = probe_env("ZKHIP_REDUCE_SPLIT_TOP"); const uint32_t t = e ? (uint32_t)atoi(e) : 0u; return t >= 2u && (t & (t - 1)) == 0 ? t : 0u; }();
    if (forced) return forced;
    return (L / 8u) % (2u * REDUCE_THREADS) == 0 ? 8u : 4u;
}
static inline uint32_t reduce_split_for(MsmPlan p) {
    static const int forced = [] { const char *e = probe_env("ZKHIP_REDUCE_SPLIT"); return e ? atoi(e) : -1; }();
    if (reduce_bits_for(p) || p.nbuckets < (1u << 14)) return 0;
    // (sets of more than 2^19 buckets: longer lanes, so that the T level stays the 2^15 points the last two launches are sized for)
    const uint32_t ch = forced >= 0 ? (uint32_t)forced : (p.nbuckets > (REDUCE_SPLIT << 15) ? p.nbuckets >> 15 : REDUCE_SPLIT);
    if (ch < 2 || (ch & (ch - 1)) != 0 || ch > p.nbuckets) return 0;
    // the last two launches take the shares and the A level together (k_msm_reduce_final2): whole tree workgroups of
    // shares, and at most one final half of partial sums, for both fan-ins
    const uint32_t L = p.nbuckets / ch;
    return L >= 8u && (L / reduce_split_top(L)) % (2u * REDUCE_THREADS) == 0 && L / TREE_IN_MIN <= REDUCE_THREADS / 2u ? ch : 0u;
}

// points of a tree's input and of every level above it (a geometric tail; upper bound for both fan-ins)
static inline uint64_t tree_points(uint64_t groups, uint64_t cnt) {
    uint64_t total = 0;
    for (;;) {
        total += groups * cnt;
        if (cnt == 1) break;
        cnt = (cnt + TREE_IN_MIN - 1) / TREE_IN_MIN;
    }
    return total + groups;      // (a one-point input still gets its output slot)
}
// scratch: chunk sums + the intermediate levels of the tree; the split form: T, its chunk sums and tree, A and its tree
uint64_t msm_reduce_scratch_points(uint32_t n_msm, MsmPlan p) {
    if (reduce_bits_for(p)) return (uint64_t)n_msm * p.sets * (p.nbuckets / 128u + 1u) * BITS_RS;      // block records (G2 blocks are the smaller)
    const uint64_t groups = (uint64_t)n_msm * p.sets;
    if (const uint32_t ch = reduce_split_for(p)) {
        const uint64_t L = p.nbuckets / ch;
        return groups * L + tree_points(groups, L / reduce_split_top((uint32_t)L) + L);      // T; shares and A side by side, the partial sums behind them
    }
    return tree_points(groups, p.nbuckets / reduce_chunk_for(p));
}

template <class F>
static void launch_reduce(XYZZ<F> *window_sums, ACCMEM *scratch, const ACCMEM *buckets, uint32_t n_msm, MsmPlan p, hipStream_t s) {
    if (skip_followups_probe()) return;
    if (reduce_bits_for(p)) {          // c sums per bucket set (msm_wsum_rc), the host finishes
        const uint32_t NE = REDUCE_THREADS / LaneModel<F>::LPE, groups = n_msm * p.sets;
        const uint32_t nblk = p.nbuckets > NE ? p.nbuckets / NE : 1u;
        const size_t lds = REDUCE_THREADS * sizeof(XYZZ<typename LaneModel<F>::R>);
        ZK_LAUNCH(k_msm_reduce_bits_block<F>, dim3(nblk, groups), dim3(REDUCE_THREADS), lds, s, scratch, window_sums, buckets, p.nbuckets, p.c, nblk);
        if (nblk > 1) ZK_LAUNCH(k_msm_reduce_bits_top<F>, dim3(groups), dim3(REDUCE_THREADS), 0, s, window_sums, scratch, nblk, p.c);
        ZK_LAUNCH_OK("msm bucket reduction (bit sums)");
        return;
    }
    const uint32_t groups = n_msm * p.sets;
    const size_t lds = REDUCE_THREADS * sizeof(XYZZ<typename LaneModel<F>::R>);
    const uint32_t TREE_IN = tree_in<F>();
    auto chunks = [&](ACCMEM *out, uint32_t out_stride, const ACCMEM *in, uint32_t n, uint32_t chunk) {      // sum_k (k+1) in[k] over n points per set -> n / chunk shares
        const uint32_t total_chunks = groups * (n / chunk);
        ZK_LAUNCH(k_msm_reduce_chunks<F>, dim3((total_chunks * LaneModel<F>::LPE + 127) / 128), dim3(128), 0, s, out, out_stride, in, n, chunk, total_chunks);
    };
    if (const uint32_t ch = reduce_split_for(p)) {
        const uint32_t L = p.nbuckets / ch, top = reduce_split_top(L), nx = L / top, per = nx + L;      // per set: nx shares, then the L points of the A level
        ACCMEM *T = scratch, *Y = T + (uint64_t)groups * L, *P = Y + (uint64_t)groups * per;
        ZK_LAUNCH(k_msm_reduce_split<F>, dim3((L * LaneModel<F>::LPE + 127) / 128, groups), dim3(128), 0, s, Y + nx, per, T, buckets, p.nbuckets, ch, L);
        chunks(Y, per, T, L, top);
        const uint32_t bx = nx / TREE_IN, ba = L / TREE_IN;        // whole workgroups of each kind (reduce_split_for)
        ZK_LAUNCH(k_msm_reduce_tree<F>, dim3(bx + ba, groups), dim3(REDUCE_THREADS), lds, s, P, window_sums, (const ACCMEM *)Y, per, 0u);
        ZK_LAUNCH(k_msm_reduce_final2<F>, dim3(groups), dim3(REDUCE_THREADS), lds, s, window_sums, (const ACCMEM *)P, bx, ba, (uint32_t)__builtin_ctz(ch));
        ZK_LAUNCH_OK("msm bucket reduction (split)");
        return;
    }
    const uint32_t chunk = reduce_chunk_for(p);
    uint32_t cnt = p.nbuckets / chunk;
    chunks(scratch, cnt, buckets, p.nbuckets, chunk);
    ACCMEM *in = scratch;
    for (;;) {
        const uint32_t blocks = (cnt + TREE_IN - 1) / TREE_IN;
        const bool last = blocks == 1;
        ACCMEM *out = in + (uint64_t)groups * cnt;
        ZK_LAUNCH(k_msm_reduce_tree<F>, dim3(blocks, groups), dim3(REDUCE_THREADS), lds, s, out, window_sums, (const ACCMEM *)in, cnt, last ? 1u : 0u);
        if (last) break;
        in = out;
        cnt = blocks;
    }
    ZK_LAUNCH_OK("msm bucket reduction");
}
void launch_msm_reduce_g1(G1XYZZ *ws, G1Acc *scratch, const G1Acc *buckets, uint32_t n_msm, MsmPlan p, hipStream_t s) {
    launch_reduce<Fq>(ws, scratch, buckets, n_msm, p, s);
}
void launch_msm_reduce_g2(G2XYZZ *ws, G2Acc *scratch, const G2Acc *buckets, uint32_t n_msm, MsmPlan p, hipStream_t s) {
    launch_reduce<Fq2>(ws, scratch, buckets, n_msm, p, s);
}

}   // namespace zk
