// Running products over Fr (include/zkhip.h, section "Grand products and batch inversion over Fr"): batch inversion, prefix
// products, the grand product of ratios and the accumulator of PLONK's permutation argument.  Nothing in the reference
// corresponds to it (it proves Groth16 only); the counterpart is round 2 of snarkjs's PLONK prover.  DESIGN.md section 27
// describes the scan and states what was measured.
//
// The identity.  With T = prod den_j, 1 / (den_0 .. den_(i-1)) = (den_i .. den_(n-1)) / T, so
//     z_i = (exclusive prefix product of num)_i * (inclusive suffix product of den)_i / T       and
//     1 / a_i = (exclusive prefix product of a)_i * (exclusive suffix product of a)_i / T:
// a prefix scan, a suffix scan and ONE inversion for the whole vector.
//
// Tiers (the lane's span, the shuffles and the uniform loads are devmem.hpp's), with the operator P_i = a_i P_(i-1) (no
// weights: a product has none):
//   lane       `seg` consecutive elements by a chain of products (ZKHIP_SCAN_SEG, read at every call)
//   wave       64 lanes: a prefix scan of the lanes' products by six __shfl_up steps, a suffix scan by six __shfl_down steps
//   workgroup  4 waves: their totals meet in LDS
//   carry      the workgroups' totals are scanned by ONE workgroup (k_scan_carry), every lane taking ceil(groups / 256) of
//              them
// Three launches: k_scan_reduce (what lies before / behind every lane within its wave, wave and workgroup totals),
// k_scan_carry, k_scan_apply (a lane runs its chain again from what lies before its segment, storing every step, then runs
// back from what lies behind it).  The one inversion is the HOST's, between the last two (launch_scan): measured, a^(r-2)
// in one lane of the carry workgroup took 0.68 ms, the round trip of 96 bytes 0.10 ms.  No atomics: which products are
// formed depends on indices only, and the arithmetic is exact, so the bytes do not depend on scheduling or on seg.
//
// Forms.  I/O is STANDARD; Fr::mul(x, y) = x y / R (R = 2^256).  A chain over standard factors is never converted: a chain
// of m such factors from a Montgomery seed carries R^-m, which depends on the lane map only, and the host hands the kernels
// the two powers of R that cancel it (ScanConsts::lift, ::tail).  A lane short of seg elements pads its chain with products
// by 1, so that every lane carries the same power.  Everything a tier above the lane touches is Montgomery.
// Field arithmetic: field.hpp's 8 x 32-bit Fr.
#include "hiputil.hpp"
#include "devmem.hpp"
#include "ptengine.hpp"
#include "lanepow.hpp"
#include "plonk_internal.hpp"

namespace {

constexpr uint32_t SC_WG = 256, SC_WAVES = SC_WG / 64;
constexpr uint32_t DEFAULT_SEG = 8, MAX_SEG = 4096;   // the default: the best of profiles/frscan_timing.txt's sweep at 2^20
constexpr uint32_t MAX_COLS = 8, MAX_LOG_N = 28;
constexpr int OP_PREFIX = 0, OP_INVERSE = 1, OP_GRAND = 2, OP_PLONK = 3;

static_assert(sizeof(Fr) == 32, "layout");

// ---------------------------------------------------------------- device
// The constants of one call, made on the host
struct ScanConsts {
    Fr lift;                                          // R^(f seg + 1), f factors an element: a lane's raw chain -> Montgomery
    Fr tail;                                          // R^e / T: what the backward chain starts with; the host sets it after k_scan_carry (launch_scan)
    Fr beta, omega;                                   // Montgomery
    Fr gamma;                                         // standard
    Fr wtab[POW_TAB];                                 // omega^(seg 2^b), Montgomery: a lane's starting power from the bits of its index
};

struct ScanArgs {
    const Fr *a;                                      // PREFIX, INVERSE: the values; GRAND: num; PLONK: wires (cols x n)
    const Fr *b;                                      // GRAND: den; PLONK: sigmas (cols x n)
    const Fr *shifts;                                 // PLONK: cols values, standard
    Fr *out;                                          // n values
    uint64_t n;
    uint32_t seg, cols, exclusive;
    const ScanConsts *k;
    Fr *lnum, *lden;                                  // per lane: what lies before it (num) / behind it (den) within its wave
    Fr *wnum, *wden;                                  // per wave: its total
    Fr *gnum, *gden;                                  // per workgroup: its total
    Fr *before, *behind;                              // per workgroup: what lies before it (num) / behind it (den)
};

__device__ __forceinline__ Fr raw_one() {             // 1 in standard form: a product by it divides by R
    Fr r = Fr::zero();
    r.v[0] = 1;
    return r;
}

// v of lane l <- v_0 .. v_l
__device__ __forceinline__ Fr wave_prefix(Fr v, uint32_t lane) {
#pragma unroll 1
    for (uint32_t k = 0; k < 6; k++) {
        const Fr t = shfl_up_fr(v, 1u << k);
        if (lane >= (1u << k)) v = Fr::mul(t, v);
    }
    return v;
}
// v of lane l <- v_l .. v_63
__device__ __forceinline__ Fr wave_suffix(Fr v, uint32_t lane) {
#pragma unroll 1
    for (uint32_t k = 0; k < 6; k++) {
        const Fr t = shfl_down_fr(v, 1u << k);
        if (lane + (1u << k) < 64) v = Fr::mul(v, t);
    }
    return v;
}

// A lane's walk over its elements: num(p, i) multiplies p by the forward factors of element i (called with rising i),
// den(s, i) multiplies s by its backward factors (any order).  PLONK builds the factors here: no num or den array exists
template <int OP>
struct Walk {
    const ScanArgs &A;
    Fr x, beta, gamma, omega;                         // PLONK: x = beta w^i, Montgomery
    __device__ __forceinline__ Walk(const ScanArgs &A_, uint64_t first_lane) : A(A_) {
        if constexpr (OP == OP_PLONK) {
            beta = load_uniform(&A.k->beta);
            gamma = load_uniform(&A.k->gamma);
            omega = load_uniform(&A.k->omega);
            x = beta;                                 // times w^(seg L), L the lane's index, by the bits of L
            const uint64_t L = first_lane + threadIdx.x;
#pragma unroll 1
            for (uint32_t b = 0; b < POW_TAB && (L >> b); b++)
                if ((L >> b) & 1) x = Fr::mul(x, load_el(A.k->wtab + b));
        }
    }
    __device__ __forceinline__ void num(Fr &p, uint64_t i) {
        if constexpr (OP == OP_PLONK) {
#pragma unroll 1
            for (uint32_t j = 0; j < A.cols; j++) {
                const Fr f = Fr::add(Fr::add(load_el(A.a + j * A.n + i), Fr::mul(x, load_uniform(A.shifts + j))), gamma);
                p = Fr::mul(p, f);
            }
            x = Fr::mul(x, omega);
        } else if constexpr (OP == OP_INVERSE) {
            const Fr v = load_el(A.a + i);
            p = Fr::mul(p, v.is_zero() ? raw_one() : v);
        } else {
            p = Fr::mul(p, load_el(A.a + i));
        }
    }
    __device__ __forceinline__ void den(Fr &s, uint64_t i) {
        if constexpr (OP == OP_PLONK) {
#pragma unroll 1
            for (uint32_t j = 0; j < A.cols; j++) {
                const Fr f = Fr::add(Fr::add(load_el(A.a + j * A.n + i), Fr::mul(beta, load_el(A.b + j * A.n + i))), gamma);
                s = Fr::mul(s, f);
            }
        } else if constexpr (OP == OP_GRAND) {
            s = Fr::mul(s, load_el(A.b + i));
        }
    }
    // the chain of a lane short of seg elements: the factors it lacks are 1
    __device__ __forceinline__ void pad(Fr &v, uint32_t cnt) {
        const uint32_t f = OP == OP_PLONK ? A.cols : 1;
#pragma unroll 1
        for (uint32_t k = (A.seg - cnt) * f; k-- > 0;) v = Fr::mul(v, raw_one());
    }
};

// lnum[L], lden[L], wnum[4 g + w], wden[4 g + w], gnum[g], gden[g] (Montgomery).  PREFIX has no den; INVERSE's den is its num
template <int OP>
__global__ __launch_bounds__(SC_WG) void k_scan_reduce(ScanArgs A) {
    __shared__ Fr shn[SC_WAVES], shd[SC_WAVES];
    constexpr bool TWO = OP == OP_GRAND || OP == OP_PLONK, DEN = OP != OP_PREFIX;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t first = (uint64_t)blockIdx.x * SC_WG, L = first + threadIdx.x;
    uint64_t lo;
    const uint32_t cnt = lane_span(lo, first, A.n, A.seg);
    Fr vn = Fr::one(), vd = Fr::one();
    if (cnt) {
        Walk<OP> wk(A, first);
#pragma unroll 1
        for (uint32_t k = 0; k < cnt; k++) {
            wk.num(vn, lo + k);
            if constexpr (TWO) wk.den(vd, lo + k);
        }
        if (cnt < A.seg) {
            wk.pad(vn, cnt);
            if constexpr (TWO) wk.pad(vd, cnt);
        }
        const Fr lift = load_uniform(&A.k->lift);
        vn = Fr::mul(vn, lift);
        if constexpr (TWO) vd = Fr::mul(vd, lift);
    }
    if constexpr (OP == OP_INVERSE) vd = vn;
    const Fr in = wave_prefix(vn, lane);
    Fr t = shfl_up_fr(in, 1);
    if (lane == 0) t = Fr::one();
    store_el(A.lnum + L, t);
    if (lane == 63) {
        store_el(A.wnum + (uint64_t)blockIdx.x * SC_WAVES + w, in);
        shn[w] = in;
    }
    if constexpr (DEN) {
        const Fr id = wave_suffix(vd, lane);
        t = shfl_down_fr(id, 1);
        if (lane == 63) t = Fr::one();
        store_el(A.lden + L, t);
        if (lane == 0) {
            store_el(A.wden + (uint64_t)blockIdx.x * SC_WAVES + w, id);
            shd[w] = id;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Fr g = shn[0];
#pragma unroll 1
        for (uint32_t j = 1; j < SC_WAVES; j++) g = Fr::mul(g, shn[j]);
        store_el(A.gnum + blockIdx.x, g);
        if constexpr (DEN) {
            g = shd[0];
#pragma unroll 1
            for (uint32_t j = 1; j < SC_WAVES; j++) g = Fr::mul(g, shd[j]);
            store_el(A.gden + blockIdx.x, g);
        }
    }
}

// what k_scan_carry takes of ScanArgs
struct CarryArgs {
    const Fr *gnum, *gden;
    Fr *before, *behind, *total;
};

// before[g] = gnum[0] .. gnum[g - 1]; with a den: behind[g] = gden[g + 1] .. gden[groups - 1], total[0] = prod gnum and
// total[1] = T = prod gden (all Montgomery).  ONE workgroup, lane l takes the totals [l cseg, (l + 1) cseg).  The host inverts
// T between this launch and k_scan_apply (launch_scan)
__global__ __launch_bounds__(SC_WG) void k_scan_carry(CarryArgs A, uint64_t groups, uint32_t cseg, uint32_t has_den) {
    __shared__ Fr shn[SC_WAVES], shd[SC_WAVES];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t lo;
    const uint32_t cnt = lane_span(lo, 0, groups, cseg);
    Fr on = Fr::one(), od = Fr::one();
#pragma unroll 1
    for (uint32_t k = 0; k < cnt; k++) {
        on = Fr::mul(on, load_el(A.gnum + lo + k));
        if (has_den) od = Fr::mul(od, load_el(A.gden + lo + k));
    }
    const Fr in = wave_prefix(on, lane), id = wave_suffix(od, lane);
    if (lane == 63) shn[w] = in;
    if (lane == 0) shd[w] = id;
    __syncthreads();
    Fr en = shfl_up_fr(in, 1), ed = shfl_down_fr(id, 1);
    if (lane == 0) en = Fr::one();
    if (lane == 63) ed = Fr::one();
#pragma unroll 1
    for (uint32_t j = 0; j < w; j++) en = Fr::mul(shn[j], en);
#pragma unroll 1
    for (uint32_t k = 0; k < cnt; k++) {
        store_el(A.before + lo + k, en);
        en = Fr::mul(en, load_el(A.gnum + lo + k));
    }
    if (!has_den) return;
#pragma unroll 1
    for (uint32_t j = SC_WAVES - 1; j > w; j--) ed = Fr::mul(ed, shd[j]);
    if (threadIdx.x == 0) {
        Fr tn = shn[0], td = shd[0];
#pragma unroll 1
        for (uint32_t j = 1; j < SC_WAVES; j++) {
            tn = Fr::mul(tn, shn[j]);
            td = Fr::mul(td, shd[j]);
        }
        store_el(A.total, tn);
        store_el(A.total + 1, td);
    }
#pragma unroll 1
    for (uint32_t k = cnt; k-- > 0;) {
        store_el(A.behind + lo + k, ed);
        ed = Fr::mul(ed, load_el(A.gden + lo + k));
    }
}

// PREFIX: out[i] = a_0 .. a_i (inclusive) or a_0 .. a_(i-1) (exclusive), standard: the chain is kept Montgomery by a
// product with R^2 per step, the stored value is the product of that chain with the standard element
__global__ __launch_bounds__(SC_WG) void k_scan_apply_prefix(ScanArgs A) {
    const uint32_t w = threadIdx.x >> 6;
    const uint64_t first = (uint64_t)blockIdx.x * SC_WG, L = first + threadIdx.x;
    uint64_t lo;
    const uint32_t cnt = lane_span(lo, first, A.n, A.seg);
    if (!cnt) return;
    Fr p = load_uniform(A.before + blockIdx.x);
#pragma unroll 1
    for (uint32_t j = 0; j < w; j++) p = Fr::mul(p, load_uniform(A.wnum + (uint64_t)blockIdx.x * SC_WAVES + j));
    p = Fr::mul(p, load_el(A.lnum + L));
    const Fr r2 = Fr::r2();
    if (A.exclusive && lo == 0) store_el(A.out, raw_one());
#pragma unroll 1
    for (uint32_t k = 0; k < cnt; k++) {
        const uint64_t i = lo + k;
        const Fr o = Fr::mul(p, load_el(A.a + i));
        if (!A.exclusive) store_el(A.out + i, o);
        else if (i + 1 < A.n) store_el(A.out + i + 1, o);
        p = Fr::mul(o, r2);
    }
}

// INVERSE: out[i] = 1 / a_i (0 for 0); GRAND, PLONK: out[i] = z_i.  Forward: the prefix chain, every step stored in out;
// backward: the suffix chain times 1 / T, multiplied into what the forward pass left
template <int OP>
__global__ __launch_bounds__(SC_WG) void k_scan_apply(ScanArgs A) {
    const uint32_t w = threadIdx.x >> 6;
    const uint64_t first = (uint64_t)blockIdx.x * SC_WG, L = first + threadIdx.x;
    uint64_t lo;
    const uint32_t cnt = lane_span(lo, first, A.n, A.seg);
    if (!cnt) return;
    const Fr *wn = A.wnum + (uint64_t)blockIdx.x * SC_WAVES, *wd = A.wden + (uint64_t)blockIdx.x * SC_WAVES;
    Fr p = load_uniform(A.before + blockIdx.x), s = Fr::mul(load_uniform(A.behind + blockIdx.x), load_uniform(&A.k->tail));
#pragma unroll 1
    for (uint32_t j = 0; j < w; j++) p = Fr::mul(p, load_uniform(wn + j));
#pragma unroll 1
    for (uint32_t j = SC_WAVES - 1; j > w; j--) s = Fr::mul(s, load_uniform(wd + j));
    p = Fr::mul(p, load_el(A.lnum + L));
    s = Fr::mul(s, load_el(A.lden + L));
    Walk<OP> wk(A, first);
#pragma unroll 1
    for (uint32_t k = 0; k < cnt; k++) {
        store_el(A.out + lo + k, p);
        wk.num(p, lo + k);
    }
    if (cnt < A.seg) wk.pad(s, cnt);
#pragma unroll 1
    for (uint32_t k = cnt; k-- > 0;) {
        const uint64_t i = lo + k;
        if constexpr (OP == OP_INVERSE) {
            const Fr v = load_el(A.a + i);
            const bool z = v.is_zero();
            store_el(A.out + i, z ? Fr::zero() : Fr::mul(load_el(A.out + i), s));
            s = Fr::mul(s, z ? raw_one() : v);
        } else {
            wk.den(s, i);
            store_el(A.out + i, Fr::mul(load_el(A.out + i), s));
        }
    }
}

// Only when T = 0.  low[block] = the lowest element of the block whose denominator is 0, n when it has none
template <int OP>
__global__ __launch_bounds__(SC_WG) void k_scan_zero_den(uint64_t *low, ScanArgs A) {
    __shared__ uint64_t sh[SC_WAVES];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * SC_WG + threadIdx.x;
    bool zero = false;
    if (i < A.n) {
        if constexpr (OP == OP_PLONK) {
            const Fr beta = load_uniform(&A.k->beta), gamma = load_uniform(&A.k->gamma);
#pragma unroll 1
            for (uint32_t j = 0; j < A.cols; j++)
                zero = zero || Fr::add(Fr::add(load_el(A.a + j * A.n + i), Fr::mul(beta, load_el(A.b + j * A.n + i))), gamma).is_zero();
        } else {
            zero = load_el(A.b + i).is_zero();
        }
    }
    const unsigned long long m = __ballot(zero);
    if (lane == 0) sh[w] = m ? (uint64_t)blockIdx.x * SC_WG + w * 64 + (uint32_t)__builtin_ctzll(m) : A.n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t r = A.n;
        for (uint32_t j = SC_WAVES; j-- > 0;)
            if (sh[j] < A.n) r = sh[j];
        low[blockIdx.x] = r;
    }
}

// ---------------------------------------------------------------- host
uint32_t seg_in_effect() { return (uint32_t)env_number("ZKHIP_SCAN_SEG", DEFAULT_SEG, 1, MAX_SEG, "a number of elements per lane from 1 to 4096", ENV_LAX); }

// the residue R^k mod r
Fr r_power(uint64_t k) {
    if (!k) {
        Fr one = Fr::zero();
        one.v[0] = 1;
        return one;
    }
    return fr_pow(Fr::r2(), k - 1);                   // Montgomery arithmetic on the value R: (R)^(k-1), times R
}

// what lies between the launches; grown, never shrunk
struct ScanWork {
    DevBuf<Fr> lane, wave, group, total;              // [2 x lanes], [2 x waves], [4 x groups]: num then den; before, behind; [2]
    DevBuf<ScanConsts> k;
    DevBuf<uint64_t> low;
    ScanConsts h;                                     // the host image: it outlives the copy (every caller drains the stream before the next call)
    uint64_t groups = 0;
    void size(uint64_t g) {
        if (!k.p) {
            k.alloc(1);
            total.alloc(2);
        }
        if (groups >= g) return;
        lane.alloc(2 * g * SC_WG);
        wave.alloc(2 * g * SC_WAVES);
        group.alloc(4 * g);
        groups = g;
    }
    static uint64_t groups_of(uint64_t n, uint32_t seg) { return (n + (uint64_t)SC_WG * seg - 1) / ((uint64_t)SC_WG * seg); }
    static uint64_t bytes_of(uint64_t groups) { return groups * (2 * SC_WG + 2 * SC_WAVES + 4) * sizeof(Fr) + sizeof(ScanConsts) + 64; }
};

// What a scan with a den tells its caller
struct ScanEnd {
    Fr last;                                          // prod num / prod den, standard
    bool den_zero = false;                            // prod den is 0: nothing was written to out
};

// The three launches of one scan over device pointers, n >= 1.  A.a, A.b, A.shifts, A.out, A.n, A.cols, A.exclusive are the
// caller's; the constants but beta, gamma, omega (w.h, the caller's too for PLONK) and the work pointers are set here.
// With a den the stream is drained once, between k_scan_carry and k_scan_apply: the two totals (64 bytes) come to the host,
// which inverts T (Fr::inv, 380 products of 32 ns) and sends back tail / T (32 bytes).  tail = R^e with e the number of
// standard factors the backward chain multiplies into an output (less one for INVERSE, whose output leaves its own element
// out), so that what that chain stores is standard.  DESIGN.md section 27: the same inversion in one lane of the carry
// workgroup took seven times as long as the round trip.
template <int OP>
ScanEnd launch_scan(ScanArgs A, uint32_t seg, ScanWork &w, hipStream_t s) {
    const uint64_t groups = ScanWork::groups_of(A.n, seg);
    if (groups >= (1ull << 31)) throw std::invalid_argument("scan: too many elements for ZKHIP_SCAN_SEG");
    w.size(groups);
    const uint64_t f = OP == OP_PLONK ? A.cols : 1;
    w.h.lift = r_power(f * seg + 1);
    w.h.tail = Fr::zero();
    if (OP == OP_PLONK) fill_pow_tab(w.h.wtab, fr_pow(w.h.omega, seg), [](Fr a) { return a; });
    HIP_TRY(hipMemcpyAsync(w.k.p, &w.h, sizeof w.h, hipMemcpyHostToDevice, s));
    A.seg = seg;
    A.k = w.k.p;
    A.lnum = w.lane.p;
    A.lden = w.lane.p + w.groups * SC_WG;
    A.wnum = w.wave.p;
    A.wden = w.wave.p + w.groups * SC_WAVES;
    A.gnum = w.group.p;
    A.gden = w.group.p + w.groups;
    A.before = w.group.p + 2 * w.groups;
    A.behind = w.group.p + 3 * w.groups;
    const uint32_t cseg = (uint32_t)((groups + SC_WG - 1) / SC_WG);
    ScanEnd end;
    ZK_LAUNCH(k_scan_reduce<OP>, dim3((uint32_t)groups), dim3(SC_WG), 0, s, A);
    ZK_LAUNCH(k_scan_carry, dim3(1), dim3(SC_WG), 0, s, CarryArgs{A.gnum, A.gden, A.before, A.behind, w.total.p}, groups, cseg,
              OP == OP_PREFIX ? 0u : 1u);
    if constexpr (OP == OP_PREFIX) {
        ZK_LAUNCH(k_scan_apply_prefix, dim3((uint32_t)groups), dim3(SC_WG), 0, s, A);
    } else {
        Fr total[2];
        HIP_TRY(hipMemcpyAsync(total, w.total.p, sizeof total, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        end.den_zero = total[1].is_zero();
        if (end.den_zero) return end;
        const Fr tinv = Fr::inv(total[1]);            // Montgomery in and out
        end.last = Fr::from_mont(Fr::mul(total[0], tinv));
        w.h.tail = Fr::mul(tinv, r_power(OP == OP_INVERSE ? seg - 1 : f * seg));
        HIP_TRY(hipMemcpyAsync(&w.k.p->tail, &w.h.tail, sizeof(Fr), hipMemcpyHostToDevice, s));
        ZK_LAUNCH(k_scan_apply<OP>, dim3((uint32_t)groups), dim3(SC_WG), 0, s, A);
    }
    ZK_LAUNCH_OK("running product");
    return end;
}

// The four operations over device pointers and a stream (standard form in and out, n >= 1)
void batch_inverse_dev(Fr *out, const Fr *in, uint64_t n, uint32_t seg, ScanWork &w, hipStream_t s) {
    ScanArgs A{};
    A.a = in, A.out = out, A.n = n;
    launch_scan<OP_INVERSE>(A, seg, w, s);
}

void prefix_product_dev(Fr *out, const Fr *in, uint64_t n, bool exclusive, uint32_t seg, ScanWork &w, hipStream_t s) {
    ScanArgs A{};
    A.a = in, A.out = out, A.n = n, A.exclusive = exclusive ? 1u : 0u;
    launch_scan<OP_PREFIX>(A, seg, w, s);
}

ScanArgs grand_args(Fr *z, const Fr *num, const Fr *den, uint64_t n) {
    ScanArgs A{};
    A.a = num, A.b = den, A.out = z, A.n = n;
    return A;
}
ScanEnd grand_product_dev(Fr *z, const Fr *num, const Fr *den, uint64_t n, uint32_t seg, ScanWork &w, hipStream_t s) {
    return launch_scan<OP_GRAND>(grand_args(z, num, den, n), seg, w, s);
}

ScanArgs plonk_args(Fr *z, const Fr *wires, const Fr *sigmas, const Fr *shifts, uint32_t cols, uint32_t log_n) {
    ScanArgs A{};
    A.a = wires, A.b = sigmas, A.shifts = shifts, A.out = z, A.n = 1ull << log_n, A.cols = cols;
    return A;
}
// beta, gamma: standard form, host
ScanEnd permutation_product_dev(Fr *z, const Fr *wires, const Fr *sigmas, const Fr *shifts, uint32_t cols, uint32_t log_n, const uint8_t beta[32],
                                const uint8_t gamma[32], uint32_t seg, ScanWork &w, hipStream_t s) {
    w.h.beta = fr_from_std(beta);
    memcpy(w.h.gamma.v, gamma, 32);
    w.h.omega = root_of_unity(log_n);
    return launch_scan<OP_PLONK>(plonk_args(z, wires, sigmas, shifts, cols, log_n), seg, w, s);
}

// the lowest element with a zero denominator, after a scan whose T was 0 (A's constants are still on the device)
template <int OP>
uint64_t lowest_zero_den(ScanArgs A, ScanWork &w, hipStream_t s) {
    const uint32_t blocks = nblocks(A.n, SC_WG);
    A.k = w.k.p;
    w.low.alloc(blocks);
    ZK_LAUNCH(k_scan_zero_den<OP>, dim3(blocks), dim3(SC_WG), 0, s, w.low.p, A);
    ZK_LAUNCH_OK("zero denominator");
    std::vector<uint64_t> low(blocks);
    HIP_TRY(hipMemcpyAsync(low.data(), w.low.p, blocks * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint64_t v : low)
        if (v < A.n) return v;
    return A.n;
}

void need_n(const char *who, uint64_t n) {
    if (n >= (1ull << 31)) throw std::invalid_argument(std::string(who) + ": n is not below 2^31");
}

void fr_batch_inverse(uint8_t *out, const uint8_t *in, uint64_t n, uint64_t *zeros, int32_t device) {
    const uint32_t seg = seg_in_effect();
    if (zeros) *zeros = 0;
    if (!n) return;
    if (!out || !in) throw std::invalid_argument("null argument");
    need_n("zk_fr_batch_inverse", n);
    check_below_r("zk_fr_batch_inverse", "value", in, n);
    if (zeros) {
        static const uint8_t zero[32] = {0};
        uint64_t z = 0;
        for (uint64_t i = 0; i < n; i++) z += memcmp(in + i * 32, zero, 32) == 0;
        *zeros = z;
    }
    DeviceGuard g(resolve_device(device));
    need_hbm("zk_fr_batch_inverse", 2 * n * sizeof(Fr) + ScanWork::bytes_of(ScanWork::groups_of(n, seg)));
    Stream st;
    hipStream_t s = st.s;
    DevBuf<Fr> di, dout;
    ScanWork w;
    di.alloc(n);
    dout.alloc(n);
    HIP_TRY(hipMemcpyAsync(di.p, in, n * sizeof(Fr), hipMemcpyHostToDevice, s));
    batch_inverse_dev(dout.p, di.p, n, seg, w, s);
    HIP_TRY(hipMemcpyAsync(out, dout.p, n * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
}

void fr_prefix_product(uint8_t *out, const uint8_t *in, uint64_t n, uint32_t flags, int32_t device) {
    const uint32_t seg = seg_in_effect();
    if (flags & ~ZK_SCAN_EXCLUSIVE) throw std::invalid_argument("zk_fr_prefix_product: flags " + std::to_string(flags) + " is unknown");
    if (!n) return;
    if (!out || !in) throw std::invalid_argument("null argument");
    need_n("zk_fr_prefix_product", n);
    check_below_r("zk_fr_prefix_product", "value", in, n);
    DeviceGuard g(resolve_device(device));
    need_hbm("zk_fr_prefix_product", 2 * n * sizeof(Fr) + ScanWork::bytes_of(ScanWork::groups_of(n, seg)));
    Stream st;
    hipStream_t s = st.s;
    DevBuf<Fr> di, dout;
    ScanWork w;
    di.alloc(n);
    dout.alloc(n);
    HIP_TRY(hipMemcpyAsync(di.p, in, n * sizeof(Fr), hipMemcpyHostToDevice, s));
    prefix_product_dev(dout.p, di.p, n, (flags & ZK_SCAN_EXCLUSIVE) != 0, seg, w, s);
    HIP_TRY(hipMemcpyAsync(out, dout.p, n * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
}

void fr_grand_product(uint8_t *z, uint8_t *last, const uint8_t *num, const uint8_t *den, uint64_t n, int32_t device) {
    const uint32_t seg = seg_in_effect();
    if (!last) throw std::invalid_argument("null argument");
    if (!n) {
        memset(last, 0, 32);
        last[0] = 1;                                  // the empty product
        return;
    }
    if (!z || !num || !den) throw std::invalid_argument("null argument");
    need_n("zk_fr_grand_product", n);
    check_below_r("zk_fr_grand_product", "numerator", num, n);
    check_below_r("zk_fr_grand_product", "denominator", den, n);
    DeviceGuard g(resolve_device(device));
    need_hbm("zk_fr_grand_product", 3 * n * sizeof(Fr) + ScanWork::bytes_of(ScanWork::groups_of(n, seg)));
    Stream st;
    hipStream_t s = st.s;
    DevBuf<Fr> dn, dd, dz;
    ScanWork w;
    dn.alloc(n);
    dd.alloc(n);
    dz.alloc(n);
    HIP_TRY(hipMemcpyAsync(dn.p, num, n * sizeof(Fr), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(dd.p, den, n * sizeof(Fr), hipMemcpyHostToDevice, s));
    const ScanEnd end = grand_product_dev(dz.p, dn.p, dd.p, n, seg, w, s);
    if (end.den_zero)
        throw std::invalid_argument("zk_fr_grand_product: denominator " + std::to_string(lowest_zero_den<OP_GRAND>(grand_args(dz.p, dn.p, dd.p, n), w, s)) +
                                    " is zero");
    HIP_TRY(hipMemcpyAsync(z, dz.p, n * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(last, end.last.v, 32);
}

void plonk_permutation_product(uint8_t *z, uint8_t *last, const uint8_t *wires, const uint8_t *sigmas, uint32_t cols, uint32_t log_n,
                               const uint8_t *shifts, const uint8_t *beta, const uint8_t *gamma, int32_t device) {
    const char *who = "zk_plonk_permutation_product";
    const uint32_t seg = seg_in_effect();
    if (!z || !last || !wires || !sigmas || !shifts || !beta || !gamma) throw std::invalid_argument("null argument");
    if (cols < 1 || cols > MAX_COLS) throw std::invalid_argument(std::string(who) + ": cols " + std::to_string(cols) + " is outside 1 .. 8");
    if (log_n > MAX_LOG_N) throw std::invalid_argument(std::string(who) + ": log_n " + std::to_string(log_n) + " is above 28");
    const uint64_t n = 1ull << log_n;
    auto check_cols = [&](const char *what, const uint8_t *v) {
        for (uint32_t j = 0; j < cols; j++) {
            const uint64_t bad = first_not_below_r(v + j * n * 32, n);
            if (bad < n)
                throw std::invalid_argument(std::string(who) + ": " + what + ": column " + std::to_string(j) + ", row " + std::to_string(bad) + " is not below r");
        }
    };
    check_cols("wires", wires);
    check_cols("sigmas", sigmas);
    check_below_r(who, "shift", shifts, cols);
    if (!below(beta, FrParams::P)) throw std::invalid_argument(std::string(who) + ": beta is not below r");
    if (!below(gamma, FrParams::P)) throw std::invalid_argument(std::string(who) + ": gamma is not below r");
    DeviceGuard g(resolve_device(device));
    need_hbm(who, (2 * cols + 1) * n * sizeof(Fr) + ScanWork::bytes_of(ScanWork::groups_of(n, seg)));
    Stream st;
    hipStream_t s = st.s;
    DevBuf<Fr> dw, ds, dsh, dz;
    ScanWork w;
    dw.alloc(cols * n);
    ds.alloc(cols * n);
    dsh.alloc(cols);
    dz.alloc(n);
    HIP_TRY(hipMemcpyAsync(dw.p, wires, cols * n * sizeof(Fr), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ds.p, sigmas, cols * n * sizeof(Fr), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(dsh.p, shifts, cols * sizeof(Fr), hipMemcpyHostToDevice, s));
    const ScanEnd end = permutation_product_dev(dz.p, dw.p, ds.p, dsh.p, cols, log_n, beta, gamma, seg, w, s);
    if (end.den_zero)
        throw std::invalid_argument(std::string(who) + ": row " +
                                    std::to_string(lowest_zero_den<OP_PLONK>(plonk_args(dz.p, dw.p, ds.p, dsh.p, cols, log_n), w, s)) +
                                    " has a zero denominator");
    HIP_TRY(hipMemcpyAsync(z, dz.p, n * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(last, end.last.v, 32);
}

}   // namespace

// ---------------------------------------------------------------- what plonkprove.hip chains (plonk_internal.hpp)
struct PlonkPerm {
    ScanWork w;
};
PlonkPerm *plonk_perm_new() { return new PlonkPerm(); }
void plonk_perm_free(PlonkPerm *p) { delete p; }
uint32_t plonk_perm_seg() { return seg_in_effect(); }
uint64_t plonk_perm_need_bytes(uint64_t n) { return ScanWork::bytes_of(ScanWork::groups_of(n, 1)); }
size_t plonk_perm_bytes(const PlonkPerm *p) { return p->w.groups ? ScanWork::bytes_of(p->w.groups) : 0; }
bool plonk_perm_dev(PlonkPerm *p, Fr *z, uint8_t last[32], const Fr *wires, const Fr *sigmas, const Fr *shifts, uint32_t log_n, const uint8_t beta[32],
                    const uint8_t gamma[32], hipStream_t s) {
    const ScanEnd end = permutation_product_dev(z, wires, sigmas, shifts, 3, log_n, beta, gamma, seg_in_effect(), p->w, s);
    if (end.den_zero) return false;
    memcpy(last, end.last.v, 32);
    return true;
}

extern "C" {

int zk_fr_batch_inverse(uint8_t *out, const uint8_t *in, uint64_t n, uint64_t *zeros, int32_t device) {
    return guarded([&] { fr_batch_inverse(out, in, n, zeros, device); });
}

int zk_fr_prefix_product(uint8_t *out, const uint8_t *in, uint64_t n, uint32_t flags, int32_t device) {
    return guarded([&] { fr_prefix_product(out, in, n, flags, device); });
}

int zk_fr_grand_product(uint8_t *z, uint8_t last[32], const uint8_t *num, const uint8_t *den, uint64_t n, int32_t device) {
    return guarded([&] { fr_grand_product(z, last, num, den, n, device); });
}

int zk_plonk_permutation_product(uint8_t *z, uint8_t last[32], const uint8_t *wires, const uint8_t *sigmas, uint32_t cols, uint32_t log_n,
                                 const uint8_t *shifts, const uint8_t beta[32], const uint8_t gamma[32], int32_t device) {
    return guarded([&] { plonk_permutation_product(z, last, wires, sigmas, cols, log_n, shifts, beta, gamma, device); });
}

}   // extern "C"
