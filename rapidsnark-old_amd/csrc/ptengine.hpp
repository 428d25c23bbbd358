// What the checks of files of points share (ptau_check.hip: is a .ptau sound; zkey_verify.hip: is a .zkey the key of its
// circuit over a .ptau): the G2 subgroup test, the pass over a row of points that says what is wrong with the first bad
// one, scalars made on the device (the powers of one s), points as the files' bytes on the host, and the chunked
// multi-scalar multiplication on device-resident inputs (DevMsm, Engine, EnginePair, power_sum) with its admission
// estimate.  One copy for both units; ptau_check.hip's header comment describes the subgroup test and the multiplication.
// mulvec.hip and kzg.hip run the same pass over their points (enqueue_classify, classified); they and frscan.hip take
// the host's scalar helpers (first_not_below_r, checked_scalar).
#pragma once
#include <errno.h>
#include <sys/random.h>

#include "hiputil.hpp"
#include "devmem.hpp"
#include "ptcheck.hpp"
#include "pairing.hpp"

namespace zkp {

constexpr uint32_t NONE = NO_BAD_POINT;
constexpr uint32_t POW_BITS = 64;                     // entries of a table of squarings: base^(2^i), i < 64
constexpr uint32_t KIND_COORD = 1, KIND_CURVE = 2, KIND_SUBGROUP = 3, KIND_INFINITY = 4;     // zk_ptau_report.bad_kind

static_assert((BN_X >> 62) == 1, "x has 63 bits: the loop of k_g2_subgroup starts below bit 62");

// ---------------------------------------------------------------- device: the subgroup test
struct PsiConsts {
    Fq2 gx, gy;                                       // xi^((q-1)/3), xi^((q-1)/2): pairing.hpp's gamma1[1], gamma1[2]
};

// psi on XYZZ: x = X / ZZ and y = Y / ZZZ, so conjugating all four and multiplying X and Y is psi of the affine point
__device__ __forceinline__ G2XYZZ psi(const G2XYZZ &p, const PsiConsts &k) {
    if (p.is_inf()) return p;
    return G2XYZZ{Fq2::mul(f2_conj(p.x), k.gx), Fq2::mul(f2_conj(p.y), k.gy), f2_conj(p.zz), f2_conj(p.zzz)};
}
__device__ __forceinline__ bool same_point(const G2XYZZ &a, const G2XYZZ &b) {
    if (a.is_inf() || b.is_inf()) return a.is_inf() && b.is_inf();
    return Fq2::mul(a.x, b.zz) == Fq2::mul(b.x, a.zz) && Fq2::mul(a.y, b.zzz) == Fq2::mul(b.y, a.zzz);
}

// Q (on the twist, not infinity) is in the order-r subgroup: psi^3([2x] Q) = [x + 1] Q + psi([x] Q) + psi^2([x] Q)
__device__ __forceinline__ bool g2_in_subgroup(const G2Affine &Q, const PsiConsts &k) {
    G2XYZZ L = G2XYZZ::from_affine(Q);                // bit 62 of x
#pragma unroll 1
    for (int b = 61; b >= 0; b--) {
        L = dbl(L);
        if ((BN_X >> b) & 1) madd(L, Q);
    }
    G2XYZZ T = psi(L, k);                             // psi([x] Q)
    madd(L, Q);                                       // [x + 1] Q
    add(L, T);
    T = psi(T, k);
    add(L, T);
    T = dbl(psi(T, k));                               // psi^3([2x] Q)
    return same_point(L, T);
}

// out[i] (when given) = 1 if pts[i] is in the order-r subgroup (infinity: 1), else 0; the lowest index outside goes to
// *err (when given).  The points are on the twist (the caller's check runs first; on other bytes the result means nothing).
template <bool PLAIN>
__global__ __launch_bounds__(64) void k_g2_subgroup(uint8_t *out, uint32_t *err, const G2Affine *__restrict__ pts, uint64_t n, PsiConsts k) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G2Affine Q = load_pt(pts + i);
    bool ok = true;
    if (!Q.is_inf()) {
        if constexpr (PLAIN) {
            Fr r;
#pragma unroll
            for (int j = 0; j < 8; j++) r.v[j] = FrParams::P[j];
            ok = scalar_mul_affine(Q, r).is_inf();
        } else {
            ok = g2_in_subgroup(Q, k);
        }
    }
    if (out) out[i] = ok ? 1 : 0;
    if (!ok && err) atomicMin(err, (uint32_t)i);
}

// ---------------------------------------------------------------- device: what a file's point may be
// err[0]: the lowest index with a coordinate >= q, err[1]: off the curve, err[3]: at infinity where that is not legal
// (err[2] is the subgroup kernel's)
template <class F>
__global__ __launch_bounds__(256) void k_ptau_classify(uint32_t *err, const Affine<F> *__restrict__ src, uint64_t n, F b, uint32_t inf_bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<F> p = load_pt(src + i);
    if (p.is_inf()) {
        if (inf_bad) atomicMin(err + 3, (uint32_t)i);
        return;
    }
    if (!(below_q(p.x) && below_q(p.y))) atomicMin(err + 0, (uint32_t)i);
    else if (!(F::sqr(p.y) == F::add(F::mul(F::sqr(p.x), p.x), b))) atomicMin(err + 1, (uint32_t)i);
}

// ---------------------------------------------------------------- device: scalars
// base^e for a lane's own e from the table of squarings tab[i] = base^(2^i) (Montgomery)
__device__ __forceinline__ Fr pow_tab(const Fr *__restrict__ tab, uint64_t e) {
    Fr acc = Fr::one();
#pragma unroll 1
    for (uint32_t b = 0; b < POW_BITS && (e >> b); b++)
        if ((e >> b) & 1) acc = Fr::mul(acc, load_el(tab + b));
    return acc;
}

// out[i] = base^(e0 + i), standard form (what the sort of a multi-scalar multiplication reads)
static __global__ __launch_bounds__(256) void k_fr_powers(Fr *out, const Fr *__restrict__ tab, uint64_t e0, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_el(out + i, Fr::from_mont(pow_tab(tab, e0 + i)));
}

// ---------------------------------------------------------------- host: scalars
inline bool below(const uint8_t a[32], const uint32_t p[8]) {
    uint32_t w[8];
    memcpy(w, a, 32);
    for (int i = 7; i >= 0; i--)
        if (w[i] != p[i]) return w[i] < p[i];
    return false;
}
inline Fr fr_from_std(const uint8_t a[32]) {
    Fr x;
    memcpy(x.v, a, 32);
    return Fr::to_mont(x);
}
inline Fr fr_small(uint64_t v) {
    Fr x = Fr::zero();
    x.v[0] = (uint32_t)v;
    x.v[1] = (uint32_t)(v >> 32);
    return Fr::to_mont(x);
}
inline void fr_to_std(uint8_t out[32], const Fr &a) {
    const Fr x = Fr::from_mont(a);
    memcpy(out, x.v, 32);
}
inline Fr fr_pow(Fr base, uint64_t e) {
    Fr acc = Fr::one();
    for (; e; e >>= 1) {
        if (e & 1) acc = Fr::mul(acc, base);
        base = Fr::sqr(base);
    }
    return acc;
}

// the lowest index of n scalars (32 bytes LE) that is not below r, n when there is none
inline uint64_t first_not_below_r(const uint8_t *sc, uint64_t n) {
    for (uint64_t i = 0; i < n; i++)
        if (!below(sc + i * 32, FrParams::P)) return i;
    return n;
}
// a caller's scalar, Montgomery; "<what> is not below r" otherwise
inline Fr checked_scalar(const uint8_t s32[32], const std::string &what) {
    if (!below(s32, FrParams::P)) throw std::invalid_argument(what + " is not below r");
    return fr_from_std(s32);
}
// the two as an entry `who` words them: "<who>: <what> <index> is not below r", "<who>: <what> is not below r"
inline void check_below_r(const char *who, const char *what, const uint8_t *v, uint64_t n) {
    const uint64_t bad = first_not_below_r(v, n);
    if (bad < n) throw std::invalid_argument(std::string(who) + ": " + what + " " + std::to_string(bad) + " is not below r");
}
inline Fr checked_one(const char *who, const char *what, const uint8_t *v) { return checked_scalar(v, std::string(who) + ": " + what); }

inline bool plain_subgroup() { return env_switch("ZKHIP_SUBGROUP_PLAIN"); }

inline PsiConsts psi_consts() {
    PairConsts pc;
    pair_consts_init(pc);
    return PsiConsts{pc.gamma1[1], pc.gamma1[2]};
}

// tab[i] = base^(2^i) on the device
struct PowTable {
    DevBuf<Fr> d;
    void build(Fr base, hipStream_t s) {
        Fr h[POW_BITS];
        for (uint32_t i = 0; i < POW_BITS; i++) {
            h[i] = base;
            base = Fr::sqr(base);
        }
        d.alloc(POW_BITS);
        HIP_TRY(hipMemcpyAsync(d.p, h, sizeof h, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));             // h leaves scope
    }
};

// ---------------------------------------------------------------- host: points as the file's bytes
template <class F>
struct Group;
template <>
struct Group<Fq> {
    typedef G1Acc Acc;
    static void add(uint8_t *acc, const uint8_t *in) { HostTail::add_affine_g1(acc, in); }
    static void mul(uint8_t *out, const uint8_t *p, const uint8_t k[32]) {
        if (zk_g1_mul(out, p, k) != 0) throw std::runtime_error(std::string("zk_g1_mul: ") + get_error());
    }
};
template <>
struct Group<Fq2> {
    typedef G2Acc Acc;
    static void add(uint8_t *acc, const uint8_t *in) { HostTail::add_affine_g2(acc, in); }
    static void mul(uint8_t *out, const uint8_t *p, const uint8_t k[32]) {
        if (zk_g2_mul(out, p, k) != 0) throw std::runtime_error(std::string("zk_g2_mul: ") + get_error());
    }
};
template <class F>
struct Pt {                                           // one affine point, the file's bytes
    uint8_t b[sizeof(Affine<F>)];
    Pt() { memset(b, 0, sizeof b); }
    explicit Pt(const void *p) { memcpy(b, p, sizeof b); }
    bool operator==(const Pt &o) const { return memcmp(b, o.b, sizeof b) == 0; }
    Pt neg() const {
        Affine<F> a;
        memcpy(&a, b, sizeof a);
        if (!a.is_inf()) a.y = F::neg(a.y);
        return Pt(&a);
    }
    Pt operator+(const Pt &o) const {
        Pt r = *this;
        Group<F>::add(r.b, o.b);
        return r;
    }
    Pt operator-(const Pt &o) const { return *this + o.neg(); }
    Pt times(const Fr &k) const {
        uint8_t k32[32];
        fr_to_std(k32, k);
        Pt r;
        Group<F>::mul(r.b, b, k32);
        return r;
    }
};

// ---------------------------------------------------------------- host: a multi-scalar multiplication on device-resident inputs
// The sequence of operators.hip's msm_generic; the buffers stay across calls of one size (the chunks of a row).
template <class F>
struct DevMsm {
    typedef typename Group<F>::Acc Acc;
    SortBufs sb;
    DevBuf<Acc> buckets, scratch, ws;
    DevBuf<XYZZ<F>> wsum;
    DevBuf<uint32_t> wkey, wflag;
    std::vector<uint8_t> w;
    uint64_t n = 0, emax = 0;
    uint32_t rc = 0;
    void size(uint64_t n_) {
        if (n_ == n) return;
        n = 0;
        sb.alloc(n_, 0);
        emax = sb.max_entries();
        const uint64_t slots = msm_accum_workspace_slots(emax);
        ws.alloc(slots);
        wkey.alloc(slots);
        wflag.alloc(slots);
        buckets.alloc(sb.total_buckets());
        scratch.alloc(msm_reduce_scratch_points(1, sb.plan));
        rc = msm_wsum_rc(sb.plan);
        wsum.alloc((uint64_t)sb.plan.sets * rc);
        w.resize((size_t)sb.plan.sets * rc * sizeof(XYZZ<F>));
        n = n_;
    }
    // out = sum sc[i] pts[i], i < n_ (n_ >= 1).  pts: the file's form, converted in place to the kernels' own; sc: standard form
    void run(uint8_t *out, Affine<F> *pts, const Fr *sc, uint64_t n_, hipStream_t s) {
        size(n_);
        launch_fq_to_internal(reinterpret_cast<Fq *>(pts), n_ * (sizeof(Affine<F>) / 32), s);
        sb.run(sc, s);
        if constexpr (sizeof(F) == sizeof(Fq)) {
            launch_msm_accum_g1(buckets.p, sb.offsets.p, sb.entries.p, pts, 0, 0, sb.total_buckets(), emax, ws.p, wkey.p, wflag.p, s);
            launch_msm_reduce_g1(wsum.p, scratch.p, buckets.p, 1, sb.plan, s);
        } else {
            launch_msm_accum_g2(buckets.p, sb.offsets.p, sb.entries.p, pts, 0, 0, sb.total_buckets(), emax, ws.p, wkey.p, wflag.p, s);
            launch_msm_reduce_g2(wsum.p, scratch.p, buckets.p, 1, sb.plan, s);
        }
        HIP_TRY(hipMemcpyAsync(w.data(), wsum.p, w.size(), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if constexpr (sizeof(F) == sizeof(Fq)) HostTail::combine_windows_g1(w.data(), sb.plan.sets, sb.plan.c, rc, out);
        else HostTail::combine_windows_g2(w.data(), sb.plan.sets, sb.plan.c, rc, out);
    }
    // An upper estimate of the HBM of size(n_), made without a device: the sort's buffers are exact; the accumulation's
    // workspace is bounded by a lane per ACC_CHUNK_MIN = 32 entries plus one full round of lanes, twice per level
    static uint64_t bytes(uint64_t n_) {
        const MsmPlan p = make_msm_plan(n_ ? n_ : 1, 0);
        const MsmSortSizes z = msm_sort_sizes(n_, p);
        const uint64_t sort = 2 * z.lo_u16 + 4 * (z.counts_u32 + z.starts_u32 + z.offsets_u32 + z.entries_u32 + z.codes_u32 + z.val_u32 + z.bin_counts_u32 + z.bin_starts_u32);
        const uint64_t slots = 5 * ((n_ ? n_ : 1) * p.W / 32 + (1ull << 19));
        return sort + slots * (sizeof(Acc) + 8) + ((uint64_t)p.sets * p.nbuckets + msm_reduce_scratch_points(1, p)) * sizeof(Acc) +
               (uint64_t)p.sets * msm_wsum_rc(p) * sizeof(XYZZ<F>) + 65536;
    }
};

// One group's buffers: a chunk of points, its scalars, the words of the checks, the multiplication's workspace
template <class F>
struct Engine {
    typedef Affine<F> Aff;
    hipStream_t s;
    StreamUploader up;
    uint64_t cap;
    DevBuf<Aff> pts;
    DevBuf<Fr> sc;
    DevBuf<uint32_t> err;                             // four words
    DevMsm<F> msm;
    Engine(hipStream_t s_, uint64_t cap_) : s(s_), up(s_), cap(cap_ ? cap_ : 1) {
        pts.alloc(cap);
        sc.alloc(cap);
        err.alloc(4);
    }
    static uint64_t bytes(uint64_t cap_) { return cap_ * (sizeof(Aff) + sizeof(Fr)) + DevMsm<F>::bytes(cap_) + 4096; }
    void load(const uint8_t *src, uint64_t cnt) { up.copy(pts.p, src, cnt * sizeof(Aff)); }
    // the lowest index of the loaded chunk that is not a point of the curve, NONE when there is none
    uint32_t first_off_curve(uint64_t cnt) {
        launch_point_check<F>(err.p, pts.p, cnt, s);
        uint32_t bad = NONE;
        HIP_TRY(hipMemcpyAsync(&bad, err.p, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return bad;
    }
    // sc[i] = base^(e0 + i), i < cnt; tab: the squarings of base
    void powers(const PowTable &tab, uint64_t e0, uint64_t cnt) {
        ZK_LAUNCH(k_fr_powers, dim3(nblocks(cnt, 256)), dim3(256), 0, s, sc.p, tab.d.p, e0, cnt);
        ZK_LAUNCH_OK("powers");
    }
    // acc += sum sc[i] pts[i] over the loaded chunk
    void accumulate(Pt<F> &acc, uint64_t cnt) {
        Pt<F> part;
        msm.run(part.b, pts.p, sc.p, cnt, s);
        acc = acc + part;
    }
};

// acc += sum_(i < n) base^(e0 + i) P_i, e.cap points at a time.  fetch(off, cnt) brings P_off .. P_(off + cnt - 1) into
// e.pts and checks them; false: it has said what is wrong, and the sum is given up
template <class F, class Fetch>
bool power_sum(Engine<F> &e, Pt<F> &acc, uint64_t n, const PowTable &tab, uint64_t e0, Fetch fetch) {
    for (uint64_t off = 0; off < n; off += e.cap) {
        const uint64_t cnt = n - off < e.cap ? n - off : e.cap;
        if (!fetch(off, cnt)) return false;
        e.powers(tab, e0 + off, cnt);
        e.accumulate(acc, cnt);
    }
    return true;
}

inline void launch_subgroup(uint8_t *d_out, uint32_t *d_err, const G2Affine *d_pts, uint64_t n, const PsiConsts &k, bool plain, hipStream_t s) {
    if (!n) return;
    if (plain) ZK_LAUNCH(k_g2_subgroup<true>, dim3(nblocks(n, 64)), dim3(64), 0, s, d_out, d_err, d_pts, n, k);
    else ZK_LAUNCH(k_g2_subgroup<false>, dim3(nblocks(n, 64)), dim3(64), 0, s, d_out, d_err, d_pts, n, k);
    ZK_LAUNCH_OK("g2 subgroup test");
}

// ---------------------------------------------------------------- host: the pass over a chunk of a file's points
// Enqueued on s: d_err's four words <- what k_ptau_classify finds in d_pts[0, n) (n >= 1; inf_bad: infinity is no legal
// point) and, for points of G2 when psi is given, the subgroup kernel's word; then the words go to h (host; pinned memory
// when the caller goes on without waiting).  The kernels record with atomicMin: the words do not depend on scheduling.
template <class F>
inline void enqueue_classify(uint32_t *h, uint32_t *d_err, const Affine<F> *d_pts, uint64_t n, bool inf_bad, const PsiConsts *psi, bool plain, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(d_err, 0xFF, 16, s));
    ZK_LAUNCH(k_ptau_classify<F>, dim3(nblocks(n, 256)), dim3(256), 0, s, d_err, d_pts, n, curve_b<F>(), inf_bad ? 1u : 0u);
    ZK_LAUNCH_OK("point check");
    if constexpr (sizeof(F) == sizeof(Fq2)) {
        if (psi) launch_subgroup(nullptr, d_err + 2, d_pts, n, *psi, plain, s);
    }
    HIP_TRY(hipMemcpyAsync(h, d_err, 16, hipMemcpyDeviceToHost, s));
}
// waits for s; the first bad point of the words enqueue_classify sent to h (kind 0: none)
inline BadPoint classified(const uint32_t *h, hipStream_t s) {
    HIP_TRY(hipStreamSynchronize(s));
    uint32_t w[4];
    memcpy(w, h, sizeof w);
    return lowest_bad(w);
}

// The two groups' engines on one stream and what the pass over their chunks needs: what zk_ptau_check and zk_zkey_verify
// are built on
struct EnginePair {
    PsiConsts psi;
    bool plain;
    Engine<Fq> e1;
    Engine<Fq2> e2;
    EnginePair(hipStream_t s, uint64_t cap) : psi(psi_consts()), plain(plain_subgroup()), e1(s, cap), e2(s, cap) {}
    static uint64_t bytes(uint64_t cap) { return Engine<Fq>::bytes(cap) + Engine<Fq2>::bytes(cap); }
    template <class F>
    Engine<F> &engine() {
        if constexpr (sizeof(F) == sizeof(Fq)) return e1;
        else return e2;
    }
    // the first bad point of the cnt points engine<F>() holds; subgroup: the points must be in G2's order-r subgroup
    template <class F>
    BadPoint classify(uint64_t cnt, bool inf_bad, bool subgroup) {
        Engine<F> &e = engine<F>();
        uint32_t h[4];
        enqueue_classify<F>(h, e.err.p, e.pts.p, cnt, inf_bad, subgroup ? &psi : nullptr, plain, e.s);
        return classified(h, e.s);
    }
};

inline void generators(Pt<Fq> &g1, Pt<Fq2> &g2) {
    // (1, 2), and the generator of G2 of EIP-197, standard form
    static const uint32_t G2_STD[4][8] = {
        {0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu},
        {0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u},
        {0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u},
        {0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u}};
    const G1Affine a{fq_std(1), fq_std(2)};
    const G2Affine b{Fq2{fq_std(G2_STD[0]), fq_std(G2_STD[1])}, Fq2{fq_std(G2_STD[2]), fq_std(G2_STD[3])}};
    g1 = Pt<Fq>(&a);
    g2 = Pt<Fq2>(&b);
}

// 32 bytes of getrandom(), redrawn until 2 <= s < r
inline void draw_scalar(uint8_t s32[32], const char *who) {
    for (;;) {
        size_t got = 0;
        while (got < 32) {
            const ssize_t k = getrandom(s32 + got, 32 - got, 0);
            if (k < 0) {
                if (errno == EINTR) continue;
                throw std::runtime_error(std::string(who) + ": the random source failed");
            }
            got += (size_t)k;
        }
        if (!is_0_or_1(s32) && below(s32, FrParams::P)) return;
    }
}

}   // namespace zkp
