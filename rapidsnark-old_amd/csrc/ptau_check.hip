// Is a Powers of Tau file sound?  (include/zkhip.h, section "Powers of Tau: check".)  Nothing in the reference corresponds
// to it: its prover reads a finished .zkey (src/main_prover.cpp:57-72); the counterpart is the arithmetic half of snarkjs
// `powersoftau verify` (the contribution transcript of section 7 is NOT read: DESIGN.md section 18 says why).
//
// What is proved about a file of N = 2^power (T = section 2, U = 3, A = 4, B = 5, beta2 = 6; G1, G2 the generators):
//   points      every coordinate below q, every point on its curve, none of sections 2 to 6 at infinity, every G2 point of
//               sections 3, 6 and 13 in the order-r subgroup;
//   generators  T_0 = G1 and U_0 = G2 (host, byte compare);
//   powers      with one scalar s drawn AFTER the file is mapped, a row P_0 .. P_(m-1) gives F = sum s^i P_i by ONE
//               multi-scalar multiplication, and from it  lo = F - s^(m-1) P_(m-1) = sum_(i<m-1) s^i P_i  and
//               hi = (F - P_0) / s = sum_(i<m-1) s^i P_(i+1).  The row is a geometric sequence of the ratio the other group's
//               tau-point fixes iff  e(lo, U_1) = e(hi, G2)  (rows of G1; e(T_1, lo) = e(G1, hi) for the row of G2), up to the
//               chance 2^29 / r that s is a root of a non-zero polynomial of degree < 2^29.  e(B_0, G2) = e(G1, beta2) ties
//               section 6 to section 5.  The five equations are one zk_pairing(group = 2) call;
//   Lagrange    when sections 12 to 15 are there: for every level p (n = 2^p)  sum_j c_j Lag_j = sum_(i<n) s^i P_i  with
//               c_j = sum_(i<n) s^i w^(ij), the FORWARD DFT of the powers of s.  The right sides are prefixes of F (it is
//               accumulated over the ranges [2^(p-1), 2^p)), the left sides one multi-scalar multiplication per level; two
//               group elements are compared after normalisation, no pairing.
//
// The G2 subgroup test (k_g2_subgroup), the hot path: a file of power 28 has 2^28 points in section 3 and twice as many
// in section 13.  With psi the twist's Frobenius map (pairing.hpp's frob_twist: conjugate, multiply x by xi^((q-1)/3) and
// y by xi^((q-1)/2)) and x = BN_X,
//     Q is in the subgroup  <=>  [x+1] Q + psi([x] Q) + psi^2([x] Q) = psi^3([2x] Q)
// (psi acts on the subgroup as multiplication by q, and (x + 1) + x q + x q^2 - 2 x q^3 = 0 mod r).  One 63-bit
// double-and-add instead of the 254 bits of [r] Q.  That the test is exact and not merely necessary is a finite check
// (tests/test_gpu_ptau_check.py repeats it on the device): the twist's group is cyclic of order
// r h2 with h2 a product of four distinct primes, an endomorphism acts on each prime-order part as a scalar, and the
// criterion fails on a point of each of the four parts.  One lane per point; the bits of x are a compile-time constant, so
// every branch on them is uniform and nothing is indexed at run time; psi on XYZZ conjugates the four coordinates and
// costs two Fq2 products; the comparison is projective (four Fq2 products, no inversion).  Points of small order meet
// P = +-Q and infinity inside [x] Q: curve.hpp's dbl / madd / add take every case.
// ZKHIP_SUBGROUP_PLAIN=1 runs k_g2_subgroup<true>, [r] Q by devmem.hpp's scalar_mul_affine, what pairing.hip does: a second
// route to the same bytes for the tests and the denominator of tools/ptau_check_timing.py.
//
// The multi-scalar multiplications are the library's own (msm_sort / msm_accum / msm_reduce, the sequence of
// operators.hip's msm_generic) on points and scalars that are already on the device; the scalars s^i and c_j are made
// there, chunk by chunk (a row of power 28 would need 8 GiB of them on the host).  Points come from the caller's mapping
// in chunks of ZKHIP_PTAU_CHUNK points (2^22 otherwise); chunk sums are added on the host (host_tail.cpp).
// c_j has the closed form (s^n - 1) / (s w^j - 1), and c_j = n where s w^j = 1: k_power_dft makes four of them per lane
// with one inversion (Montgomery's trick inside the lane), exact for every s < r.
//
// Fields: curve.hpp's 8 x 32-bit Montgomery forms (R = 2^256), the .ptau's own bytes, as ptau_prepare.hip and scale.hip.
//
// The subgroup kernel, the point pass, the powers of s, the root of unity and the chunked multiplication (DevMsm, Engine,
// EnginePair, power_sum) are in ptengine.hpp: zkey_verify.hip runs the same code over a key's sections.
#include "ptengine.hpp"

namespace {

constexpr uint64_t DEFAULT_CHUNK = 1ull << 22;        // points per chunk: 512 MiB of G2 input
constexpr uint32_t MAX_LOG_N = 28;

// a^(r-2); the exponent is shifted, not indexed
__device__ __forceinline__ Fr fr_inv_dev(const Fr &a) {
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = FrParams::P[i];
    e[0] -= 2;
    Fr result = Fr::one(), base = a;
#pragma unroll 1
    for (int i = 0; i < 254; i++) {
        if (e[0] & 1u) result = Fr::mul(result, base);
        base = Fr::sqr(base);
#pragma unroll
        for (int q = 0; q < 7; q++) e[q] = (e[q] >> 1) | (e[q + 1] << 31);
        e[7] >>= 1;
    }
    return result;
}

// out[t] = c_(j0 + t) = sum_(i<n) s^i w^(i (j0 + t)) for t < cnt, standard form, n = 2^log_n and w its root of unity:
// (s^n - 1) / (s w^j - 1), and n where s w^j = 1.  tab: the squarings of w_(2^28); w^j = w_(2^28)^(j << shift).
// num = s^n - 1, nval = n, all Montgomery.  A lane makes DFT_PER_LANE consecutive values with one inversion.
constexpr uint32_t DFT_PER_LANE = 4;
__global__ __launch_bounds__(256) void k_power_dft(Fr *out, const Fr *__restrict__ tab, uint32_t shift, Fr s, Fr w, Fr num, Fr nval, uint64_t j0, uint64_t cnt) {
    const uint64_t t0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * DFT_PER_LANE;
    if (t0 >= cnt) return;
    Fr x = Fr::mul(s, pow_tab(tab, (j0 + t0) << shift));                       // s w^j
    Fr d[DFT_PER_LANE], pre[DFT_PER_LANE];
    bool unit[DFT_PER_LANE];
#pragma unroll
    for (uint32_t k = 0; k < DFT_PER_LANE; k++) {
        d[k] = Fr::sub(x, Fr::one());
        unit[k] = d[k].is_zero();
        if (unit[k]) d[k] = Fr::one();
        pre[k] = k ? Fr::mul(pre[k - 1], d[k]) : d[k];
        x = Fr::mul(x, w);
    }
    Fr inv = fr_inv_dev(pre[DFT_PER_LANE - 1]);
#pragma unroll
    for (int k = DFT_PER_LANE - 1; k >= 0; k--) {
        const Fr ik = k ? Fr::mul(inv, pre[k - 1]) : inv;                       // 1 / d[k]
        inv = Fr::mul(inv, d[k]);
        if (t0 + k < cnt) store_el(out + t0 + k, Fr::from_mont(unit[k] ? nval : Fr::mul(num, ik)));
    }
}

uint64_t chunk_points() { return env_number("ZKHIP_PTAU_CHUNK", DEFAULT_CHUNK, 1, 1ull << 28, "a number of points from 1 to 2^28", ENV_LAX); }

// the scalars c_j of one transform size
struct DftScalars {
    uint32_t log_n, shift;
    Fr s, w, num, nval;
    DftScalars(const Fr &s_, uint32_t log_n_) : log_n(log_n_), shift(MAX_LOG_N - log_n_), s(s_), w(root_of_unity(log_n_)) {
        Fr sn = s;
        for (uint32_t i = 0; i < log_n; i++) sn = Fr::sqr(sn);
        num = Fr::sub(sn, Fr::one());
        nval = fr_small(1ull << log_n);
    }
    // d_out[t] = c_(j0 + t), t < cnt
    void launch(Fr *d_out, const PowTable &wtab, uint64_t j0, uint64_t cnt, hipStream_t st) const {
        const uint64_t lanes = (cnt + DFT_PER_LANE - 1) / DFT_PER_LANE;
        ZK_LAUNCH(k_power_dft, dim3(nblocks(lanes, 256)), dim3(256), 0, st, d_out, wtab.d.p, shift, s, w, num, nval, j0, cnt);
        ZK_LAUNCH_OK("power dft");
    }
};

// ---------------------------------------------------------------- the operators
void g2_in_subgroup(uint8_t *out, const uint8_t *points, uint64_t n, int32_t device) {
    if (!n) return;
    if (!out || !points) throw std::invalid_argument("null argument");
    const uint64_t chunk = chunk_points(), cap = n < chunk ? n : chunk;
    const bool plain = plain_subgroup();
    const PsiConsts k = psi_consts();
    DeviceGuard g(resolve_device(device));
    need_hbm("zk_g2_in_subgroup", cap * (sizeof(G2Affine) + 1) + 65536);
    Stream st;
    StreamUploader up(st.s);
    DevBuf<G2Affine> pts;
    DevBuf<uint8_t> flags;
    DevBuf<uint32_t> err;
    pts.alloc(cap);
    flags.alloc(cap);
    err.alloc(1);
    for (uint64_t off = 0; off < n; off += cap) {
        const uint64_t cnt = n - off < cap ? n - off : cap;
        up.copy(pts.p, points + off * sizeof(G2Affine), cnt * sizeof(G2Affine));
        launch_point_check<Fq2>(err.p, pts.p, cnt, st.s);
        launch_subgroup(flags.p, nullptr, pts.p, cnt, k, plain, st.s);
        uint32_t bad = NONE;
        HIP_TRY(hipMemcpyAsync(&bad, err.p, 4, hipMemcpyDeviceToHost, st.s));
        HIP_TRY(hipMemcpyAsync(out + off, flags.p, cnt, hipMemcpyDeviceToHost, st.s));
        HIP_TRY(hipStreamSynchronize(st.s));
        if (bad != NONE) throw std::invalid_argument("zk_g2_in_subgroup: point " + std::to_string(off + bad) + " is not on the curve");
    }
}

template <class F>
void power_msm(uint8_t *out, const uint8_t *points, uint64_t n, const uint8_t s32[32], uint64_t first_exp, int32_t device, const char *who) {
    if (!out || !s32 || (n && !points)) throw std::invalid_argument("null argument");
    const Fr s = checked_scalar(s32, std::string(who) + ": the scalar");
    if (first_exp + n < first_exp) throw std::invalid_argument(std::string(who) + ": first_exp + n exceeds 2^64");
    memset(out, 0, sizeof(Affine<F>));
    if (!n) return;
    const uint64_t chunk = chunk_points(), cap = n < chunk ? n : chunk;
    DeviceGuard g(resolve_device(device));
    need_hbm(who, Engine<F>::bytes(cap));
    Stream st;
    PowTable stab;
    stab.build(s, st.s);
    Engine<F> e(st.s, cap);
    Pt<F> acc;
    power_sum(e, acc, n, stab, first_exp, [&](uint64_t off, uint64_t cnt) {
        e.load(points + off * sizeof(Affine<F>), cnt);
        const uint32_t bad = e.first_off_curve(cnt);
        if (bad != NONE) throw std::invalid_argument(std::string(who) + ": point " + std::to_string(off + bad) + " is not on the curve");
        return true;
    });
    memcpy(out, acc.b, sizeof acc.b);
}

void fr_power_dft(uint8_t *out, const uint8_t s32[32], uint32_t log_n, int32_t device) {
    if (!out || !s32) throw std::invalid_argument("null argument");
    if (log_n > MAX_LOG_N) throw std::invalid_argument("zk_fr_power_dft: log_n " + std::to_string(log_n) + " exceeds 28");
    const DftScalars ds(checked_scalar(s32, "zk_fr_power_dft: the scalar"), log_n);
    const uint64_t n = 1ull << log_n, chunk = chunk_points(), cap = n < chunk ? n : chunk;
    DeviceGuard g(resolve_device(device));
    need_hbm("zk_fr_power_dft", cap * sizeof(Fr) + 65536);
    Stream st;
    PowTable wtab;
    wtab.build(root_of_unity(MAX_LOG_N), st.s);
    DevBuf<Fr> d;
    d.alloc(cap);
    for (uint64_t off = 0; off < n; off += cap) {
        const uint64_t cnt = n - off < cap ? n - off : cap;
        ds.launch(d.p, wtab, off, cnt, st.s);
        HIP_TRY(hipMemcpyAsync(out + off * sizeof(Fr), d.p, cnt * sizeof(Fr), hipMemcpyDeviceToHost, st.s));
        HIP_TRY(hipStreamSynchronize(st.s));
    }
}

// ---------------------------------------------------------------- the whole file
constexpr int POWER_SECS[4] = {2, 3, 4, 5}, LAGRANGE_SECS[4] = {12, 13, 14, 15};

struct FilePlan {
    uint32_t power = 0;
    bool prepared = false;
    uint64_t n = 0, cap = 0, device_bytes = 0;
    uint64_t points[16] = {};                         // per section
    uint32_t top[16] = {};                            // the highest level (Lagrange sections) / prefix (power sections)
};

uint64_t point_bytes(int sec) { return sec == 3 || sec == 6 || sec == 13 ? 128 : 64; }

void check_view(const zk_ptau_file_view *v, FilePlan &pl) {
    if (!v) throw std::invalid_argument("null argument");
    int have = 0, missing = 0;
    for (int sec : LAGRANGE_SECS) {
        if (v->sec[sec]) have++;
        else if (!missing) missing = sec;
    }
    if (have && have < 4)
        throw std::invalid_argument("ptau has only some of the Lagrange sections 12 to 15 (section " + std::to_string(missing) + " is missing): it is neither prepared for phase 2 nor not");
    pl.prepared = have == 4;
    const uint32_t max_power = pl.prepared ? 27 : 28;
    if (v->power < 1 || v->power > max_power)
        throw std::invalid_argument("ptau power " + std::to_string(v->power) + " is not supported (1 to " + std::to_string(max_power) +
                                    (pl.prepared ? ": level power + 1 of section 12 needs a 2^(power+1)-th root of unity)" : ")"));
    pl.power = v->power;
    pl.n = 1ull << v->power;
    const uint64_t n = pl.n;
    pl.points[2] = 2 * n - 1;
    pl.points[3] = pl.points[4] = pl.points[5] = n;
    pl.points[6] = 1;
    pl.top[2] = v->power + 1;
    pl.top[3] = pl.top[4] = pl.top[5] = v->power;
    if (pl.prepared) {
        pl.points[12] = 4 * n - 1;
        pl.points[13] = pl.points[14] = pl.points[15] = 2 * n - 1;
        pl.top[12] = v->power + 1;
        pl.top[13] = pl.top[14] = pl.top[15] = v->power;
    }
    for (int sec = 2; sec < 16; sec++) {
        if (!pl.points[sec]) continue;
        if (!v->sec[sec]) throw std::invalid_argument("ptau has no section " + std::to_string(sec));
        const uint64_t need = pl.points[sec] * point_bytes(sec);
        if (v->sec_bytes[sec] < need)
            throw std::invalid_argument("ptau section " + std::to_string(sec) + " is short: " + std::to_string(v->sec_bytes[sec]) + " bytes, power " +
                                        std::to_string(v->power) + " needs " + std::to_string(need));
    }
    const uint64_t chunk = chunk_points(), most = pl.prepared ? 2 * n : n;     // the largest range or level
    pl.cap = most < chunk ? most : chunk;
    pl.device_bytes = EnginePair::bytes(pl.cap) + 2 * POW_BITS * sizeof(Fr) + 65536;
}

struct Checker : EnginePair {
    const zk_ptau_file_view *v;
    const FilePlan &pl;
    zk_ptau_report *rep;
    hipStream_t st;
    Fr s;
    PowTable stab, wtab;
    Checker(const zk_ptau_file_view *v_, const FilePlan &pl_, zk_ptau_report *rep_, const Fr &s_, hipStream_t st_)
        : EnginePair(st_, pl_.cap), v(v_), pl(pl_), rep(rep_), st(st_), s(s_) {
        stab.build(s, st);
        wtab.build(root_of_unity(MAX_LOG_N), st);
    }

    // Loads points [first, first + cnt) of section `sec` and checks them; false: the report names a malformed point
    template <class F>
    bool load_checked(int sec, uint64_t first, uint64_t cnt) {
        engine<F>().load(static_cast<const uint8_t *>(v->sec[sec]) + first * sizeof(Affine<F>), cnt);
        const BadPoint bad = classify<F>(cnt, sec < 12, sec == 3 || sec == 6 || sec == 13);
        if (!bad.kind) return true;
        rep->verdict = 2;
        rep->bad_section = (uint32_t)sec;
        rep->bad_kind = bad.kind;
        rep->bad_index = first + bad.index;
        return false;
    }

    // prefix[p] = sum_(i < min(2^p, m)) s^i P_i of the m points of section `sec`, p <= top; false: malformed
    template <class F>
    bool power_row(int sec, std::vector<Pt<F>> &prefix) {
        const uint64_t m = pl.points[sec];
        const uint32_t top = pl.top[sec];
        prefix.assign(top + 1, Pt<F>());
        Pt<F> acc;
        for (uint32_t p = 0; p <= top; p++) {
            const uint64_t lo = p ? 1ull << (p - 1) : 0, full = 1ull << p, hi = full < m ? full : m;
            if (lo < hi && !power_sum(engine<F>(), acc, hi - lo, stab, lo, [&](uint64_t off, uint64_t cnt) { return load_checked<F>(sec, lo + off, cnt); }))
                return false;
            prefix[p] = acc;
        }
        return true;
    }

    // bit p of the result: level p of Lagrange section `sec` is not the Lagrange form of the row with these prefixes
    template <class F>
    bool lagrange_section(int sec, const std::vector<Pt<F>> &prefix, uint32_t &failed) {
        Engine<F> &e = engine<F>();
        failed = 0;
        for (uint32_t p = 0; p <= pl.top[sec]; p++) {
            const uint64_t n = 1ull << p, base = n - 1;
            const DftScalars ds(s, p);
            Pt<F> acc;
            for (uint64_t off = 0; off < n; off += e.cap) {
                const uint64_t cnt = n - off < e.cap ? n - off : e.cap;
                if (!load_checked<F>(sec, base + off, cnt)) return false;
                ds.launch(e.sc.p, wtab, off, cnt, st);
                e.accumulate(acc, cnt);
            }
            if (!(acc == prefix[p])) failed |= 1u << p;
        }
        return true;
    }
};

// lo = F - s^(m-1) P_(m-1), hi = (F - P_0) / s
template <class F>
void shifted_sums(Pt<F> &lo, Pt<F> &hi, const Pt<F> &sum, const void *row, uint64_t m, const Fr &s) {
    const uint8_t *b = static_cast<const uint8_t *>(row);
    lo = sum - Pt<F>(b + (m - 1) * sizeof(Affine<F>)).times(fr_pow(s, m - 1));
    hi = (sum - Pt<F>(b)).times(Fr::inv(s));
}

void ptau_check(const zk_ptau_file_view *v, const uint8_t *s32_in, int32_t device, zk_ptau_report *rep) {
    if (!rep) throw std::invalid_argument("null argument");
    memset(rep, 0, sizeof *rep);
    FilePlan pl;
    check_view(v, pl);                                // the file is checked before the device is touched
    uint8_t s32[32];
    if (s32_in) {
        memcpy(s32, s32_in, 32);
        if (is_0_or_1(s32) || !below(s32, FrParams::P)) throw std::invalid_argument("zk_ptau_check: the check scalar must be at least 2 and below r");
    } else {
        draw_scalar(s32, "zk_ptau_check");                             // after the file is mapped: its maker did not know s
    }
    const Fr s = fr_from_std(s32);
    Pt<Fq> g1;
    Pt<Fq2> g2;
    generators(g1, g2);
    const uint8_t *T = static_cast<const uint8_t *>(v->sec[2]), *U = static_cast<const uint8_t *>(v->sec[3]);
    uint32_t failed = 0;
    if (!(Pt<Fq>(T) == g1) || !(Pt<Fq2>(U) == g2)) failed |= 1u;

    const int dev = resolve_device(device);
    DeviceGuard g(dev);
    need_hbm("zk_ptau_check", pl.device_bytes);
    Stream st;
    Checker c(v, pl, rep, s, st.s);
    std::vector<Pt<Fq>> pre2, pre4, pre5;
    std::vector<Pt<Fq2>> pre3;
    if (!c.power_row<Fq>(2, pre2) || !c.power_row<Fq2>(3, pre3) || !c.power_row<Fq>(4, pre4) || !c.power_row<Fq>(5, pre5)) return;
    if (!c.load_checked<Fq2>(6, 0, 1)) return;
    uint32_t lag[4] = {0, 0, 0, 0};
    if (pl.prepared) {
        if (!c.lagrange_section<Fq>(12, pre2, lag[0]) || !c.lagrange_section<Fq2>(13, pre3, lag[1]) || !c.lagrange_section<Fq>(14, pre4, lag[2]) ||
            !c.lagrange_section<Fq>(15, pre5, lag[3]))
            return;
    }

    // the five equations, each a product of two pairings that must be 1
    const Pt<Fq> T1(T + 64), B0(v->sec[5]);
    const Pt<Fq2> U1(U + 128), beta2(v->sec[6]);
    Pt<Fq> lo2, hi2, lo4, hi4, lo5, hi5;
    Pt<Fq2> lo3, hi3;
    shifted_sums(lo2, hi2, pre2.back(), v->sec[2], pl.points[2], s);
    shifted_sums(lo3, hi3, pre3.back(), v->sec[3], pl.points[3], s);
    shifted_sums(lo4, hi4, pre4.back(), v->sec[4], pl.points[4], s);
    shifted_sums(lo5, hi5, pre5.back(), v->sec[5], pl.points[5], s);
    const Pt<Fq> ng1 = g1.neg();
    const Pt<Fq> p1[10] = {lo2, hi2.neg(), T1, ng1, lo4, hi4.neg(), lo5, hi5.neg(), B0, ng1};
    const Pt<Fq2> p2[10] = {U1, g2, lo3, hi3, U1, g2, U1, g2, g2, beta2};
    static const uint32_t bit[5] = {2, 3, 4, 5, 6};
    uint8_t b1[10 * 64], b2[10 * 128], gt[5 * 384];
    for (int i = 0; i < 10; i++) {
        memcpy(b1 + 64 * i, p1[i].b, 64);
        memcpy(b2 + 128 * i, p2[i].b, 128);
    }
    if (zk_pairing(gt, b1, b2, 10, 2, dev) != 0) throw std::runtime_error(std::string("zk_ptau_check: ") + get_error());
    for (int e = 0; e < 5; e++) {
        const uint8_t *o = gt + 384 * e;
        bool one = o[0] == 1;
        for (int i = 1; i < 384 && one; i++) one = o[i] == 0;
        if (!one) failed |= 1u << bit[e];
    }
    rep->failed = failed;
    for (int i = 0; i < 4; i++) rep->lagrange_failed[i] = lag[i];
    rep->verdict = failed || lag[0] || lag[1] || lag[2] || lag[3] ? 1 : 0;
}

}   // namespace

extern "C" {

int zk_g2_in_subgroup(uint8_t *out, const uint8_t *points, uint64_t n, int32_t device) {
    return guarded([&] { g2_in_subgroup(out, points, n, device); });
}
int zk_g1_power_msm(uint8_t out[64], const uint8_t *points, uint64_t n, const uint8_t s[32], uint64_t first_exp, int32_t device) {
    return guarded([&] { power_msm<Fq>(out, points, n, s, first_exp, device, "zk_g1_power_msm"); });
}
int zk_g2_power_msm(uint8_t out[128], const uint8_t *points, uint64_t n, const uint8_t s[32], uint64_t first_exp, int32_t device) {
    return guarded([&] { power_msm<Fq2>(out, points, n, s, first_exp, device, "zk_g2_power_msm"); });
}
int zk_fr_power_dft(uint8_t *out, const uint8_t s[32], uint32_t log_n, int32_t device) {
    return guarded([&] { fr_power_dft(out, s, log_n, device); });
}

int zk_ptau_check_sizes(const zk_ptau_file_view *ptau, zk_ptau_check_sizes_t *sizes) {
    return guarded([&] {
        if (!sizes) throw std::invalid_argument("null argument");
        FilePlan pl;
        check_view(ptau, pl);
        sizes->prepared = pl.prepared ? 1 : 0;
        sizes->chunk_points = pl.cap;
        sizes->device_bytes = pl.device_bytes;
    });
}

int zk_ptau_check(const zk_ptau_file_view *ptau, const uint8_t *s32, int32_t device, zk_ptau_report *report) {
    return guarded([&] { ptau_check(ptau, s32, device, report); });
}

}   // extern "C"
