// Column-overflow check of field29.hpp's Montgomery products (host build, g++ -DZK_CHECK_COLUMNS).
// Every v_mad_i64_i32 of the kernels is `acc + a*b` in ONE signed 64-bit register; with the lower eight reduction digits
// unmasked the budget is 18 * 2^58 of operand terms (field29.hpp).  Here each MAD is evaluated in 128 bits and a column that
// leaves int64 is counted.  Shapes covered — every job the kernels run, with the limb ranges their callers produce:
//   JMul tight x tight, JMul tight x wide (one lazily added / doubled operand: DIT butterflies, f2_sqr), JSqr of a tight value,
//   JMulAdd2 of four tight operands, JMulAdd4 with two products of each sign (G2 lane pair's Y3), in Fq and (but JMulAdd4) Fr;
//   plus chains of G1 and G2 mixed additions (curve29.hpp) over random operands, which exercise sub_nc / neg_lazy / dbl_lazy as used;
//   plus the butterfly schedules of nttpair.hip (lazy DIT adds, DIF settle) over the extreme-operand families of
//   tests/extreme_inputs.py — the element whose limbs are all 2^29 - 1 in every register, r - 1, masks, strides — with the
//   all-sums element of a constant vector checked for its VALUE (2^11 v after a tile), and G1 additions with X on full limbs;
//   plus G2 chains through BOTH bound-tracked mixed additions of curve29.hpp: madd(XYZZ<Fq2r>&, ...) as it is, and the lane-pair
//   madd(XYZZ<Fq2s>&, ...) — device-only, it is written with DPP builtins — in a restatement below that keeps the two lanes side
//   by side and follows the kernel statement for statement (the carries of R and D, the operand signs of JMulAdd4, the run3
//   with zz' and zzz' in place).  The chains: random operands; X components T_MAX, q - 1 as held internally (q - 32), 1, 2
//   and 0 in every pairing, a point meeting itself and its negative; those points on a running sum; and the half-zero shapes
//   of tests/extreme_inputs.py (half_zero_g2: P or R zero in exactly one component, y or x with a zero component).  After
//   every addition the lane-pair accumulator must equal the Fq2r one, component by component in canonical form.
//   plus csrc/plonkquot.hip: the per-point statements of k_plonk_quotient and the product of k_coset_load / k_coset_store over
//   cross products of T_MAX, r - 1, 1, 0 and random words, every value checked against 64-bit-word arithmetic; and the loop of
//   spmv_row (csrc/fieldops.hip), 8 products between reductions, for its largest running sum.
// Prints the peak |column| of every block as a multiple of 2^58 and exits 1 on any overflow, wrong all-sums value, lane-pair
// result that differs from the Fq2r one, P, -P that does not end at infinity, wrong PLONK value, or running sum outside (-16r, 16r).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>
#include "curve29.hpp"

using namespace zk;

static std::mt19937_64 rng(20260929);
static const int32_t TIGHT = (1 << 29) + 16, WIDE = (1 << 30) + 32;

// sign: +1 limbs in [0, bound], -1 limbs in [-bound, 0], 0 mixed signs; extreme: every limb at the bound
template <class F>
static F limbs(int32_t bound, int sign, bool extreme) {
    F r;
    for (int i = 0; i < 9; i++) {
        int32_t v = extreme ? bound : (int32_t)(rng() % ((uint64_t)bound + 1));
        if (sign < 0 || (sign == 0 && (rng() & 1))) v = -v;
        r.l[i] = v;
    }
    // limb 8 carries the value's magnitude: at most 16p -> |l8| < 16 * 2^22; keep it within the tight bound anyway
    return r;
}

template <class F>
static void job_shapes(const char *name, bool with_add4) {
    for (int round = 0; round < 20000; round++) {
        const bool ext = round < 64;
        const int sa = ext ? ((round & 1) ? 1 : -1) : 0, sb = ext ? ((round & 2) ? 1 : -1) : 0;
        F a = limbs<F>(TIGHT, sa, ext), b = limbs<F>(TIGHT, sb, ext), w = limbs<F>(WIDE, sb, ext);
        F c = limbs<F>(TIGHT, ext ? sa : 0, ext), d = limbs<F>(TIGHT, ext ? sb : 0, ext);
        (void)F::mul(a, b);
        (void)F::mul(a, w);                     // one lazily added operand
        (void)F::sqr(a);
        (void)F::mul_add2(a, b, c, d);          // extreme rounds: both products of one sign
        F r0, r1;
        F::mul2(r0, a, b, r1, c, w);
        F::sqr2(r0, a, r1, c);
        if (with_add4) {
            // two products >= 0 and two <= 0 (the caller's arrangement): non-negative operands, two of them negated
            F e = limbs<F>(TIGHT, 1, ext), f = limbs<F>(TIGHT, 1, ext), g = limbs<F>(TIGHT, 1, ext), h = limbs<F>(TIGHT, 1, ext);
            F p = limbs<F>(TIGHT, 1, ext), q = limbs<F>(TIGHT, 1, ext), u = limbs<F>(TIGHT, 1, ext), v = limbs<F>(TIGHT, 1, ext);
            (void)F::run1(typename F::JMulAdd4{e, f, g, h, F::neg_lazy(p), q, F::neg_lazy(u), v});
        }
    }
    printf("%-4s job shapes : peak |column| = %.3f * 2^58, overflows %ld\n", name, (double)zk_column_peak() / 288230376151711744.0, zk_column_overflows());
}

template <class F>
static F random_canonical() {
    u32 w[8];
    for (int i = 0; i < 8; i++) w[i] = (u32)rng();
    w[7] &= 0x1fffffffu;                        // < 2^253 < p
    return F::from_words(w);
}

// ---- The butterfly schedules of nttpair.hip (stage / run_window / dif_settle) on the eight registers of a thread, over the
// extreme-operand families of tests/extreme_inputs.py: every register the element whose limbs are all 2^29 - 1 (T_MAX), or
// r - 1 as the kernels hold it (r - 32), or one of them beside zeros (a mask / a stride), against random canonical elements.
// Twiddles are canonical elements as the tables hold them.  Constant registers take the all-sums chain to its end: element 0
// doubles in every stage of a window and its limbs stay full.
static const bool DIT_CARRY_AFTER_SECOND = true;     // run_window: "carried after the second and the last" stage of a window
static const bool DIF_SETTLE = true;                 // run_plan: dif_settle after every window

static Fr29 fr_from_int_limbs(const int32_t (&l)[9]) {
    Fr29 r;
    for (int i = 0; i < 9; i++) r.l[i] = l[i];
    return r;
}

// all_sums: the thread that holds the all-sums elements of a constant vector; their twiddle is 1 (as a table entry: a product)
static void dit_window(Fr29 (&x)[8], int ns, bool first_window, bool all_sums) {
    typedef Fr29 F;
    for (int s = 0; s < ns; s++) {
        const int hb = 1 << s;
        const bool carry_out = ((s & 1) && DIT_CARRY_AFTER_SECOND) || s + 1 == ns;
        for (int k = 0; k < 8; k++) {
            if (k & hb) continue;
            if (first_window && s == 0) {            // level 0: w = 1, carried
                const F u = x[k], v = x[k | hb];
                x[k] = F::add(u, v);
                x[k | hb] = F::sub(u, v);
                continue;
            }
            // the first window is uniform: the butterflies whose twiddle is 1 (the lowest of a sub-transform) skip the product
            const F r = first_window && (k & (hb - 1)) == 0 ? x[k | hb] : F::mul(x[k | hb], all_sums ? F::one() : random_canonical<F>());
            const F u = x[k];
            x[k] = carry_out ? F::add(u, r) : F::add_nc(u, r);
            x[k | hb] = carry_out ? F::sub(u, r) : F::sub_nc(u, r);
        }
    }
}

static void dif_window(Fr29 (&x)[8], int ns, bool all_sums) {
    typedef Fr29 F;
    for (int s = ns - 1; s >= 0; s--) {
        const int hb = 1 << s;
        for (int k = 0; k < 8; k++) {
            if (k & hb) continue;
            const F f = F::sub_nc(x[k], x[k | hb]);
            x[k] = F::add(x[k], x[k | hb]);
            x[k | hb] = F::mul(f, all_sums ? F::one() : random_canonical<F>());
        }
    }
    if (DIF_SETTLE) x[0] = F::reduce_near_zero(x[0]);
}

static bool same_value(const Fr29 &a, const Fr29 &b) {
    const Fr29 ca = Fr29::canonical(a), cb = Fr29::canonical(b);
    for (int i = 0; i < 9; i++)
        if (ca.l[i] != cb.l[i]) return false;
    return true;
}

// pattern: 0 = every register v, 1 = v / 0 alternating (a mask), 2 = v in register 0 only (a stride), 3 = random canonical.
// A tile is 11 bits (plan_windows): a window of two stages and three of three, DIT in this order, DIF backwards.  For a
// constant vector the all-sums element must come out as 2^11 v in both directions.  -> wrong all-sums values
static long family_windows(const char *name, const Fr29 &v, int pattern, int rounds) {
    static const int dit_ns[4] = {2, 3, 3, 3};
    zk_column_peak() = 0;
    const long before = zk_column_overflows();
    long wrong = 0;
    int32_t top = 0;
    Fr29 want = Fr29::canonical(v);
    for (int i = 0; i < 11; i++) want = Fr29::canonical(Fr29::dbl(want));
    for (int round = 0; round < rounds; round++) {
        Fr29 x[8];
        for (int k = 0; k < 8; k++)
            x[k] = pattern == 3 ? random_canonical<Fr29>() : (pattern == 0 || (pattern == 1 && !(k & 1)) || k == 0) ? v : Fr29::zero();
        Fr29 y[8];
        for (int k = 0; k < 8; k++) y[k] = x[k];
        for (int w = 0; w < 4; w++) {
            dit_window(x, dit_ns[w], w == 0, pattern == 0);
            dif_window(y, dit_ns[3 - w], pattern == 0);
            for (int k = 0; k < 8; k++) {
                const int32_t a = x[k].l[8] < 0 ? -x[k].l[8] : x[k].l[8], b = y[k].l[8] < 0 ? -y[k].l[8] : y[k].l[8];
                if (a > top) top = a;
                if (b > top) top = b;
            }
            // a constant vector: every register but 0 is now zero (mod r), and the exchange in front of the next window brings
            // eight all-sums elements together in one thread
            if (pattern == 0)
                for (int k = 1; k < 8; k++) {
                    x[k] = x[0];
                    y[k] = y[0];
                }
        }
        if (pattern == 0 && !(same_value(x[0], want) && same_value(y[0], want))) wrong++;
        for (int k = 0; k < 8; k++) (void)Fr29::canonical(Fr29::mul(x[k], y[k]));
    }
    printf("Fr   windows, %-24s: peak |column| = %.3f * 2^58, peak |value| = %.1f p, overflows %ld, wrong all-sums %ld\n", name,
           (double)zk_column_peak() / 288230376151711744.0, (double)top / 3171406.0, zk_column_overflows() - before, wrong);
    return wrong;
}

static Fq29 &tmax_fq() {                              // the T_MAX element of Fq as families() converted it
    static Fq29 v = Fq29::zero();
    return v;
}

static int families() {
    // the word whose internal value is T_MAX, through the conversion the operators run: limbs 0..7 must come out full
    // T_MAX * 32^-1 mod r and mod q, T_MAX = 3171406 * 2^232 - 1 (tests/extreme_inputs.py: T_MAX_WORD_FR, T_MAX_WORD_FQ)
    static const u32 tmax_word_fr[8] = {0x9f800000u, 0x8a1f0facu, 0x43cdcb84u, 0xe9419f42u, 0xb40c0ac2u, 0x4dc2822du, 0x97098d01u, 0x030644e3u};
    static const u32 tmax_word_fq[8] = {0x6b99d60bu, 0x833764b0u, 0x8311c995u, 0x44e50498u, 0x2d14f783u, 0xfc79b21bu, 0x91dbab1du, 0x244b3ad2u};
    Fr wr;
    Fq wq;
    for (int i = 0; i < 8; i++) {
        wr.v[i] = tmax_word_fr[i];
        wq.v[i] = tmax_word_fq[i];
    }
    const Fr29 tr = Fr29::from_mont256(wr);
    const Fq29 tq = Fq29::from_mont256(wq);
    tmax_fq() = tq;
    for (int i = 0; i < 9; i++) {
        const int32_t want = i < 8 ? (1 << 29) - 1 : 3171405;
        if (tr.l[i] != want || tq.l[i] != want) {
            printf("FAIL: the T_MAX word does not convert to full limbs (limb %d: Fr %d, Fq %d)\n", i, tr.l[i], tq.l[i]);
            return 1;
        }
    }
    int32_t top_l[9];                                // r - 1 as the kernels hold it: (r - 1) * 2^5 = r - 32
    for (int i = 0; i < 9; i++) top_l[i] = Fr29Params::P[i];
    top_l[0] -= 32;
    const Fr29 top = fr_from_int_limbs(top_l);
    long wrong = family_windows("all_ones_limbs", tr, 0, 4);
    wrong += family_windows("all_top", top, 0, 4);
    family_windows("mask of all_ones_limbs", tr, 1, 2000);
    family_windows("stride of all_ones_limbs", tr, 2, 2000);
    family_windows("random", tr, 3, 2000);
    if (wrong) {
        printf("FAIL: the all-sums element of a constant vector came out wrong\n");
        return 1;
    }
    // G1 mixed additions with X on full limbs: the point meets itself (the doubling branch) and its negative (infinity) in turn
    zk_column_peak() = 0;
    XYZZ<Fq29> acc = XYZZ<Fq29>::inf();
    for (int i = 0; i < 4000; i++) {
        Affine<Fq29> p{tq, (i & 4) ? tq : random_canonical<Fq29>()};
        if (i & 1) negate_y(p);
        madd(acc, p);
        if ((i & 7) == 7) madd(acc, p);
    }
    printf("G1 mixed additions, X = T_MAX  : peak |column| = %.3f * 2^58, overflows %ld\n", (double)zk_column_peak() / 288230376151711744.0,
           zk_column_overflows());
    return 0;
}

// ---- The lane-pair G2 mixed addition of curve29.hpp (madd(XYZZ<Fq2s>&, ...)) restated for the host.  The device version holds
// the real component of an Fq2 value in an even lane and the imaginary one in its odd neighbour and exchanges operands with
// DPP moves; here a "register" is the pair of values the two lanes hold (Reg), the exchanges are plain copies, and every
// statement runs for lane 0 (even) and lane 1 (odd) in turn.  Everything else is the kernel's, statement for statement: sub_nc
// for P and sub for R, sqr_operands, prepare, and the run3 of JMulAdd2, JMulAdd2 and JMulAdd4 with zz' and zzz' in place.
struct Reg {
    Fq29 l[2];
};
struct Fq2h {
    Reg v;
    typedef Fq29 B;
    static Reg other(const Reg &a) { return Reg{{a.l[1], a.l[0]}}; }          // quad_perm [1,0,3,2]
    static Reg from_even(const Reg &a) { return Reg{{a.l[0], a.l[0]}}; }      // quad_perm [0,0,2,2]
    static Reg from_odd(const Reg &a) { return Reg{{a.l[1], a.l[1]}}; }       // quad_perm [1,1,3,3]
    template <class Fn>
    static Reg lanes(Fn f) { return Reg{{f(0), f(1)}}; }                      // f(lane): what the lane computes; odd() == (lane == 1)
    static bool both(bool even, bool odd) { return even && odd; }             // the AND over the pair
    static Fq2h zero() { return Fq2h{Reg{{B::zero(), B::zero()}}}; }
    static Fq2h one() { return Fq2h{Reg{{B::one(), B::zero()}}}; }            // sel(odd(), zero, one)
    bool is_zero() const { return both(v.l[0].is_zero(), v.l[1].is_zero()); }
    bool is_zero_raw() const { return both(v.l[0].is_zero_raw(), v.l[1].is_zero_raw()); }
    static Fq2h add(const Fq2h &x, const Fq2h &y) { return Fq2h{lanes([&](int k) { return B::add(x.v.l[k], y.v.l[k]); })}; }
    static Fq2h sub(const Fq2h &x, const Fq2h &y) { return Fq2h{lanes([&](int k) { return B::sub(x.v.l[k], y.v.l[k]); })}; }
    static Fq2h dbl(const Fq2h &x) { return Fq2h{lanes([&](int k) { return B::dbl(x.v.l[k]); })}; }
    struct Pre {
        Reg a0, a1s;
    };
    static Pre prepare(const Fq2h &x) {
        const Reg a1 = from_odd(x.v);
        return Pre{from_even(x.v), lanes([&](int k) { return k ? a1.l[k] : B::neg_lazy(a1.l[k]); })};      // sel(odd(), a1, -a1)
    }
    static Fq2h mul(const Fq2h &x, const Fq2h &y) {
        const Pre p = prepare(x);
        const Reg yo = other(y.v);
        return Fq2h{lanes([&](int k) { return B::mul_add2(p.a0.l[k], y.v.l[k], p.a1s.l[k], yo.l[k]); })};
    }
    static void sqr_operands(Reg &u, Reg &w, const Fq2h &x) {
        const Reg a0 = from_even(x.v), xo = other(x.v);
        const Reg t = lanes([&](int k) { return k ? B::zero() : xo.l[k]; });  // xo & keep, keep = odd() ? 0 : -1
        u = lanes([&](int k) { return B::add_nc(a0.l[k], xo.l[k]); });
        w = lanes([&](int k) { return B::sub(x.v.l[k], t.l[k]); });
    }
    static Fq2h sqr(const Fq2h &x) {
        Reg u, w;
        sqr_operands(u, w, x);
        return Fq2h{lanes([&](int k) { return B::mul(u.l[k], w.l[k]); })};
    }
    static void mul2(Fq2h &r0, const Pre &x0, const Fq2h &y0, Fq2h &r1, const Pre &x1, const Fq2h &y1) {
        const Reg yo0 = other(y0.v), yo1 = other(y1.v);
        for (int k = 0; k < 2; k++)
            B::run2(r0.v.l[k], B::JMulAdd2{x0.a0.l[k], y0.v.l[k], x0.a1s.l[k], yo0.l[k]}, r1.v.l[k], B::JMulAdd2{x1.a0.l[k], y1.v.l[k], x1.a1s.l[k], yo1.l[k]});
    }
    static void mul2(Fq2h &r0, const Fq2h &x0, const Fq2h &y0, Fq2h &r1, const Fq2h &x1, const Fq2h &y1) {
        mul2(r0, prepare(x0), y0, r1, prepare(x1), y1);
    }
    static void sqr2(Fq2h &r0, const Fq2h &x0, Fq2h &r1, const Fq2h &x1) {
        Reg u0, w0, u1, w1;
        sqr_operands(u0, w0, x0);
        sqr_operands(u1, w1, x1);
        for (int k = 0; k < 2; k++) B::mul2(r0.v.l[k], u0.l[k], w0.l[k], r1.v.l[k], u1.l[k], w1.l[k]);
    }
};

static void madd(XYZZ<Fq2h> &acc, const Affine<Fq2h> &p) {
    typedef Fq29 B;
    typedef Fq2h F;
    if (p.is_inf()) return;
    if (acc.is_inf()) {
        acc = XYZZ<F>{p.x, F{F::lanes([&](int k) { return B::carry(p.y.v.l[k]); })}, F::one(), F::one()};
        return;
    }
    F U2, S2;
    F::mul2(U2, p.x, acc.zz, S2, p.y, acc.zzz);
    F P{F::lanes([&](int k) { return B::sub_nc(U2.v.l[k], acc.x.v.l[k]); })};
    F R{F::lanes([&](int k) { return B::sub(S2.v.l[k], acc.y.v.l[k]); })};
    if (P.is_zero()) {
        if (R.is_zero()) acc = dbl_affine(Affine<F>{p.x, F{F::lanes([&](int k) { return B::carry(p.y.v.l[k]); })}});
        else acc = XYZZ<F>::inf();
        return;
    }
    F PP, R2;
    F::sqr2(PP, P, R2, R);
    const F::Pre pp = F::prepare(PP);
    F PPP, Q;
    F::mul2(PPP, pp, P, Q, pp, acc.x);
    const F::Pre ppp = F::prepare(PPP);
    for (int k = 0; k < 2; k++) {
        for (int i = 0; i < 9; i++) acc.x.v.l[k].l[i] = R2.v.l[k].l[i] - PPP.v.l[k].l[i] - (Q.v.l[k].l[i] << 1);
        acc.x.v.l[k] = B::carry(acc.x.v.l[k]);                                 // X3
    }
    const Reg D = F::lanes([&](int k) { return B::sub(Q.v.l[k], acc.x.v.l[k]); }), Do = F::other(D);
    const Reg ny = F::lanes([&](int k) { return B::neg_lazy(acc.y.v.l[k]); }), nyo = F::other(ny);
    const F::Pre rp = F::prepare(R);
    const Reg zzo = F::other(acc.zz.v), zzzo = F::other(acc.zzz.v);
    Reg Y3;
    for (int k = 0; k < 2; k++)
        B::run3(acc.zz.v.l[k], B::JMulAdd2{pp.a0.l[k], acc.zz.v.l[k], pp.a1s.l[k], zzo.l[k]},                     // zz', zzz' in place
                acc.zzz.v.l[k], B::JMulAdd2{ppp.a0.l[k], acc.zzz.v.l[k], ppp.a1s.l[k], zzzo.l[k]},
                Y3.l[k], B::JMulAdd4{rp.a0.l[k], D.l[k], rp.a1s.l[k], Do.l[k], ppp.a0.l[k], ny.l[k], ppp.a1s.l[k], nyo.l[k]});
    acc.y = F{Y3};
}

static Fq2h lane_form(const Fq2r &x) { return Fq2h{Reg{{x.a, x.b}}}; }

// A chain: points added in turn, the accumulator reset to infinity in front of a step where `fresh` is set.
struct Step {
    Affine<Fq2r> p;
    bool fresh;
};
typedef std::vector<Step> Chain;

// the accumulator after a step: infinity or eight canonical components
struct Snap {
    bool inf;
    Fq29 c[8];
};
static Snap snap(const XYZZ<Fq2r> &a) {
    Snap s{a.is_inf(), {}};
    const Fq29 *src[8] = {&a.x.a, &a.x.b, &a.y.a, &a.y.b, &a.zz.a, &a.zz.b, &a.zzz.a, &a.zzz.b};
    for (int i = 0; i < 8; i++) s.c[i] = Fq29::canonical(*src[i]);
    return s;
}
static Snap snap(const XYZZ<Fq2h> &a) {
    Snap s{a.is_inf(), {}};
    const Fq29 *src[8] = {&a.x.v.l[0], &a.x.v.l[1], &a.y.v.l[0], &a.y.v.l[1], &a.zz.v.l[0], &a.zz.v.l[1], &a.zzz.v.l[0], &a.zzz.v.l[1]};
    for (int i = 0; i < 8; i++) s.c[i] = Fq29::canonical(*src[i]);
    return s;
}
static bool same(const Snap &a, const Snap &b) {
    if (a.inf != b.inf) return false;
    if (a.inf) return true;
    for (int i = 0; i < 8; i++)
        for (int k = 0; k < 9; k++)
            if (a.c[i].l[k] != b.c[i].l[k]) return false;
    return true;
}

// Runs the chain through the Fq2r madd, then through the lane-pair restatement, and compares the accumulator after every step.
// want_inf: indices of steps after which the accumulator must be infinity (a point met its negative).  -> 0, or 1 after FAIL
static int run_chain(const char *name, const Chain &ch, const std::vector<size_t> &want_inf) {
    const long before = zk_column_overflows();
    std::vector<Snap> ref;
    ref.reserve(ch.size());
    zk_column_peak() = 0;
    XYZZ<Fq2r> acc = XYZZ<Fq2r>::inf();
    long infs = 0;
    for (const Step &s : ch) {
        if (s.fresh) acc = XYZZ<Fq2r>::inf();
        madd(acc, s.p);
        ref.push_back(snap(acc));
        infs += acc.is_inf();
    }
    const double peak_r = (double)zk_column_peak() / 288230376151711744.0;
    for (size_t i : want_inf)
        if (!ref[i].inf) {
            printf("FAIL: %s: step %zu of the Fq2r chain did not end at infinity\n", name, i);
            return 1;
        }
    zk_column_peak() = 0;
    XYZZ<Fq2h> acch = XYZZ<Fq2h>::inf();
    for (size_t i = 0; i < ch.size(); i++) {
        if (ch[i].fresh) acch = XYZZ<Fq2h>::inf();
        madd(acch, Affine<Fq2h>{lane_form(ch[i].p.x), lane_form(ch[i].p.y)});
        if (!same(snap(acch), ref[i])) {
            printf("FAIL: %s: the lane-pair addition differs from the Fq2r one at step %zu\n", name, i);
            return 1;
        }
    }
    printf("G2 %-28s: %6zu additions (%ld to infinity), peak |column| = %.3f * 2^58 (Fq2r), %.3f * 2^58 (lane pair), overflows %ld\n", name,
           ch.size(), infs, peak_r, (double)zk_column_peak() / 288230376151711744.0, zk_column_overflows() - before);
    return 0;
}

static Fq29 small_fq(int32_t v) {
    Fq29 r = Fq29::zero();
    r.l[0] = v;
    return r;
}

static Affine<Fq2r> with_neg_y(Affine<Fq2r> p) {
    negate_y(p);
    return p;
}

static int g2_chains(const Fq29 &tq) {
    Fq29 qm = Fq29::zero();                          // q - 1 as the kernels hold it: (q - 1) * 2^5 = q - 32
    for (int i = 0; i < 9; i++) qm.l[i] = Fq29Params::P[i];
    qm.l[0] -= 32;
    int bad = 0;
    // random operands: the chain of main(), now through both additions
    Chain rnd;
    for (int i = 0; i < 10000; i++) {
        Affine<Fq2r> p{Fq2r{random_canonical<Fq29>(), random_canonical<Fq29>()}, Fq2r{random_canonical<Fq29>(), random_canonical<Fq29>()}};
        if (i & 1) negate_y(p);
        rnd.push_back(Step{p, false});
    }
    bad |= run_chain("random chain", rnd, {});
    // extreme X: every pairing of T_MAX, q - 32, 1, 2 and 0 for the two components, Y random or extreme as well
    const Fq29 comp[5] = {tq, qm, small_fq(1), small_fq(2), Fq29::zero()};
    std::vector<Affine<Fq2r>> ext;
    for (int a = 0; a < 5; a++)
        for (int b = 0; b < 5; b++) {
            if (a == 4 && b == 4) continue;
            ext.push_back(Affine<Fq2r>{Fq2r{comp[a], comp[b]}, Fq2r{random_canonical<Fq29>(), random_canonical<Fq29>()}});
            ext.push_back(Affine<Fq2r>{Fq2r{comp[a], comp[b]}, Fq2r{comp[b == 4 ? 0 : b], comp[a == 4 ? 1 : a]}});
        }
    // a point meets itself (the doubling branch), then its negative twice: 2P - P is a general addition whose result is P
    // again with zz != 1, and P - P ends at infinity from there
    Chain self;
    std::vector<size_t> ends;
    for (size_t i = 0; i < ext.size(); i++)
        for (int neg_first = 0; neg_first < 2; neg_first++) {
            const Affine<Fq2r> p = neg_first ? with_neg_y(ext[i]) : ext[i], m = neg_first ? ext[i] : with_neg_y(ext[i]);
            self.push_back(Step{p, true});
            self.push_back(Step{p, false});
            self.push_back(Step{m, false});
            self.push_back(Step{m, false});
            ends.push_back(self.size() - 1);
            self.push_back(Step{p, true});           // and the plain pair P, -P on a fresh accumulator
            self.push_back(Step{m, false});
            ends.push_back(self.size() - 1);
        }
    bad |= run_chain("extreme X, self and negative", self, ends);
    // general additions: a running accumulator takes the extreme points in turn, random ones between them
    Chain gen;
    for (int round = 0; round < 40; round++)
        for (size_t i = 0; i < ext.size(); i++) {
            Affine<Fq2r> p = ext[(i * 7 + round) % ext.size()];
            if ((i + round) & 1) negate_y(p);
            gen.push_back(Step{p, false});
            if (i % 3 == 2) gen.push_back(Step{Affine<Fq2r>{Fq2r{random_canonical<Fq29>(), random_canonical<Fq29>()}, Fq2r{random_canonical<Fq29>(), random_canonical<Fq29>()}}, false});
        }
    bad |= run_chain("extreme X, running sum", gen, {});
    // the half-zero shapes of tests/extreme_inputs.py (half_zero_g2), a fresh affine accumulator meeting the second point:
    //   (a) / (b) P = U2 - x zero in one component only;  (c) R = 0 with P != 0, and R zero in one component only;
    //   (d) y with a zero component: P, -P gives P = 0 with R = -2y half zero (infinity, not the doubling), P, P the doubling;
    //   (e) x with a zero component.  Each pair in both orders.
    Chain half;
    std::vector<size_t> hends;
    const Fq29 vals[4] = {tq, qm, small_fq(3), random_canonical<Fq29>()};
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            if (i == j) continue;
            const Fq29 s = vals[i], t1 = vals[j], t2 = vals[(j + 1) % 4 == i ? (j + 2) % 4 : (j + 1) % 4];
            const Fq2r y1{random_canonical<Fq29>(), vals[(i + j) % 4]}, y2{vals[(i + 2 * j) % 4], random_canonical<Fq29>()};
            const Fq2r y3{y1.a, y2.b}, y4{y2.a, y1.b};
            const Affine<Fq2r> pairs[][2] = {
                {{Fq2r{s, t1}, y1}, {Fq2r{s, t2}, y2}},              // (a)
                {{Fq2r{t1, s}, y1}, {Fq2r{t2, s}, y2}},              // (b)
                {{Fq2r{s, t1}, y1}, {Fq2r{t1, t2}, y1}},             // (c) R = 0
                {{Fq2r{s, t1}, y1}, {Fq2r{t1, t2}, y3}},             // R = (0, *)
                {{Fq2r{s, t1}, y1}, {Fq2r{t1, t2}, y4}},             // R = (*, 0)
                {{Fq2r{s, t1}, y1}, {Fq2r{s, t2}, y3}},              // P = (0, *) and R = (0, *)
                {{Fq2r{s, t1}, y1}, {Fq2r{s, t2}, y4}},              // P = (0, *) and R = (*, 0)
            };
            for (const auto &pr : pairs)
                for (int order = 0; order < 2; order++) {
                    half.push_back(Step{pr[order], true});
                    half.push_back(Step{pr[1 - order], false});
                    half.push_back(Step{with_neg_y(pr[order]), false});     // and a general addition on top of the result
                }
            const Affine<Fq2r> zc[4] = {{Fq2r{s, t1}, Fq2r{t2, Fq29::zero()}}, {Fq2r{s, t1}, Fq2r{Fq29::zero(), t2}},     // (d)
                                        {Fq2r{s, Fq29::zero()}, y1}, {Fq2r{Fq29::zero(), s}, y2}};                         // (e)
            for (const auto &p : zc) {
                half.push_back(Step{p, true});
                half.push_back(Step{with_neg_y(p), false});
                hends.push_back(half.size() - 1);
                half.push_back(Step{with_neg_y(p), true});
                half.push_back(Step{with_neg_y(p), false});               // the doubling branch with lazily negated y
                half.push_back(Step{p, false});
                half.push_back(Step{p, false});
                hends.push_back(half.size() - 1);
            }
        }
    bad |= run_chain("half-zero shapes", half, hends);
    return bad;
}

// ---- csrc/plonkquot.hip on the host: the per-point statements of k_plonk_quotient one for one (the mul2 pairs, the run2 of
// the two JMulAdd2 jobs, add / sub exactly where the kernel has them) and the product of k_coset_load / k_coset_store with
// its running power, every result checked for its VALUE against arithmetic that shares nothing with field29.hpp: 4 x 64-bit
// Montgomery products in unsigned __int128 (mont64), K(x, y) = x y 2^-261 = mont64(mont64(x, y), 2^251).
// -DPLONK_MUTANT=K (0: the kernel as it is) builds one of the deliberate changes of DESIGN.md section 10 into the restatement;
// the argument `plonk` runs these blocks alone and exits 1 when the change is seen (a wrong value or an overflow).
struct U256 {
    uint64_t w[4];
};
static U256 R64;                                      // r
static uint64_t R64_N0;                               // -r^-1 mod 2^64
static bool u_ge(const U256 &a, const U256 &b) {
    for (int i = 3; i >= 0; i--)
        if (a.w[i] != b.w[i]) return a.w[i] > b.w[i];
    return true;
}
static U256 u_sub_raw(const U256 &a, const U256 &b) {
    U256 r;
    unsigned __int128 br = 0;
    for (int i = 0; i < 4; i++) {
        const unsigned __int128 d = (unsigned __int128)a.w[i] - b.w[i] - br;
        r.w[i] = (uint64_t)d;
        br = (d >> 64) & 1;
    }
    return r;
}
static U256 u_add(const U256 &a, const U256 &b) {     // mod r, operands below r < 2^254
    U256 r;
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; i++) {
        c += (unsigned __int128)a.w[i] + b.w[i];
        r.w[i] = (uint64_t)c;
        c >>= 64;
    }
    return u_ge(r, R64) ? u_sub_raw(r, R64) : r;
}
static U256 u_sub(const U256 &a, const U256 &b) { return u_ge(a, b) ? u_sub_raw(a, b) : u_sub_raw(R64, u_sub_raw(b, a)); }     // r - (b - a)
static U256 mont64(const U256 &a, const U256 &b) {    // a b 2^-256 mod r
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        unsigned __int128 c = 0;
        for (int j = 0; j < 4; j++) {
            c += (unsigned __int128)a.w[j] * b.w[i] + t[j];
            t[j] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[4] = (uint64_t)c;
        t[5] = (uint64_t)(c >> 64);
        const uint64_t m = t[0] * R64_N0;
        c = ((unsigned __int128)m * R64.w[0] + t[0]) >> 64;
        for (int j = 1; j < 4; j++) {
            c += (unsigned __int128)m * R64.w[j] + t[j];
            t[j - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = t[5] + (uint64_t)(c >> 64);
    }
    U256 r{{t[0], t[1], t[2], t[3]}};
    return (t[4] || u_ge(r, R64)) ? u_sub_raw(r, R64) : r;
}
static U256 u_from_limbs(const int32_t (&l)[9]) {     // non-negative limbs below 2^29, value below 2^256
    U256 r{{0, 0, 0, 0}};
    for (int i = 0; i < 9; i++) {
        const int bit = 29 * i, w = bit >> 6, s = bit & 63;
        r.w[w] |= (uint64_t)(uint32_t)l[i] << s;
        if (s > 35 && w < 3) r.w[w + 1] |= (uint64_t)(uint32_t)l[i] >> (64 - s);
    }
    return r;
}
static U256 u_of(const Fr29 &x) { return u_from_limbs(Fr29::canonical(x).l); }
static U256 K(const U256 &x, const U256 &y) {
    static const U256 two251{{0, 0, 0, 1ull << 59}};
    return mont64(mont64(x, y), two251);
}
static bool u_eq(const U256 &a, const U256 &b) { return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3]; }
static void u_init() {
    R64 = u_from_limbs(Fr29Params::P);
    uint64_t inv = 1;                                 // Newton: r^-1 mod 2^64
    for (int i = 0; i < 6; i++) inv *= 2 - R64.w[0] * inv;
    R64_N0 = 0 - inv;
}
static double in_units_of_r(const Fr29 &x) {          // the value the limbs stand for, over r
    long double v = 0, r = 0;
    for (int i = 8; i >= 0; i--) {
        v = v * 536870912.0L + x.l[i];
        r = r * 536870912.0L + Fr29Params::P[i];
    }
    return (double)(v / r);
}

#ifndef PLONK_MUTANT
#define PLONK_MUTANT 0
#endif
struct QuotRows {                                     // what a lane loads for one point: canonical words
    Fr29 a, b, c, z, zw, ql, qr, qm, qo, qc, s1, s2, s3, l1, pi;
};
struct QuotK {                                        // QuotConsts, and the lane's 1 / Z_H
    Fr29 alpha, alpha2, beta, gamma, bk1, bk2, zh, step;
};
struct QuotStats {
    double num_peak = 0, sum_peak = 0;
    long points = 0, wrong = 0;
};
// the body of k_plonk_quotient's loop; x is the lane's running point and moves on.  M: the deliberate change
template <int M>
static Fr29 quot_point(const QuotRows &v, const QuotK &k, Fr29 &x, bool has_pi, QuotStats &st) {
    typedef Fr29 F;
    const F &a = v.a, &b = v.b, &c = v.c, &z = v.z, &alpha = k.alpha, &alpha2 = k.alpha2, &beta = k.beta, &gamma = k.gamma, &bk1 = k.bk1, &bk2 = k.bk2;
    F ab, bx, b1x, b2x, bs1, bs2, bs3, bz;
    F::mul2(ab, a, b, bx, beta, x);
    F::mul2(b1x, bk1, x, b2x, bk2, x);
    const F f1 = M == 1 ? F::add_nc(F::add_nc(a, bx), gamma) : F::add(F::add(a, bx), gamma);
    const F f2 = M == 1 ? F::add_nc(F::add_nc(b, b1x), gamma) : F::add(F::add(b, b1x), gamma), f3 = F::add(F::add(c, b2x), gamma);
    F::mul2(bs1, beta, v.s1, bs2, beta, v.s2);
    F::mul2(bs3, beta, v.s3, bz, M == 6 ? z : F::sub(z, F::one()), v.l1);
    const F g1 = M == 7 ? F::add_nc(F::add_nc(a, bs1), gamma) : F::add(F::add(a, bs1), gamma);
    const F g2 = M == 7 ? F::add_nc(F::add_nc(b, bs2), gamma) : F::add(F::add(b, bs2), gamma), g3 = F::add(F::add(c, bs3), gamma);
    F p12, q12, p3, q3, P, Q, G1, G2, aD, T2, t, xn;
    F::mul2(p12, f1, f2, q12, g1, g2);
    F::mul2(p3, f3, z, q3, g3, v.zw);
    F::mul2(P, p12, p3, Q, q12, q3);
    {
        F c3 = c;                                     // M == 3: c + 3r summed lazily, the same value mod r
        if (M == 3)
            for (int i = 0; i < 9; i++) c3.l[i] += 3 * Fr29Params::P[i];
        F::run2(G1, F::JMulAdd2{v.ql, a, v.qr, b}, G2, F::JMulAdd2{v.qm, ab, v.qo, c3});
    }
    F::mul2(aD, alpha, M == 5 ? F::sub_nc(Q, P) : F::sub(P, Q), T2, alpha2, bz);
    F num;
    if (M == 2) {
        num = F::add_nc(F::add_nc(G1, G2), F::add_nc(v.qc, aD));
        num = F::add_nc(num, T2);
        if (has_pi) num = F::add_nc(num, v.pi);
    } else {
        num = F::add(F::add(G1, G2), F::add(v.qc, aD));
        num = F::add(num, T2);
        if (has_pi) num = F::add(num, v.pi);
    }
    F::mul2(t, num, k.zh, xn, x, k.step);
    // the same point in 64-bit words
    const U256 ux = u_of(x), ua = u_of(a), ub = u_of(b), uc = u_of(c), uz = u_of(z), ube = u_of(beta), uga = u_of(gamma);
    const U256 uf1 = u_add(u_add(ua, K(ube, ux)), uga), uf2 = u_add(u_add(ub, K(u_of(bk1), ux)), uga), uf3 = u_add(u_add(uc, K(u_of(bk2), ux)), uga);
    const U256 ug1 = u_add(u_add(ua, K(ube, u_of(v.s1))), uga), ug2 = u_add(u_add(ub, K(ube, u_of(v.s2))), uga), ug3 = u_add(u_add(uc, K(ube, u_of(v.s3))), uga);
    const U256 up = K(K(uf1, uf2), K(uf3, uz)), uq = K(K(ug1, ug2), K(ug3, u_of(v.zw)));
    U256 un = u_add(u_add(K(u_of(v.ql), ua), K(u_of(v.qr), ub)), u_add(K(u_of(v.qm), K(ua, ub)), K(u_of(v.qo), uc)));
    un = u_add(un, u_of(v.qc));
    if (has_pi) un = u_add(un, u_of(v.pi));
    un = u_add(un, K(u_of(alpha), u_sub(up, uq)));
    un = u_add(un, K(u_of(alpha2), K(u_sub(uz, u_of(F::one())), u_of(v.l1))));
    const F tc = F::canonical(t);                     // F::store
    st.points++;
    if (!u_eq(u_from_limbs(tc.l), K(un, u_of(k.zh))) || !u_eq(u_of(xn), K(ux, u_of(k.step)))) st.wrong++;
    const double nv = in_units_of_r(num), fv[6] = {in_units_of_r(f1), in_units_of_r(f2), in_units_of_r(f3), in_units_of_r(g1), in_units_of_r(g2), in_units_of_r(g3)};
    if ((nv < 0 ? -nv : nv) > st.num_peak) st.num_peak = nv < 0 ? -nv : nv;
    for (double f : fv)
        if (f > st.sum_peak) st.sum_peak = f;
    x = xn;
    return tc;
}

static Fr29 fr_extreme(int which) {                   // T_MAX, r - 1, 1, 0 as canonical words; 4: a random canonical word
    Fr29 r = Fr29::zero();
    switch (which) {
    case 0:
        for (int i = 0; i < 9; i++) r.l[i] = i < 8 ? (1 << 29) - 1 : 3171405;
        break;
    case 1:
        for (int i = 0; i < 9; i++) r.l[i] = Fr29Params::P[i];
        r.l[0] -= 1;
        break;
    case 2: r.l[0] = 1; break;
    case 3: break;
    default: r = random_canonical<Fr29>();
    }
    return r;
}
static Fr29 fr_drawn() { return fr_extreme((int)(rng() % 5)); }

// Operands.  Pass 1: the cross product of {T_MAX, r - 1, 1, 0, random} over the wires a, b, c, z and over alpha, beta, gamma
// (5^7 points), every other loaded word, 1 / Z_H and the step drawn from the same five by the generator.  Pass 2: the cross
// product over ql, qr, qm, qo, qc, the three sigmas as one, z(w x) and L1 (5^8), the wires and challenges drawn.  beta k1,
// beta k2 are beta k by the reference product (k1 = 2, k2 = 3 in that form), alpha^2 likewise.  x: a word of the five at
// the start of a lane, then the raw product x step of the previous point, as on the device.  PI present at every second point.
template <int M>
static int plonk_quotient_points() {
    zk_column_peak() = 0;
    const long before = zk_column_overflows();
    QuotStats st;
    auto word = [](const U256 &u) {                   // canonical value -> limbs
        u32 w[8];
        for (int i = 0; i < 4; i++) w[2 * i] = (u32)u.w[i], w[2 * i + 1] = (u32)(u.w[i] >> 32);
        return Fr29::from_words(w);
    };
    const U256 one = u_of(Fr29::one());
    const U256 two = u_add(one, one), three = u_add(two, one);
    Fr29 x = fr_drawn();
    long idx = 0;
    auto point = [&](QuotRows &v, QuotK &k) {
        k.alpha2 = word(K(u_of(k.alpha), u_of(k.alpha)));
        k.bk1 = word(K(u_of(k.beta), two));
        k.bk2 = word(K(u_of(k.beta), three));
        if (idx % 16 == 0) x = fr_drawn();            // a new lane
        (void)quot_point<M>(v, k, x, (idx & 1) == 0, st);
        idx++;
    };
    for (int i = 0; i < 78125; i++) {                 // 5^7
        QuotRows v;
        QuotK k;
        int d = i;
        Fr29 *cross[7] = {&v.a, &v.b, &v.c, &v.z, &k.alpha, &k.beta, &k.gamma};
        for (Fr29 *p : cross) *p = fr_extreme(d % 5), d /= 5;
        Fr29 *rest[13] = {&v.zw, &v.ql, &v.qr, &v.qm, &v.qo, &v.qc, &v.s1, &v.s2, &v.s3, &v.l1, &v.pi, &k.zh, &k.step};
        for (Fr29 *p : rest) *p = fr_drawn();
        point(v, k);
    }
    for (int i = 0; i < 390625; i++) {                // 5^8
        QuotRows v;
        QuotK k;
        int d = i;
        Fr29 *cross[8] = {&v.ql, &v.qr, &v.qm, &v.qo, &v.qc, &v.s1, &v.zw, &v.l1};
        for (Fr29 *p : cross) *p = fr_extreme(d % 5), d /= 5;
        v.s2 = v.s3 = v.s1;
        Fr29 *rest[10] = {&v.a, &v.b, &v.c, &v.z, &v.pi, &k.alpha, &k.beta, &k.gamma, &k.zh, &k.step};
        for (Fr29 *p : rest) *p = fr_drawn();
        point(v, k);
    }
    const long over = zk_column_overflows() - before;
    printf("PLONK quotient point: peak |column| / 2^58 = %.3f, largest |num| / r = %.3f, largest f / r = %.3f, %ld points, wrong values %ld, overflows %ld\n",
           (double)zk_column_peak() / 288230376151711744.0, st.num_peak, st.sum_peak, st.points, st.wrong, over);
    return st.wrong || over;
}

// k_coset_load: store(x p), p the lane's power: a word at the start, then the raw product p step.  k_coset_store: the same
// product made canonical, and the raw-limb zero test that feeds t_len, which must say "zero" exactly where the value is 0
template <int M>
static int plonk_coset_products() {
    zk_column_peak() = 0;
    const long before = zk_column_overflows();
    long wrong = 0, products = 0;
    for (int i = 0; i < 125 * 40; i++) {
        const Fr29 step = fr_extreme(i % 5), seed = fr_extreme(i / 5 % 5);
        Fr29 p = seed;
        for (int k = 0; k < 16; k++) {
            const Fr29 x = k % 5 == 4 ? fr_extreme(i / 25 % 5) : fr_drawn();
            const Fr29 prod = Fr29::mul(x, p), o = M == 4 ? prod : Fr29::canonical(prod);
            const U256 want = K(u_of(x), u_of(p));
            bool same = true;
            Fr29 w = Fr29::zero();
            {
                u32 ww[8];
                for (int j = 0; j < 4; j++) ww[2 * j] = (u32)want.w[j], ww[2 * j + 1] = (u32)(want.w[j] >> 32);
                w = Fr29::from_words(ww);
            }
            for (int j = 0; j < 9; j++) same = same && o.l[j] == w.l[j];
            if (!same || o.is_zero_raw() != w.is_zero_raw()) wrong++;
            products++;
            p = Fr29::mul(p, step);
        }
    }
    const long over = zk_column_overflows() - before;
    printf("PLONK coset load / store: peak |column| / 2^58 = %.3f, %ld products, wrong values %ld, overflows %ld\n",
           (double)zk_column_peak() / 288230376151711744.0, products, wrong, over);
    return wrong || over;
}

// spmv_row of csrc/fieldops.hip (k_spmv_abc, k_spmv_abc_long): a sum reduced after every 8 products, which csrc/r1cs.hip says
// "touches the bound".  Rows of 64 terms of the witness word 2^256 - 1 (a valid operand: below 6 r) times the coefficient word
// r - 1, and of words within 2^24 below them; the largest running sum in units of r must stay inside (-16, 16).  (A product
// of non-negative operands below 2^256 and r lies in [0, r + r / 32): eight of them on a sum below r stay below 9.25 r.)
static int spmv_row_bound() {
    zk_column_peak() = 0;
    const long before = zk_column_overflows();
    u32 ones[8];
    for (int i = 0; i < 8; i++) ones[i] = 0xffffffffu;
    double peak = 0;
    bool right = true;
    // row 0: the two words themselves; then rows of words just below them, whose products' reduction parts differ
    for (int row = 0; row < 2048; row++) {
        u32 ww[8];
        for (int i = 0; i < 8; i++) ww[i] = ones[i];
        Fr29 v = fr_extreme(1);
        if (row) {
            ww[0] -= (u32)(rng() & 0xffffff);
            v.l[0] -= (int32_t)(rng() & 0xffffff);          // r - 1 - k, k < 2^24 < the low limb of r
        }
        const Fr29 w = Fr29::from_words(ww);
        U256 uw{{((uint64_t)ww[1] << 32) | ww[0], ~0ull, ~0ull, ~0ull}};
        while (u_ge(uw, R64)) uw = u_sub_raw(uw, R64);
        Fr29 sum = Fr29::zero();
        uint32_t pending = 0;
        U256 want{{0, 0, 0, 0}};
        for (int k = 0; k < 64; k++) {
            sum = Fr29::add(sum, Fr29::mul(w, v));
            want = u_add(want, K(uw, u_of(v)));
            const double s = in_units_of_r(sum);
            if ((s < 0 ? -s : s) > peak) peak = s < 0 ? -s : s;
            if (++pending == 8) {
                sum = Fr29::reduce_near_zero(sum);
                pending = 0;
            }
        }
        right = right && u_eq(u_of(Fr29::reduce_near_zero(sum)), want);
    }
    const long over = zk_column_overflows() - before;
    printf("spmv_row, 8 products between reductions: largest |running sum| / r = %.3f (operand range 16), value %s, overflows %ld\n", peak,
           right ? "right" : "WRONG", over);
    return !right || over || peak >= 16.0;
}

static int plonk_blocks() {
    u_init();
    // the reference arithmetic against known words: K(2^261, 2^261) = 2^261, and one product of field29.hpp
    const U256 one = u_from_limbs(Fr29Params::ONE);
    const Fr29 a = random_canonical<Fr29>(), b = random_canonical<Fr29>();
    if (!u_eq(K(one, one), one) || !u_eq(u_of(Fr29::mul(a, b)), K(u_of(a), u_of(b)))) {
        printf("FAIL: the 64-bit reference arithmetic disagrees with itself\n");
        return 1;
    }
    int bad = plonk_quotient_points<PLONK_MUTANT>();
    bad |= plonk_coset_products<PLONK_MUTANT>();
    return bad;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "plonk") {          // the PLONK blocks alone (builds with -DPLONK_MUTANT=K)
        const int bad = plonk_blocks();
        printf(bad ? "FAIL: PLONK blocks (change %d)\n" : "OK: PLONK blocks (change %d)\n", PLONK_MUTANT);
        return bad;
    }
    if (families()) return 1;
    zk_column_peak() = 0;
    job_shapes<Fq29>("Fq", true);
    const long fq_over = zk_column_overflows();
    zk_column_peak() = 0;
    job_shapes<Fr29>("Fr", false);
    zk_column_peak() = 0;
    // chains of mixed additions over random field elements (no curve equation needed for bounds: the formulas see the same ranges)
    XYZZ<Fq29> acc = XYZZ<Fq29>::inf();
    for (int i = 0; i < 20000; i++) {
        Affine<Fq29> p{random_canonical<Fq29>(), random_canonical<Fq29>()};
        if (i & 1) negate_y(p);
        madd(acc, p);
    }
    XYZZ<Fq2r> acc2 = XYZZ<Fq2r>::inf();
    for (int i = 0; i < 10000; i++) {
        Affine<Fq2r> p{Fq2r{random_canonical<Fq29>(), random_canonical<Fq29>()}, Fq2r{random_canonical<Fq29>(), random_canonical<Fq29>()}};
        if (i & 1) negate_y(p);
        madd(acc2, p);
    }
    printf("G1 / G2 mixed-addition chains: peak |column| = %.3f * 2^58, overflows %ld\n", (double)zk_column_peak() / 288230376151711744.0,
           zk_column_overflows());
    (void)fq_over;
    if (g2_chains(tmax_fq())) return 1;
    if (plonk_blocks()) {
        printf("FAIL: the PLONK quotient or coset products\n");
        return 1;
    }
    if (spmv_row_bound()) {
        printf("FAIL: spmv_row's running sum\n");
        return 1;
    }
    if (zk_column_overflows()) {
        printf("FAIL: %ld column overflows\n", zk_column_overflows());
        return 1;
    }
    printf("OK: no column left int64\n");
    return 0;
}
