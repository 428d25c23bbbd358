// Column-overflow check of field29.hpp's Montgomery products (host build, g++ -DZK_CHECK_COLUMNS).
// Every v_mad_i64_i32 of the kernels is `acc + a*b` in ONE signed 64-bit register; with the lower eight reduction digits
// unmasked the budget is 18 * 2^58 of operand terms (field29.hpp).  Here each MAD is evaluated in 128 bits and a column that
// leaves int64 is counted.  Shapes covered — every job the kernels run, with the limb ranges their callers produce:
//   JMul tight x tight, JMul tight x wide (one lazily added / doubled operand: DIT butterflies, f2_sqr), JSqr of a tight value,
//   JMulAdd2 of four tight operands, JMulAdd4 with two products of each sign (G2 lane pair's Y3), in Fq and (but JMulAdd4) Fr;
//   plus chains of G1 and G2 mixed additions (curve29.hpp) over random operands, which exercise sub_nc / neg_lazy / dbl_lazy as used;
//   plus the butterfly schedules of nttpair.hip (lazy DIT adds, DIF settle) over the extreme-operand families of
//   tests/extreme_inputs.py — the element whose limbs are all 2^29 - 1 in every register, r - 1, masks, strides — with the
//   all-sums element of a constant vector checked for its VALUE (2^11 v after a tile), and G1 additions with X on full limbs.
// Prints the peak |column| as a multiple of 2^58 and exits 1 on any overflow or wrong all-sums value.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
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

int main() {
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
    if (zk_column_overflows()) {
        printf("FAIL: %ld column overflows\n", zk_column_overflows());
        return 1;
    }
    printf("OK: no column left int64\n");
    return 0;
}
