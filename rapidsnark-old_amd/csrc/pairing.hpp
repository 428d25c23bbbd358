// The optimal ate pairing on BN254 over field.hpp's Fq and curve.hpp's Fp2T: the tower, the line steps, the Miller loop
// pieces and the final exponentiation, as host + device functions (pairing.hip runs them one lane per job; a host build
// of the same text is what the arithmetic was first checked with).  Nothing in the reference corresponds to it.
//
// Construction (the textbook one, the same as the test oracle's so that the 12 coefficients compare one by one):
//   Fq2 = Fq[u]/(u^2 + 1);  Fq6 = Fq2[v]/(v^3 - xi), xi = 9 + u;  Fq12 = Fq6[w]/(w^2 - v), so w^6 = xi and an element is
//   sum c_ij v^j w^i = sum over k = 2j + i of c_k w^k.
//   G2 is on the D-type sextic twist E': y^2 = x^3 + 3/xi, untwisted by (x', y') -> (x' w^2, y' w^3).
//   A line through points of E' evaluated at P = (xP, yP) of G1 is  s yP + (t xP) w + c w^3  with s, t, c in Fq2: the three
//   non-zero coefficients sit at w^0, w^1 and w^3 = v w.
//
// What differs from the slow textbook route, and why the value is the same: the running point T is homogeneous projective
// (x = X/Z, y = Y/Z), so a step has no inversion and its line comes out multiplied by a non-zero element of Fq2 (2 y Z^3
// for a tangent, (x_Q Z - X) for a chord).  Every element of Fq2* has order dividing q^2 - 1, which divides the easy part
// q^6 - 1 of the final exponentiation: the factor becomes 1.  The hard part (q^4 - q^2 + 1)/r is computed EXACTLY (not a
// multiple of it, which some faster chains use and which would give another element of GT): with f already in the
// cyclotomic subgroup, where 1/f = conj(f),
//   f^((q^4 - q^2 + 1)/r) = f^(q^3) f^((6x^2 + 1) q^2) f^((-36x^3 - 18x^2 - 12x + 1) q) f^(-36x^3 - 30x^2 - 18x - 2)
// by three powers f^x, f^(x^2), f^(x^3) and the vectorial addition chain of Scott, Benger, Charlemagne, Dominguez Perez
// and Kachisa ("On the final exponentiation for calculating pairings on ordinary elliptic curves", 2009).
//
// Special cases of the steps.  Q has order r (pairing.hip checks it before any loop) and is not infinity, and the loop
// holds T = k Q with 1 < k < r at every chord (k runs over the prefixes of 6x + 2 < r), so T != +-Q: no chord degenerates
// into a tangent or a vertical.  The two Frobenius chords add pi(Q) = [q] Q and -pi^2(Q) = [-q^2] Q to [6x + 2] Q and to
// [6x + 2 + q] Q: 6x + 2 = +-q and 6x + 2 + q = +-q^2 (mod r) are false for this x.  A tangent needs Y != 0: a point with
// y = 0 has order 2, and r is odd.  So the steps carry no branches; the G1 side has none to begin with (P enters only as
// two multipliers).
//
// Call structure.  One Fq product is ~400 instructions inlined, an Fq12 product 54 of them; inlining the tower would make
// kernels of several hundred thousand instructions.  The Fq6 products, the steps and the larger operations are therefore
// real functions (ZK_NI) that take references, with the Fq2 products inlined into them: on the device their operands
// live in the lane's private memory (scratch), 192 B read per ~7000 instructions of arithmetic in an Fq6 product.
// DESIGN.md section 17 states the cost.
#pragma once
#include "curve.hpp"

#if defined(__HIPCC__)
#define ZK_NI inline __host__ __device__ __noinline__
#else
#define ZK_NI inline
#endif

namespace zk {

struct Fq6 {
    Fq2 c0, c1, c2;
};
struct Fq12 {
    Fq6 c0, c1;
};
struct G2Proj {
    Fq2 x, y, z;
};
// s yP + (t xP) w + c w^3
struct Line {
    Fq2 s, t, c;
};

// The constants of the pairing, made by pair_consts_init() (nothing here is typed in): gamma1[k-1] = xi^(k (q-1)/6),
// gamma2[k-1] = xi^(k (q^2-1)/6) (in Fq), the twist's b' = 3/xi and 3 b'.
struct PairConsts {
    Fq2 gamma1[5];
    Fq gamma2[5];
    Fq2 bt, bt3;
};

constexpr u64 BN_X = 4965661367192848881ull;
constexpr u64 ATE_LOW = 6 * BN_X + 2;                 // 6x + 2 = 2^64 + ATE_LOW: 65 bits, the top one implicit
static_assert(6 * (unsigned __int128)BN_X + 2 == ((unsigned __int128)1 << 64) + ATE_LOW && (BN_X >> 62) == 1, "6x + 2 = 2^64 + ATE_LOW, x has 63 bits");

// ---------------------------------------------------------------- Fq, Fq2
ZK_NI void fq_mul(Fq &r, const Fq &a, const Fq &b) { r = Fq::mul(a, b); }
// inlined into their callers: the Fq6 products, the steps and the Frobenius maps are the leaf functions (as called functions
// of their own the two were 13 % slower in k_verify_miller and 15 % in k_verify_final, at half the code size)
ZK_HD void f2_mul(Fq2 &r, const Fq2 &a, const Fq2 &b) { r = Fq2::mul(a, b); }
ZK_HD void f2_sqr(Fq2 &r, const Fq2 &a) { r = Fq2::sqr(a); }
ZK_HD void f2_mul_fq(Fq2 &r, const Fq2 &a, const Fq &k) {
    fq_mul(r.a, a.a, k);
    fq_mul(r.b, a.b, k);
}
ZK_HD Fq2 f2_conj(const Fq2 &a) { return Fq2{a.a, Fq::neg(a.b)}; }
ZK_HD Fq2 f2_mul_xi(const Fq2 &a) {                   // (a0 + a1 u)(9 + u) = (9 a0 - a1) + (9 a1 + a0) u
    const Fq2 a8 = Fq2::dbl(Fq2::dbl(Fq2::dbl(a)));
    return Fq2{Fq::sub(Fq::add(a8.a, a.a), a.b), Fq::add(Fq::add(a8.b, a.b), a.a)};
}
ZK_NI void f2_inv(Fq2 &r, const Fq2 &a) {
    Fq n, d;
    fq_mul(n, a.a, a.a);
    fq_mul(d, a.b, a.b);
    n = Fq::add(n, d);
    d = Fq::one();                                    // n^(q-2), square and multiply from the top bit
    u32 e[8];
    for (int i = 0; i < 8; i++) e[i] = FqParams::P[i];
    e[0] -= 2;
    for (int i = 255; i >= 0; i--) {
        fq_mul(d, d, d);
        if ((e[i >> 5] >> (i & 31)) & 1u) fq_mul(d, d, n);
    }
    fq_mul(r.a, a.a, d);
    fq_mul(r.b, a.b, d);
    r.b = Fq::neg(r.b);
}

// ---------------------------------------------------------------- Fq6
ZK_HD void f6_add(Fq6 &r, const Fq6 &a, const Fq6 &b) {
    r.c0 = Fq2::add(a.c0, b.c0);
    r.c1 = Fq2::add(a.c1, b.c1);
    r.c2 = Fq2::add(a.c2, b.c2);
}
ZK_HD void f6_sub(Fq6 &r, const Fq6 &a, const Fq6 &b) {
    r.c0 = Fq2::sub(a.c0, b.c0);
    r.c1 = Fq2::sub(a.c1, b.c1);
    r.c2 = Fq2::sub(a.c2, b.c2);
}
ZK_HD void f6_neg(Fq6 &r, const Fq6 &a) {
    r.c0 = Fq2::neg(a.c0);
    r.c1 = Fq2::neg(a.c1);
    r.c2 = Fq2::neg(a.c2);
}
ZK_HD void f6_mul_v(Fq6 &r, const Fq6 &a) {           // a v = (xi a2, a0, a1)
    const Fq2 t = f2_mul_xi(a.c2);
    r.c2 = a.c1;
    r.c1 = a.c0;
    r.c0 = t;
}
ZK_NI void f6_mul(Fq6 &r, const Fq6 &a, const Fq6 &b) {   // Karatsuba: 6 Fq2 products
    Fq2 t0, t1, t2, s, c0, c1, c2;
    f2_mul(t0, a.c0, b.c0);
    f2_mul(t1, a.c1, b.c1);
    f2_mul(t2, a.c2, b.c2);
    f2_mul(s, Fq2::add(a.c1, a.c2), Fq2::add(b.c1, b.c2));
    c0 = Fq2::add(t0, f2_mul_xi(Fq2::sub(Fq2::sub(s, t1), t2)));
    f2_mul(s, Fq2::add(a.c0, a.c1), Fq2::add(b.c0, b.c1));
    c1 = Fq2::add(Fq2::sub(Fq2::sub(s, t0), t1), f2_mul_xi(t2));
    f2_mul(s, Fq2::add(a.c0, a.c2), Fq2::add(b.c0, b.c2));
    c2 = Fq2::add(Fq2::sub(Fq2::sub(s, t0), t2), t1);
    r.c0 = c0;
    r.c1 = c1;
    r.c2 = c2;
}
// a (b0 + b1 v): 5 Fq2 products
ZK_NI void f6_mul_01(Fq6 &r, const Fq6 &a, const Fq2 &b0, const Fq2 &b1) {
    Fq2 t0, t1, s, c0, c1, c2;
    f2_mul(t0, a.c0, b0);
    f2_mul(t1, a.c1, b1);
    f2_mul(s, Fq2::add(a.c1, a.c2), b1);
    c0 = Fq2::add(t0, f2_mul_xi(Fq2::sub(s, t1)));    // a0 b0 + xi a2 b1
    f2_mul(s, Fq2::add(a.c0, a.c1), Fq2::add(b0, b1));
    c1 = Fq2::sub(Fq2::sub(s, t0), t1);               // a0 b1 + a1 b0
    f2_mul(s, Fq2::add(a.c0, a.c2), b0);
    c2 = Fq2::add(Fq2::sub(s, t0), t1);               // a2 b0 + a1 b1
    r.c0 = c0;
    r.c1 = c1;
    r.c2 = c2;
}
ZK_NI void f6_mul_f2(Fq6 &r, const Fq6 &a, const Fq2 &k) {
    f2_mul(r.c0, a.c0, k);
    f2_mul(r.c1, a.c1, k);
    f2_mul(r.c2, a.c2, k);
}
ZK_NI void f6_inv(Fq6 &r, const Fq6 &a) {
    Fq2 t0, t1, t2, s, d;
    f2_sqr(t0, a.c0);
    f2_mul(s, a.c1, a.c2);
    t0 = Fq2::sub(t0, f2_mul_xi(s));
    f2_sqr(t1, a.c2);
    f2_mul(s, a.c0, a.c1);
    t1 = Fq2::sub(f2_mul_xi(t1), s);
    f2_sqr(t2, a.c1);
    f2_mul(s, a.c0, a.c2);
    t2 = Fq2::sub(t2, s);
    f2_mul(d, a.c2, t1);
    f2_mul(s, a.c1, t2);
    d = f2_mul_xi(Fq2::add(d, s));
    f2_mul(s, a.c0, t0);
    d = Fq2::add(d, s);
    f2_inv(d, d);
    f2_mul(r.c0, t0, d);
    f2_mul(r.c1, t1, d);
    f2_mul(r.c2, t2, d);
}

// ---------------------------------------------------------------- Fq12
ZK_HD void f12_one(Fq12 &r) {
    r.c0.c0 = Fq2::one();
    r.c0.c1 = r.c0.c2 = r.c1.c0 = r.c1.c1 = r.c1.c2 = Fq2::zero();
}
ZK_HD bool f12_is_one(const Fq12 &a) {
    return a.c0.c0 == Fq2::one() && a.c0.c1.is_zero() && a.c0.c2.is_zero() && a.c1.c0.is_zero() && a.c1.c1.is_zero() && a.c1.c2.is_zero();
}
ZK_NI void f12_mul(Fq12 &r, const Fq12 &a, const Fq12 &b) {   // 3 Fq6 products
    Fq6 t0, t1, sa, sb;
    f6_mul(t0, a.c0, b.c0);
    f6_mul(t1, a.c1, b.c1);
    f6_add(sa, a.c0, a.c1);
    f6_add(sb, b.c0, b.c1);
    f6_mul(sa, sa, sb);
    f6_sub(sa, sa, t0);
    f6_sub(r.c1, sa, t1);
    f6_mul_v(t1, t1);
    f6_add(r.c0, t0, t1);
}
ZK_NI void f12_sqr(Fq12 &r, const Fq12 &a) {          // (a0 + a1 w)^2 = (a0 + a1)(a0 + v a1) - t - v t + 2 t w, t = a0 a1
    Fq6 t, s0, s1;
    f6_mul(t, a.c0, a.c1);
    f6_add(s0, a.c0, a.c1);
    f6_mul_v(s1, a.c1);
    f6_add(s1, s1, a.c0);
    f6_mul(s0, s0, s1);
    f6_sub(s0, s0, t);
    f6_add(r.c1, t, t);
    f6_mul_v(t, t);
    f6_sub(r.c0, s0, t);
}
ZK_HD void f12_conj(Fq12 &r, const Fq12 &a) {         // a^(q^6)
    r.c0 = a.c0;
    f6_neg(r.c1, a.c1);
}
ZK_NI void f12_inv(Fq12 &r, const Fq12 &a) {
    Fq6 t0, t1;
    f6_mul(t0, a.c0, a.c0);
    f6_mul(t1, a.c1, a.c1);
    f6_mul_v(t1, t1);
    f6_sub(t0, t0, t1);
    f6_inv(t0, t0);
    f6_mul(r.c0, a.c0, t0);
    f6_mul(t1, a.c1, t0);
    f6_neg(r.c1, t1);
}
// a^q: the coefficient of w^k is conjugated and multiplied by gamma1[k-1] = (w^k)^(q-1)
ZK_NI void f12_frob(Fq12 &r, const Fq12 &a, const PairConsts &k) {
    r.c0.c0 = f2_conj(a.c0.c0);
    f2_mul(r.c1.c0, f2_conj(a.c1.c0), k.gamma1[0]);   // w
    f2_mul(r.c0.c1, f2_conj(a.c0.c1), k.gamma1[1]);   // v = w^2
    f2_mul(r.c1.c1, f2_conj(a.c1.c1), k.gamma1[2]);   // v w = w^3
    f2_mul(r.c0.c2, f2_conj(a.c0.c2), k.gamma1[3]);   // v^2 = w^4
    f2_mul(r.c1.c2, f2_conj(a.c1.c2), k.gamma1[4]);   // v^2 w = w^5
}
// a^(q^2): no conjugation, the multipliers are in Fq
ZK_NI void f12_frob2(Fq12 &r, const Fq12 &a, const PairConsts &k) {
    r.c0.c0 = a.c0.c0;
    f2_mul_fq(r.c1.c0, a.c1.c0, k.gamma2[0]);
    f2_mul_fq(r.c0.c1, a.c0.c1, k.gamma2[1]);
    f2_mul_fq(r.c1.c1, a.c1.c1, k.gamma2[2]);
    f2_mul_fq(r.c0.c2, a.c0.c2, k.gamma2[3]);
    f2_mul_fq(r.c1.c2, a.c1.c2, k.gamma2[4]);
}
// f <- f (a + b w + c w^3), the line's three coefficients: 13 Fq2 products
ZK_NI void f12_mul_line(Fq12 &f, const Fq2 &a, const Fq2 &b, const Fq2 &c) {
    Fq6 t0, t1, s;
    f6_mul_f2(t0, f.c0, a);                           // f0 (a, 0, 0)
    f6_mul_01(t1, f.c1, b, c);                        // f1 (b, c, 0)
    f6_add(s, f.c0, f.c1);
    f6_mul_01(s, s, Fq2::add(a, b), c);
    f6_sub(s, s, t0);
    f6_sub(f.c1, s, t1);
    f6_mul_v(t1, t1);
    f6_add(f.c0, t0, t1);
}
// the line evaluated at P, multiplied into f
ZK_HD void f12_mul_line_at(Fq12 &f, const Line &l, const G1Affine &P) {
    Fq2 a, b;
    f2_mul_fq(a, l.s, P.y);
    f2_mul_fq(b, l.t, P.x);
    f12_mul_line(f, a, b, l.c);
}

// ---------------------------------------------------------------- the steps on the twist
// T <- 2T and the tangent at T times 2 y Z^3 (a = 0 doubling of Costello, Lange, Naehrig 2010, scaled by 4 to avoid 1/2):
// s = 2YZ, t = -3X^2, c = Y^2 - 3b'Z^2
ZK_NI void step_dbl(G2Proj &T, Line &l, const PairConsts &k) {
    Fq2 B, C, E, F, H, XY, X2, t;
    f2_sqr(B, T.y);
    f2_sqr(C, T.z);
    f2_mul(E, C, k.bt3);
    F = Fq2::add(Fq2::dbl(E), E);
    f2_sqr(H, Fq2::add(T.y, T.z));
    H = Fq2::sub(H, Fq2::add(B, C));                  // 2YZ
    f2_mul(XY, T.x, T.y);
    f2_sqr(X2, T.x);
    l.s = H;
    l.t = Fq2::neg(Fq2::add(Fq2::dbl(X2), X2));
    l.c = Fq2::sub(B, E);
    f2_mul(T.x, Fq2::dbl(XY), Fq2::sub(B, F));        // 2XY (B - F)
    f2_sqr(t, Fq2::add(B, F));
    f2_sqr(E, E);
    E = Fq2::dbl(Fq2::dbl(Fq2::add(Fq2::dbl(E), E))); // 12 E^2
    T.y = Fq2::sub(t, E);
    f2_mul(t, B, H);
    T.z = Fq2::dbl(Fq2::dbl(t));                      // 4 B H
}
// T <- T + Q (Q affine, T != +-Q: see the head of the file) and the chord times (X - xQ Z): with theta = Y - yQ Z,
// lambda = X - xQ Z:  s = lambda, t = -theta, c = theta xQ - lambda yQ
ZK_NI void step_add(G2Proj &T, Line &l, const G2Affine &Q) {
    Fq2 th, la, C, D, E, F, G, H, t;
    f2_mul(t, Q.y, T.z);
    th = Fq2::sub(T.y, t);
    f2_mul(t, Q.x, T.z);
    la = Fq2::sub(T.x, t);
    f2_sqr(C, th);
    f2_sqr(D, la);
    f2_mul(E, la, D);
    f2_mul(F, T.z, C);
    f2_mul(G, T.x, D);
    H = Fq2::sub(Fq2::add(E, F), Fq2::dbl(G));
    f2_mul(T.x, la, H);
    f2_mul(t, th, Fq2::sub(G, H));
    f2_mul(G, E, T.y);
    T.y = Fq2::sub(t, G);
    f2_mul(T.z, T.z, E);
    l.s = la;
    l.t = Fq2::neg(th);
    f2_mul(t, th, Q.x);
    f2_mul(G, la, Q.y);
    l.c = Fq2::sub(t, G);
}
// pi(Q) and -pi^2(Q) on the twist
ZK_NI void frob_twist(G2Affine &q1, G2Affine &q2neg, const G2Affine &Q, const PairConsts &k) {
    f2_mul(q1.x, f2_conj(Q.x), k.gamma1[1]);          // xi^((q-1)/3)
    f2_mul(q1.y, f2_conj(Q.y), k.gamma1[2]);          // xi^((q-1)/2)
    f2_mul_fq(q2neg.x, Q.x, k.gamma2[1]);
    f2_mul_fq(q2neg.y, Q.y, k.gamma2[2]);
    q2neg.y = Fq2::neg(q2neg.y);
}
// The loop's schedule, the same for every Q: step i < 64 is a doubling, followed by a chord with Q when bit 63 - i of
// ATE_LOW is set; then the chords with pi(Q) and -pi^2(Q).  MILLER_LINES counts the lines.
constexpr int popcount64(u64 v) { return v ? (int)(v & 1) + popcount64(v >> 1) : 0; }
constexpr int MILLER_LINES = 64 + popcount64(ATE_LOW) + 2;
ZK_HD bool ate_bit(int i) { return (ATE_LOW >> (63 - i)) & 1; }

// out[i], i < MILLER_LINES: line i of the loop over q in that schedule, to be evaluated at any P (f12_mul_line_at)
ZK_NI void line_table(Line *out, const G2Affine &q, const PairConsts &k) {
    G2Proj T{q.x, q.y, Fq2::one()};
    Line l;
    int at = 0;
    for (int i = 0; i < 64; i++) {
        step_dbl(T, l, k);
        out[at++] = l;
        if (ate_bit(i)) {
            step_add(T, l, q);
            out[at++] = l;
        }
    }
    G2Affine q1, q2;
    frob_twist(q1, q2, q, k);
    step_add(T, l, q1);
    out[at++] = l;
    step_add(T, l, q2);
    out[at++] = l;
}

// ---------------------------------------------------------------- the final exponentiation
ZK_NI void f12_pow_x(Fq12 &r, const Fq12 &a) {        // a^x, x = BN_X (63 bits), square and multiply from the top
    Fq12 t = a;
    for (int i = 61; i >= 0; i--) {
        f12_sqr(t, t);
        if ((BN_X >> i) & 1) f12_mul(t, t, a);
    }
    r = t;
}
ZK_NI void final_exp(Fq12 &r, const Fq12 &f_in, const PairConsts &k) {
    Fq12 f, t0, t1, fx, fx2, fx3, y0, y2, y3, y4, y6;
    // easy part: f^((q^6 - 1)(q^2 + 1))
    f12_inv(t0, f_in);
    f12_conj(t1, f_in);
    f12_mul(t0, t1, t0);
    f12_frob2(t1, t0, k);
    f12_mul(f, t1, t0);
    // hard part.  y0 = f^q f^(q^2) f^(q^3), y1 = 1/f, y2 = (f^(x^2))^(q^2), y3 = 1/(f^x)^q, y4 = 1/(f^x (f^(x^2))^q),
    // y5 = 1/f^(x^2), y6 = 1/(f^(x^3) (f^(x^3))^q);  result = y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36
    f12_pow_x(fx, f);
    f12_pow_x(fx2, fx);
    f12_pow_x(fx3, fx2);
    f12_frob(t0, f, k);
    f12_frob2(t1, f, k);
    f12_mul(y0, t0, t1);
    f12_frob(t0, t1, k);
    f12_mul(y0, y0, t0);
    f12_frob2(y2, fx2, k);
    f12_frob(t0, fx, k);
    f12_conj(y3, t0);
    f12_frob(t0, fx2, k);
    f12_mul(t0, t0, fx);
    f12_conj(y4, t0);
    f12_frob(t0, fx3, k);
    f12_mul(t0, t0, fx3);
    f12_conj(y6, t0);
    f12_conj(fx2, fx2);                               // y5
    f12_conj(fx, f);                                  // y1
    f12_sqr(t0, y6);
    f12_mul(t0, t0, y4);
    f12_mul(t0, t0, fx2);                             // y6^2 y4 y5
    f12_mul(t1, y3, fx2);
    f12_mul(t1, t1, t0);                              // y3 y5 t0
    f12_mul(t0, t0, y2);
    f12_sqr(t1, t1);
    f12_mul(t1, t1, t0);
    f12_sqr(t1, t1);
    f12_mul(t0, t1, fx);                              // . y1
    f12_mul(t1, t1, y0);
    f12_sqr(t0, t0);
    f12_mul(r, t0, t1);
}

// ---------------------------------------------------------------- the constants
ZK_NI void pair_consts_init(PairConsts &k) {
    Fq2 xi, three, g, t;
    Fq nine = Fq::one();
    for (int i = 0; i < 3; i++) nine = Fq::dbl(nine);
    nine = Fq::add(nine, Fq::one());
    xi = Fq2{nine, Fq::one()};
    three = Fq2{Fq::add(Fq::dbl(Fq::one()), Fq::one()), Fq::zero()};
    f2_inv(t, xi);
    f2_mul(k.bt, t, three);
    k.bt3 = Fq2::add(Fq2::dbl(k.bt), k.bt);
    u32 e[8];                                         // (q - 1) / 6
    u64 rem = 0;
    for (int i = 7; i >= 0; i--) {
        const u64 cur = (rem << 32) | (FqParams::P[i] - (i == 0 ? 1u : 0u));
        e[i] = (u32)(cur / 6);
        rem = cur % 6;
    }
    g = Fq2::one();
    for (int i = 255; i >= 0; i--) {
        f2_sqr(g, g);
        if ((e[i >> 5] >> (i & 31)) & 1u) f2_mul(g, g, xi);
    }
    k.gamma1[0] = g;
    for (int i = 1; i < 5; i++) f2_mul(k.gamma1[i], k.gamma1[i - 1], g);
    for (int i = 0; i < 5; i++) {                     // xi^(k (q^2-1)/6) = gamma1 gamma1^q: the norm, in Fq
        f2_mul(t, k.gamma1[i], f2_conj(k.gamma1[i]));
        k.gamma2[i] = t.a;
    }
}

}   // namespace zk
