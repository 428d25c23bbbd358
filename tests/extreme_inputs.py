"""Input families that sit at the edges of the nine-limb (9 x 29 bit) arithmetic of csrc/field29.hpp, for operators that the
suite otherwise feeds uniformly random data ("Extreme-operand inputs").  A plain helper module: nothing here needs
a GPU, tests/test_extreme_operands_host.py checks that every family is what it claims to be.

The operators take x * 2^256 bytes and convert with ONE Montgomery product by 2^266 (Fp29::from_mont256), so the value the
kernels hold is bytes * 2^5 mod p.  A word that must become T inside the kernel is therefore T * 32^-1 mod p.  That product
leaves (bytes * K_IN + M p) / 2^261 with 0 <= bytes, K_IN < p and M within 2^235 of [0, 2^261): a representative of T in
(-p / 2^20, p + p / 160).  For p - p / 160 > T > p / 160 the representative is T itself, limb for limb (internal_limbs()).

The coset entries of csrc/plonkquot.hip do NOT convert that way: see held / held_families below.

G1 points (extreme_g1) are in the group whatever their coordinates; G2 points with a chosen coordinate (extreme_g2, half_zero_g2)
are on the twist but outside its order-r subgroup: see the section comment there for what may receive them.
"""
import functools

import numpy as np

from oracle import bn254 as bn
from oracle import c_oracle as co

R, Q = bn.R_MOD, bn.Q_MOD
LIMB_BITS, LIMB_MASK = 29, (1 << 29) - 1
TOP_LIMB = 3171406                                   # limb 8 of both BN254 primes
T_MAX = TOP_LIMB * (1 << 232) - 1                    # limbs 0..7 = 2^29 - 1, limb 8 = 3171405
TILE_BITS = 11                                       # m: the bits one tile of csrc/nttpair.hip transforms


def limbs29(v):
    """The nine 29-bit limbs of a non-negative integer below 2^261."""
    assert 0 <= v < 1 << 261
    return [(v >> (LIMB_BITS * i)) & LIMB_MASK for i in range(9)]


for _p in (R, Q):
    assert limbs29(_p)[8] == TOP_LIMB and any(limbs29(_p)[:8])
assert T_MAX < R and T_MAX < Q
assert limbs29(T_MAX) == [LIMB_MASK] * 8 + [TOP_LIMB - 1]


def word_for_internal(t, p):
    """The canonical 256-bit value whose bytes the kernels turn into t (mod p): t * 32^-1."""
    return t * pow(32, -1, p) % p


def internal_value(word, p):
    """What a kernel holds after converting `word`: bytes * 2^5 mod p."""
    return word * 32 % p


def internal_limbs(word, p):
    """The limbs Fp29::from_mont256 leaves for `word`: the product by K_IN = 2^266 mod p with the exact Montgomery quotient
    (the device's quotient differs from it by a multiple of 2^261 only within 2^-26 of the ends of its range)."""
    k_in = (1 << 266) % p
    m = (-word * k_in * pow(p, -1, 1 << 261)) % (1 << 261)
    v, rem = divmod(word * k_in + m * p, 1 << 261)
    assert rem == 0 and v % p == internal_value(word, p)
    return limbs29(v)


T_MAX_WORD_FR = word_for_internal(T_MAX, R)
T_MAX_WORD_FQ = word_for_internal(T_MAX, Q)
assert internal_value(T_MAX_WORD_FR, R) == T_MAX and internal_value(T_MAX_WORD_FQ, Q) == T_MAX
assert internal_limbs(T_MAX_WORD_FR, R) == limbs29(T_MAX) and internal_limbs(T_MAX_WORD_FQ, Q) == limbs29(T_MAX)


# ---------------------------------------------------------------------------------------------------------------- Fr vectors
def word_bytes(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)


def constant(n, v):
    return np.tile(word_bytes(v), n)


def all_top(n):
    """Every word r - 1."""
    return constant(n, R - 1)


def all_ones_limbs(n):
    """Every word the one whose internal value is T_MAX: eight limbs of 2^29 - 1 under the largest top limb below r's."""
    return constant(n, T_MAX_WORD_FR)


def mask01(n, seed):
    """Each word 0 or r - 1, chosen by a seeded bit."""
    bits = np.random.default_rng(seed).integers(0, 2, size=n, dtype=np.uint8).astype(bool)
    out = np.zeros((n, 32), dtype=np.uint8)
    out[bits] = word_bytes(R - 1)
    return out.reshape(-1)


def alternating(n):
    """r - 1, 1, r - 1, 1, ..."""
    out = np.zeros((n, 32), dtype=np.uint8)
    out[0::2] = word_bytes(R - 1)
    out[1::2] = word_bytes(1)
    return out.reshape(-1)


def stride(n, s, v):
    """v where i mod 2^s == 0, else 0: every sub-transform along the zeroed bits sees a constant vector, so each of its
    butterflies adds equal values stage after stage."""
    out = np.zeros((n, 32), dtype=np.uint8)
    out[0::1 << s] = word_bytes(v)
    return out.reshape(-1)


def preimage(y):
    """ifft(y) by the C restatement: the forward transform on the device then ENDS at y, the inverse starts from it."""
    return np.frombuffer(co.fr_fft(y, inverse=True), dtype=np.uint8)


STRIDE_BITS = (1, 3, 6, TILE_BITS)
STRIDE_VALUES = (("top", R - 1), ("tmax", T_MAX_WORD_FR))


def fr_families(logn, preimages=True):
    """[(name, vector)] at n = 2^logn: every family, the strided ones at s in {1, 3, 6, 11} as far as the size has those bits
    and at s = m + 1 = 12 where the size has strided bits, each with v = r - 1 and v = the T_MAX word; then the preimage of
    each of them."""
    n = 1 << logn
    fams = [("all_top", all_top(n)), ("all_ones_limbs", all_ones_limbs(n)), ("mask01", mask01(n, 1000 + logn)), ("alternating", alternating(n))]
    for s in STRIDE_BITS + (TILE_BITS + 1,):
        if s <= logn:
            fams += [("stride(%d,%s)" % (s, vn), stride(n, s, v)) for vn, v in STRIDE_VALUES]
    if preimages:
        fams += [("preimage(%s)" % name, preimage(x)) for name, x in list(fams)]
    return fams


def big_size_inputs(logn):
    """The four inputs of the sizes whose pass plans do not exist below them (2^22, 2^23)."""
    n = 1 << logn
    return [("all_top", all_top(n)), ("all_ones_limbs", all_ones_limbs(n)), ("stride(11,top)", stride(n, TILE_BITS, R - 1)),
            ("stride(12,tmax)", stride(n, TILE_BITS + 1, T_MAX_WORD_FR))]


# ------------------------------------------------------------------------------------------ Fr rows for the coset transforms
# csrc/plonkquot.hip does not convert with from_mont256: k_coset_load turns a STANDARD row v_i into the canonical word of
# v_i g^i 2^261 mod r (one product with the lane's power, then Fr29::store), and that word is what the transform and the
# quotient kernel load.  Canonical: the limbs are those of the integer itself, for every target in [0, r).
INV_261 = pow(1 << 261, -1, R)


def held(t):
    """The standard value whose device word, after k_coset_load at row 0 (or with g = 1), has the limbs of t."""
    assert 0 <= t < R
    return t * INV_261 % R


def loaded_word(v, i=0, g=1):
    """What the kernels hold for the standard row v at index i on the coset of g: v g^i 2^261 mod r, canonical."""
    return v * pow(g, i, R) % R * (1 << 261) % R


@functools.lru_cache(maxsize=8)
def _inverse_powers(n, g):
    gi, x, out = pow(g, -1, R), 1, []
    for _ in range(n):
        out.append(x)
        x = x * gi % R
    return out


def held_rows(targets, g=1):
    """Standard rows v_i = T_i 2^-261 g^-i: row i is loaded as the word T_i on the coset of g.  A list of integers."""
    targets = list(targets)
    if g == 1:
        return [held(t) for t in targets]
    return [held(t) * p % R for t, p in zip(targets, _inverse_powers(len(targets), g))]


def _family_targets(logn):
    """[(name, targets)]: the words of the families above as TARGETS of the load, integers in [0, r)."""
    n = 1 << logn
    bits = np.random.default_rng(1000 + logn).integers(0, 2, size=n, dtype=np.uint8)
    fams = [("all_top", [R - 1] * n), ("all_ones_limbs", [T_MAX] * n), ("mask01", [(R - 1) * int(b) for b in bits]),
            ("alternating", [R - 1, 1] * (n // 2))]
    for s in STRIDE_BITS:
        if s <= logn:
            fams += [("stride(%d,%s)" % (s, vn), [v if i % (1 << s) == 0 else 0 for i in range(n)]) for vn, v in (("top", R - 1), ("tmax", T_MAX))]
    return fams


def held_families(logn, g=1):
    """[(name, rows)] at m = 2^logn, rows lists of standard integers: all_top, all_ones_limbs, mask01, alternating and
    stride(s, v) at STRIDE_BITS as words the transform LOADS on the coset of g (forward: the shift in use; inverse: g = 1,
    its load keeps no power).  The families above aim at x 32 through from_mont256; the coset entry does not pass through it."""
    return [(name, held_rows(t, g)) for name, t in _family_targets(logn)]


def coset_preimages(logn, g=1):
    """[(name, rows)]: for each family the standard rows whose FORWARD transform on the coset of g ends at it, the
    transform's last stage leaving the family's words: the C restatement's inverse transform of held(T), times g^-i."""
    out = []
    for name, t in _family_targets(logn):
        c = unpack(co.fr_fft(pack(held_rows(t)), inverse=True))
        out.append(("coset_preimage(%s)" % name, [v * p % R for v, p in zip(c, _inverse_powers(len(c), g))]))
    return out


@functools.lru_cache(maxsize=2)
def big_coset_inputs(logn, g=1):
    """The four inputs of big_size_inputs as loaded words, for one large size."""
    n = 1 << logn
    t = [("all_top", [R - 1] * n), ("all_ones_limbs", [T_MAX] * n), ("stride(11,top)", [R - 1 if i % (1 << TILE_BITS) == 0 else 0 for i in range(n)]),
         ("stride(12,tmax)", [T_MAX if i % (2 << TILE_BITS) == 0 else 0 for i in range(n)])]
    return [(name, held_rows(v, g)) for name, v in t]


def unpack(b):
    b = bytes(b) if not isinstance(b, np.ndarray) else b.tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def pack(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8)


# ----------------------------------------------------------------------------------------------------------------- G1 points
def _g1_targets():
    """Internal X coordinates aimed at, kind by kind: all eight low limbs 2^29 - 1 under a falling top limb; just below q
    (the largest canonical values); just above 0 (all limbs but the lowest empty)."""
    def full():
        j = TOP_LIMB
        while True:
            yield j * (1 << 232) - 1
            j -= 1

    def high():
        k = 1
        while True:
            yield Q - k
            k += 1

    def low():
        k = 1
        while True:
            yield k
            k += 1

    return (("full_limbs", full()), ("below_q", high()), ("above_zero", low()))


def extreme_g1(count=24):
    """[(kind, T, (x, y))]: for each kind the first targets T for which x = T * 2^-261 has x^3 + 3 a square, each with both
    roots — count / 3 points of each kind, negatives included.  G1 has cofactor 1: every point of the curve is in the group."""
    assert count % 6 == 0
    out = []
    inv261 = pow(1 << 261, -1, Q)
    for kind, targets in _g1_targets():
        found = 0
        for t in targets:
            assert 0 < t < Q
            x = t * inv261 % Q
            rhs = (x * x * x + 3) % Q
            y = pow(rhs, (Q + 1) // 4, Q)                # q = 3 mod 4
            if y * y % Q != rhs:
                continue
            for P in ((x, y), (x, Q - y)):
                assert bn.G1.is_on_curve(P)
                b = bn.g1_to_bytes(P)
                assert internal_value(int.from_bytes(b[:32], "little"), Q) == t
                out.append((kind, t, P))
            found += 2
            if found == count // 3:
                break
    return out


def extreme_g1_points(count=24):
    """The points of extreme_g1 in the affine Montgomery bytes the ABI takes, 64 each."""
    return [bn.g1_to_bytes(P) for _, _, P in extreme_g1(count)]


def mixed_scalars(n, seed=40):
    """0, 1, r - 1, r, 2^256 - 1, 2, r + 1, r - 2 and random 256-bit and sub-r values up to n: raw 256-bit integers, as the MSM takes."""
    import random
    rng = random.Random(seed)
    ks = [0, 1, R - 1, R, (1 << 256) - 1, 2, R + 1, R - 2]
    while len(ks) < n:
        ks.append(rng.randrange(R) if len(ks) % 4 else rng.randrange(R, 1 << 256))
    return ks[:n]


def scalars_bytes(ks):
    return np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in ks), dtype=np.uint8)


# ----------------------------------------------------------------------------------------------------------------- G2 points
# The twist y^2 = x^3 + b' over Fq2 has about q^2 points and r divides that count once: the cofactor is about q, and a point
# built from a chosen coordinate lies OUTSIDE the order-r subgroup (tests/test_extreme_operands_host.py checks [r]P != inf).
# The group law still holds for such points, but k P depends on k itself and not on k mod r: only operators that take the
# scalar as a plain integer may receive them, and only with scalars below r (g2_scalars_below_r).
def f2_pow(a, e):
    out = bn.F2_ONE
    for bit in bin(e)[2:]:
        out = bn.f2_mul(out, out)
        if bit == "1":
            out = bn.f2_mul(out, a)
    return out


def _fq_sqrt(a):
    s = pow(a, (Q + 1) // 4, Q)                          # q = 3 mod 4
    return s if s * s % Q == a % Q else None


def f2_sqrt(a):
    """A square root of a in Fq2 = Fq[u] / (u^2 + 1), or None for a non-square (the complex method: with n = sqrt(a0^2 + a1^2)
    a root is x0 + x1 u, x0^2 = (a0 + n) / 2 or (a0 - n) / 2, x1 = a1 / (2 x0))."""
    a0, a1 = a[0] % Q, a[1] % Q
    if a1 == 0:
        s = _fq_sqrt(a0)
        if s is not None:
            return (s, 0)
        return (0, _fq_sqrt(Q - a0))                     # -1 is a non-square: exactly one of a0, -a0 has a root
    n = _fq_sqrt((a0 * a0 + a1 * a1) % Q)
    if n is None:                                        # the norm of a square is a square
        return None
    half = (Q + 1) // 2
    x0 = _fq_sqrt((a0 + n) * half % Q)
    if x0 is None:
        x0 = _fq_sqrt((a0 - n) * half % Q)
    if x0 is None or x0 == 0:
        return None
    x = (x0, a1 * pow(2 * x0, -1, Q) % Q)
    return x if bn.f2_mul(x, x) == (a0, a1) else None


_F2_ORDER = Q * Q - 1
_CBRT = {}


def _cbrt_constants():
    """q^2 - 1 = 3^s m with 3 not dividing m, a generator z of the 3-Sylow subgroup of Fq2*, and the Bezout pair of 3^s and m."""
    if not _CBRT:
        s, m = 0, _F2_ORDER
        while m % 3 == 0:
            s, m = s + 1, m // 3
        assert s == 2                                    # v3(q^2 - 1) = 2
        g = next((i, 1) for i in range(1, 100) if f2_pow((i, 1), _F2_ORDER // 3) != bn.F2_ONE)      # a non-cube
        z = f2_pow(g, m)                                 # order exactly 3^s
        assert f2_pow(z, 3 ** (s - 1)) != bn.F2_ONE and f2_pow(z, 3 ** s) == bn.F2_ONE
        a = pow(3 ** s, -1, m)                           # a 3^s + b m = 1
        b = (1 - a * 3 ** s) // m
        _CBRT.update(s=s, m=m, z=z, a=a, b=b % 3 ** s, third=pow(3, -1, m))
    return _CBRT


def f2_cbrt(c):
    """A cube root of c in Fq2, or None for a non-cube: Tonelli-Shanks for exponent 3.  c = (c^(3^s))^a (c^m)^b splits c into a
    part of order prime to 3, whose cube root is a power of it, and a part in the 3-Sylow subgroup <z>, whose logarithm to the
    base z is found one base-3 digit at a time; c is a cube iff that logarithm is a multiple of 3."""
    c = (c[0] % Q, c[1] % Q)
    if c == bn.F2_ZERO:
        return c
    if f2_pow(c, _F2_ORDER // 3) != bn.F2_ONE:
        return None
    k = _cbrt_constants()
    s, m, z = k["s"], k["m"], k["z"]
    t = f2_pow(c, m)                                     # in <z>: t = z^e
    e, zinv = 0, f2_pow(z, 3 ** s - 1)
    w = f2_pow(z, 3 ** (s - 1))                          # order 3: the digit is read off against its powers
    for d in range(s):                                   # digit d of e
        probe = f2_pow(bn.f2_mul(t, f2_pow(zinv, e)), 3 ** (s - 1 - d))
        digit = next(j for j in range(3) if f2_pow(w, j) == probe)
        e += digit * 3 ** d
    assert f2_pow(z, e) == t and e % 3 == 0
    x = bn.f2_mul(f2_pow(f2_pow(c, 3 ** s), k["a"] * k["third"] % m), f2_pow(z, e // 3 * k["b"] % 3 ** s))
    assert f2_pow(x, 3) == c
    return x


def _twist_rhs(x):
    return bn.f2_add(bn.f2_mul(bn.f2_mul(x, x), x), bn.G2_B)


def _twist_points_at(x):
    """Both points of the twist over x, or () where x^3 + b' is no square (or zero)."""
    y = f2_sqrt(_twist_rhs(x))
    if y is None or y == bn.F2_ZERO:
        return ()
    pts = ((x, y), (x, bn.f2_neg(y)))
    assert all(bn.G2.is_on_curve(P) for P in pts)
    return pts


def g2_internal_x(P):
    """(Ta, Tb): what the kernels hold for the two components of P's x after converting its bytes."""
    b = bn.g2_to_bytes(P)
    return tuple(internal_value(int.from_bytes(b[32 * i:32 * i + 32], "little"), Q) for i in range(2))


# every pairing of the three G1 target kinds for (re x, im x); the two that come last get the smaller share of an uneven count
G2_KINDS = (("full_limbs", "full_limbs"), ("full_limbs", "below_q"), ("full_limbs", "above_zero"), ("below_q", "full_limbs"),
            ("above_zero", "full_limbs"), ("below_q", "above_zero"), ("above_zero", "below_q"), ("below_q", "below_q"),
            ("above_zero", "above_zero"))


def extreme_g2(count=32):
    """[(kind, (Ta, Tb), P)] with x = (Ta, Tb) * 2^-261: for each of the nine kinds (kind_a + "/" + kind_b) the first target pairs
    — the i-th target of kind_a beside the (i + 1)-th of kind_b, so the components differ within a kind — for which x^3 + b' is
    a square, each with both roots.  count / 2 target pairs are dealt round the kinds: 32 gives two pairs to the first seven
    kinds and one to the last two.  The points are on the twist and NOT in the order-r subgroup (see the section comment)."""
    assert count % 2 == 0 and count // 2 >= len(G2_KINDS)
    share = [(count // 2 - i + len(G2_KINDS) - 1) // len(G2_KINDS) for i in range(len(G2_KINDS))]
    inv261 = pow(1 << 261, -1, Q)
    out = []
    for (ka, kb), want in zip(G2_KINDS, share):
        gens = dict(_g1_targets())
        ga, gb = gens[ka], dict(_g1_targets())[kb]
        next(gb)
        found = tried = 0
        while found < want:
            ta, tb = next(ga), next(gb)
            tried += 1
            assert 0 < ta < Q and 0 < tb < Q and tried <= 10
            x = (ta * inv261 % Q, tb * inv261 % Q)
            for P in _twist_points_at(x):
                assert g2_internal_x(P) == (ta, tb)
                out.append((ka + "/" + kb, (ta, tb), P))
            found += bool(_twist_points_at(x))
    assert len(out) == count
    return out


def extreme_g2_points(count=32):
    """The points of extreme_g2 in the affine Montgomery bytes the ABI takes, 128 each."""
    return [bn.g2_to_bytes(P) for _, _, P in extreme_g2(count)]


def _fq_beta():
    """A primitive cube root of unity in Fq."""
    for g in range(2, 50):
        beta = pow(g, (Q - 1) // 3, Q)
        if beta != 1:
            assert beta * beta % Q * beta % Q == 1
            return beta


def half_zero_g2():
    """(pairs, points), all found by scanning small integers.
    pairs: [(shape, P1, P2)], two points of the twist whose difference of x (what a mixed addition onto a fresh affine
    accumulator forms as P = U2 - x) or of y (R = S2 - y) is zero in exactly the stated way:
      "a"  equal re(x), different im(x);  "b"  equal im(x), different re(x)  — P has exactly one zero component;
      "c"  (x, y) and (beta x, y), beta a primitive cube root of unity in Fq (x^3 and with it b' unchanged): R = 0 with P != 0,
           both components of P non-zero; "c-" the same with -y on the second point: R = -2y.
    points: [(shape, P)], points with a zero component of their own:
      "d_re" y = (t, 0), "d_im" y = (0, t) (x a cube root of y^2 - b'): with -P they give P = 0 and R = -2y half zero;
      "e_re" x = (t, 0), "e_im" x = (0, t)."""
    pairs, points = [], []
    # (a), (b): the first two fixed components with two partners each
    for shape, make in (("a", lambda fix, var: (fix, var)), ("b", lambda fix, var: (var, fix))):
        got = 0
        for fix in range(1, 50):
            on = [_twist_points_at(make(fix, var)) for var in range(1, 12)]
            on = [p[0] for p in on if p]
            if len(on) >= 2:
                pairs += [(shape, on[0], on[1]), (shape, on[0], bn.G2.neg(on[1]))]
                got += 1
            if got == 2:
                break
        assert got == 2
    beta = _fq_beta()
    got = 0
    for s in range(1, 50):
        for P in _twist_points_at((s, s + 1))[:1]:
            Pb = (bn.f2_scalar(P[0], beta), P[1])
            assert bn.G2.is_on_curve(Pb) and Pb[0] != P[0]
            pairs += [("c", P, Pb), ("c-", P, bn.G2.neg(Pb))]
            got += 1
        if got == 2:
            break
    assert got == 2
    # (d): y with one zero component; (e): x with one zero component
    for shape, make in (("d_re", lambda t: (t, 0)), ("d_im", lambda t: (0, t))):
        got = 0
        for t in range(1, 50):
            y = make(t)
            x = f2_cbrt(bn.f2_sub(bn.f2_mul(y, y), bn.G2_B))
            if x is not None:
                assert bn.G2.is_on_curve((x, y))
                points.append((shape, (x, y)))
                got += 1
            if got == 2:
                break
        assert got == 2
    for shape, make in (("e_re", lambda t: (t, 0)), ("e_im", lambda t: (0, t))):
        got = 0
        for t in range(1, 50):
            for P in _twist_points_at(make(t))[:1]:
                points.append((shape, P))
                got += 1
            if got == 2:
                break
        assert got == 2
    return pairs, points


def g2_scalars_below_r(n, seed=41):
    """0, 1, 2, r - 1, r - 2 and random values, ALL below r, up to n.  The extreme G2 points lie outside the order-r subgroup:
    for them k P and (k mod r) P differ, and zk_msm_g2 reduces a scalar at or above r by subtracting r while the references
    take its raw digits — the two agree on such points only for k < r."""
    import random
    rng = random.Random(seed)
    ks = [0, 1, 2, R - 1, R - 2]
    while len(ks) < n:
        ks.append(rng.randrange(R))
    ks = ks[:n]
    assert all(0 <= k < R for k in ks)                   # never at or above r: see the docstring
    return ks


# ----------------------------------------------------------------------------------------------- Montgomery-product operands
def EDGE_FIELD(p):
    """Operands for the 8 x 32 CIOS product of csrc/field.hpp (zk_fr_mul_vec / zk_fq_mul_vec)."""
    fullest = ((p >> 224) << 224) - 1                  # the largest value below p with its seven low 32-bit words full
    assert fullest < p and fullest & ((1 << 224) - 1) == (1 << 224) - 1
    vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (1 << 256) % p, (1 << 512) % p, (1 << 261) % p, word_for_internal(T_MAX, p), fullest]
    vals += [1 << k for k in (31, 32, 63, 64, 224, 253)]
    assert all(0 <= v < p for v in vals)
    return vals


def edge_cross_product(p):
    """(a bytes, b bytes, expected a b R^-1 mod p as ints) over the full cross product of EDGE_FIELD(p)."""
    e = EDGE_FIELD(p)
    a = [x for x in e for _ in e]
    b = [y for _ in e for y in e]
    rinv = pow(bn.MONT_R, -1, p)
    return pack(a), pack(b), [x * y * rinv % p for x, y in zip(a, b)]
