"""Input families that sit at the edges of the nine-limb (9 x 29 bit) arithmetic of csrc/field29.hpp, for operators that the
suite otherwise feeds uniformly random data ("Extreme-operand inputs").  A plain helper module: nothing here needs
a GPU, tests/test_extreme_operands_host.py checks that every family is what it claims to be.

The operators take x * 2^256 bytes and convert with ONE Montgomery product by 2^266 (Fp29::from_mont256), so the value the
kernels hold is bytes * 2^5 mod p.  A word that must become T inside the kernel is therefore T * 32^-1 mod p.  That product
leaves (bytes * K_IN + M p) / 2^261 with 0 <= bytes, K_IN < p and M within 2^235 of [0, 2^261): a representative of T in
(-p / 2^20, p + p / 160).  For p - p / 160 > T > p / 160 the representative is T itself, limb for limb (internal_limbs()).
"""
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
