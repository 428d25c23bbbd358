#!/usr/bin/env python3
"""Makes tests/golden/g2_cofactor_points.json: points of BN254's twist E'(Fq2): y^2 = x^3 + 3/(9 + u) that are NOT in the
order-r subgroup, from the big-integer oracle alone (no GPU, no library).

#E'(Fq2) = r h2 with h2 = 2q - r = 10069 * 5864401 * 1875725156269 * 1976...6909: four distinct primes, none of them r, so
the group is cyclic and has exactly one subgroup of each of these orders.  The file holds
  cofactor   one point of each prime order l | h2: a random twist point times r h2 / l (drawn again if that is infinity);
  outside    eight random twist points (each checked: r P is not infinity).
A point's order-l component is where an endomorphism-based subgroup test could be wrong and the plain [r] Q is not: the
device test (tests/test_gpu_ptau_check.py) must reject all of them.  Coordinates are decimal strings, standard form,
x = x0 + x1 u as [x0, x1].  The seed is fixed: running this again reproduces the committed file byte for byte
(tests/test_ptau_check_host.py does).

usage: gen_g2_cofactor_points.py [out.json]   (default: tests/golden/g2_cofactor_points.json; "-" prints)"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import bn254 as bn  # noqa: E402

Q, R = bn.Q_MOD, bn.R_MOD
SEED = 0x67325F636F66                                  # "g2_cof"
H2 = 2 * Q - R
H2_PRIMES = (10069, 5864401, 1875725156269, 197620364512881247228717050342013327560683201906968909)
N_OUTSIDE = 8


def is_prime(n, rng):
    """Miller-Rabin, 40 random bases"""
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for _ in range(40):
        x = pow(rng.randrange(2, n - 1), d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def fq_sqrt(a):
    """a square root in Fq (q = 3 mod 4), or None"""
    x = pow(a, (Q + 1) // 4, Q)
    return x if x * x % Q == a % Q else None


def f2_sqrt(a):
    """a square root of a = a0 + a1 u in Fq2 = Fq[u]/(u^2 + 1), or None.  (x0 + x1 u)^2 = a gives x0^2 - x1^2 = a0 and
    2 x0 x1 = a1, so x0^2 = (a0 +- sqrt(a0^2 + a1^2)) / 2."""
    a0, a1 = a
    if a1 == 0:
        x = fq_sqrt(a0)
        if x is not None:
            return (x, 0)
        x = fq_sqrt(-a0 % Q)                          # -1 is not a square in Fq: a0 = -(x^2) = (x u)^2
        return (0, x)
    n = fq_sqrt((a0 * a0 + a1 * a1) % Q)
    if n is None:
        return None
    half = pow(2, -1, Q)
    for sign in (1, -1):
        x0 = fq_sqrt((a0 + sign * n) * half % Q)
        if x0:
            x = (x0, a1 * pow(2 * x0, -1, Q) % Q)
            if bn.f2_mul(x, x) == (a0 % Q, a1 % Q):
                return x
    return None


def random_twist_point(rng):
    while True:
        x = (rng.randrange(Q), rng.randrange(Q))
        y = f2_sqrt(bn.f2_add(bn.f2_mul(bn.f2_mul(x, x), x), bn.G2_B))
        if y is None:
            continue
        if rng.randrange(2):
            y = bn.f2_neg(y)
        P = (x, y)
        assert bn.G2.is_on_curve(P)
        return P


def make():
    rng = random.Random(SEED)
    prod = 1
    for p in H2_PRIMES:
        assert is_prime(p, rng), p
        prod *= p
    assert is_prime(R, rng) and prod == H2 and len(set(H2_PRIMES + (R,))) == 5      # r h2 is squarefree: the group is cyclic
    assert bn.G2.mul(bn.G2.gen, R) is None
    enc = lambda P: {"x": [str(P[0][0]), str(P[0][1])], "y": [str(P[1][0]), str(P[1][1])]}
    cof = []
    for l in H2_PRIMES:
        while True:
            P = bn.G2.mul(random_twist_point(rng), R * H2 // l)
            if P is not None:
                break
        assert bn.G2.is_on_curve(P) and bn.G2.mul(P, l) is None                   # the group's order is r h2, and P has order l
        cof.append(dict(order=str(l), **enc(P)))
    outside = []
    while len(outside) < N_OUTSIDE:
        P = random_twist_point(rng)
        if bn.G2.mul(P, R) is not None:
            outside.append(enc(P))
    return {"curve": "BN254 twist y^2 = x^3 + 3/(9+u) over Fq[u]/(u^2+1)", "seed": SEED, "h2": str(H2), "cofactor": cof, "outside": outside}


def text():
    return json.dumps(make(), indent=1) + "\n"


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "g2_cofactor_points.json")
    if out == "-":
        sys.stdout.write(text())
    else:
        with open(out, "w") as f:
            f.write(text())
