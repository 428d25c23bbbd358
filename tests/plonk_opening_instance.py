"""Rounds 4 and 5 of a three-column PLONK proof in Python integers: two independent references for the linearisation
polynomial F, the opening quotients and r(zeta) (helper of test_plonk_opening_host.py and test_gpu_plonk_opening.py; not
collected).  Instances, the quotient t and the polynomial helpers are tests/plonk_instance.py's.

Reference A is the prover's side: F coefficient by coefficient, as a sum of 14 rows times scalars, q_C and one constant at
index 0 (the formula of include/zkhip.h, section "PLONK evaluations and opening proofs"), then the division by X - zeta by
the recurrence q_(i-1) = c_i + zeta q_i, whose remainder is F(zeta).
Reference B is the verifier's side: from the six values and the challenges alone the scalar r0; from scalar multiples of
the POLYNOMIALS qM .. s3, z and the parts of t the polynomial D(X); and a check, by multiplying a quotient back out, of
    D + sum v^i p_i - (r0 + E + r(zeta)) = (X - zeta) q,      r(zeta) = 0 on a valid instance.
They share only the instance and oracle.bn254."""
import random

import plonk_instance as pi
from oracle.bn254 import R_MOD as R, fr_root

K1, K2 = pi.K1, pi.K2


def split(t, n, blind=None):
    """t -> (t_lo, t_mid, t_hi) with t = t_lo + X^n t_mid + X^2n t_hi; t_hi without its top zeros (one coefficient at
    least).  blind (b10, b11): the usual blinding of the parts, t_lo + b10 X^n, t_mid - b10 + b11 X^n, t_hi - b11."""
    k = max(pi.t_len_of(t), 2 * n + 1)
    lo, mid, hi = list(t[:n]), list(t[n:2 * n]), list(t[2 * n:k])
    if blind:
        b10, b11 = blind
        lo.append(b10 % R)
        mid[0] = (mid[0] - b10) % R
        mid.append(b11 % R)
        hi[0] = (hi[0] - b11) % R
    return lo, mid, hi


class Round45:
    """inst, parts, zeta, v, pi_zeta and what the references make of them: evals (six ints), F, q_zeta, q_zw (the two
    quotients), f_zeta, E, r_zeta"""


def challenges(seed):
    rng = random.Random(seed)
    return rng.randrange(2, R), rng.randrange(2, R)


def evaluations(I, zeta):
    w = fr_root(I.log_n)
    return [pi.horner(p, zeta) for p in (I.a, I.b, I.c, I.s1, I.s2)] + [pi.horner(I.z, zeta * w % R)]


def _l1_zh(n, zeta):
    zh = (pow(zeta, n, R) - 1) % R
    if zeta == 1:
        return 1, zh
    return (zh * pow(n * (zeta - 1) % R, -1, R) % R), zh


def divide(coeffs, z):
    """(q, y): (p - y) / (X - z) and y = p(z) by the recurrence"""
    q, acc = [0] * (len(coeffs) - 1), 0
    for i in range(len(coeffs) - 1, -1, -1):
        acc = (coeffs[i] + z * acc) % R
        if i:
            q[i - 1] = acc
    return q, acc


# ---------------------------------------------------------------- reference A: the prover's side
def reference_a(I, parts, zeta, v, pi_zeta=None, evals=None):
    n, al, be, ga = I.n, I.alpha, I.beta, I.gamma
    w = fr_root(I.log_n)
    ev = evaluations(I, zeta) if evals is None else list(evals)
    a, b, c, s1, s2, zw = ev
    if pi_zeta is None:
        pi_zeta = pi.horner(I.pi, zeta)
    l1, zh = _l1_zh(n, zeta)
    zn = pow(zeta, n, R)
    g12 = (a + be * s1 + ga) * (b + be * s2 + ga) % R
    rows = [(I.qm, a * b), (I.ql, a), (I.qr, b), (I.qo, c),
            (I.z, al * (a + be * zeta + ga) % R * (b + be * K1 * zeta + ga) % R * (c + be * K2 * zeta + ga) + al * al * l1),
            (I.s3, -al * g12 % R * be % R * zw),
            (parts[0], -zh), (parts[1], -zh * zn), (parts[2], -zh * zn * zn),
            (I.a, v), (I.b, pow(v, 2, R)), (I.c, pow(v, 3, R)), (I.s1, pow(v, 4, R)), (I.s2, pow(v, 5, R)), (I.qc, 1)]
    L = max(len(p) for p, _ in rows)
    F = [0] * L
    for i in range(L):
        acc = 0
        for p, s in rows:
            if i < len(p):
                acc += p[i] * (s % R)
        F[i] = acc % R
    F[0] = (F[0] + pi_zeta - g12 * zw % R * al % R * (c + ga) - al * al * l1) % R
    o = Round45()
    o.inst, o.parts, o.zeta, o.v, o.pi_zeta, o.evals, o.F = I, parts, zeta, v, pi_zeta, ev, F
    o.q_zeta, o.f_zeta = divide(F, zeta)
    o.q_zw, zw_again = divide(I.z, zeta * w % R)
    assert evals is not None or zw_again == zw
    o.E = sum(pow(v, j + 1, R) * ev[j] for j in range(5)) % R
    o.r_zeta = (o.f_zeta - o.E) % R
    return o


# ---------------------------------------------------------------- reference B: the verifier's side
def r0_of(n, evals, zeta, alpha, beta, gamma, pi_zeta):
    """the scalar the verifier makes of the six values and the challenges: D(zeta) = r0 on a valid proof"""
    a, b, c, s1, s2, zw = evals
    l1, _ = _l1_zh(n, zeta)
    return (alpha * (a + beta * s1 + gamma) % R * (b + beta * s2 + gamma) % R * (c + gamma) % R * zw + alpha * alpha * l1 - pi_zeta) % R


def d_poly(I, parts, evals, zeta):
    """D(X) from scalar multiples of the polynomials (the verifier forms the same combination of their commitments)"""
    n, al, be, ga = I.n, I.alpha, I.beta, I.gamma
    a, b, c, s1, s2, zw = evals
    l1, zh = _l1_zh(n, zeta)
    gate = pi._add(pi._scale(I.qm, a * b % R), pi._scale(I.ql, a), pi._scale(I.qr, b), pi._scale(I.qo, c), I.qc)
    f = (a + be * zeta + ga) * (b + be * K1 * zeta + ga) % R * (c + be * K2 * zeta + ga) % R
    perm_z = pi._scale(I.z, (al * f + al * al * l1) % R)
    g = (a + be * s1 + ga) * (b + be * s2 + ga) % R
    perm_s3 = pi._scale(I.s3, (R - al * g % R * be % R * zw % R) % R)
    zn = pow(zeta, n, R)
    t_at = pi._add(parts[0], pi._scale(parts[1], zn), pi._scale(parts[2], zn * zn % R))
    return pi._add(gate, perm_z, perm_s3, pi._scale(t_at, (R - zh) % R))


def reference_b(I, parts, zeta, v, pi_zeta=None):
    """F, E, r0 and r(zeta) = D(zeta) - r0 the verifier's way"""
    ev = evaluations(I, zeta)
    if pi_zeta is None:
        pi_zeta = pi.horner(I.pi, zeta)
    o = Round45()
    o.inst, o.parts, o.zeta, o.v, o.pi_zeta, o.evals = I, parts, zeta, v, pi_zeta, ev
    o.r0 = r0_of(I.n, ev, zeta, I.alpha, I.beta, I.gamma, pi_zeta)
    o.D = d_poly(I, parts, ev, zeta)
    o.r_zeta = (pi.horner(o.D, zeta) - o.r0) % R
    o.E = sum(pow(v, j + 1, R) * ev[j] for j in range(5)) % R
    o.batch = pi._add(o.D, *[pi._scale(p, pow(v, j + 1, R)) for j, p in enumerate((I.a, I.b, I.c, I.s1, I.s2))])
    o.F = pi._add(o.batch, [(R - o.r0) % R])            # r(X) = D(X) - r0
    return o


def check_b(o, q_zeta, q_zw, r_zeta):
    """the quotients multiplied back out: D + sum v^i p_i - (r0 + E + r_zeta) = (X - zeta) q_zeta, z - z'w = (X - zeta w) q_zw"""
    w = fr_root(o.inst.log_n)
    lhs = pi._add(o.batch, [(R - (o.r0 + o.E + r_zeta) % R) % R])
    rhs = pi._mul([(R - o.zeta) % R, 1], q_zeta) if q_zeta else [0]
    k = max(len(lhs), len(rhs))
    if lhs + [0] * (k - len(lhs)) != rhs + [0] * (k - len(rhs)):
        return False
    zw = o.zeta * w % R
    lhs = pi._add(o.inst.z, [(R - o.evals[5]) % R])
    rhs = pi._mul([(R - zw) % R, 1], q_zw) if q_zw else [0]
    k = max(len(lhs), len(rhs))
    return lhs + [0] * (k - len(lhs)) == rhs + [0] * (k - len(rhs))


def make(seed, log_n, blind=pi.BLIND, t=None, blind_parts=True, zeta=None, v=None, **kw):
    """(instance, parts, zeta, v): plonk_instance.make, oracle A's t (or the t given) and its split"""
    I = pi.make(seed, log_n, blind, **kw)
    if t is None:
        t = pi.oracle_a(I)[0]                          # a broken gate leaves a remainder, which is dropped: r(zeta) is then its value at zeta
    rng = random.Random(seed * 7 + 1)
    parts = split(t, I.n, (rng.randrange(1, R), rng.randrange(1, R)) if blind_parts else None)
    z0, v0 = challenges(seed * 7 + 2)
    return I, parts, z0 if zeta is None else zeta, v0 if v is None else v
