"""A whole three-column PLONK proof in Python integers (helper of test_plonk_prover_host.py and test_gpu_plonk_prover.py; not
collected): Keccak-256 and the transcript written from the layout of include/zkhip.h, section "PLONK prover and verifier";
a builder that turns an instance of tests/plonk_instance.py into (witness, maps, publics); a reference prover; and a
reference verifier that needs no pairing because tau is known.

The reference prover shares nothing with the library but the header's text: challenges from the transcript below, z from
plonk_instance.make called again with the transcript's beta and gamma, t from plonk_instance's oracle A (schoolbook and long
division; from log_n 10 on oracle B, the coset route, because A's products take minutes there: the two are compared with
each other by the tests of round 3), the split and the openings from plonk_opening_instance (split, reference_a), and
commitments as [p(tau)] G over oracle.bn254.

The builder's two layouts.  "circom": witness = [1, publics .., the distinct cell values shuffled]; index 0 is then a wire's
only if some cell holds 1, which a random instance does not.  "plain": the shuffled distinct values alone, so that index 0
and index n_witness - 1 are both some row's wire."""
import random

import plonk_instance as pi
import plonk_opening_instance as po
from oracle import bn254 as bn

R, Q = bn.R_MOD, bn.Q_MOD
K1, K2 = pi.K1, pi.K2
PROOF_BYTES = 768
ORACLE_A_BELOW = 10

# ---------------------------------------------------------------- Keccak-256 (the original padding 0x01)
_RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001, 0x8000000080008081,
       0x8000000000008009, 0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A, 0x000000008000808B, 0x800000000000008B,
       0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080, 0x000000000000800A, 0x800000008000000A, 0x8000000080008081,
       0x8000000000008080, 0x0000000080000001, 0x8000000080008008]
_M64 = (1 << 64) - 1
_RHO = [[0] * 5 for _ in range(5)]


def _rho_offsets():
    x, y = 1, 0
    for t in range(24):
        _RHO[x][y] = (t + 1) * (t + 2) // 2 % 64
        x, y = y, (2 * x + 3 * y) % 5


_rho_offsets()


def _rot(x, k):
    k %= 64
    return ((x << k) | (x >> (64 - k))) & _M64 if k else x


def _f1600(a):
    """a[x][y], 24 rounds: theta, rho and pi, chi, iota as the Keccak reference states them"""
    for rc in _RC:
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
        d = [c[(x - 1) % 5] ^ _rot(c[(x + 1) % 5], 1) for x in range(5)]
        a = [[a[x][y] ^ d[x] for y in range(5)] for x in range(5)]
        b = [[0] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                b[y][(2 * x + 3 * y) % 5] = _rot(a[x][y], _RHO[x][y])
        a = [[b[x][y] ^ ((~b[(x + 1) % 5][y]) & _M64 & b[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
        a[0][0] ^= rc
    return a


def keccak256(data):
    data = bytes(data)
    rate = 136
    pad = rate - len(data) % rate
    data += (b"\x81" if pad == 1 else b"\x01" + bytes(pad - 2) + b"\x80")
    a = [[0] * 5 for _ in range(5)]
    for off in range(0, len(data), rate):
        for i in range(rate // 8):
            a[i % 5][i // 5] ^= int.from_bytes(data[off + 8 * i:off + 8 * i + 8], "little")
        a = _f1600(a)
    return b"".join(a[i % 5][i // 5].to_bytes(8, "little") for i in range(4))


# ---------------------------------------------------------------- the transcript
def _enc(item):
    """an int: a scalar, 32 bytes big-endian; a pair or None: a point, x | y big-endian, infinity 64 zero bytes"""
    if item is None:
        return bytes(64)
    if isinstance(item, tuple):
        return int(item[0]).to_bytes(32, "big") + int(item[1]).to_bytes(32, "big")
    return int(item).to_bytes(32, "big")


def challenge(*items):
    return int.from_bytes(keccak256(b"".join(_enc(x) for x in items)), "big") % R


class Challenges:
    pass


def challenges(vk_points, publics, pts, evals):
    """the six challenges from the key's eight commitments (the transcript's order), the publics, the proof's nine points
    (a, b, c, z, t_lo, t_mid, t_hi, W_zeta, W_zeta_omega; later ones may be missing) and its six values"""
    c = Challenges()
    c.beta = challenge(*vk_points, *publics, *pts[0:3])
    c.gamma = challenge(c.beta)
    if len(pts) > 3:
        c.alpha = challenge(c.beta, c.gamma, pts[3])
    if len(pts) > 6:
        c.zeta = challenge(c.alpha, *pts[4:7])
    if evals is not None:
        c.v = challenge(c.zeta, *evals)
    if len(pts) > 8:
        c.u = challenge(pts[7], pts[8])
    return c


# ---------------------------------------------------------------- instance -> (witness, maps, publics)
class Case:
    """inst (unblinded, by the seed), witness, maps (a_map, b_map, c_map), publics, n_witness, n_public"""


def build(seed, log_n, n_public=2, layout="plain", **kw):
    assert layout in ("plain", "circom")
    I = pi.make(seed, log_n, None, alpha=1, beta=1, gamma=1, public=n_public > 0, **kw)
    n = I.n
    assert n_public in (0, 2, n)
    pi_v = bn.ntt(I.pi)
    publics = [(R - pi_v[i]) % R for i in range(n_public)]
    cells = I.a_v + I.b_v + I.c_v
    distinct = sorted(set(cells))
    assert len(distinct) < len(cells)                    # copy cycles share values: indices repeat
    rng = random.Random(seed * 11 + 5)
    rng.shuffle(distinct)
    head = [1] + publics if layout == "circom" else []
    witness = head + distinct
    where = {v: len(head) + i for i, v in enumerate(distinct)}
    idx = [where[v] for v in cells]
    c = Case()
    c.seed, c.log_n, c.kw = seed, log_n, dict(kw)
    c.inst, c.witness, c.publics, c.n_witness, c.n_public = I, witness, publics, len(witness), n_public
    c.maps = (idx[:n], idx[n:2 * n], idx[2 * n:])
    assert max(idx) == c.n_witness - 1 and (layout == "circom" or min(idx) == 0)
    return c


# ---------------------------------------------------------------- the reference prover
def at_tau(coeffs, tau):
    return bn.G1.mul(bn.G1_GEN, pi.horner(coeffs, tau)) if any(coeffs) else None


def _blinded(p, n, r):
    """p + (r[0] + r[1] X + ..) (X^n - 1)"""
    p = list(p) + [0] * (n + len(r) - len(p))
    for j, rj in enumerate(r):
        p[j] = (p[j] - rj) % R
        p[n + j] = (p[n + j] + rj) % R
    return p


class Proof:
    """points (nine affine pairs or None), evals (six ints), and what made them: challenges ch, inst, parts"""

    def to_bytes(self):
        return b"".join(bn.g1_to_bytes(P) for P in self.points) + pi.le(self.evals)


def vkey_points(I, tau):
    return [at_tau(getattr(I, k), tau) for k in ("qm", "ql", "qr", "qo", "qc", "s1", "s2", "s3")]


def prove(case, blind, tau):
    """blind: b1 .. b11 (ints).  None when the witness is refused: returns the refusal's text instead of a proof"""
    b = [int(x) % R for x in blind]
    assert len(b) == 11
    I0 = case.inst
    n = I0.n
    vk = vkey_points(I0, tau)
    a = _blinded(I0.a, n, [b[1], b[0]])
    bb = _blinded(I0.b, n, [b[3], b[2]])
    c = _blinded(I0.c, n, [b[5], b[4]])
    pts = [at_tau(p, tau) for p in (a, bb, c)]
    ch = challenges(vk, case.publics, pts, None)
    # z with the transcript's beta and gamma: the instance again, every challenge given so that the seed draws the same circuit
    I = pi.make(case.seed, case.log_n, None, alpha=1, beta=ch.beta, gamma=ch.gamma, public=case.n_public > 0, **case.kw)
    assert I.a == I0.a and I.s3 == I0.s3
    z = _blinded(I.z, n, [b[8], b[7], b[6]])
    pts.append(at_tau(z, tau))
    ch = challenges(vk, case.publics, pts, None)
    I.alpha, I.a, I.b, I.c, I.z = ch.alpha, a, bb, c, z
    t = pi.oracle_a(I)[0] if case.log_n < ORACLE_A_BELOW else pi.oracle_b(I)
    if pi.t_len_of(t) > 3 * n + 6:
        return "zk_plonk_prove: the witness does not satisfy the gates"
    parts = po.split(t, n, (b[9], b[10]))
    pts += [at_tau(p, tau) for p in parts]
    ch = challenges(vk, case.publics, pts, None)
    evals = po.evaluations(I, ch.zeta)
    ch = challenges(vk, case.publics, pts, evals)
    ref = po.reference_a(I, parts, ch.zeta, ch.v, evals=evals)
    if ref.r_zeta != 0:
        return "zk_plonk_prove: the witness does not satisfy the gates"
    pts += [at_tau(ref.q_zeta, tau), at_tau(ref.q_zw, tau)]
    out = Proof()
    out.points, out.evals, out.inst, out.parts = pts, evals, I, parts
    out.ch = challenges(vk, case.publics, pts, evals)
    return out


# ---------------------------------------------------------------- the reference verifier
def parse(proof_bytes):
    """768 bytes -> (nine points, six values); None when a point is not on the curve or a value is not below r"""
    b = bytes(proof_bytes)
    assert len(b) == PROOF_BYTES
    pts = []
    for i in range(9):
        raw = b[i * 64:(i + 1) * 64]
        if int.from_bytes(raw[:32], "little") >= Q or int.from_bytes(raw[32:], "little") >= Q:
            return None
        P = bn.g1_from_bytes(raw)
        if not bn.G1.is_on_curve(P):
            return None
        pts.append(P)
    evals = pi.ints(b[576:])
    if any(v >= R for v in evals):
        return None
    return pts, evals


def verify(vk, log_n, publics, proof_bytes, tau):
    """True / False / None (malformed).  With tau known the pairing equation is one in G1:
    [tau] (W_zeta + u W_zeta_omega) = zeta W_zeta + u zeta w W_zeta_omega + F - E"""
    parsed = parse(proof_bytes)
    if parsed is None:
        return None
    pts, ev = parsed
    G, n = bn.G1, 1 << log_n
    w = bn.fr_root(log_n)
    ch = challenges(vk, publics, pts, ev)
    al, be, ga, ze, v, u = ch.alpha, ch.beta, ch.gamma, ch.zeta, ch.v, ch.u
    a, b, c, s1, s2, zw = ev
    pi_v = [(R - p) % R for p in publics] + [0] * (n - len(publics))
    pi_zeta = pi.horner(bn.ntt(pi_v, inverse=True), ze)
    r0 = po.r0_of(n, ev, ze, al, be, ga, pi_zeta)
    l1, zh = po._l1_zh(n, ze)
    zn = pow(ze, n, R)
    qm, ql, qr, qo, qc, c1, c2, c3 = vk
    A, B, C, Z, TLO, TMID, THI, WZ, WZW = pts

    def lin(*terms):
        acc = None
        for P, k in terms:
            acc = G.add(acc, G.mul(P, k % R))
        return acc

    f = (a + be * ze + ga) * (b + be * K1 * ze + ga) % R * (c + be * K2 * ze + ga) % R
    g = (a + be * s1 + ga) * (b + be * s2 + ga) % R
    D = lin((qm, a * b), (ql, a), (qr, b), (qo, c), (qc, 1), (Z, al * f + al * al * l1 + u), (c3, -(al * g % R * be % R * zw)),
            (TLO, -zh), (TMID, -zh * zn), (THI, -zh * zn % R * zn))
    F = G.add(D, lin((A, v), (B, pow(v, 2, R)), (C, pow(v, 3, R)), (c1, pow(v, 4, R)), (c2, pow(v, 5, R))))
    e = (r0 + sum(pow(v, j + 1, R) * ev[j] for j in range(5)) + u * zw) % R
    left = G.mul(G.add(WZ, G.mul(WZW, u)), tau % R)
    right = G.add(lin((WZ, ze), (WZW, u * ze % R * w)), G.sub(F, G.mul(bn.G1_GEN, e)))
    return left == right
