"""zk_pairing on the GPU: the 384 output bytes against the Python oracle's pairing, bilinearity lane by lane across a wave
border, groups that share one squaring chain, and the refusal of points that are off their curve or outside the subgroup."""
import functools
import importlib.util
import os
import random

import numpy as np
import pytest

from conftest import ROOT, golden_json, golden_path

from oracle import bn254 as bn, pairing as opair
from rapidsnark_old_amd import synth

pytestmark = pytest.mark.gpu
RM, QM = bn.R_MOD, bn.Q_MOD
G1, G2 = synth.g1_gen_bytes(), synth.g2_gen_bytes()
ONE = (1).to_bytes(32, "little") + bytes(352)          # the encoding of 1 in GT: first Fq = 1, the other eleven 0
_spec = importlib.util.spec_from_file_location("refcheck_verify", os.path.join(ROOT, "tools", "refcheck", "verify.py"))
refverify = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(refverify)


def gt_bytes(f):
    """the oracle's nested tuples flattened: c0.c0.re, c0.c0.im, c0.c1.re, ... as 32-byte little-endian values"""
    return b"".join(int(c).to_bytes(32, "little") for six in f for two in six for c in two)


def rows(out):
    out = bytes(out)
    return [out[i:i + 384] for i in range(0, len(out), 384)]


def f2_sqrt(a):
    """a square root of a in Fq2 for q = 3 mod 4 (Adj, Rodriguez-Henriquez 2012, algorithm 9), None when a is no square"""
    a1 = opair.f2_pow(a, (QM - 3) // 4)
    alpha = bn.f2_mul(bn.f2_mul(a1, a1), a)
    if bn.f2_mul(opair.f2_conj(alpha), alpha) == (QM - 1, 0):
        return None
    x0 = bn.f2_mul(a1, a)
    if alpha == (QM - 1, 0):
        x = bn.f2_mul((0, 1), x0)
    else:
        x = bn.f2_mul(opair.f2_pow(bn.f2_add(bn.F2_ONE, alpha), (QM - 1) // 2), x0)
    return x if bn.f2_mul(x, x) == a else None


@functools.lru_cache(maxsize=None)
def twist_point_outside_the_subgroup(seed=7):
    """a point of the twist y^2 = x^3 + 3/xi that is NOT in the order-r subgroup (the cofactor is about 2^254, so the
    first root found qualifies; asserted)"""
    rng = random.Random(seed)
    while True:
        x = (rng.randrange(QM), rng.randrange(QM))
        y = f2_sqrt(bn.f2_add(bn.f2_mul(bn.f2_mul(x, x), x), bn.G2_B))
        if y is not None:
            break
    pt = (x, y)
    assert bn.G2.is_on_curve(pt) and bn.G2.mul(pt, RM) is not None
    return pt


@pytest.fixture(scope="module")
def seeded():
    """65 seeded pairs (a_i G1, b_i G2): a = 1 and a = r - 1 among them, P = infinity at lane 0, Q = infinity at lane 64"""
    rng = random.Random(2024)
    a = [rng.randrange(1, RM) for _ in range(65)]
    b = [rng.randrange(1, RM) for _ in range(65)]
    a[0], a[1], a[2], b[64] = 0, 1, RM - 1, 0
    return a, b


def test_against_the_oracle(zk):
    rng = random.Random(11)
    a, b = rng.randrange(1, RM), rng.randrange(1, RM)
    P, Q = bn.G1.mul(bn.G1.gen, a), bn.G2.mul(bn.G2.gen, b)
    got = rows(zk.pairing(G1 + bn.g1_to_bytes(P), G2 + bn.g2_to_bytes(Q)))
    assert got[0] == gt_bytes(opair.pairing(bn.G1.gen, bn.G2.gen))
    assert got[1] == gt_bytes(opair.pairing(P, Q))
    assert got[0] != ONE and got[1] != got[0]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_bilinearity_lane_by_lane(zk, seeded, n):
    a, b = seeded[0][:n], seeded[1][:n]
    P = zk.fixed_base_g1(G1, a) if n else np.zeros(0, np.uint8)
    Q = zk.fixed_base_g2(G2, b) if n else np.zeros(0, np.uint8)
    left = zk.pairing(P, Q)
    assert left.dtype == np.uint8 and left.shape == (384 * n,)
    PQ = zk.fixed_base_g1(G1, [x * y % RM for x, y in zip(a, b)]) if n else np.zeros(0, np.uint8)
    right = zk.pairing(PQ, G2 * n)
    left, right = rows(left), rows(right)
    for i in range(n):
        assert left[i] == right[i], i                   # e(a G1, b G2) = e(ab G1, G2), byte for byte
        if a[i] == 0 or b[i] == 0:
            assert left[i] == ONE, i                    # a point at infinity contributes 1
        else:
            assert left[i] != ONE, i
    assert len(set(left)) == n - max(0, sum(1 for x, y in zip(a, b) if x == 0 or y == 0) - 1)      # no lane repeats another's value


def test_group_of_a_pair_and_its_negative(zk):
    P = bn.G1.mul(bn.G1.gen, 31337)
    Q = bn.G2.mul(bn.G2.gen, 271828)
    negP = (P[0], (-P[1]) % QM)
    out = zk.pairing(bn.g1_to_bytes(P) + bn.g1_to_bytes(negP), bn.g2_to_bytes(Q) * 2, group=2)
    assert bytes(out) == ONE
    assert rows(zk.pairing(bn.g1_to_bytes(P) + bn.g1_to_bytes(negP), bn.g2_to_bytes(Q) * 2, group=1))[0] != ONE


def test_group_of_the_four_pairs_of_a_proof(zk):
    name = "r1cs_n64"
    vk = refverify.vk_from_zkey(golden_path(name, "circuit.zkey"))
    pj = golden_json(name, "proof.json")
    A, B, C = refverify.g1(pj["pi_a"]), refverify.g2(pj["pi_b"]), refverify.g1(pj["pi_c"])
    negA = (A[0], (-A[1]) % QM)

    def four(pub):
        vk_x = vk["IC"][0]
        for s, ic in zip(pub, vk["IC"][1:]):
            vk_x = bn.G1.add(vk_x, bn.G1.mul(ic, s))
        g1 = b"".join(bn.g1_to_bytes(p) for p in (negA, vk["alpha1"], vk_x, C))
        g2 = b"".join(bn.g2_to_bytes(q) for q in (B, vk["beta2"], vk["gamma2"], vk["delta2"]))
        return bytes(zk.pairing(g1, g2, group=4))

    pub = [int(x) for x in golden_json(name, "public.json")]
    assert four(pub) == ONE
    pub[1] = (pub[1] + 1) % RM
    assert four(pub) != ONE


def test_groups_of_three_with_a_short_last_group(zk):
    rng = random.Random(3)
    a = [rng.randrange(1, RM) for _ in range(7)]
    b = [rng.randrange(1, RM) for _ in range(7)]
    got = rows(zk.pairing(zk.fixed_base_g1(G1, a), zk.fixed_base_g2(G2, b), group=3))
    assert len(got) == 3
    # prod e(a_i G1, b_i G2) over a group = e((sum a_i b_i) G1, G2): the bilinear rewrite, one pair per group
    sums = [sum(x * y for x, y in zip(a[i:i + 3], b[i:i + 3])) % RM for i in (0, 3, 6)]
    want = rows(zk.pairing(zk.fixed_base_g1(G1, sums), G2 * 3))
    assert got == want and ONE not in got


def test_refusals_name_the_index_and_nothing_faults(zk):
    n = 40
    rng = random.Random(40)
    P = bytearray(zk.fixed_base_g1(G1, [rng.randrange(1, RM) for _ in range(n)]).tobytes())
    Q = bytearray(zk.fixed_base_g2(G2, [rng.randrange(1, RM) for _ in range(n)]).tobytes())
    good = bytes(zk.pairing(bytes(P), bytes(Q)))

    off1 = (1, 3)                                       # 9 != 1 + 3
    assert not bn.G1.is_on_curve(off1)
    bad = bytearray(P)
    bad[64 * 37:64 * 38] = bn.g1_to_bytes(off1)
    with pytest.raises(zk.ZkHipError, match=r"pairing: G1 point 37 is not on the curve"):
        zk.pairing(bytes(bad), bytes(Q))

    g = bn.G2.gen
    off2 = (((g[0][0] + 1) % QM, g[0][1]), g[1])
    assert not bn.G2.is_on_curve(off2)
    bad = bytearray(Q)
    bad[128 * 5:128 * 6] = bn.g2_to_bytes(off2)
    with pytest.raises(zk.ZkHipError, match=r"pairing: G2 point 5 is not on the curve"):
        zk.pairing(bytes(P), bytes(bad))

    bad = bytearray(Q)
    bad[128 * 39:128 * 40] = bn.g2_to_bytes(twist_point_outside_the_subgroup())
    with pytest.raises(zk.ZkHipError, match=r"pairing: G2 point 39 is not in the subgroup"):
        zk.pairing(bytes(P), bytes(bad))

    bad = bytearray(P)
    bad[64 * 2:64 * 2 + 32] = QM.to_bytes(32, "little")    # a coordinate that is not below q
    with pytest.raises(zk.ZkHipError, match=r"pairing: G1 point 2 is not on the curve"):
        zk.pairing(bytes(bad), bytes(Q))

    with pytest.raises(zk.ZkHipError, match="group"):
        zk.pairing(bytes(P), bytes(Q), group=0)
    assert bytes(zk.pairing(bytes(P), bytes(Q))) == good    # a correct call afterwards still works
