"""zk_pairing's two paths (a lane per group, a workgroup per group): the cooperative path against the Python oracle, and the
two paths against each other byte for byte at the shapes the tools use, with ZKHIP_PAIRING_COOP_MAX forced both ways and
pairing_last_path() asserted.  Errors name the same index on both paths."""
import random

import pytest

from oracle import bn254 as bn, pairing as opair
from test_gpu_pairing import G1, G2, ONE, gt_bytes, rows, twist_point_outside_the_subgroup

pytestmark = pytest.mark.gpu
RM, QM = bn.R_MOD, bn.Q_MOD
LANES, COOP = 0, 1


def both_paths(zk, monkeypatch, g1, g2, group):
    """the bytes of the cooperative path, after asserting the lane path gives the same"""
    monkeypatch.setenv("ZKHIP_PAIRING_COOP_MAX", "0")
    lanes = bytes(zk.pairing(g1, g2, group=group))
    assert zk.pairing_last_path() == LANES
    monkeypatch.setenv("ZKHIP_PAIRING_COOP_MAX", "4096")
    coop = bytes(zk.pairing(g1, g2, group=group))
    assert zk.pairing_last_path() == COOP
    assert coop == lanes
    return coop


def test_the_cooperative_path_against_the_oracle(zk, monkeypatch):
    rng = random.Random(12)
    a, b = rng.randrange(1, RM), rng.randrange(1, RM)
    P, Q = bn.G1.mul(bn.G1.gen, a), bn.G2.mul(bn.G2.gen, b)
    abP = bn.G1.mul(bn.G1.gen, a * b % RM)
    got = rows(both_paths(zk, monkeypatch, G1 + bn.g1_to_bytes(P) + bn.g1_to_bytes(abP), G2 + bn.g2_to_bytes(Q) + G2, 1))
    assert got[0] == gt_bytes(opair.pairing(bn.G1.gen, bn.G2.gen))        # all 384 bytes
    assert got[1] == gt_bytes(opair.pairing(P, Q))
    assert got[1] == got[2] and got[0] != ONE and got[1] != got[0]         # e(aP, bQ) = e(abP, Q)


def test_groups_whose_product_is_one_and_points_at_infinity(zk, monkeypatch):
    P = bn.G1.mul(bn.G1.gen, 31337)
    Q = bn.G2.mul(bn.G2.gen, 271828)
    negP = (P[0], (-P[1]) % QM)
    p, n, q = bn.g1_to_bytes(P), bn.g1_to_bytes(negP), bn.g2_to_bytes(Q)
    assert both_paths(zk, monkeypatch, p + n, q * 2, 2) == ONE
    lone = both_paths(zk, monkeypatch, p, q, 1)
    assert lone != ONE
    assert both_paths(zk, monkeypatch, p + bytes(64), q * 2, 2) == lone    # a pair with P at infinity contributes 1
    assert both_paths(zk, monkeypatch, p * 2, bytes(128) + q, 2) == lone   # and one with Q at infinity
    assert both_paths(zk, monkeypatch, bytes(64), q, 1) == ONE


@pytest.mark.parametrize("pairs,group", [(10, 2), (6, 2), (70, 1), (5, 5), (7, 3)])
def test_path_against_path(zk, monkeypatch, pairs, group):
    rng = random.Random(pairs * 100 + group)
    a = [rng.randrange(1, RM) for _ in range(pairs)]
    b = [rng.randrange(1, RM) for _ in range(pairs)]
    out = rows(both_paths(zk, monkeypatch, zk.fixed_base_g1(G1, a), zk.fixed_base_g2(G2, b), group))
    assert len(out) == (pairs + group - 1) // group and len(set(out)) == len(out) and ONE not in out


def test_the_threshold_counts_groups(zk, monkeypatch):
    monkeypatch.setenv("ZKHIP_PAIRING_COOP_MAX", "2")
    zk.pairing(G1 * 4, G2 * 4, group=2)
    assert zk.pairing_last_path() == COOP
    zk.pairing(G1 * 5, G2 * 5, group=2)
    assert zk.pairing_last_path() == LANES
    monkeypatch.setenv("ZKHIP_PAIRING_COOP_MAX", "lots")
    with pytest.raises(zk.ZkHipError, match=r"ZKHIP_PAIRING_COOP_MAX: a number of groups from 0 to 2\^24 expected"):
        zk.pairing(G1, G2)


@pytest.mark.parametrize("threshold", ["0", "4096"])
def test_errors_name_the_same_index_on_both_paths(zk, monkeypatch, threshold):
    monkeypatch.setenv("ZKHIP_PAIRING_COOP_MAX", threshold)
    n = 12
    rng = random.Random(40)
    P = zk.fixed_base_g1(G1, [rng.randrange(1, RM) for _ in range(n)]).tobytes()
    Q = zk.fixed_base_g2(G2, [rng.randrange(1, RM) for _ in range(n)]).tobytes()
    bad = bytearray(P)
    bad[64 * 9:64 * 10] = bn.g1_to_bytes((1, 3))
    bad[64 * 11:64 * 12] = bn.g1_to_bytes((1, 3))
    with pytest.raises(zk.ZkHipError, match=r"pairing: G1 point 9 is not on the curve"):
        zk.pairing(bytes(bad), Q, group=2)
    g = bn.G2.gen
    off2 = (((g[0][0] + 1) % QM, g[0][1]), g[1])
    assert not bn.G2.is_on_curve(off2)
    bad = bytearray(Q)
    bad[128 * 5:128 * 6] = bn.g2_to_bytes(off2)
    with pytest.raises(zk.ZkHipError, match=r"pairing: G2 point 5 is not on the curve"):
        zk.pairing(P, bytes(bad), group=2)
    bad = bytearray(Q)
    bad[128 * 11:128 * 12] = bn.g2_to_bytes(twist_point_outside_the_subgroup())
    bad[128 * 3:128 * 4] = bn.g2_to_bytes(twist_point_outside_the_subgroup())
    with pytest.raises(zk.ZkHipError, match=r"pairing: G2 point 3 is not in the subgroup"):
        zk.pairing(P, bytes(bad), group=2)
    assert zk.pairing_last_path() == (COOP if threshold != "0" else LANES)
