"""n points times n different scalars on the GPU: zk_g1_mul_vec / zk_g2_mul_vec against two independent routes (the
fixed-base kernel on the discrete logs, the Python oracle) and against their own plain double-and-add, their errors, and
zk_g1_power_scale / zk_g2_power_scale, which make their scalars on the device, against the operators on host-made scalars."""
import random

import numpy as np
import pytest

from conftest import golden_json

from oracle import bn254 as bn
from rapidsnark_old_amd import synth
from test_mulvec_host import split_edge_scalars

pytestmark = pytest.mark.gpu
RM, QM = bn.R_MOD, bn.Q_MOD
G1, G2 = synth.g1_gen_bytes(), synth.g2_gen_bytes()
EDGE = split_edge_scalars()
GROUPS = ["g1", "g2"]


def ops(zk, group):
    """(the operator, the fixed-base kernel on the group's generator, bytes a point)"""
    if group == "g1":
        return zk.g1_mul_vec, (lambda s: zk.fixed_base_g1(G1, s)), 64
    return zk.g2_mul_vec, (lambda s: zk.fixed_base_g2(G2, s)), 128


def logs_for(n, rng):
    """n discrete logs a_i: infinity at the first, a middle and the last place, 1 and r - 1 among them"""
    a = [rng.randrange(1, RM) for _ in range(n)]
    for i, v in zip(range(1, n - 1), (1, RM - 1)):
        a[i] = v
    for i in {0, n // 2, n - 1} if n > 2 else ():
        a[i] = 0
    return a


def mixed_scalars(n, rng):
    """seeded random scalars with the edge scalars cycled through every other place: both kinds in every wave"""
    return [EDGE[(i // 2) % len(EDGE)] if i % 2 == 0 else rng.randrange(RM) for i in range(n)]


def check_against_fixed_base(zk, group, a, k):
    mul_vec, fixed, nb = ops(zk, group)
    pts = fixed(a) if a else np.zeros(0, np.uint8)
    want = fixed([x * y % RM for x, y in zip(a, k)]) if a else np.zeros(0, np.uint8)
    got = mul_vec(pts, k)
    assert got.shape == (nb * len(a),)
    bad = [i for i in range(len(a)) if not np.array_equal(got[nb * i:nb * i + nb], want[nb * i:nb * i + nb])]
    assert not bad, (bad[:8], [k[i] for i in bad[:8]])
    return got


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_operator_against_the_fixed_base_kernel(zk, group, n):
    rng = random.Random(900 + n)
    check_against_fixed_base(zk, group, logs_for(n, rng), mixed_scalars(n, rng))


@pytest.mark.parametrize("group", GROUPS)
def test_a_wave_of_edge_scalars(zk, group):
    """n = 65 (two waves, the second one lane wide), every lane's scalar an edge scalar: k = 0 (its split is a lattice
    vector: the sum is reached through P + (-P)), small k, +-lambda, +-lambda +- 1, where the accumulator meets +- the
    point it adds"""
    rng = random.Random(65)
    a = [rng.randrange(1, RM) for _ in range(65)]
    k = [EDGE[i % len(EDGE)] for i in range(65)]
    got = check_against_fixed_base(zk, group, a, k)
    nb = got.size // 65
    zeros = [i for i in range(65) if k[i] == 0]
    assert len(zeros) >= 2 and all(not got[nb * i:nb * i + nb].any() for i in zeros)
    assert all(got[nb * i:nb * i + nb].any() for i in range(65) if k[i])


def test_operators_against_the_python_oracle(zk):
    rng = random.Random(8)
    a = [rng.randrange(1, RM) for _ in range(8)]
    a[3] = 0
    k = [rng.randrange(RM) for _ in range(8)]
    k[5] = RM - 2
    for curve, gen, fixed, mul_vec, to_bytes, nb in ((bn.G1, G1, zk.fixed_base_g1, zk.g1_mul_vec, bn.g1_to_bytes, 64),
                                                    (bn.G2, G2, zk.fixed_base_g2, zk.g2_mul_vec, bn.g2_to_bytes, 128)):
        pts = fixed(gen, a)
        want = b"".join(to_bytes(curve.mul(curve.mul(curve.gen, x), y)) if x else bytes(nb) for x, y in zip(a, k))
        assert mul_vec(pts, k).tobytes() == want


@pytest.mark.parametrize("group", GROUPS)
def test_the_plain_route_gives_the_same_bytes(zk, group, monkeypatch):
    rng = random.Random(66)
    mul_vec, fixed, _ = ops(zk, group)
    a, k = logs_for(65, rng), mixed_scalars(65, rng)
    pts = fixed(a)
    fast = mul_vec(pts, k)
    monkeypatch.setenv("ZKHIP_MULVEC_PLAIN", "1")
    assert np.array_equal(mul_vec(pts, k), fast)
    assert np.array_equal(fast, fixed([x * y % RM for x, y in zip(a, k)]))


@pytest.mark.parametrize("group", GROUPS)
def test_operator_errors(zk, group):
    rng = random.Random(9)
    n = 70
    mul_vec, fixed, nb = ops(zk, group)
    name = "zk_%s_mul_vec" % group
    pts = fixed([rng.randrange(1, RM) for _ in range(n)])
    k = [rng.randrange(RM) for _ in range(n)]
    for at in (0, n - 1):
        for big in (RM, (1 << 256) - 1):
            with pytest.raises(zk.ZkHipError, match=r"%s: scalar %d is not below r" % (name, at)):
                mul_vec(pts, k[:at] + [big] + k[at + 1:])
        off = pts.copy()
        off[nb * at + nb // 2] ^= 1                                 # y changed: off the curve
        with pytest.raises(zk.ZkHipError, match=r"%s: point %d is not on the curve" % (name, at)):
            mul_vec(off, k)
        big = pts.copy()
        big[nb * at:nb * at + 32] = np.frombuffer(QM.to_bytes(32, "little"), np.uint8)          # a coordinate = q
        with pytest.raises(zk.ZkHipError, match=r"%s: point %d has a coordinate that is not below q" % (name, at)):
            mul_vec(big, k)
    both = pts.copy()
    both[nb * 5 + nb // 2] ^= 1
    both[nb * 40 + nb // 2] ^= 1
    with pytest.raises(zk.ZkHipError, match="point 5 is"):             # the lowest failing index
        mul_vec(both, k)
    with pytest.raises(zk.ZkHipError, match="scalar 3 is"):
        mul_vec(pts, k[:3] + [RM] + k[4:60] + [RM + 1] + k[61:])
    with pytest.raises(ValueError, match="scalars"):
        mul_vec(pts, k[:-1])


@pytest.mark.parametrize("group", GROUPS)
def test_chunks_on_both_buffer_sets_name_the_lowest_bad_point(zk, group, monkeypatch):
    """13 points in chunks of 4: four chunks, the last of one point, so both buffer sets are used again and then drained"""
    rng = random.Random(13)
    mul_vec, fixed, nb = ops(zk, group)
    name = "zk_%s_mul_vec" % group
    pts = fixed([rng.randrange(1, RM) for _ in range(13)])
    k = [rng.randrange(RM) for _ in range(13)]
    whole = mul_vec(pts, k)                                             # one chunk
    monkeypatch.setenv("ZKHIP_PTAU_CONTRIB_CHUNK", "4")

    def off_curve(p, at):
        p[nb * at + nb // 2] ^= 1                                       # y changed

    # chunks 1 and 2, one per buffer set and both in flight; the last chunk alone, seen only in the final drain; chunks 2
    # and 3, both seen in the final drain, which runs oldest first
    for flipped, named in (((6, 9), 6), ((12,), 12), ((9, 12), 9)):
        bad = pts.copy()
        for at in flipped:
            off_curve(bad, at)
        with pytest.raises(zk.ZkHipError, match=r"%s: point %d is not on the curve" % (name, named)):
            mul_vec(bad, k)
    assert np.array_equal(mul_vec(pts, k), whole)
    # two kinds, one per buffer set
    bad = pts.copy()
    bad[nb * 6:nb * 6 + 32] = np.frombuffer(QM.to_bytes(32, "little"), np.uint8)                # a coordinate = q
    off_curve(bad, 9)
    with pytest.raises(zk.ZkHipError, match=r"%s: point 6 has a coordinate that is not below q" % name):
        mul_vec(bad, k)
    if group == "g2":
        p = golden_json("g2_cofactor_points.json")["outside"][0]
        bad = pts.copy()
        bad[128 * 5:128 * 6] = np.frombuffer(bn.g2_to_bytes(((int(p["x"][0]), int(p["x"][1])), (int(p["y"][0]), int(p["y"][1])))), np.uint8)
        off_curve(bad, 9)
        with pytest.raises(zk.ZkHipError, match=r"zk_g2_mul_vec: point 5 is not in the subgroup"):
            mul_vec(bad, k)


def test_a_g2_point_outside_the_subgroup_is_refused(zk):
    """on the twist, but the endomorphism is no multiplication by a constant there"""
    d = golden_json("g2_cofactor_points.json")
    dec = lambda p: bn.g2_to_bytes(((int(p["x"][0]), int(p["x"][1])), (int(p["y"][0]), int(p["y"][1]))))
    rng = random.Random(10)
    n = 67
    good = zk.fixed_base_g2(G2, [rng.randrange(1, RM) for _ in range(n)])
    k = [rng.randrange(RM) for _ in range(n)]
    for at, p in ((66, d["outside"][0]), (0, d["cofactor"][0]), (31, d["outside"][3])):
        pts = good.copy()
        pts[128 * at:128 * at + 128] = np.frombuffer(dec(p), np.uint8)
        with pytest.raises(zk.ZkHipError, match=r"zk_g2_mul_vec: point %d is not in the subgroup" % at):
            zk.g2_mul_vec(pts, k)
        with pytest.raises(zk.ZkHipError, match=r"zk_g2_power_scale: point %d is not in the subgroup" % at):
            zk.g2_power_scale(pts, 3)


@pytest.mark.parametrize("group", GROUPS)
def test_power_scale_against_the_operator(zk, group, monkeypatch):
    """n = 130 in chunks of 64: two full chunks and one of two points, the exponent running on across them"""
    monkeypatch.setenv("ZKHIP_PTAU_CONTRIB_CHUNK", "64")
    rng = random.Random(130)
    mul_vec, fixed, nb = ops(zk, group)
    power_scale = zk.g1_power_scale if group == "g1" else zk.g2_power_scale
    n = 130
    a = logs_for(n, rng)
    pts = fixed(a)
    for first_exp, factor in ((0, 1), (1, rng.randrange(1, RM)), ((1 << 20) - 3, RM - 1)):
        base = rng.randrange(2, RM)
        k = [factor * pow(base, first_exp + i, RM) % RM for i in range(n)]
        got = power_scale(pts, base, first_exp=first_exp, factor=factor)
        assert np.array_equal(got, mul_vec(pts, k)), first_exp
        assert np.array_equal(got, fixed([x * y % RM for x, y in zip(a, k)])), first_exp
    assert np.array_equal(power_scale(pts, 1), pts)                     # every scalar 1: the points themselves
    assert power_scale(np.zeros(0, np.uint8), 5).size == 0
    for kw in (dict(base=RM), dict(base=5, factor=RM)):
        with pytest.raises(zk.ZkHipError, match="not below r"):
            power_scale(pts, **kw)
