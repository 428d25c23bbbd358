"""GPU parity of the G2 operators at the edges of the nine-limb arithmetic: the lane-pair mixed addition of csrc/curve29.hpp
(madd(XYZZ<Fq2s>&, ...): k_msm_accum_l1_g2s and, through LaneModel<Fq2>, every merge and reduction kernel), the table kernels'
madd(XYZZ<Fq2r>&, ...) (k_precomp_walk) and the 8 x 32-bit G2 code of the fixed-base, chain and Lagrange operators, on the G2
families of tests/extreme_inputs.py — x components on full limbs, just below q and just above 0 in every pairing, points and
differences of points with exactly one zero component — against oracle/c_oracle.py (byte equality; the tiny cases against
oracle/bn254.py as well).  Everything goes through the C ABI wrappers of lib.py.

The families lie on the twist but OUTSIDE its order-r subgroup (the cofactor is about q; tests/test_extreme_operands_host.py
checks [r]P != infinity).  The group law holds for them, but k P depends on k and not on k mod r, so they go only to entry
points that take the scalar as a plain integer, and only with scalars below r (extreme_inputs.g2_scalars_below_r):
  zk_msm_g2           checks nothing; a scalar at or above r is reduced by subtracting r (msm_sort.hip), one below r is recoded
                      into signed digits whose sum is the scalar itself — as the unsigned digits of oracle_msm_g2
  zk_prover_create /  the prover checks no point; witness values are below r and go through the same digits, the precomputed
  zk_prove*           rows are 2^(c j) P by doubling
  zk_fixed_base_g2    plain double-and-add over the 256 raw bits
  zk_synth_chain_g2   P0 + i Q by additions
  zk_g2_lagrange      checks the curve, not the subgroup; every twiddle and 1 / n is a standard-form value below r read bit by bit
  zk_g2_mul           (host code) plain double-and-add
Deliberately left out, they get no extreme point:
  zk_g2_mul_vec, zk_g2_power_scale    split the scalar by the endomorphism (glv.hpp, mulglv.hpp), which is a multiplication by
                                      a constant only inside the subgroup; they test the subgroup first and refuse these points
  zk_g2_power_msm                     makes its scalars s^i on the device as products reduced mod r
  zk_g2_in_subgroup                   IS the subgroup test; tests/test_gpu_ptau_check.py feeds it points outside the subgroup
  zk_pairing, zk_verify*, zk_vkey_*   refuse a G2 point outside the subgroup (and a pairing is not defined on one)
  zk_kzg_*, zk_ptau_check, zk_ptau_contribute, zk_zkey_verify, zk_zkey_contribute
                                      check the subgroup of every G2 point they read, or multiply through the GLV lanes
  zk_setup / zkeynew                  take no G2 point from the caller but the .ptau's, which zk_ptau_check vouches for"""
import random

import numpy as np
import pytest

import extreme_inputs as xi
from oracle import bn254 as bn
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

R = bn.R_MOD
G2 = bn.G2
# 2^64 - 1: every window width c <= 64 sees low bits 2^c - 1 >= 2^(c-1), a NEGATIVE signed digit (-1, carry 1: the carry runs
# through the all-ones windows, which become empty, and ends as one positive digit at bit 64) — below r, as every scalar here
NEG_LOW_DIGIT = (1 << 64) - 1
COMMON_SCALARS = (1, NEG_LOW_DIGIT)
assert all(0 < k < R for k in COMMON_SCALARS)            # the points below are outside the subgroup: see the module docstring

_CACHE = {}


def _families():
    """(extreme points, half-zero pairs, zero-component points), built once."""
    if "fam" not in _CACHE:
        ext = xi.extreme_g2(32)
        pairs, points = xi.half_zero_g2()
        _CACHE["fam"] = (ext, pairs, points)
    return _CACHE["fam"]


def _singles():
    """Every extreme point (negatives included) and every zero-component point with its negative: (name, P)."""
    ext, _, points = _families()
    out = [("%s#%d" % (kind, i), P) for i, (kind, _, P) in enumerate(ext)]
    for shape, P in points:
        out += [(shape, P), (shape + "-", G2.neg(P))]
    return out


def _msm(zk, pts, ks):
    """zk.msm_g2 and the C restatement on the same bytes -> the device's bytes, after asserting the two agree."""
    assert all(0 <= k < R for k in ks)                    # never at or above r on these points: see the module docstring
    bases = b"".join(bn.g2_to_bytes(P) for P in pts)
    sc = xi.scalars_bytes(ks)
    got = zk.msm_g2(bases, sc)
    assert got == co.msm_g2(bases, sc), "device and C restatement differ"
    return got


def _times(P, k):
    return bn.g2_to_bytes(G2.mul(P, k)) if P is not None else bytes(128)


# ------------------------------------------------------------------------------ a. tiny MSMs: one bucket, two or three points
# n = 2 or 3 with one common scalar is one bucket per non-empty window: a fresh affine accumulator (zz = 1) meets the second
# point, through the whole sort, level-1, merge and reduce pipeline of msm_generic
@pytest.mark.parametrize("k", COMMON_SCALARS)
def test_tiny_msm_half_zero_pairs_in_both_orders(zk, k):
    """P = U2 - x with exactly one zero component (shapes a, b), R = 0 with P != 0 and R = -2y (c, c-): a pair predicate that
    ORed its two lanes would take the doubling branch or the branch to infinity here."""
    _, pairs, _ = _families()
    for shape, P1, P2 in pairs:
        want = _times(G2.add(P1, P2), k)
        assert want != bytes(128)
        for a, b in ((P1, P2), (P2, P1)):
            assert _msm(zk, [a, b], [k, k]) == want, shape


@pytest.mark.parametrize("k", COMMON_SCALARS)
def test_tiny_msm_point_and_its_negative(zk, k):
    """P, -P gives infinity (for a y with a zero component, shape d: P = 0 and R = -2y half zero), and P, -P, P2 gives P2: the
    state after the branch to infinity.  On every extreme point and every zero-component point."""
    _, pairs, _ = _families()
    singles = _singles()
    for i, (name, P) in enumerate(singles):
        assert _msm(zk, [P, G2.neg(P)], [k, k]) == bytes(128), name
        P2 = singles[(i + 5) % len(singles)][1] if i % 2 else pairs[i % len(pairs)][2]
        assert P2 not in (P, G2.neg(P))
        assert _msm(zk, [P, G2.neg(P), P2], [k, k, k]) == _times(P2, k), name


@pytest.mark.parametrize("k", COMMON_SCALARS)
def test_tiny_msm_doubling_branch(zk, k):
    """P, P: the doubling branch on every extreme point and every zero-component point (shapes d, e); with the negative low
    digit neg_lazy runs on the y of the point first."""
    for name, P in _singles():
        assert _msm(zk, [P, P], [k, k]) == _times(G2.dbl(P), k), name
        assert _msm(zk, [P, P, P], [k, k, k]) == _times(G2.add(G2.dbl(P), P), k), name


# ------------------------------------------------------------------------------------------- b. the extreme set, many buckets
def test_msm_g2_extreme_points_scalars_below_r(zk):
    """The 32 extreme points and their negatives with 0, 1, 2, r - 1, r - 2 and random scalars below r: most buckets hold one
    point, so the extreme coordinates reach the general additions of the merge and reduction kernels with zz = 1."""
    ext, _, _ = _families()
    pts = [P for _, _, P in ext] + [G2.neg(P) for _, _, P in ext]
    ks = xi.g2_scalars_below_r(64)
    got = _msm(zk, pts, ks)
    assert got != bytes(128)
    _, pairs, points = _families()
    more = [P for _, P1, P2 in pairs for P in (P1, P2)] + [P for _, P in points] + [G2.neg(P) for _, P in points]
    assert _msm(zk, more, xi.g2_scalars_below_r(len(more), seed=43)) != bytes(128)


# ---------------------------------------------------------------------------------------------------- c. n = 2048, long buckets
def _bases_2048():
    """2048 bases: the chain of test_msm_g2_known_dlog, every fourth base an extreme, half-zero or zero-component point (with
    their negatives), cycled.  -> (points, pool)"""
    if "bases" not in _CACHE:
        n = 2048
        rng = random.Random(2048)
        a, d = rng.randrange(1, R), rng.randrange(1, R)
        P, D = G2.mul(G2.gen, a), G2.mul(G2.gen, d)
        pts = []
        for _ in range(n):
            pts.append(P)
            P = G2.add(P, D)
        ext, pairs, points = _families()
        pool = [Q for _, _, Q in ext]
        for _, P1, P2 in pairs:
            pool += [P1, P2, G2.neg(P1), G2.neg(P2)]
        for _, Q in points:
            pool += [Q, G2.neg(Q)]
        assert len(pool) < n // 8                           # every one of them several times
        for j, i in enumerate(range(0, n, 4)):
            pts[i] = pool[j % len(pool)]
        _CACHE["bases"] = (pts, pool)
    return _CACHE["bases"]


def test_msm_g2_2048_with_extreme_bases(zk):
    """Random scalars below r, every seventh in {0, 1, 2, r - 1}: k_msm_accum_pair and the wave-level merges with G2 partials."""
    pts, _ = _bases_2048()
    rng = random.Random(2049)
    ks = [rng.choice([0, 1, 2, R - 1]) if i % 7 == 0 else rng.randrange(R) for i in range(len(pts))]
    assert _msm(zk, pts, ks) != bytes(128)


def test_msm_g2_2048_all_scalars_one(zk):
    """The same bases, every scalar 1: one long bucket cut by many chunk edges, in which every extreme point meets itself and
    its negative.  The expected value is the plain sum of the points, and it is not infinity."""
    pts, pool = _bases_2048()
    want = None
    for P in pts:
        want = G2.add(want, P)
    assert want is not None
    got = _msm(zk, pts, [1] * len(pts))
    assert got == bn.g2_to_bytes(want)
    # the special points alone: each one beside its negative several times over — the sum is infinity
    closed = pool + [G2.neg(P) for P in pool]
    assert _msm(zk, closed * 3, [1] * (3 * len(closed))) == bytes(128)


# ------------------------------------------------------------------------------------------------------------- d. the prover
@pytest.mark.parametrize("precomp", [False, True, 2])
def test_prover_with_extreme_points_in_the_a_b1_and_b2_tables(zk, precomp):
    """The k = 10 synthetic key of test_gpu_synth.py with every fifth row of pointsB2 an extreme G2 point and, as in
    test_prover_with_extreme_points_in_the_a_and_b1_tables, of A and B1 an extreme G1 point; witness values at those rows 1, 2
    and r - 1 in turn.  Plain tables run the lane-pair madd; the precomputed tables send the extreme G2 points through
    k_precomp_walk (the Fq2r madd), the HALF variant through the second bucket set as well."""
    import torch
    from rapidsnark_old_amd import synth
    from test_gpu_synth import _prover
    k = 10
    wl = dict(co.synth_workload(k))
    ext1 = np.stack([np.frombuffer(P, dtype=np.uint8) for P in xi.extreme_g1_points(24)])
    ext2 = np.stack([np.frombuffer(P, dtype=np.uint8) for P in xi.extreme_g2_points(32)])
    for j, (name, ext, nb) in enumerate((("pointsA", ext1, 64), ("pointsB1", ext1, 64), ("pointsB2", ext2, 128))):
        t = np.array(wl[name]).reshape(-1, nb)
        rows = np.arange(j, t.shape[0], 5)
        t[rows] = ext[(np.arange(rows.size) + 7 * j) % ext.shape[0]]
        wl[name] = t.reshape(-1)
    w = synth.make_witness(k, seed=3).copy().reshape(-1, 32)
    for i in range(5, w.shape[0] - 2, 5):                           # rows 5, 10, ... of A, 6, 11, ... of B1, 7, 12, ... of B2
        for j in range(3):
            v = (1, 2, R - 1)[(i // 5 + j) % 3]
            assert v < R
            w[i + j] = xi.word_bytes(v)
    w = w.reshape(-1)
    view = co.ZkeyView(wl)
    p = _prover(zk, wl, precomp=precomp)
    wd = torch.from_numpy(w).to("cuda:0")
    r, s = 0xabcdef0123456789, (1 << 247) + 12345
    try:
        assert p.prove_msm_dev(wd.data_ptr()) == co.prove_msm(view, w)
        assert p.prove_dev(wd.data_ptr(), r, s) == co.prove(view, w, r, s)
        assert p.info()["precomputed_tables"] == int(precomp)          # the table mode asked for is the one that ran
    finally:
        p.lib.zk_prover_destroy(p.h)


# ------------------------------------------------------------------- e. the other G2 entry points (8 x 32-bit field, field.hpp)
def _some_bases():
    """One extreme point of each kind, a point of each zero-component shape and the generator: (name, bytes)."""
    ext, _, points = _families()
    seen, out = set(), []
    for kind, _, P in ext:
        if kind not in seen:
            seen.add(kind)
            out.append((kind, P))
    out += [(shape, P) for shape, P in points[::2]]
    out.append(("generator", G2.gen))
    return out


def test_fixed_base_g2_and_host_mul_with_extreme_bases(zk):
    rng = random.Random(67)
    ks = [0, 1, 2, R - 1, R - 2] + [rng.randrange(R) for _ in range(3)]
    assert max(ks) < R
    for name, P in _some_bases():
        base = bn.g2_to_bytes(P)
        want = b"".join(bn.g2_to_bytes(G2.mul(P, k)) for k in ks)
        assert b"".join(co.g2_mul(base, k) for k in ks) == want, name
        assert zk.fixed_base_g2(base, ks).tobytes() == want, name
        assert b"".join(zk.g2_mul(base, k) for k in ks) == want, name


def test_synth_chain_g2_with_extreme_ends(zk):
    """P0 + i Q with an extreme start, an extreme step and both (n = 130: three segments of the walk, the last one short)."""
    bases = _some_bases()
    gen = bn.g2_to_bytes(G2.gen)
    ordinary = co.g2_mul(gen, 7654321)
    for i, (name, P) in enumerate(bases[:-1]):
        e = bn.g2_to_bytes(P)
        other = bn.g2_to_bytes(bases[(i + 1) % (len(bases) - 1)][1])
        for p0, q in ((e, ordinary), (ordinary, e), (e, other)):
            assert zk.synth_chain_g2(130, p0, q).tobytes() == co.chainp_g2(130, p0, q).tobytes(), name


def test_g2_lagrange_with_extreme_points(zk):
    """log_n = 5 against the big-integer inverse DFT of test_gpu_ptau_prepare.py: every third input an extreme, half-zero or
    zero-component point, among ordinary ones."""
    from test_gpu_ptau_prepare import run_op
    ext, pairs, points = _families()
    special = [P for _, _, P in ext[::3]] + [pairs[0][1], pairs[0][2], pairs[4][1], pairs[4][2]] + [P for _, P in points[::2]]
    rng = random.Random(55)
    pts = [G2.mul(G2.gen, rng.randrange(1, R)) for _ in range(32)]
    for j, i in enumerate(range(0, 32, 3)):
        pts[i] = special[j % len(special)]
    run_op(zk, "g2", pts, 5)
