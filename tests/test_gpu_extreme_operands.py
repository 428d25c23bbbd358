"""GPU parity at the edges of the nine-limb arithmetic (csrc/field29.hpp): the transforms, the h pipeline, the 8 x 32 product
and the G1 operators on the input families of tests/extreme_inputs.py — constant vectors of r - 1 and of the word whose limbs
are all 2^29 - 1, masks, strides that keep every butterfly of a sub-transform adding equal values, their preimages, and curve
points whose X sits on full limbs, just below q and just above 0 — against the references the suite already trusts
(oracle/c_oracle.py, oracle/bn254.py).  Byte equality throughout; everything goes through the C ABI."""
import random

import numpy as np
import pytest

import extreme_inputs as xi
from oracle import bn254 as bn
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

R = bn.R_MOD


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def _assert_same(got, want, what):
    got, want = _u8(got), _u8(want)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got.reshape(-1, 32) != want.reshape(-1, 32)).any(axis=1))
        raise AssertionError("%s: %d of %d words differ, first at %d" % (what, bad.size, got.size // 32, int(bad[0])))


# ------------------------------------------------------------------------------------------------------------- a. zk.fr_ntt
# logn 3, 4, 5, 9, 10, 11: a single tile with window remainders 0, 1, 2; 12, 13: one strided pass of 1 and 2 bits; 14: the
# first full strided window; 17: two strided windows (NttPair::build / plan_windows, csrc/nttpair.hip)
@pytest.mark.parametrize("logn", [3, 4, 5, 9, 10, 11, 12, 13, 14, 17])
def test_ntt_every_family_both_directions(zk, logn):
    for name, x in xi.fr_families(logn):
        for inverse in (False, True):
            _assert_same(zk.fr_ntt(x, inverse=inverse), co.fr_fft(x, inverse=inverse), "%s, 2^%d, inverse=%s" % (name, logn, inverse))


# 22: an 11-bit outer pass of 512 threads; 23: two strided groups with the T2 table — shapes that do not exist below
@pytest.mark.parametrize("which", [0, 1, 2, 3])
@pytest.mark.parametrize("logn", [22, 23])
def test_ntt_large_plans(zk, logn, which):
    name, x = xi.big_size_inputs(logn)[which]
    for inverse in (False, True):
        _assert_same(zk.fr_ntt(x, inverse=inverse), co.fr_fft(x, inverse=inverse), "%s, 2^%d, inverse=%s" % (name, logn, inverse))


@pytest.mark.parametrize("n", [1, 2, 4])
def test_ntt_radix2_sizes(zk, n):
    """n = 1, 2, 4 go to k_ntt_pass (csrc/ntt.hip)."""
    for name, x in (("all_top", xi.all_top(n)), ("all_ones_limbs", xi.all_ones_limbs(n)), ("alternating", xi.alternating(n))):
        for inverse in (False, True):
            got = zk.fr_ntt(x, inverse=inverse)
            _assert_same(got, co.fr_fft(x, inverse=inverse), "%s, n=%d, inverse=%s" % (name, n, inverse))
            assert xi.unpack(got) == bn.ntt(xi.unpack(x), inverse=inverse)


def test_ntt_round_trip_on_the_device(zk):
    for name, x in xi.fr_families(14):
        _assert_same(zk.fr_ntt(zk.fr_ntt(x, inverse=False), inverse=True), x, "ifft(fft(%s))" % name)


# ---------------------------------------------------------------------------------------------------------- b. zk.fr_abc_to_h
def _abc_pairs(logn, constant_only=False):
    n = 1 << logn
    pairs = [("all_top,all_top", xi.all_top(n), xi.all_top(n)), ("all_ones_limbs,all_top", xi.all_ones_limbs(n), xi.all_top(n))]
    if not constant_only:
        pairs += [("mask01(1),mask01(2)", xi.mask01(n, 1), xi.mask01(n, 2)),
                  ("stride(3,top),alternating", xi.stride(n, 3, R - 1), xi.alternating(n)),
                  ("preimage(all_top),preimage(mask01(3))", xi.preimage(xi.all_top(n)), xi.preimage(xi.mask01(n, 3)))]
    return pairs


def _check_h(zk, logn, pairs):
    from test_gpu_field_ntt import abc_to_h_reference, coset_powers
    n = 1 << logn
    rng = np.random.default_rng(7700 + logn)
    pw = coset_powers(logn)
    rinv = pow(bn.MONT_R, -1, R)
    nonzero = 0
    for name, a, b in pairs:
        ab, ce = abc_to_h_reference(a, b, logn, pw)
        got = _u8(zk.fr_abc_to_h(a, b))
        idx = range(n) if logn <= 14 else sorted(set(int(i) for i in rng.choice(n, 4096, replace=False)) | {0, 1, n - 1, n // 2, 2047, 2048})
        assert len(idx) >= min(n, 4096)                             # all positions up to 2^14, 4096 distinct sampled ones above
        for i in idx:
            x = int.from_bytes(ab[32 * i:32 * i + 32].tobytes(), "little")
            z = int.from_bytes(ce[32 * i:32 * i + 32].tobytes(), "little")
            want = (x - z) * rinv % R
            assert int.from_bytes(got[32 * i:32 * i + 32].tobytes(), "little") == want, (name, logn, i)
            nonzero += want != 0
        if name.split(",")[0] in ("all_top", "all_ones_limbs"):   # constant a and b: a.b - c vanishes on the whole coset
            assert not got.any(), (name, logn)
    return nonzero


@pytest.mark.parametrize("logn", [3, 5, 11, 12, 14, 17])
def test_abc_to_h_extreme_pairs(zk, logn):
    assert _check_h(zk, logn, _abc_pairs(logn)) > 0                 # the constant pairs (h = 0) are not the only case


@pytest.mark.parametrize("pair", [0, 1])
def test_abc_to_h_constant_pairs_at_2p22(zk, pair):
    """2^22 (the 11-bit outer pass): the two constant pairs only; the expected h is identically zero, checked at the sampled
    positions against the restatement and everywhere against zero.  The random pair of
    test_abc_to_h_against_the_c_restatement_at_every_pass_plan[22] is the non-zero case of this size."""
    _check_h(zk, 22, [_abc_pairs(22, constant_only=True)[pair]])


# ------------------------------------------------------------------------------------------- c. zk.fr_mul_vec / zk.fq_mul_vec
@pytest.mark.parametrize("field,p", [("fr", bn.R_MOD), ("fq", bn.Q_MOD)])
def test_mont_mul_edge_cross_product(zk, field, p):
    """The 8 x 32 CIOS product of csrc/field.hpp (what the pairing kernels are built on) over EDGE_FIELD x EDGE_FIELD."""
    a, b, want = xi.edge_cross_product(p)
    fn = zk.fr_mul_vec if field == "fr" else zk.fq_mul_vec
    got = xi.unpack(fn(a, b))
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    e = xi.EDGE_FIELD(p)
    assert not bad, "a = %#x, b = %#x" % (e[bad[0] // len(e)], e[bad[0] % len(e)])


# ------------------------------------------------------------------------------------------- d. G1 with extreme coordinates
_CACHE = {}


def _extreme_bytes():
    if "ext" not in _CACHE:
        _CACHE["ext"] = xi.extreme_g1_points(24)
    return _CACHE["ext"]


def _bases_5000():
    """5000 bases: every fifth an extreme point, cycled through; the rest from test_gpu_msm's chain."""
    if "bases" not in _CACHE:
        from test_gpu_msm import _chain_points
        n = 5000
        pts, _, _ = _chain_points(n, 4321)
        rows = [bn.g1_to_bytes(P) for P in pts]
        ext = _extreme_bytes()
        for j, i in enumerate(range(0, n, 5)):
            rows[i] = ext[j % len(ext)]
        _CACHE["bases"] = b"".join(rows)
    return _CACHE["bases"]


def test_msm_g1_extreme_points_mixed_scalars(zk):
    """The 24 extreme points and their negatives (every point twice: the set is closed under negation), scalars 0, 1, r - 1, r,
    2^256 - 1 and random ones, against the C restatement and the Python oracle."""
    ext = xi.extreme_g1(24)
    pts = [P for _, _, P in ext] + [bn.G1.neg(P) for _, _, P in ext]
    ks = xi.mixed_scalars(48)
    assert ks[:40] == xi.mixed_scalars(40)
    bases = b"".join(bn.g1_to_bytes(P) for P in pts)
    sc = xi.scalars_bytes(ks)
    got = zk.msm_g1(bases, sc)
    assert got == co.msm_g1(bases, sc)
    want = None
    for P, k in zip(pts, ks):
        want = bn.G1.add(want, bn.G1.mul(P, k))
    assert got == bn.g1_to_bytes(want)


def test_msm_g1_sorted_path_with_extreme_points(zk):
    """n = 5000 (the sorted path: every kernel of the pipeline): 1000 of the bases are the 24 extreme points over and over, so
    inside a bucket an extreme point meets itself (the doubling branch) and its negative (the branch to infinity), both on top
    of maximal limbs.  Random scalars, every seventh in {0, 1, 2, r - 1}."""
    n = 5000
    bases = _bases_5000()
    rng = random.Random(5000)
    ks = [rng.choice([0, 1, 2, R - 1]) if i % 7 == 0 else rng.randrange(R) for i in range(n)]
    sc = xi.scalars_bytes(ks)
    assert zk.msm_g1(bases, sc) == co.msm_g1(bases, sc)


def test_msm_g1_sorted_path_all_scalars_one(zk):
    """The same 5000 bases, each scalar 1: one bucket, in which every extreme point and its negative occur ~42 times each; the
    expected value is the plain sum of the points."""
    n = 5000
    bases = _bases_5000()
    sc = xi.scalars_bytes([1] * n)
    got = zk.msm_g1(bases, sc)
    assert got == co.msm_g1(bases, sc)
    assert got != bytes(64)


def _six_scalars():
    rng = random.Random(66)
    return [1, 2, R - 1] + [rng.randrange(R) for _ in range(3)]


def test_fixed_base_and_host_mul_with_extreme_bases(zk):
    ks = _six_scalars()
    for i, base in enumerate(_extreme_bytes()):
        want = b"".join(co.g1_mul(base, k) for k in ks)
        assert zk.fixed_base_g1(base, ks).tobytes() == want, i
        assert b"".join(zk.g1_mul(base, k) for k in ks) == want, i


def test_g1_mul_vec_with_extreme_points(zk):
    ext = _extreme_bytes()
    ks = _six_scalars()
    pts = [P for P in ext for _ in ks]
    sc = [k for _ in ext for k in ks]
    want = b"".join(co.g1_mul(P, k) for P, k in zip(pts, sc))
    assert zk.g1_mul_vec(b"".join(pts), sc).tobytes() == want


def test_g1_scale_with_extreme_points(zk):
    """The extreme points stand among ordinary ones (an odd count: not a multiple of any block)."""
    ext = _extreme_bytes()
    gen = bn.g1_to_bytes(bn.G1.gen)
    pts = []
    for i, P in enumerate(ext):
        pts += [P, co.g1_mul(gen, 1000 + i)]
    pts.append(gen)
    for k in _six_scalars():
        want = b"".join(co.g1_mul(P, k) for P in pts)
        assert zk.g1_scale(b"".join(pts), k).tobytes() == want, k


def test_prover_with_extreme_points_in_the_a_and_b1_tables(zk):
    """The smallest synthetic key of test_gpu_synth.py (k = 10) with every fifth row of the A and B1 tables an extreme point
    (a workload is a dict of arrays: the caller owns the tables), witness entries at those rows 1, 2, r - 1 in turn: the five MSM
    sums and the proof against the C restatement, as test_synthetic_prove_bit_exact_vs_c_oracle."""
    import torch
    from rapidsnark_old_amd import synth
    from test_gpu_synth import _prover
    k = 10
    wl = dict(co.synth_workload(k))
    ext = np.stack([_u8(P) for P in _extreme_bytes()])
    for j, name in enumerate(("pointsA", "pointsB1")):
        t = np.array(wl[name]).reshape(-1, 64)
        rows = np.arange(j, t.shape[0], 5)
        t[rows] = ext[(np.arange(rows.size) + 7 * j) % ext.shape[0]]
        wl[name] = t.reshape(-1)
    w = synth.make_witness(k, seed=3).copy().reshape(-1, 32)
    for i in range(5, w.shape[0] - 1, 5):                           # rows 5, 10, ... of A and 6, 11, ... of B1 hold extreme points
        w[i] = xi.word_bytes((1, 2, R - 1)[(i // 5) % 3])
        w[i + 1] = xi.word_bytes((R - 1, 1, 2)[(i // 5) % 3])
    w = w.reshape(-1)
    view = co.ZkeyView(wl)
    p = _prover(zk, wl)
    wd = torch.from_numpy(w).to("cuda:0")
    r, s = 0xabcdef0123456789, (1 << 247) + 12345
    assert p.prove_msm_dev(wd.data_ptr()) == co.prove_msm(view, w)
    assert p.prove_dev(wd.data_ptr(), r, s) == co.prove(view, w, r, s)
    p.lib.zk_prover_destroy(p.h)
