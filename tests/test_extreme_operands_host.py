"""The extreme-operand families of tests/extreme_inputs.py are what they claim to be, and the two references the GPU tests
trust (oracle/bn254.py in Python integers, oracle/c_oracle.py in C) agree on all of them.  No GPU: a disagreement here is a
finding about an oracle, to be settled before tests/test_gpu_extreme_operands.py means anything."""
import numpy as np
import pytest

import extreme_inputs as xi
from oracle import bn254 as bn
from oracle import c_oracle as co

R, Q = bn.R_MOD, bn.Q_MOD


def test_t_max_is_the_all_ones_limb_value_below_both_primes():
    assert xi.T_MAX == 3171406 * (1 << 232) - 1
    assert xi.T_MAX < R and xi.T_MAX < Q
    assert xi.limbs29(xi.T_MAX) == [(1 << 29) - 1] * 8 + [3171405]
    for p, w in ((R, xi.T_MAX_WORD_FR), (Q, xi.T_MAX_WORD_FQ)):
        assert 0 <= w < p and w * 32 % p == xi.T_MAX
        assert xi.limbs29(p)[8] == 3171406 and all(xi.limbs29(p)[:8])
        # the one product of the conversion leaves T_MAX itself, not T_MAX + p: the limbs the kernels start from
        assert xi.internal_limbs(w, p) == xi.limbs29(xi.T_MAX)
        # r - 1 and q - 1 as words: internal value p - 32
        assert xi.internal_value(p - 1, p) == p - 32


def test_fr_families_are_what_they_claim():
    n = 64
    assert xi.unpack(xi.all_top(n)) == [R - 1] * n
    assert [v * 32 % R for v in xi.unpack(xi.all_ones_limbs(n))] == [xi.T_MAX] * n
    m = xi.unpack(xi.mask01(n, 5))
    assert set(m) == {0, R - 1} and m == xi.unpack(xi.mask01(n, 5)) and m != xi.unpack(xi.mask01(n, 6))
    assert xi.unpack(xi.alternating(n)) == [R - 1, 1] * (n // 2)
    assert xi.unpack(xi.alternating(1)) == [R - 1]
    for s in (1, 3, 6):
        assert xi.unpack(xi.stride(n, s, 7)) == [7 if i % (1 << s) == 0 else 0 for i in range(n)]
    names = [name for name, _ in xi.fr_families(14)]
    assert len(names) == len(set(names)) == 2 * (4 + 2 * 5)
    assert [name for name, _ in xi.fr_families(5, preimages=False)] == ["all_top", "all_ones_limbs", "mask01", "alternating", "stride(1,top)",
                                                                        "stride(1,tmax)", "stride(3,top)", "stride(3,tmax)"]
    for name, x in xi.fr_families(12) + xi.big_size_inputs(13):
        assert x.dtype == np.uint8 and x.size % 32 == 0, name
        assert max(xi.unpack(x)) < R, name


def test_fr_families_are_built_without_a_loop_over_n():
    import time
    n = 1 << 23
    for make in (xi.all_top, xi.all_ones_limbs, xi.alternating, lambda k: xi.mask01(k, 1), lambda k: xi.stride(k, 11, R - 1),
                 lambda k: xi.stride(k, 12, xi.T_MAX_WORD_FR)):
        t0 = time.perf_counter()
        x = make(n)
        dt = time.perf_counter() - t0
        assert x.size == 32 * n and x.dtype == np.uint8
        assert dt < 2.0, dt                         # 2^23 words: a loop over n in Python takes far longer than this
        del x


@pytest.mark.parametrize("n", [8, 64, 2048])
def test_c_restatement_and_python_oracle_agree_on_every_fr_family(n):
    logn = n.bit_length() - 1
    for name, x in xi.fr_families(logn):
        v = xi.unpack(x)
        for inverse in (False, True):
            got = xi.unpack(co.fr_fft(x, inverse=inverse))
            assert got == bn.ntt(v, inverse=inverse), (name, inverse)
        if name.startswith("preimage("):
            continue
        fwd = xi.unpack(co.fr_fft(x))
        if name in ("all_top", "all_ones_limbs"):            # fft of a constant c is (n c, 0, ..., 0)
            assert fwd == [n * v[0] % R] + [0] * (n - 1), name
        if name == "alternating":                            # a, b, a, b, ...: n/2 (a + b) at 0, n/2 (a - b) at n/2
            want = [0] * n
            want[0], want[n // 2] = n // 2 * (v[0] + v[1]) % R, n // 2 * (v[0] - v[1]) % R
            assert fwd == want
        if name.startswith("stride("):                       # v at the multiples of 2^s: v n / 2^s at the multiples of n / 2^s
            s = int(name[7:].split(",")[0])
            assert fwd == [(n >> s) * v[0] % R if k % (n >> s) == 0 else 0 for k in range(n)], name
    # the preimage really is one: fft(preimage(y)) == y
    y = xi.mask01(n, 9)
    assert co.fr_fft(xi.preimage(y)) == y.tobytes()


def test_extreme_g1_points_are_on_the_curve_with_the_intended_x():
    pts = xi.extreme_g1(24)
    assert len(pts) == 24 and len({P for _, _, P in pts}) == 24
    assert [k for k, _, _ in pts] == ["full_limbs"] * 8 + ["below_q"] * 8 + ["above_zero"] * 8
    for i, (kind, t, P) in enumerate(pts):
        assert bn.G1.is_on_curve(P) and P[1] != 0
        b = bn.g1_to_bytes(P)
        assert int.from_bytes(b[:32], "little") * 32 % Q == t
        if kind == "full_limbs":
            assert xi.limbs29(t)[:8] == [(1 << 29) - 1] * 8 and 3171406 - 64 < xi.limbs29(t)[8] < 3171406
            assert xi.internal_limbs(int.from_bytes(b[:32], "little"), Q) == xi.limbs29(t)
        elif kind == "below_q":
            assert 0 < Q - t < 64
        else:
            assert 0 < t < 64
        if i % 2:
            assert P == bn.G1.neg(pts[i - 1][2])
    assert xi.extreme_g1_points(24) == [bn.g1_to_bytes(P) for _, _, P in pts]


def test_c_restatement_and_python_oracle_agree_on_the_extreme_msm():
    n = 40
    ext = xi.extreme_g1(24)
    pts = [ext[i % 24][2] for i in range(n)]
    ks = xi.mixed_scalars(n)
    for k in (0, 1, R - 1, R, (1 << 256) - 1):
        assert k in ks
    want = None
    for P, k in zip(pts, ks):
        want = bn.G1.add(want, bn.G1.mul(P, k))
    got = co.msm_g1(b"".join(bn.g1_to_bytes(P) for P in pts), xi.scalars_bytes(ks))
    assert got == bn.g1_to_bytes(want)
    # every point alone, with the scalars the device tests use
    for _, _, P in ext:
        for k in (1, 2, R - 1):
            assert co.g1_mul(bn.g1_to_bytes(P), k) == bn.g1_to_bytes(bn.G1.mul(P, k))


@pytest.mark.parametrize("field,p", [("fr", R), ("fq", Q)])
def test_c_restatement_product_on_the_edge_cross_product(field, p):
    e = xi.EDGE_FIELD(p)
    assert len(e) == len(set(e)) == 17
    a, b, want = xi.edge_cross_product(p)
    assert a.size == b.size == 32 * 17 * 17
    fn = co.fr_mul_vec if field == "fr" else co.fq_mul_vec
    assert xi.unpack(fn(a, b)) == want
