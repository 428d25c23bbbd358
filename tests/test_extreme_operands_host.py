"""The extreme-operand families of tests/extreme_inputs.py are what they claim to be, and the two references the GPU tests
trust (oracle/bn254.py in Python integers, oracle/c_oracle.py in C) agree on all of them.  No GPU: a disagreement here is a
finding about an oracle, to be settled before tests/test_gpu_extreme_operands.py and tests/test_gpu_extreme_operands_g2.py mean
anything."""
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


def test_f2_sqrt_and_f2_cbrt():
    import random
    rng = random.Random(2)
    roots = cubes = 0
    for i in range(40):
        a = (rng.randrange(Q), rng.randrange(Q) if i % 4 else 0)
        for x in ((a[0], a[1]), bn.f2_mul(a, a), xi.f2_pow(a, 3)):
            s, c = xi.f2_sqrt(x), xi.f2_cbrt(x)
            assert s is None or bn.f2_mul(s, s) == x
            assert c is None or xi.f2_pow(c, 3) == x
            roots += s is not None
            cubes += c is not None
        assert xi.f2_sqrt(bn.f2_mul(a, a)) in (a, bn.f2_neg(a))
        assert xi.f2_cbrt(xi.f2_pow(a, 3)) is not None
    assert 40 < roots < 120 and 40 < cubes < 120          # squares and cubes are found, non-squares and non-cubes refused
    assert xi.f2_sqrt((Q - 4, 0)) in ((0, 2), (0, Q - 2))   # -4 = (2u)^2
    # an element is a square iff its (q^2 - 1) / 2-th power is 1: None exactly for the others
    for i in range(1, 12):
        assert (xi.f2_sqrt((i, 1)) is None) == (xi.f2_pow((i, 1), (Q * Q - 1) // 2) != bn.F2_ONE)


def test_extreme_g2_points_are_on_the_twist_with_the_intended_x():
    pts = xi.extreme_g2(32)
    assert len(pts) == 32 and len({P for _, _, P in pts}) == 32
    kinds = [k for k, _, _ in pts]
    assert set(kinds) == {a + "/" + b for a in ("full_limbs", "below_q", "above_zero") for b in ("full_limbs", "below_q", "above_zero")}
    assert all(kinds.count(k) in (2, 4) for k in kinds)
    for i, (kind, t, P) in enumerate(pts):
        assert bn.G2.is_on_curve(P) and P[1] != bn.F2_ZERO
        b = bn.g2_to_bytes(P)
        words = [int.from_bytes(b[32 * j:32 * j + 32], "little") for j in range(2)]
        assert tuple(w * 32 % Q for w in words) == t == xi.g2_internal_x(P)
        for comp_kind, tc, w in zip(kind.split("/"), t, words):
            if comp_kind == "full_limbs":
                assert xi.limbs29(tc)[:8] == [(1 << 29) - 1] * 8 and 3171406 - 64 < xi.limbs29(tc)[8] < 3171406
                assert xi.internal_limbs(w, Q) == xi.limbs29(tc)
            elif comp_kind == "below_q":
                assert 0 < Q - tc < 64
            else:
                assert 0 < tc < 64
        if i % 2:
            assert P == bn.G2.neg(pts[i - 1][2])
    assert xi.extreme_g2_points(32) == [bn.g2_to_bytes(P) for _, _, P in pts]


def test_extreme_g2_points_are_outside_the_order_r_subgroup():
    """Why the G2 families go only to operators that take the scalar as a plain integer, with scalars below r."""
    ext = xi.extreme_g2(32)
    pairs, points = xi.half_zero_g2()
    for P in (ext[0][2], ext[18][2], pairs[0][1], points[0][1]):
        assert bn.G2.mul(P, R) is not None
    assert bn.G2.mul(bn.G2.gen, R) is None
    ks = xi.g2_scalars_below_r(300)
    assert ks[:5] == [0, 1, 2, R - 1, R - 2] and len(ks) == 300 and max(ks) < R and len(set(ks)) == 300
    assert xi.g2_scalars_below_r(3) == [0, 1, 2]


def test_half_zero_g2_shapes_are_what_they_claim():
    pairs, points = xi.half_zero_g2()
    assert sorted({s for s, _, _ in pairs}) == ["a", "b", "c", "c-"] and len(pairs) == 12
    assert sorted({s for s, _ in points}) == ["d_im", "d_re", "e_im", "e_re"] and len(points) == 8
    beta = xi._fq_beta()
    assert beta != 1 and pow(beta, 3, Q) == 1
    for shape, P1, P2 in pairs:
        assert bn.G2.is_on_curve(P1) and bn.G2.is_on_curve(P2) and P1 != P2
        dx, dy = bn.f2_sub(P2[0], P1[0]), bn.f2_sub(P2[1], P1[1])
        # the kernels hold x * 2^261: a component is zero there exactly when it is zero here
        ix = bn.f2_sub(xi.g2_internal_x(P2), xi.g2_internal_x(P1))
        assert [v == 0 for v in ix] == [v == 0 for v in dx]
        if shape == "a":
            assert dx[0] == 0 and dx[1] != 0
        elif shape == "b":
            assert dx[0] != 0 and dx[1] == 0
        else:
            assert P2[0] == bn.f2_scalar(P1[0], beta) and dx[0] != 0 and dx[1] != 0
            assert dy == bn.F2_ZERO if shape == "c" else dy == bn.f2_neg(bn.f2_scalar(P1[1], 2))
        if shape in ("a", "b"):
            assert dy[0] != 0 and dy[1] != 0
    for shape, P in points:
        assert bn.G2.is_on_curve(P)
        (xa, xb), (ya, yb) = P
        zero = {"d_re": yb, "d_im": ya, "e_re": xb, "e_im": xa}[shape]
        rest = [v for v in (xa, xb, ya, yb)]
        assert zero == 0 and rest.count(0) == 1
        if shape.startswith("d"):                            # P and -P: P = 0 and R = -2y with exactly one zero component
            r = bn.f2_sub(bn.G2.neg(P)[1], P[1])
            assert (r[0] == 0) != (r[1] == 0)


def _g2_host_set():
    """16 points: two of each mixed kind, the half-zero pairs of every shape and a point of each zero-component shape."""
    ext = xi.extreme_g2(32)
    pairs, points = xi.half_zero_g2()
    pts = [ext[i][2] for i in (0, 5, 8, 13, 16, 22, 28, 31)]
    pts += [pairs[0][1], pairs[0][2], pairs[4][2], pairs[8][2], pairs[9][2]] + [points[i][1] for i in (0, 2, 5)]
    assert len(pts) == 16
    return pts


def test_c_restatement_and_python_oracle_agree_on_the_extreme_g2_msm():
    """The C restatement is the reference of tests/test_gpu_extreme_operands_g2.py; the Python integers settle it here (16
    points: a G2 multiplication in Python takes about half a second)."""
    pts = _g2_host_set()
    ks = xi.g2_scalars_below_r(16)
    want = None
    for P, k in zip(pts, ks):
        want = bn.G2.add(want, bn.G2.mul(P, k))
    bases = b"".join(bn.g2_to_bytes(P) for P in pts)
    assert co.msm_g2(bases, xi.scalars_bytes(ks)) == bn.g2_to_bytes(want)
    # all scalars one: the plain sum
    want = None
    for P in pts:
        want = bn.G2.add(want, P)
    assert co.msm_g2(bases, xi.scalars_bytes([1] * 16)) == bn.g2_to_bytes(want)
    for P, k in zip(pts[:6], (1, 2, R - 1, R - 2, ks[5], ks[6])):
        assert co.g2_mul(bn.g2_to_bytes(P), k) == bn.g2_to_bytes(bn.G2.mul(P, k))


def test_c_restatement_adds_the_half_zero_pairs_like_the_python_oracle():
    """Two and three points under one common scalar: what the tiny device MSMs compare with."""
    pairs, points = xi.half_zero_g2()
    cases = [(P1, P2) for _, P1, P2 in pairs] + [(P2, P1) for _, P1, P2 in pairs]
    cases += [(P, bn.G2.neg(P)) for _, P in points] + [(P, P) for _, P in points]
    one = xi.scalars_bytes([1, 1])
    for P1, P2 in cases:
        got = co.msm_g2(bn.g2_to_bytes(P1) + bn.g2_to_bytes(P2), one)
        assert got == bn.g2_to_bytes(bn.G2.add(P1, P2))
    P, P2 = points[0][1], pairs[0][1]
    got = co.msm_g2(b"".join(bn.g2_to_bytes(X) for X in (P, bn.G2.neg(P), P2)), xi.scalars_bytes([1, 1, 1]))
    assert got == bn.g2_to_bytes(P2)


@pytest.mark.parametrize("field,p", [("fr", R), ("fq", Q)])
def test_c_restatement_product_on_the_edge_cross_product(field, p):
    e = xi.EDGE_FIELD(p)
    assert len(e) == len(set(e)) == 17
    a, b, want = xi.edge_cross_product(p)
    assert a.size == b.size == 32 * 17 * 17
    fn = co.fr_mul_vec if field == "fr" else co.fq_mul_vec
    assert xi.unpack(fn(a, b)) == want


# ------------------------------------------------------------------------------------------ rows for the coset transforms
COSET_SHIFTS = (1, 5, xi.held(xi.T_MAX), R - 1)


def test_held_values_are_loaded_as_their_targets():
    assert xi.limbs29(xi.loaded_word(xi.held(xi.T_MAX))) == [(1 << 29) - 1] * 8 + [3171405]
    assert xi.loaded_word(xi.held(R - 1)) == R - 1
    assert xi.limbs29(xi.loaded_word(xi.held(1))) == [1] + [0] * 8
    assert xi.loaded_word(1) == (1 << 261) % R and xi.held((1 << 261) % R) == 1
    # the shift whose own word, the first entry of the lane's power table, sits on full limbs
    assert xi.limbs29(xi.held(xi.T_MAX) * (1 << 261) % R) == xi.limbs29(xi.T_MAX)


@pytest.mark.parametrize("g", COSET_SHIFTS)
def test_held_families_are_loaded_as_the_families_they_name(g):
    """the limbs of v_i g^i 2^261 mod r equal the targets, row by row"""
    logn, n = 7, 128
    bits = xi.unpack(xi.mask01(n, 1000 + logn))
    want = {"all_top": [R - 1] * n, "all_ones_limbs": [xi.T_MAX] * n, "mask01": bits, "alternating": [R - 1, 1] * (n // 2)}
    for s in (1, 3, 6):
        want["stride(%d,top)" % s] = [R - 1 if i % (1 << s) == 0 else 0 for i in range(n)]
        want["stride(%d,tmax)" % s] = [xi.T_MAX if i % (1 << s) == 0 else 0 for i in range(n)]
    fams = xi.held_families(logn, g)
    assert [name for name, _ in fams] == list(want)
    for name, rows in fams:
        assert len(rows) == n and all(0 <= v < R for v in rows), name
        assert [xi.limbs29(xi.loaded_word(v, i, g)) for i, v in enumerate(rows)] == [xi.limbs29(t) for t in want[name]], name
    assert [name for name, _ in xi.held_families(12)][-2:] == ["stride(11,top)", "stride(11,tmax)"]
    assert xi.held_rows([5, 6, 7], g) == [xi.held(t) * pow(g, -i, R) % R for i, t in enumerate((5, 6, 7))]


@pytest.mark.parametrize("g", COSET_SHIFTS)
def test_coset_preimages_end_at_the_families(g):
    """the forward transform on the coset of g, in Python integers, leaves words with the targets' limbs"""
    import plonk_instance as pi
    logn = 6
    ends = dict(xi.held_families(logn))
    pre = xi.coset_preimages(logn, g)
    assert [name for name, _ in pre] == ["coset_preimage(%s)" % name for name in ends]
    for name, rows in pre:
        out = pi.coset_ext(rows, logn, g)
        assert out == ends[name[15:-1]], name
        assert [xi.loaded_word(v) for v in out] == [xi.loaded_word(v) for v in ends[name[15:-1]]]
    big = xi.big_coset_inputs(13, 5)
    assert [name for name, _ in big] == [name for name, _ in xi.big_size_inputs(13)]
    assert xi.loaded_word(big[3][1][4096], 4096, 5) == xi.T_MAX and big[3][1][2048] == 0 and xi.loaded_word(big[2][1][2048], 2048, 5) == R - 1
