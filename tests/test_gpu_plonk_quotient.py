"""PLONK round 3 on the GPU: coset transforms and the quotient t = num / Z_H.  Exact arithmetic: every expected value comes
from Python integers (tests/plonk_instance.py: schoolbook products and long division, or the coset route over
oracle.bn254.ntt), and the comparison is byte for byte over all 4n rows and t_len."""
import ctypes
import functools

import numpy as np
import pytest

import plonk_instance as pi
from oracle import bn254 as bn

pytestmark = pytest.mark.gpu

R = bn.R_MOD
BIG = 0x1A3C09F0A58A7E8500E0A7EB8EF62ABC402D111E41112ED49BD61B6E725B19EF       # 253 bits, below r
TAU, ALPHA, BETA = 0x1F3A9C5E77D1B2A49E0C6F5D3B8A17264C9E0F1D2B3A4958, 0x2B7E151628AED2A6ABF7158809CF4F3C, 0x3243F6A8885A308D313198A2E0370734
SHIFTS = {"none": None, "5": 5, "big": BIG}


def le(values):
    return np.frombuffer(pi.le(values), dtype=np.uint8)


ints = pi.ints


@functools.lru_cache(maxsize=None)
def instance(seed, log_n, blind=None, **kw):
    return pi.make(seed, log_n, blind, **dict(kw))


@functools.lru_cache(maxsize=None)
def expected_a(seed, log_n, blind=None, **kw):
    t, rem = pi.oracle_a(instance(seed, log_n, blind, **kw))
    assert not any(rem)
    return t


@functools.lru_cache(maxsize=None)
def expected_b(seed, log_n, blind=None, g=5, **kw):
    return pi.oracle_b(instance(seed, log_n, blind, **kw), g)


def quotient(zk, inst, basis="monomial", shift=None, with_pi=True):
    with zk.PlonkCircuit(*[le(v) for v in inst.circuit(basis)], pi.K1, pi.K2, basis=basis, shift=shift) as c:
        return c.quotient(le(inst.a), le(inst.b), le(inst.c), le(inst.z), inst.alpha, inst.beta, inst.gamma, pi=le(inst.pi) if with_pi else None)


def check(got, want):
    t, t_len = got
    assert t.size == len(want) * 32
    assert ints(t) == want
    assert t_len == pi.t_len_of(want)


# ---------------------------------------------------------------- fr_coset_ntt
@pytest.mark.parametrize("shift", list(SHIFTS))
@pytest.mark.parametrize("n_in", ["one", "quarter", "full"])
@pytest.mark.parametrize("log_m", [2, 3, 11, 12])      # the radix-2 path, the pipeline's smallest size, one tile, the first strided pass
def test_coset_ntt_matches_python_integers(zk, log_m, n_in, shift):
    m = 1 << log_m
    k = {"one": 1, "quarter": m // 4 + 3, "full": m}[n_in]
    g = SHIFTS[shift]
    rng = np.random.RandomState(log_m * 100 + k % 97)
    for edge in (0, 1, R - 1):                           # at index 0 and at n_in - 1 (m - 1 when the vector is full)
        v = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(k)]
        v[0] = v[k - 1] = edge
        out = zk.fr_coset_ntt(v, log_m=log_m, shift=g)
        assert ints(out) == pi.coset_ext(v, log_m, g or 1)
        if g is None and k == m:
            assert bytes(out) == zk.fr_ntt(pi.le(v))
        back = zk.fr_coset_ntt(out, log_m=log_m, shift=g, inverse=True)
        assert ints(back) == v + [0] * (m - k)


def test_coset_ntt_edge_values_at_the_last_row_and_log_m_from_the_length(zk):
    for log_m in (2, 3, 11):
        m = 1 << log_m
        for edge in (0, 1, R - 1):
            v = [7] * (m - 1) + [edge]
            assert ints(zk.fr_coset_ntt(v, shift=BIG)) == pi.coset_ext(v, log_m, BIG)
    assert ints(zk.fr_coset_ntt([3, 4, 5])) == pi.coset_ext([3, 4, 5], 2, 1)
    assert ints(zk.fr_coset_ntt([9], log_m=0, shift=5)) == [9]


# ---------------------------------------------------------------- quotient against oracle A
@pytest.mark.parametrize("log_n,blind", [(1, None), (2, None), (3, None), (3, pi.BLIND), (4, pi.BLIND), (6, pi.BLIND), (8, pi.BLIND)])
def test_quotient_matches_schoolbook_and_long_division(zk, log_n, blind):
    inst = instance(2900 + log_n, log_n, blind)
    want = expected_a(2900 + log_n, log_n, blind)
    assert pi.t_len_of(want) == (3 * inst.n + 6 if blind else 3 * inst.n - 3)
    check(quotient(zk, inst), want)


def test_quotient_with_unequal_lengths(zk):
    inst = instance(2931, 3, (0, 2, 5, 3))
    assert [len(p) for p in (inst.a, inst.b, inst.c, inst.z)] == [8, 10, 13, 11]
    check(quotient(zk, inst), expected_a(2931, 3, (0, 2, 5, 3)))


def test_quotient_without_public_inputs(zk):
    inst = instance(2932, 4, pi.BLIND, public=False)
    assert not any(inst.pi)
    want = expected_a(2932, 4, pi.BLIND, public=False)
    check(quotient(zk, inst, with_pi=False), want)
    check(quotient(zk, inst, with_pi=True), want)


@pytest.mark.parametrize("zero", ["alpha", "beta", "gamma"])
def test_quotient_with_a_zero_challenge(zk, zero):
    kw = {zero: 0}
    inst = instance(2933, 4, pi.BLIND, **kw)
    check(quotient(zk, inst), expected_a(2933, 4, pi.BLIND, **kw))


# ---------------------------------------------------------------- quotient against oracle B
@pytest.mark.parametrize("log_n", [9, 10, 11])
def test_quotient_matches_the_coset_route(zk, log_n):
    inst = instance(2940 + log_n, log_n, pi.BLIND)
    want = expected_b(2940 + log_n, log_n, pi.BLIND)
    assert pi.t_len_of(want) == 3 * inst.n + 6
    check(quotient(zk, inst), want)


def test_quotient_at_a_larger_size_satisfies_the_identity(zk):
    """log_n = 14: t(zeta) Z_H(zeta) = num(zeta) at two fixed zeta, and t_len = 3n + 6"""
    inst = pi.make(2954, 14, pi.BLIND, intt=lambda v: ints(zk.fr_ntt(pi.le(v), inverse=True)))
    t, t_len = quotient(zk, inst, basis="lagrange")
    n = inst.n
    assert t_len == 3 * n + 6
    coeffs = ints(t)
    assert not any(coeffs[t_len:])
    for zeta in (TAU, BIG):
        assert pi.horner(coeffs[:t_len], zeta) * (pow(zeta, n, R) - 1) % R == pi.num_at(inst, zeta)


# ---------------------------------------------------------------- bytes independent of settings
@pytest.mark.parametrize("seg", ["1", "3", None])
def test_quotient_bytes_do_not_depend_on_the_segment(zk, monkeypatch, seg):
    """2^11 points: eight workgroups of one point a lane, three of three (the last lanes take two), one of sixteen (the lanes take eight)"""
    if seg is None:
        monkeypatch.delenv("ZKHIP_QUOT_SEG", raising=False)
    else:
        monkeypatch.setenv("ZKHIP_QUOT_SEG", seg)
    inst = instance(2949, 9, pi.BLIND)
    with zk.PlonkCircuit(*[le(v) for v in inst.circuit()], pi.K1, pi.K2) as c:
        check(c.quotient(le(inst.a), le(inst.b), le(inst.c), le(inst.z), inst.alpha, inst.beta, inst.gamma, pi=le(inst.pi)), expected_b(2949, 9, pi.BLIND))
        info = c.info()
    assert info["seg"] == (int(seg) if seg else 16) and info["log_n"] == 9 and info["points"] == 2048
    assert info["last_launches"] >= 5 and info["device_bytes"] >= 76 * 512 * 32
    v = list(range(1, 300))
    assert ints(zk.fr_coset_ntt(v, log_m=9, shift=5)) == pi.coset_ext(v, 9, 5)


@pytest.mark.parametrize("shift", [None, 7, BIG])
@pytest.mark.parametrize("basis", ["monomial", "lagrange"])
def test_quotient_bytes_do_not_depend_on_the_shift_or_the_basis(zk, shift, basis):
    check(quotient(zk, instance(2906, 6, pi.BLIND), basis=basis, shift=shift), expected_a(2906, 6, pi.BLIND))


def test_lagrange_basis_at_the_smallest_sizes(zk):
    for log_n in (1, 2, 3):                              # the inverse transform of size n: radix-2 below 8
        check(quotient(zk, instance(2900 + log_n, log_n), basis="lagrange"), expected_a(2900 + log_n, log_n))


# ---------------------------------------------------------------- a broken gate
def test_a_broken_gate_gives_the_interpolant_and_a_full_length(zk):
    inst = instance(2904, 4, pi.BLIND, break_gate=3)
    want = expected_b(2904, 4, pi.BLIND, break_gate=3)
    assert pi.t_len_of(want) == 4 * inst.n
    check(quotient(zk, inst), want)


# ---------------------------------------------------------------- refusals
def test_refusals_of_the_c_entries(zk, monkeypatch):
    from rapidsnark_old_amd import lib as L
    lib = zk.load_library()
    P = lambda a: ctypes.c_void_p(a.ctypes.data)       # noqa: E731

    def err(rc):
        assert rc == 1
        return lib.zk_last_error().decode()

    n = 4
    good, bad = le([1, 2, 3, 4]).copy(), le([1, 2, R, R + 1]).copy()
    names = ("ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3")

    def create(log_n=2, shift=None, k1=2, swap=None, basis=0):
        v = L.zk_plonk_circuit_view()
        v.log_n, v.basis = log_n, basis
        for name in names:
            setattr(v, name, (bad if name == swap else good).ctypes.data)
        ctypes.memmove(v.k1, pi.le([k1]), 32)
        ctypes.memmove(v.k2, pi.le([3]), 32)
        sb = le([shift]).copy() if shift is not None else None
        v.shift = sb.ctypes.data if sb is not None else None
        h = ctypes.c_void_p()
        return lib.zk_plonk_circuit_create(ctypes.byref(h), ctypes.byref(v), -1), h

    for g in (1, bn.fr_root(4)):
        assert err(create(shift=g)[0]) == "zk_plonk_circuit_create: shift^(4n) is 1: Z_H vanishes on the coset"
    assert err(create(shift=0)[0]) == "zk_plonk_circuit_create: shift is zero"
    assert err(create(shift=R)[0]) == "zk_plonk_circuit_create: shift is not below r"
    assert err(create(k1=R)[0]) == "zk_plonk_circuit_create: k1 is not below r"
    assert err(create(log_n=0)[0]) == "zk_plonk_circuit_create: log_n 0 is outside 1 .. 25"
    assert err(create(log_n=26)[0]) == "zk_plonk_circuit_create: log_n 26 is outside 1 .. 25"
    assert err(create(basis=7)[0]) == "zk_plonk_circuit_create: basis 7 is unknown"
    for name in names:
        assert err(create(swap=name)[0]) == "zk_plonk_circuit_create: %s 2 is not below r" % name
    rc, h = create()
    assert rc == 0 and h
    t, t_len, one = np.zeros(16 * 32, dtype=np.uint8), ctypes.c_uint64(0), le([1]).copy()
    big, nine, six, seven = le([R]).copy(), le([1] * 9).copy(), le([1] * 6).copy(), le([1] * 7).copy()

    def q(a=good, al=n, b=good, bl=n, c=good, cl=n, z=good, zl=n, p=None, alpha=one, beta=one, gamma=one):
        return lib.zk_plonk_quotient(h, P(t), ctypes.byref(t_len), P(a), al, P(b), bl, P(c), cl, P(z), zl, P(p) if p is not None else None,
                                     P(alpha), P(beta), P(gamma))

    assert err(q(al=0)) == "zk_plonk_quotient: a_len 0 is outside 1 .. 2n = 8"
    assert err(q(c=nine, cl=9)) == "zk_plonk_quotient: c_len 9 is outside 1 .. 2n = 8"
    assert err(q(a=six, al=6, b=six, bl=6, c=six, cl=6, z=seven, zl=7)) \
        == "zk_plonk_quotient: a_len + b_len + c_len + z_len = 25 exceeds 5n + 3 = 23: t would have more than 4n coefficients"
    assert err(q(a=bad)) == "zk_plonk_quotient: a 2 is not below r"
    assert err(q(b=bad)) == "zk_plonk_quotient: b 2 is not below r"
    assert err(q(c=bad)) == "zk_plonk_quotient: c 2 is not below r"
    assert err(q(z=bad)) == "zk_plonk_quotient: z 2 is not below r"
    assert err(q(p=bad)) == "zk_plonk_quotient: pi 2 is not below r"
    assert err(q(alpha=big)) == "zk_plonk_quotient: alpha is not below r"
    assert err(q(beta=big)) == "zk_plonk_quotient: beta is not below r"
    assert err(q(gamma=big)) == "zk_plonk_quotient: gamma is not below r"
    for value in ("0", "4097", "x"):
        monkeypatch.setenv("ZKHIP_QUOT_SEG", value)
        assert err(q()) == "ZKHIP_QUOT_SEG: a number of points per lane from 1 to 4096 expected"
    monkeypatch.setenv("ZKHIP_QUOT_SEG", "4096")
    assert q() == 0
    monkeypatch.delenv("ZKHIP_QUOT_SEG")
    lib.zk_plonk_circuit_destroy(h)
    out = np.zeros(8 * 32, dtype=np.uint8)
    eight = le([1, 2, 3, 4, 5, R, 7, 8]).copy()
    assert err(lib.zk_fr_coset_ntt(P(out), P(eight), 8, 3, None, 0, -1)) == "zk_fr_coset_ntt: value 5 is not below r"
    assert err(lib.zk_fr_coset_ntt(P(out), P(good), 4, 3, P(le([0]).copy()), 0, -1)) == "zk_fr_coset_ntt: shift is zero"
    assert err(lib.zk_fr_coset_ntt(P(out), P(good), 4, 3, P(big), 0, -1)) == "zk_fr_coset_ntt: shift is not below r"
    assert err(lib.zk_fr_coset_ntt(P(out), P(good), 4, 29, None, 0, -1)) == "zk_fr_coset_ntt: log_m 29 is above 28"
    assert err(lib.zk_fr_coset_ntt(P(out), P(nine), 9, 3, None, 0, -1)) == "zk_fr_coset_ntt: n_in 9 is outside 1 .. 2^log_m = 8"
    assert err(lib.zk_fr_coset_ntt(P(out), P(good), 4, 3, None, 1, -1)) == "zk_fr_coset_ntt: n_in 4 is not 2^log_m = 8"


def test_python_refusals_and_use_after_close(zk):
    inst = instance(2902, 2)
    rows = [le(v) for v in inst.circuit()]
    for g in (1, bn.fr_root(4)):
        with pytest.raises(ValueError, match="shift\\^\\(4n\\) is 1"):
            zk.PlonkCircuit(*rows, pi.K1, pi.K2, shift=g)
    with pytest.raises(ValueError, match="shift is zero"):
        zk.PlonkCircuit(*rows, pi.K1, pi.K2, shift=0)
    c = zk.PlonkCircuit(*rows, pi.K1, pi.K2)
    with pytest.raises(ValueError, match="a_len \\+ b_len \\+ c_len \\+ z_len = 25 exceeds 5n \\+ 3 = 23"):      # the usual blinding at n = 4
        c.quotient([1] * 6, [1] * 6, [1] * 6, [1] * 7, 1, 2, 3)
    with pytest.raises(ValueError, match="b_len 9 is outside 1 .. 2n = 8"):
        c.quotient([1] * 4, [1] * 9, [1] * 4, [1] * 4, 1, 2, 3)
    with pytest.raises(zk.ZkHipError, match="zk_plonk_quotient: c 1 is not below r"):
        c.quotient(le([1] * 4), le([1] * 4), le([1, R, 3, 4]), le([1] * 4), 1, 2, 3)
    check(c.quotient(le(inst.a), le(inst.b), le(inst.c), le(inst.z), inst.alpha, inst.beta, inst.gamma, pi=le(inst.pi)), expected_a(2902, 2))
    c.close()
    c.close()
    with pytest.raises(zk.ZkHipError, match="the PlonkCircuit object is closed"):
        c.quotient(le(inst.a), le(inst.b), le(inst.c), le(inst.z), 1, 2, 3)
    with pytest.raises(zk.ZkHipError, match="the PlonkCircuit object is closed"):
        c.info()


# ---------------------------------------------------------------- INTEGRATION section 16, steps 2 and 3
def test_rounds_two_and_three_commit_to_the_quotient(zk, tmp_path):
    """z from plonk_permutation_product, blinded; t from quotient; the commitment of t is [num(tau) / Z_H(tau)] G"""
    path = str(tmp_path / "p6.ptau")
    zk.write_trapdoor_ptau(6, TAU, ALPHA, BETA, path)
    inst = instance(2964, 4, pi.BLIND)
    n = inst.n
    z, last = zk.plonk_permutation_product([inst.a_v, inst.b_v, inst.c_v], [inst.s1_v, inst.s2_v, inst.s3_v], [1, pi.K1, pi.K2], inst.beta, inst.gamma)
    assert last == 1 and ints(z) == inst.z_v
    z_coeffs = bn.ntt(ints(z), inverse=True) + [0] * 3
    blinding = [(inst.z[n + j]) % R for j in range(3)]  # the instance's own multiple of Z_H on the device's accumulator
    for j, r in enumerate(blinding):
        z_coeffs[j] = (z_coeffs[j] - r) % R
        z_coeffs[n + j] = (z_coeffs[n + j] + r) % R
    assert z_coeffs == inst.z
    with zk.PlonkCircuit(*[le(v) for v in inst.circuit("lagrange")], pi.K1, pi.K2, basis="lagrange") as c:
        t, t_len = c.quotient(le(inst.a), le(inst.b), le(inst.c), le(z_coeffs), inst.alpha, inst.beta, inst.gamma, pi=le(inst.pi))
    assert t_len == 3 * n + 6 == 54
    at_tau = pi.num_at(inst, TAU) * pow(pow(TAU, n, R) - 1, -1, R) % R
    with zk.Kzg.from_ptau(path) as k:
        assert bytes(k.commit(t[:t_len * 32])) == bn.g1_to_bytes(bn.G1.mul(bn.G1_GEN, at_tau))
