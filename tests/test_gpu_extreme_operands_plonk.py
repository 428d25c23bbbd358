"""GPU parity of csrc/plonkquot.hip at the edges of the nine-limb arithmetic (csrc/field29.hpp): k_coset_load, k_coset_store
and k_plonk_quotient on operands that random instances never produce.  What the quotient kernel multiplies are coset
evaluations; tests/plonk_instance.py builds instances whose evaluations are CHOSEN words (constant polynomials at every
point, 2n coefficients at every second point, n at every fourth), tests/extreme_inputs.py gives the standard values whose
loaded word has the limbs of a target (held): T_MAX (eight limbs of 2^29 - 1), r - 1, one lone low limb.  Such instances
break the gate identity: t is then the interpolant of num / Z_H, what oracle B computes in Python integers.  The data-dependent
zeros are here too: the empty circuit (num = 0, t_len = 0 out of the block maxima), P = Q, z = 1, alpha = 0.
Byte equality throughout, all 4n rows and t_len; everything goes through the C ABI."""
import functools

import numpy as np
import pytest

import extreme_inputs as xi
import plonk_instance as pi
from oracle import bn254 as bn
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

R = bn.R_MOD
LOG_N = (3, 7, 9, 10)              # 32 points: part of one workgroup; 512: two; 2^11: one transform tile; 2^12: the first strided pass


def le(values):
    return np.frombuffer(pi.le(values), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def instance(name, log_n, g=5):
    return pi.extreme_instance(name, log_n, g)


@functools.lru_cache(maxsize=None)
def expected(name, log_n, g=5):
    return pi.oracle_b(instance(name, log_n, g), g)


def quotient(zk, inst, basis="monomial", shift=None, with_pi=True):
    with zk.PlonkCircuit(*[le(v) for v in inst.circuit(basis)], pi.K1, pi.K2, basis=basis, shift=shift) as c:
        return c.quotient(le(inst.a), le(inst.b), le(inst.c), le(inst.z), inst.alpha, inst.beta, inst.gamma, pi=le(inst.pi) if with_pi else None)


def check(got, want, what):
    t, t_len = got
    assert t.size == len(want) * 32
    have = pi.ints(t)
    if have != want:
        bad = [i for i, (x, y) in enumerate(zip(have, want)) if x != y]
        raise AssertionError("%s: %d of %d rows differ, first at %d" % (what, len(bad), len(want), bad[0]))
    assert t_len == pi.t_len_of(want), what


# ---------------------------------------------------------------- the quotient
@pytest.mark.parametrize("log_n", LOG_N)
@pytest.mark.parametrize("name", pi.EXTREME_FAMILIES)
def test_quotient_on_chosen_coset_evaluations(zk, name, log_n):
    want = expected(name, log_n)
    m = 4 << log_n
    if name == "empty":
        assert not any(want)                             # t_len = 0 out of k_coset_store's block maxima
    elif name in pi.CONSTANT_FAMILIES:
        assert pi.t_len_of(want) == pi.constant_t_len(name, m // 4)
    check(quotient(zk, instance(name, log_n)), want, "%s, log_n %d" % (name, log_n))


def test_the_degenerate_identities_are_the_ones_named(zk):
    """sigma the identity with a constant z: P = Q at every point and t is the interpolant of alpha^2 (c - 1) L1 / Z_H =
    alpha^2 (c - 1) / (n (x - 1)); the empty circuit gives t_len = 0 and 4n zero rows from the device itself."""
    log_n = 7
    inst = instance("sigma_identity", log_n)
    n, m, g = inst.n, 4 * inst.n, 5
    wm, x, ev = bn.fr_root(log_n + 2), g, []
    c = inst.z[0]
    for _ in range(m):
        ev.append(inst.alpha * inst.alpha * (c - 1) * pow(n * (x - 1), -1, R) % R)
        x = x * wm % R
    assert expected("sigma_identity", log_n) == pi.interpolate_on_coset(ev, g)
    t, t_len = quotient(zk, instance("empty", log_n))
    assert t_len == 0 and not t.any()


@pytest.mark.parametrize("seg", ["1", "3"])
@pytest.mark.parametrize("name", ["const_tmax", "dealt1", "even_alternating", "empty"])
def test_quotient_families_do_not_depend_on_the_segment(zk, monkeypatch, name, seg):
    monkeypatch.setenv("ZKHIP_QUOT_SEG", seg)
    check(quotient(zk, instance(name, 9)), expected(name, 9), "%s, seg %s" % (name, seg))


@pytest.mark.parametrize("name", ["const_tmax", "even_mask01"])
def test_quotient_families_in_the_lagrange_basis(zk, name):
    check(quotient(zk, instance(name, 7), basis="lagrange"), expected(name, 7), name)


def test_quotient_families_without_public_inputs(zk):
    inst = instance("const_tmax_nopi", 7)
    assert not any(inst.pi)
    check(quotient(zk, inst, with_pi=False), expected("const_tmax_nopi", 7), "pi=None")


# ---------------------------------------------------------------- fr_coset_ntt
T_MAX_SHIFT = xi.held(xi.T_MAX)                          # the lane's running power starts on full limbs
SHIFTS = {"none": None, "5": 5, "tmax": T_MAX_SHIFT, "minus_one": R - 1}      # r - 1: the power alternates between 1 and -1


def _pre(rows, g):
    """rows_i g^i: what the plain transform of the reference takes"""
    if g == 1:
        return list(rows)
    out, x = [], 1
    for v in rows:
        out.append(v * x % R)
        x = x * g % R
    return out


def _post(rows, g):
    gi = pow(g, -1, R)
    return _pre(rows, gi)


def _forward(rows, log_m, g):
    if log_m <= 12:
        return pi.coset_ext(rows, log_m, g)
    return xi.unpack(co.fr_fft(xi.pack(_pre(rows, g) + [0] * ((1 << log_m) - len(rows)))))


def _inverse(rows, log_m, g):
    if log_m <= 12:
        return _post(bn.ntt(rows, inverse=True), g)
    return _post(xi.unpack(co.fr_fft(xi.pack(rows), inverse=True)), g)


def _same(got, want, what):
    got = xi.unpack(got)
    if got != want:
        bad = [i for i, (x, y) in enumerate(zip(got, want)) if x != y]
        raise AssertionError("%s: %d of %d rows differ, first at %d" % (what, len(bad), len(want), bad[0]))


# 3: the pipeline's smallest size; 5: a single tile with a window remainder; 11: one whole tile; 12: the first strided pass;
# 14: the first full strided window
@pytest.mark.parametrize("shift", list(SHIFTS))
@pytest.mark.parametrize("log_m", [3, 5, 11, 12, 14])
def test_coset_ntt_every_family_both_directions(zk, log_m, shift):
    g = SHIFTS[shift] or 1
    m = 1 << log_m
    for name, rows in xi.held_families(log_m, g) + xi.coset_preimages(log_m, g):
        if name == "all_ones_limbs":                     # the family is what it claims: the word the transform loads, limb for limb
            assert xi.limbs29(xi.loaded_word(rows[m - 1], m - 1, g)) == xi.limbs29(xi.T_MAX)
        _same(zk.fr_coset_ntt(rows, log_m=log_m, shift=SHIFTS[shift]), _forward(rows, log_m, g), "%s, 2^%d, shift %s, forward" % (name, log_m, shift))
    for name, rows in xi.held_families(log_m, 1) + xi.coset_preimages(log_m, g):
        _same(zk.fr_coset_ntt(rows, log_m=log_m, shift=SHIFTS[shift], inverse=True), _inverse(rows, log_m, g), "%s, 2^%d, shift %s, inverse" % (name, log_m, shift))


@pytest.mark.parametrize("shift", ["5", "tmax"])
def test_coset_ntt_partial_input_beside_extreme_rows(zk, shift):
    """n_in = m / 4 + 3: the zero-fill branch of k_coset_load beside rows on full limbs"""
    g, log_m = SHIFTS[shift], 11
    k = (1 << log_m) // 4 + 3
    for name, rows in xi.held_families(log_m, g):
        _same(zk.fr_coset_ntt(rows[:k], log_m=log_m, shift=g), _forward(rows[:k], log_m, g), "%s, n_in %d, shift %s" % (name, k, shift))


def test_coset_ntt_round_trip_on_the_device(zk):
    log_m, g = 14, T_MAX_SHIFT
    for name, rows in xi.held_families(log_m, g) + xi.coset_preimages(log_m, g):
        fwd = zk.fr_coset_ntt(rows, log_m=log_m, shift=g)
        _same(zk.fr_coset_ntt(fwd, log_m=log_m, shift=g, inverse=True), rows, "round trip of %s" % name)


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_coset_ntt_at_2p17(zk, which):
    """two strided windows, with the four inputs of the large transform sizes"""
    log_m, g = 17, 5
    name, rows = xi.big_coset_inputs(log_m, g)[which]
    _same(zk.fr_coset_ntt(rows, log_m=log_m, shift=g), _forward(rows, log_m, g), "%s, 2^17, forward" % name)
    name, rows = xi.big_coset_inputs(log_m, 1)[which]
    _same(zk.fr_coset_ntt(rows, log_m=log_m, shift=g, inverse=True), _inverse(rows, log_m, g), "%s, 2^17, inverse" % name)
