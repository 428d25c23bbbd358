"""PLONK rounds 4 and 5 without a device: the header declares the entries with their exact prototypes and documents the
knob, the formulas and what is not checked; every export is bound and re-exported; the refusals that need no device carry
the header's text; and the two references of tests/plonk_opening_instance.py, which the device tests compare against,
agree with each other."""
import ctypes
import os
import re

import numpy as np
import pytest

import plonk_instance as pi
import plonk_opening_instance as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkhip.h")
ENTRIES = {"zk_fr_poly_eval": 6, "zk_plonk_opening_create": 4, "zk_plonk_opening_destroy": 1, "zk_plonk_opening_info": 2, "zk_plonk_evaluate": 11,
           "zk_plonk_open": 17}
R = pi.R


def test_header_declares_the_entries():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    for decl in ("int zk_fr_poly_eval(uint8_t *ys, const uint8_t *coeffs, uint64_t n, uint64_t m, const uint8_t *zs, int32_t device);",
                 "typedef struct zk_plonk_opening zk_plonk_opening;",
                 "int zk_plonk_opening_create(zk_plonk_opening **out, zk_kzg *kzg, const zk_plonk_circuit_view *v, int32_t device);",
                 "void zk_plonk_opening_destroy(zk_plonk_opening *o);",
                 "int zk_plonk_opening_info(zk_plonk_opening *o, zk_plonk_opening_plan *plan);",
                 "int zk_plonk_evaluate(zk_plonk_opening *o, uint8_t evals[6 * 32], const uint8_t *a, uint64_t a_len, const uint8_t *b, uint64_t b_len, "
                 "const uint8_t *cc, uint64_t c_len, const uint8_t *z, uint64_t z_len, const uint8_t zeta[32]);",
                 "int zk_plonk_open(zk_plonk_opening *o, uint8_t w_zeta[64], uint8_t w_zeta_omega[64], uint8_t r_zeta[32], uint8_t *f, uint64_t *f_len, "
                 "const uint8_t *t_lo, uint64_t lo_len, const uint8_t *t_mid, uint64_t mid_len, const uint8_t *t_hi, uint64_t hi_len, "
                 "const uint8_t pi_zeta[32], const uint8_t alpha[32], const uint8_t beta[32], const uint8_t gamma[32], const uint8_t v[32]);"):
        assert decl in flat, decl
    section = text[text.index("PLONK evaluations and opening proofs"):]
    for words in ("ZKHIP_OPEN_SEG", "STANDARD form", "ZKHIP_OPEN_SEG: a number of coefficients per lane from 1 to 4096 expected",
                  "zk_fr_poly_eval: n is 0", "zk_fr_poly_eval: polynomial 2, coefficient 5 is not below r", "zk_fr_poly_eval: z 3 is not below r",
                  "zk_plonk_opening_create: log_n 26 is outside 1 .. 25", "zk_plonk_opening_create: qm 5 is not below r", "exceeds the kzg's max_coeffs =",
                  "is not the kzg's device", "destroying the kzg before the object is the caller's error",
                  "zk_plonk_evaluate: b_len 0 is outside 1 .. max_coeffs =", "zk_plonk_evaluate: z 5 is not below r",
                  "zk_plonk_open: no evaluation is pending: call zk_plonk_evaluate first", "zk_plonk_open: t_lo 5 is not below r",
                  "F(X)    = r + v a + v^2 b + v^3 c + v^4 s1 + v^5 s2", "r_zeta  = r(zeta) = F(zeta) - E", "- Z_H(zeta) (t_lo + zeta^n t_mid + zeta^2n t_hi)",
                  "NOT checked: that r(zeta) = 0; that the t parts are the split of the round-3 quotient; that k1 and k2 give disjoint"):
        assert words in section, words


def test_every_export_is_bound_and_re_exported():
    from rapidsnark_old_amd import lib as L
    import rapidsnark_old_amd as zk
    lib = L.load_library()
    for name, nargs in ENTRIES.items():
        assert name in L.EXPORTS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert ctypes.sizeof(L.zk_plonk_opening_plan) == 32
    assert zk.fr_poly_eval is zk.plonk.fr_poly_eval and zk.PlonkOpening is zk.plonk.PlonkOpening


def test_c_entries_refuse_bad_arguments_before_a_device_is_touched():
    from rapidsnark_old_amd import lib as L
    lib = L.load_library()
    P = lambda a: ctypes.c_void_p(a.ctypes.data)       # noqa: E731
    le = lambda v: np.frombuffer(pi.le(v), dtype=np.uint8).copy()      # noqa: E731
    ys = np.zeros(3 * 32, dtype=np.uint8)

    def ev(coeffs, n, m, zs):
        assert lib.zk_fr_poly_eval(P(ys), P(coeffs), n, m, P(zs), -1) == 1
        return lib.zk_last_error().decode()

    good = le([1, 2, 3, 4, 5, 6])
    assert ev(good, 0, 1, le([1])) == "zk_fr_poly_eval: n is 0"
    assert ev(good, 1 << 31, 1, le([1])) == "zk_fr_poly_eval: n is not below 2^31"
    assert ev(le([1, 2, 3, 4, 5, R]), 2, 3, le([1, 2, 3])) == "zk_fr_poly_eval: polynomial 2, coefficient 1 is not below r"
    assert ev(good, 2, 3, le([1, 2, R])) == "zk_fr_poly_eval: z 2 is not below r"
    assert lib.zk_fr_poly_eval(None, None, 4, 0, None, -1) == 0          # m = 0 is legal
    assert lib.zk_fr_poly_eval(None, P(good), 2, 3, P(good), -1) == 1 and lib.zk_last_error().decode() == "null argument"
    h = ctypes.c_void_p()
    v = L.zk_plonk_circuit_view()
    assert lib.zk_plonk_opening_create(ctypes.byref(h), None, ctypes.byref(v), -1) == 1 and lib.zk_last_error().decode() == "null argument" and not h
    assert lib.zk_plonk_evaluate(None, P(ys), P(good), 1, P(good), 1, P(good), 1, P(good), 1, P(good)) == 1
    assert lib.zk_last_error().decode() == "null argument"
    plan = L.zk_plonk_opening_plan()
    assert lib.zk_plonk_opening_info(None, ctypes.byref(plan)) == 1 and lib.zk_last_error().decode() == "null argument"
    lib.zk_plonk_opening_destroy(None)


def test_python_refuses_bad_arguments_before_any_library_call(monkeypatch):
    from rapidsnark_old_amd import lib as L, plonk as P, kzg as K

    def never(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(L, "load_library", never)
    with pytest.raises(ValueError, match="coeffs: value 1 is not in 0 .. r - 1"):
        P.fr_poly_eval([0, R], 1)
    with pytest.raises(ValueError, match="coeffs: at least one coefficient"):
        P.fr_poly_eval([], 1)
    with pytest.raises(ValueError, match="zs: 2 values for 1 polynomials"):
        P.fr_poly_eval([1, 2], [1, 2])
    with pytest.raises(ValueError, match="coeffs: the polynomials must have one length"):
        P.fr_poly_eval([[1, 2], [1]], [1, 2])
    q = [1, 2, 3, 4]
    ok = [q] * 8
    with pytest.raises(TypeError, match="a Kzg expected"):
        P.PlonkOpening(None, *ok, 2, 3)
    k = K.Kzg.__new__(K.Kzg)                            # never made on a device: the checks that come first still answer
    k.max_coeffs, k.device, k._h = 9, 0, None
    with pytest.raises(ValueError, match="basis 'evaluation' is unknown"):
        P.PlonkOpening(k, *ok, 2, 3, basis="evaluation")
    with pytest.raises(ValueError, match="qo has 8 rows, ql has 4: the eight circuit vectors must have one length"):
        P.PlonkOpening(k, q, q, q, q * 2, q, q, q, q, 2, 3)
    with pytest.raises(ValueError, match="n = 3 is not a power of two"):
        P.PlonkOpening(k, *([[1, 2, 3]] * 8), 2, 3)
    with pytest.raises(ValueError, match="log_n 0 is outside 1 .. 25"):
        P.PlonkOpening(k, *([[7]] * 8), 2, 3)
    with pytest.raises(ValueError, match="s2: value 2 is not in 0 .. r - 1"):
        P.PlonkOpening(k, q, q, q, q, q, q, [1, 2, R, 4], q, 2, 3)
    with pytest.raises(ValueError, match="k2: one value expected"):
        P.PlonkOpening(k, *ok, 2, [3, 4])
    with pytest.raises(ValueError, match="n \\+ 6 = 10 exceeds the kzg's max_coeffs = 9"):
        P.PlonkOpening(k, *ok, 2, 3)
    k.max_coeffs = 10
    with pytest.raises(L.ZkHipError, match="the Kzg object is closed"):
        P.PlonkOpening(k, *ok, 2, 3)
    o = P.PlonkOpening.__new__(P.PlonkOpening)
    o.kzg, o.n, o.log_n, o.max_coeffs, o._h = k, 4, 2, 10, None
    p = [1] * 6
    with pytest.raises(ValueError, match="c_len 0 is outside 1 .. max_coeffs = 10"):
        o.evaluate(p, p, [], p, 5)
    with pytest.raises(ValueError, match="z_len 11 is outside 1 .. max_coeffs = 10"):
        o.evaluate(p, p, p, [1] * 11, 5)
    with pytest.raises(ValueError, match="b: value 1 is not in 0 .. r - 1"):
        o.evaluate(p, [0, R], p, p, 5)
    with pytest.raises(ValueError, match="zeta: value 0 is not in"):
        o.evaluate(p, p, p, p, R)
    with pytest.raises(L.ZkHipError, match="the PlonkOpening object is closed"):
        o.evaluate(p, p, p, p, 5)
    with pytest.raises(ValueError, match="mid_len 0 is outside 1 .. max_coeffs = 10"):
        o.open(p, [], p, 1, 2, 3, 4)
    with pytest.raises(ValueError, match="t_hi: rows of 32 bytes"):
        o.open(p, p, bytes(33), 1, 2, 3, 4)
    with pytest.raises(ValueError, match="v: value 0 is not in"):
        o.open(p, p, p, 1, 2, 3, R)
    with pytest.raises(ValueError, match="pi_zeta: one value expected"):
        o.open(p, p, p, 1, 2, 3, 4, pi_zeta=[1, 2])
    with pytest.raises(L.ZkHipError, match="the PlonkOpening object is closed"):
        o.open(p, p, p, 1, 2, 3, 4)
    with pytest.raises(L.ZkHipError, match="the PlonkOpening object is closed"):
        o.info()


# ---------------------------------------------------------------- the two references
@pytest.mark.parametrize("log_n", [3, 4, 6])
def test_the_two_references_agree_and_r_zeta_is_zero(log_n):
    """F coefficient for coefficient, n + 6 of them with the usual blinding; r(zeta) = 0 both ways; A's quotients pass B's
    check by multiplication and a changed quotient or value does not"""
    I, parts, zeta, v = po.make(3000 + log_n, log_n)
    assert [len(p) for p in parts] == [I.n + 1, I.n + 1, I.n + 6]
    a, b = po.reference_a(I, parts, zeta, v), po.reference_b(I, parts, zeta, v)
    assert a.F == b.F and len(a.F) == I.n + 6 and a.F[-1] != 0
    assert a.evals == b.evals and a.E == b.E
    assert a.r_zeta == 0 and b.r_zeta == 0
    assert pi.horner(b.D, zeta) == b.r0
    assert po.check_b(b, a.q_zeta, a.q_zw, 0)
    bad = list(a.q_zeta)
    bad[1] = (bad[1] + 1) % R
    assert not po.check_b(b, bad, a.q_zw, 0) and not po.check_b(b, a.q_zeta, a.q_zw, 1) and not po.check_b(b, a.q_zeta, a.q_zw[:-1] + [5], 0)


def test_the_references_agree_unblinded():
    I, parts, zeta, v = po.make(3013, 3, None, blind_parts=False)
    assert [len(p) for p in parts] == [I.n, I.n, I.n - 3]
    a, b = po.reference_a(I, parts, zeta, v), po.reference_b(I, parts, zeta, v)
    assert a.F == b.F and len(a.F) == I.n and a.r_zeta == b.r_zeta == 0 and po.check_b(b, a.q_zeta, a.q_zw, 0)


@pytest.mark.parametrize("zeta", ["zero", "one", "omega"])
def test_the_references_agree_where_z_h_vanishes_and_at_zero(zeta):
    z = {"zero": 0, "one": 1, "omega": pi.fr_root(4)}[zeta]
    I, parts, _, v = po.make(3024, 4)
    a, b = po.reference_a(I, parts, z, v), po.reference_b(I, parts, z, v)
    assert a.F == b.F and a.r_zeta == b.r_zeta == 0 and po.check_b(b, a.q_zeta, a.q_zw, 0)


def test_a_broken_gate_leaves_r_zeta_non_zero():
    I, parts, zeta, v = po.make(3034, 4, break_gate=3)
    a, b = po.reference_a(I, parts, zeta, v), po.reference_b(I, parts, zeta, v)
    assert a.F == b.F and a.r_zeta == b.r_zeta != 0
    assert po.check_b(b, a.q_zeta, a.q_zw, a.r_zeta) and not po.check_b(b, a.q_zeta, a.q_zw, 0)
