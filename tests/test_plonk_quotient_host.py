"""PLONK round 3 without a device: the header declares the entries with their exact prototypes and documents the knob and
the conventions, every export is bound and re-exported, the Python side refuses bad arguments before any library call, and
the two oracles of tests/plonk_instance.py, which the device tests compare against, agree with each other."""
import os
import re

import numpy as np
import pytest

import plonk_instance as pi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkhip.h")
ENTRIES = {"zk_fr_coset_ntt": 7, "zk_plonk_circuit_create": 3, "zk_plonk_circuit_destroy": 1, "zk_plonk_circuit_info": 2, "zk_plonk_quotient": 15}
R = pi.R


def test_header_declares_the_entries():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    for decl in ("int zk_fr_coset_ntt(uint8_t *out, const uint8_t *in, uint64_t n_in, uint32_t log_m, const uint8_t shift[32], int inverse, int32_t device);",
                 "typedef struct zk_plonk_circuit zk_plonk_circuit;",
                 "uint32_t log_n, basis; const uint8_t *ql, *qr, *qm, *qo, *qc, *s1, *s2, *s3; uint8_t k1[32], k2[32]; const uint8_t *shift; } zk_plonk_circuit_view;",
                 "int zk_plonk_circuit_create(zk_plonk_circuit **out, const zk_plonk_circuit_view *v, int32_t device);",
                 "void zk_plonk_circuit_destroy(zk_plonk_circuit *c);",
                 "int zk_plonk_circuit_info(zk_plonk_circuit *c, zk_plonk_circuit_plan *plan);",
                 "int zk_plonk_quotient(zk_plonk_circuit *c, uint8_t *t, uint64_t *t_len, const uint8_t *a, uint64_t a_len, const uint8_t *b, uint64_t b_len, "
                 "const uint8_t *cc, uint64_t c_len, const uint8_t *z, uint64_t z_len, const uint8_t *pi, const uint8_t alpha[32], "
                 "const uint8_t beta[32], const uint8_t gamma[32]);"):
        assert decl in flat, decl
    section = text[text.index("PLONK quotient and coset transforms"):]
    for words in ("ZKHIP_QUOT_SEG", "STANDARD form", "NOT checked", "ZKHIP_QUOT_SEG: a number of points per lane from 1 to 4096 expected",
                  "5n + 3", "It does not replace a gate check", "zk_fr_coset_ntt: shift is zero", "zk_fr_coset_ntt: value 5 is not below r",
                  "zk_plonk_circuit_create: log_n 26 is outside 1 .. 25", "zk_plonk_circuit_create: shift^(4n) is 1: Z_H vanishes on",
                  "zk_plonk_circuit_create: qm 5 is not below r", "zk_plonk_quotient: b_len 17 is outside 1 .. 2n =",
                  "zk_plonk_quotient: a_len + b_len + c_len + z_len = 25 exceeds 5n + 3 = 23", "zk_plonk_quotient: z 5 is not below r"):
        assert words in section, words


def test_every_export_is_bound_and_re_exported():
    from rapidsnark_old_amd import lib as L
    import rapidsnark_old_amd as zk
    lib = L.load_library()
    for name, nargs in ENTRIES.items():
        assert name in L.EXPORTS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    import ctypes as C
    assert C.sizeof(L.zk_plonk_circuit_plan) == 32 and C.sizeof(L.zk_plonk_circuit_view) == 8 + 8 * 8 + 64 + 8
    assert zk.fr_coset_ntt is zk.plonk.fr_coset_ntt and zk.PlonkCircuit is zk.plonk.PlonkCircuit


def test_python_refuses_bad_arguments_before_any_library_call(monkeypatch):
    from rapidsnark_old_amd import lib as L, plonk as P

    def never(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(L, "load_library", never)
    # the transform
    with pytest.raises(ValueError, match="values: value 1 is not in 0 .. r - 1"):
        P.fr_coset_ntt([0, R])
    with pytest.raises(ValueError, match="values: rows of 32 bytes"):
        P.fr_coset_ntt(bytes(33))
    with pytest.raises(ValueError, match="values: at least one value"):
        P.fr_coset_ntt([])
    with pytest.raises(ValueError, match="n_in 5 is outside 1 .. 2\\^log_m = 4"):
        P.fr_coset_ntt([1] * 5, log_m=2)
    with pytest.raises(ValueError, match="n_in 3 is not 2\\^log_m = 4"):
        P.fr_coset_ntt([1] * 3, log_m=2, inverse=True)
    with pytest.raises(ValueError, match="log_m 29 is outside 0 .. 28"):
        P.fr_coset_ntt([1], log_m=29)
    with pytest.raises(ValueError, match="shift is zero"):
        P.fr_coset_ntt([1, 2], shift=0)
    with pytest.raises(ValueError, match="shift: value 0 is not in 0 .. r - 1"):
        P.fr_coset_ntt([1, 2], shift=R)
    # the circuit
    q = [1, 2, 3, 4]
    ok = [q] * 8
    with pytest.raises(ValueError, match="basis 'evaluation' is unknown"):
        P.PlonkCircuit(*ok, 2, 3, basis="evaluation")
    with pytest.raises(ValueError, match="qo has 8 rows, ql has 4: the eight circuit vectors must have one length"):
        P.PlonkCircuit(q, q, q, q * 2, q, q, q, q, 2, 3)
    with pytest.raises(ValueError, match="n = 3 is not a power of two"):
        P.PlonkCircuit(*([[1, 2, 3]] * 8), 2, 3)
    with pytest.raises(ValueError, match="n = 0 is not a power of two"):
        P.PlonkCircuit(*([[]] * 8), 2, 3)
    with pytest.raises(ValueError, match="log_n 0 is outside 1 .. 25"):
        P.PlonkCircuit(*([[7]] * 8), 2, 3)
    with pytest.raises(ValueError, match="s2: value 2 is not in 0 .. r - 1"):
        P.PlonkCircuit(q, q, q, q, q, q, [1, 2, R, 4], q, 2, 3)
    with pytest.raises(ValueError, match="qc: rows of 32 bytes"):
        P.PlonkCircuit(q, q, q, q, bytes(4 * 32 + 1), q, q, q, 2, 3)
    with pytest.raises(ValueError, match="k1: value 0 is not in"):
        P.PlonkCircuit(*ok, R, 3)
    with pytest.raises(ValueError, match="k2: one value expected"):
        P.PlonkCircuit(*ok, 2, [3, 4])
    with pytest.raises(ValueError, match="shift is zero"):
        P.PlonkCircuit(*ok, 2, 3, shift=0)
    for g in (1, R - 1, pi.fr_root(4)):                 # orders 1, 2 and 4n = 16
        with pytest.raises(ValueError, match="shift\\^\\(4n\\) is 1: Z_H vanishes on the coset"):
            P.PlonkCircuit(*ok, 2, 3, shift=g)
    # the quotient: an object that was never made on a device still checks its arguments first
    c = P.PlonkCircuit.__new__(P.PlonkCircuit)
    c.n, c.log_n, c._h = 4, 2, None
    p = [1] * 4
    with pytest.raises(ValueError, match="c_len 0 is outside 1 .. 2n = 8"):
        c.quotient(p, p, [], p, 1, 2, 3)
    with pytest.raises(ValueError, match="z_len 9 is outside 1 .. 2n = 8"):
        c.quotient(p, p, p, [1] * 9, 1, 2, 3)
    with pytest.raises(ValueError, match="a_len \\+ b_len \\+ c_len \\+ z_len = 25 exceeds 5n \\+ 3 = 23"):
        c.quotient([1] * 6, [1] * 6, [1] * 6, [1] * 7, 1, 2, 3)
    with pytest.raises(ValueError, match="b: value 1 is not in 0 .. r - 1"):
        c.quotient(p, [0, R], p, p, 1, 2, 3)
    with pytest.raises(ValueError, match="z: rows of 32 bytes"):
        c.quotient(p, p, p, np.zeros(65, dtype=np.uint8), 1, 2, 3)
    with pytest.raises(ValueError, match="pi: 3 values, n = 4 expected"):
        c.quotient(p, p, p, p, 1, 2, 3, pi=[1, 2, 3])
    with pytest.raises(ValueError, match="alpha: value 0 is not in"):
        c.quotient(p, p, p, p, R, 2, 3)
    with pytest.raises(ValueError, match="gamma: one value expected"):
        c.quotient(p, p, p, p, 1, 2, [3, 4])
    with pytest.raises(L.ZkHipError, match="the PlonkCircuit object is closed"):
        c.quotient(p, p, p, p, 1, 2, 3)


@pytest.mark.parametrize("log_n,blind", [(1, None), (2, None), (3, None), (6, None), (3, pi.BLIND), (6, pi.BLIND)])
def test_the_two_oracles_agree(log_n, blind):
    """schoolbook and long division (remainder zero) against the coset route, coefficient for coefficient; the length is
    3n - 3 unblinded and 3n + 6 with the usual blinding"""
    inst = pi.make(2900 + log_n, log_n, blind)
    ta, rem = pi.oracle_a(inst)
    assert not any(rem)
    assert ta == pi.oracle_b(inst) == pi.oracle_b(inst, g=7)
    assert pi.t_len_of(ta) == (3 * inst.n + 6 if blind else 3 * inst.n - 3)


def test_a_broken_gate_leaves_a_remainder_and_fills_the_interpolant():
    inst = pi.make(2904, 4, pi.BLIND, break_gate=3)
    assert any(pi.oracle_a(inst)[1])
    assert pi.t_len_of(pi.oracle_b(inst)) == 4 * inst.n


def test_c_entries_refuse_bad_arguments_before_a_device_is_touched():
    """the checks of values and shapes come first: they answer on a machine without a device"""
    import ctypes
    from rapidsnark_old_amd import lib as L
    lib = L.load_library()
    P = lambda a: ctypes.c_void_p(a.ctypes.data)       # noqa: E731
    le = lambda v: np.frombuffer(pi.le(v), dtype=np.uint8).copy()      # noqa: E731
    good, bad = le([1, 2, 3, 4]), le([1, 2, R, R + 1])

    def create(log_n=2, shift=None, k2=3, swap=None, basis=0):
        v = L.zk_plonk_circuit_view()
        v.log_n, v.basis = log_n, basis
        for name in ("ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3"):
            setattr(v, name, (bad if name == swap else good).ctypes.data)
        ctypes.memmove(v.k1, pi.le([2]), 32)
        ctypes.memmove(v.k2, pi.le([k2]), 32)
        sb = le([shift]) if shift is not None else None
        v.shift = sb.ctypes.data if sb is not None else None
        h = ctypes.c_void_p()
        assert lib.zk_plonk_circuit_create(ctypes.byref(h), ctypes.byref(v), -1) == 1 and not h
        return lib.zk_last_error().decode()

    for g in (1, R - 1, pi.fr_root(4)):
        assert create(shift=g) == "zk_plonk_circuit_create: shift^(4n) is 1: Z_H vanishes on the coset"
    assert create(shift=0) == "zk_plonk_circuit_create: shift is zero"
    assert create(shift=R) == "zk_plonk_circuit_create: shift is not below r"
    assert create(k2=R) == "zk_plonk_circuit_create: k2 is not below r"
    assert create(log_n=0) == "zk_plonk_circuit_create: log_n 0 is outside 1 .. 25"
    assert create(log_n=26) == "zk_plonk_circuit_create: log_n 26 is outside 1 .. 25"
    assert create(basis=7) == "zk_plonk_circuit_create: basis 7 is unknown"
    assert create(swap="s3") == "zk_plonk_circuit_create: s3 2 is not below r"
    out = np.zeros(8 * 32, dtype=np.uint8)

    def ntt(values, n_in, log_m, shift, inverse):
        assert lib.zk_fr_coset_ntt(P(out), P(values), n_in, log_m, P(shift) if shift is not None else None, inverse, -1) == 1
        return lib.zk_last_error().decode()

    assert ntt(le([1, 2, 3, 4, 5, R, 7, 8]), 8, 3, None, 0) == "zk_fr_coset_ntt: value 5 is not below r"
    assert ntt(good, 4, 3, le([0]), 0) == "zk_fr_coset_ntt: shift is zero"
    assert ntt(good, 4, 3, le([R]), 0) == "zk_fr_coset_ntt: shift is not below r"
    assert ntt(good, 4, 29, None, 0) == "zk_fr_coset_ntt: log_m 29 is above 28"
    assert ntt(le([1] * 9), 9, 3, None, 0) == "zk_fr_coset_ntt: n_in 9 is outside 1 .. 2^log_m = 8"
    assert ntt(good, 4, 3, None, 1) == "zk_fr_coset_ntt: n_in 4 is not 2^log_m = 8"


# ---------------------------------------------------------------- instances with chosen coset evaluations
@pytest.mark.parametrize("log_n", [1, 3, 7])
def test_the_two_oracles_agree_on_the_empty_circuit(log_n):
    inst = pi.extreme_instance("empty", log_n)
    ta, rem = pi.oracle_a(inst)
    assert not any(rem) and not any(ta)
    assert ta == pi.oracle_b(inst) == pi.oracle_b(inst, g=7)
    assert pi.t_len_of(ta) == 0


@pytest.mark.parametrize("log_n", [1, 3, 7, 9])
def test_constant_instances_fill_the_interpolant(log_n):
    """a constant instance breaks the gate identity: oracle B's t has all 4n coefficients (fewer where alpha = 0 or z = 1)"""
    for name in pi.CONSTANT_FAMILIES if log_n < 9 else ("const_tmax", "const_top", "const_one"):
        inst = pi.extreme_instance(name, log_n)
        assert pi.t_len_of(pi.oracle_b(inst)) == pi.constant_t_len(name, inst.n), name
        assert any(pi.oracle_a(inst)[1]), name            # and long division leaves a remainder


def test_the_builders_hold_the_evaluations_they_name():
    import extreme_inputs as xi
    log_n, g = 4, 5
    n = 1 << log_n
    inst = pi.extreme_instance("even_alternating", log_n, g)
    assert [len(p) for p in (inst.a, inst.b, inst.c, inst.z)] == [2 * n, 2 * n, 1, 1]
    a = pi.coset_ext(inst.a, log_n + 2, g)
    b = pi.coset_ext(inst.b, log_n + 2, g)
    assert [xi.loaded_word(v) for v in a[0::2]] == [R - 1, 1] * n and [xi.loaded_word(v) for v in b[0::2]] == [1, R - 1] * n
    assert [xi.loaded_word(v) for v in pi.coset_ext(inst.ql, log_n + 2, g)[0::4]] == [R - 1, 1] * (n // 2)
    assert inst.ql_v == pi.ntt(inst.ql) and pi.ntt(inst.ql_v, inverse=True) == inst.ql
    inst = pi.extreme_instance("even_mask01", log_n, g)
    assert set(xi.loaded_word(v) for v in pi.coset_ext(inst.a, log_n + 2, g)[0::2]) == {0, R - 1}
    assert set(xi.loaded_word(v) for v in pi.coset_ext(inst.z, log_n + 2, g)) == {R - 1}
    # a builder that is handed the wrong evaluations says so: the assertion is the check
    with pytest.raises(AssertionError):
        pi.even_point_instance(log_n, [1] * n, [1] * 2 * n, {}, {}, (1, 2, 3))
    inst = pi.extreme_instance("longest", log_n)
    assert [len(p) for p in (inst.a, inst.b, inst.c, inst.z)] == [2 * n, 2 * n, n, 3] and inst.a[-1] == inst.b[-1] == R - 1
    # sigma the identity with a constant z: the permutation term vanishes at any point
    inst = pi.extreme_instance("sigma_identity", log_n)
    zeta = 0x1234567
    assert pi.num_at(inst, zeta) == inst.alpha * inst.alpha * (inst.z[0] - 1) * (pow(zeta, n, R) - 1) * pow(n * (zeta - 1), -1, R) % R
