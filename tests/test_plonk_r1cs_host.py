"""PLONK from an R1CS without a device: the generator's circuits are satisfiable and the Python compile of
tests/plonk_r1cs_instance.py, which the device tests compare with byte for byte, passes check() for every shape and fails it
once a coefficient, a map entry or a pair of sigma is changed; N and n_witness follow the header's formula; the header declares
the entries and the binding agrees with it; the refusals that need no device carry the header's text."""
import ctypes
import os
import re

import numpy as np
import pytest

import plonk_r1cs_instance as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkhip.h")
ENTRIES = {"zk_plonk_r1cs_create": 5, "zk_plonk_r1cs_destroy": 1, "zk_plonk_r1cs_info": 2, "zk_plonk_r1cs_circuit": 5, "zk_plonk_r1cs_extend": 4,
           "zk_plonk_prover_create_r1cs": 5, "zk_plonk_prove_r1cs": 5}
R = pr.R
ALL = sorted(pr.SHAPES) + [pr.WIDE]


def compiled(name):
    c = pr.case(name)
    return c, pr.compile_r1cs(c.data)


# ---------------------------------------------------------------- the reference compile
@pytest.mark.parametrize("name", ALL)
def test_check_passes_for_every_shape(name):
    c, k = compiled(name)
    w = pr.extend(k, c.witness)
    assert len(w) == k.n_witness and w[:k.n_wires] == c.witness
    assert pr.check(k, w, c.publics) is None


@pytest.mark.parametrize("name", ALL)
def test_rows_and_witness_length_follow_the_formula(name):
    c, k = compiled(name)
    N, adds = pr.expected_rows(c.data)
    assert (k.rows, k.n_additions, k.n_witness) == (N, adds, len(c.witness) + adds)
    assert k.log_n == max(3, (N - 1).bit_length()) and k.n == 1 << k.log_n
    assert all(len(v) == k.n for v in k.vectors + k.maps)
    for v in k.vectors[:5]:
        assert not any(v[N:])
    assert not any(m[i] for m in k.maps for i in range(N, k.n))


def test_the_shapes_are_the_ones_they_claim():
    assert [compiled(n)[1].rows for n in ("one_constraint", "rows_16", "rows_17", "rows_16_public_2")] == [1, 16, 17, 16]
    assert [compiled(n)[1].log_n for n in ("one_constraint", "rows_16", "rows_17", "proof_3", "proof_4", "proof_6", "proof_8")] == [3, 4, 5, 3, 4, 6, 8]
    k = compiled("long_row")[1]
    assert k.n_additions == 999 and sum(1 for e in k.ext if e[2]) == 1
    c, k = compiled("wire_in_all_columns")
    assert all(3 in m for m in k.maps) and not any(5 in m for m in k.maps)
    c, k = compiled("all_inputs_public")
    assert k.n_public == 5
    c, k = compiled(pr.WIDE)
    assert k.log_n == 17 and k.rows == k.n and k.n_witness > 1 << 16
    assert k.maps[1][0] == 0 and k.maps[0][k.n - 1] == 0 and k.maps[2][k.n - 1] == 0


@pytest.mark.parametrize("name", ["chains", "constants", "proof_4"])
def test_check_fails_after_one_change(name):
    c, k = compiled(name)
    w = pr.extend(k, c.witness)
    row = k.rows - 1
    a, b, cc = (w[m[row]] for m in k.maps)
    for j, moved in enumerate((a, b, a * b % R, cc, 1)):    # one coefficient: the gate moves by what it multiplies
        vec = [list(v) for v in k.vectors]
        vec[j][row] = (vec[j][row] + 1) % R
        assert pr.check(k._replace(vectors=vec), w, c.publics) == ("gate %d" % row if moved else None), j
    assert a and b and cc
    maps = [list(m) for m in k.maps]                        # one map entry: the gate, or at the least the cycles
    maps[2][row] = 1 if maps[2][row] != 1 else 2
    assert pr.check(k._replace(maps=maps), w, c.publics) is not None
    vec = [list(v) for v in k.vectors]                      # one swapped pair of sigma
    vec[5][0], vec[6][1] = vec[6][1], vec[5][0]
    assert pr.check(k._replace(vectors=vec), w, c.publics) in ("the cycle of wire %d" % x for x in range(k.n_witness))
    vec = [list(v) for v in k.vectors]
    vec[7][2] = vec[7][3]                                   # no permutation any more
    assert pr.check(k._replace(vectors=vec), w, c.publics) == "sigma is not a permutation of the cells"
    bad = list(w)
    bad[-1] = (bad[-1] + 1) % R                             # one changed private value
    assert pr.check(k, bad, c.publics).startswith("gate ")
    if k.n_public:
        assert pr.check(k, w, [(c.publics[0] + 1) % R] + c.publics[1:]) == "gate 0"


def test_wire_0_twice_is_refused_by_the_reference_too():
    from rapidsnark_old_amd.r1cs import write_r1cs_rows
    one = [(1, 1)]
    A = [one, one, [(0, 1), (1, 1), (0, 0)], one]
    B = [one, one, [(0, 2), (2, 1), (0, 3)], [(0, 1), (0, 1)]]
    C = [one, [(0, 0), (0, 0)], [(0, 1), (0, 1)], one]
    with pytest.raises(ValueError, match="zk_plonk_r1cs_create: constraint 2: B names wire 0 twice"):
        pr.compile_r1cs(write_r1cs_rows(A, B, C, 3, 0))


# ---------------------------------------------------------------- header and binding
def test_header_declares_the_entries():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    for decl in ("typedef struct zk_plonk_r1cs zk_plonk_r1cs;",
                 "int zk_plonk_r1cs_create(zk_plonk_r1cs **out, const zk_r1cs_view *view, const uint8_t k1[32], const uint8_t k2[32], int32_t device);",
                 "void zk_plonk_r1cs_destroy(zk_plonk_r1cs *c);",
                 "int zk_plonk_r1cs_info(zk_plonk_r1cs *c, zk_plonk_r1cs_plan *plan);",
                 "int zk_plonk_r1cs_circuit(zk_plonk_r1cs *c, uint8_t *vectors, uint32_t *a_map, uint32_t *b_map, uint32_t *c_map);",
                 "int zk_plonk_r1cs_extend(zk_plonk_r1cs *c, uint8_t *out, const uint8_t *wtns, uint32_t nVars);",
                 "int zk_plonk_prover_create_r1cs(zk_plonk_prover **out, zk_kzg *kzg, zk_plonk_r1cs *compiled, const uint8_t *shift, int32_t device);",
                 "int zk_plonk_prove_r1cs(zk_plonk_prover *p, uint8_t proof[ZK_PLONK_PROOF_BYTES], const uint8_t *wtns, uint32_t nVars, "
                 "const uint8_t *blind);"):
        assert decl in flat, decl
    section = text[text.index("PLONK from an R1CS"):]
    for words in ("parity with snarkjs is UNPINNED", "ZKHIP_R1CS_SEG: a number of elements per lane from 1 to 4096 expected", "t_L = 0: (wire 0, 0)",
                  "qm = c_A c_B, ql = c_A k_B, qr = k_A c_B, qo = -c_C, qc = k_A k_B - k_C", "log_n = max(3, ceil(log2 N))",
                  "New wires are numbered nWires + q", "index col n + row", "padding included", "A wire no cell", "names has no cycle",
                  "zk_plonk_r1cs_create: constraint 5: B names wire 0 twice", "A before B before C", "rows exceed 2^25", "is not below 2^32",
                  "do not name three different cosets", "witness has 5 values, the r1cs 7 wires", "zk_plonk_prove_r1cs: the prover was not made from an r1cs"):
        assert words in section, words


def test_every_export_is_bound_and_re_exported():
    from rapidsnark_old_amd import lib as L
    import rapidsnark_old_amd as zk
    lib = L.load_library()
    for name, nargs in ENTRIES.items():
        assert name in L.EXPORTS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert ctypes.sizeof(L.zk_plonk_r1cs_plan) == 80
    assert L.zk_plonk_r1cs_plan.rows.offset == 8 and L.zk_plonk_r1cs_plan.device_bytes.offset == 56 and L.zk_plonk_r1cs_plan.last_launches.offset == 72
    assert zk.PlonkR1cs is zk.plonk.PlonkR1cs
    assert callable(zk.PlonkProver.from_r1cs) and callable(zk.PlonkProver.prove_r1cs)


# ---------------------------------------------------------------- refusals before a device is touched
def _view(L, case):
    from rapidsnark_old_amd.r1cs import open_r1cs
    h, sec = open_r1cs(case.data)
    keep = np.frombuffer(sec, dtype=np.uint8)
    return L.zk_r1cs_view(h.nWires, h.nPubOut, h.nPubIn, h.nPrvIn, h.nConstraints, keep.ctypes.data, keep.size), keep


def _k(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8).copy()


def test_c_entries_refuse_bad_arguments_before_a_device_is_touched(monkeypatch):
    from rapidsnark_old_amd import lib as L
    from oracle.bn254 import fr_root
    lib = L.load_library()
    P = lambda a: ctypes.c_void_p(a.ctypes.data)       # noqa: E731
    err = lambda: lib.zk_last_error().decode()          # noqa: E731
    v, keep = _view(L, pr.case("chains"))
    h = ctypes.c_void_p()
    two, three = _k(2), _k(3)

    def create(k1, k2, view=v):
        a, b = _k(k1), _k(k2)                           # alive during the call
        return lib.zk_plonk_r1cs_create(ctypes.byref(h), ctypes.byref(view), P(a), P(b), -1)

    assert lib.zk_plonk_r1cs_create(None, ctypes.byref(v), P(two), P(three), -1) == 1 and err() == "null argument"
    assert lib.zk_plonk_r1cs_create(ctypes.byref(h), None, P(two), P(three), -1) == 1 and err() == "null argument"
    assert lib.zk_plonk_r1cs_create(ctypes.byref(h), ctypes.byref(v), None, P(three), -1) == 1 and err() == "null argument"
    assert create(R, 3) == 1 and err() == "zk_plonk_r1cs_create: k1 is not below r"
    assert create(2, R + 5) == 1 and err() == "zk_plonk_r1cs_create: k2 is not below r"
    assert create(0, 3) == 1 and err() == "zk_plonk_r1cs_create: k1 or k2 is zero"
    cosets = "zk_plonk_r1cs_create: 1, k1 and k2 do not name three different cosets of the n-th roots of unity"
    for k1, k2 in ((7, 7), (1, 3), (2, fr_root(3)), (2, 2 * fr_root(2) % R)):
        assert create(k1, k2) == 1 and err() == cosets, (k1, k2)
    monkeypatch.setenv("ZKHIP_R1CS_SEG", "0")
    assert create(2, 3) == 1 and err() == "ZKHIP_R1CS_SEG: a number of elements per lane from 1 to 4096 expected"
    monkeypatch.setenv("ZKHIP_R1CS_SEG", "8x")
    assert create(2, 3) == 1 and err() == "ZKHIP_R1CS_SEG: a number of elements per lane from 1 to 4096 expected"
    monkeypatch.delenv("ZKHIP_R1CS_SEG")
    short = L.zk_r1cs_view(v.nWires, v.nPubOut, v.nPubIn, v.nPrvIn, v.nConstraints, v.constraints, v.constraints_bytes - 36)
    assert create(2, 3, short) == 1 and err().startswith("r1cs constraints section is truncated (constraint ")
    nopriv = L.zk_r1cs_view(2, 0, 2, 0, v.nConstraints, v.constraints, v.constraints_bytes)
    assert create(2, 3, nopriv) == 1 and err() == "zk_plonk_r1cs_create: nPublic 2 is not below nWires = 2"
    assert not h
    buf = np.zeros(768, dtype=np.uint8)
    plan = L.zk_plonk_r1cs_plan()
    assert lib.zk_plonk_r1cs_info(None, ctypes.byref(plan)) == 1 and err() == "null argument"
    assert lib.zk_plonk_r1cs_circuit(None, P(buf), P(buf), P(buf), P(buf)) == 1 and err() == "null argument"
    assert lib.zk_plonk_r1cs_extend(None, P(buf), P(buf), 1) == 1 and err() == "null argument"
    assert lib.zk_plonk_prover_create_r1cs(ctypes.byref(h), None, None, None, -1) == 1 and err() == "null argument"
    assert lib.zk_plonk_prove_r1cs(None, P(buf), P(buf), 1, None) == 1 and err() == "null argument"
    lib.zk_plonk_r1cs_destroy(None)


def test_python_refuses_before_any_library_call(monkeypatch):
    from rapidsnark_old_amd import lib as L, plonk as P

    def never(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(L, "load_library", never)
    data = pr.case("one_constraint").data
    with pytest.raises(ValueError, match="k1: value 0 is not in 0 .. r - 1"):
        P.PlonkR1cs(data, k1=R)
    with pytest.raises(ValueError, match="r1cs file is truncated"):
        P.PlonkR1cs(data[:40])
    with pytest.raises(TypeError, match="a Kzg expected"):
        P.PlonkProver.from_r1cs(None, data)
    c = P.PlonkR1cs.__new__(P.PlonkR1cs)
    c._h, c._circuit, c.n_witness = None, None, 3
    c.header = type("H", (), {"nWires": 3})()
    for call in (lambda: c.vectors, lambda: c.maps, c.info, lambda: c.extend(np.zeros(96, dtype=np.uint8))):
        with pytest.raises(L.ZkHipError, match="the PlonkR1cs object is closed"):
            call()
    p = P.PlonkProver.__new__(P.PlonkProver)
    p._h = None
    with pytest.raises(L.ZkHipError, match="the PlonkProver object is closed"):
        p.prove_r1cs(np.zeros(96, dtype=np.uint8))
