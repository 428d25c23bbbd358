"""The KZG layer without a device: the header declares the entries and the structs, the ctypes structs have the C layout
(a C program prints sizeof and the offsets), every export is bound, and the Python side refuses bad shapes, ints out of
range and unknown bases before any library call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkhip.h")
VIEW = ["power", "tau_g1", "tau_g1_bytes", "tau_g2", "tau_g2_bytes", "lagrange_g1", "lagrange_g1_bytes"]
PLAN = ["size", "lagrange_log_n", "max_coeffs", "device_bytes", "seg", "last_launches"]
ENTRIES = ["zk_fr_poly_divide", "zk_kzg_create", "zk_kzg_destroy", "zk_kzg_info", "zk_kzg_commit", "zk_kzg_open", "zk_kzg_verify",
           "zk_kzg_verify_batch"]
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def test_header_declares_the_entries_and_the_structs():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    for decl in ("int zk_fr_poly_divide(uint8_t *q, uint8_t y[32], const uint8_t *coeffs, uint64_t n, const uint8_t z[32], int32_t device);",
                 "int zk_kzg_create(zk_kzg **out, const zk_kzg_view *view, uint64_t max_coeffs, uint32_t lagrange_log_n, int32_t device);",
                 "void zk_kzg_destroy(zk_kzg *kzg);",
                 "int zk_kzg_info(zk_kzg *kzg, zk_kzg_plan *plan);",
                 "int zk_kzg_commit(zk_kzg *kzg, uint8_t *out, const uint8_t *coeffs, uint64_t n, uint64_t m, uint32_t basis);",
                 "int zk_kzg_open(zk_kzg *kzg, uint8_t *ys, uint8_t *proofs, const uint8_t *coeffs, uint64_t n, uint64_t m, const uint8_t *zs);",
                 "int zk_kzg_verify(zk_kzg *kzg, const uint8_t *commitments, const uint8_t *zs, const uint8_t *ys, const uint8_t *proofs, uint64_t m, uint8_t *verdict);",
                 "int zk_kzg_verify_batch(zk_kzg *kzg, const uint8_t *commitments, const uint8_t *zs, const uint8_t *ys, const uint8_t *proofs, uint64_t m, "
                 "const uint8_t *scalars16, uint8_t *verdict);"):
        assert decl in flat, decl
    assert "} zk_kzg_view;" in flat and "} zk_kzg_plan;" in flat and "typedef struct zk_kzg zk_kzg;" in flat
    assert "#define ZK_KZG_MONOMIAL 0" in text and "#define ZK_KZG_LAGRANGE 1" in text and "#define ZK_KZG_NO_LAGRANGE 0xffffffffu" in text
    # the conventions, the knob, what create does not check, and the warning about known scalars
    for words in ("KZG polynomial commitments over a .ptau", "ZKHIP_KZG_SEG", "NOT checked", "FOR TESTS ONLY", "zk_g1_lagrange", "STANDARD form"):
        assert words in text, words
    # the verdict constants are the ones zk_vkey_verify has
    assert text.count("#define ZK_VERIFY_OK 0") == 1


def test_ctypes_structs_have_the_c_layout(tmp_path):
    from rapidsnark_old_amd import lib as L
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkhip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(zk_kzg_view));\n'
                   + "".join('    printf(" %%zu", offsetof(zk_kzg_view, %s));\n' % f for f in VIEW)
                   + '    printf(" %zu", sizeof(zk_kzg_plan));\n'
                   + "".join('    printf(" %%zu", offsetof(zk_kzg_plan, %s));\n' % f for f in PLAN)
                   + '    printf("\\n");\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert [name for name, _ in L.zk_kzg_view._fields_] == VIEW and [name for name, _ in L.zk_kzg_plan._fields_] == PLAN
    want = ([ctypes.sizeof(L.zk_kzg_view)] + [getattr(L.zk_kzg_view, f).offset for f in VIEW]
            + [ctypes.sizeof(L.zk_kzg_plan)] + [getattr(L.zk_kzg_plan, f).offset for f in PLAN])
    assert got == want
    assert got[0] == 56 and got[len(VIEW) + 1] == 32


def test_every_export_is_bound():
    from rapidsnark_old_amd import lib as L
    import rapidsnark_old_amd as zk
    lib = L.load_library()
    for name in ENTRIES:
        assert name in L.EXPORTS and hasattr(lib, name), name
    assert (L.ZK_KZG_MONOMIAL, L.ZK_KZG_LAGRANGE, L.ZK_KZG_NO_LAGRANGE) == (0, 1, 0xffffffff)
    assert len(lib.zk_kzg_create.argtypes) == 5 and lib.zk_kzg_create.argtypes[1]._type_ is L.zk_kzg_view
    assert len(lib.zk_kzg_commit.argtypes) == 6 and len(lib.zk_kzg_open.argtypes) == 7
    assert len(lib.zk_kzg_verify.argtypes) == 7 and len(lib.zk_kzg_verify_batch.argtypes) == 8
    assert len(lib.zk_fr_poly_divide.argtypes) == 6 and lib.zk_kzg_info.argtypes[1]._type_ is L.zk_kzg_plan
    assert zk.Kzg is zk.kzg.Kzg and zk.fr_poly_divide is zk.kzg.fr_poly_divide and hasattr(zk.PtauFile, "kzg_view")


def test_python_refuses_bad_arguments_before_any_library_call(monkeypatch):
    from rapidsnark_old_amd import lib as L, kzg as K

    def never(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(L, "load_library", never)
    k = K.Kzg.__new__(K.Kzg)                            # an object without a device: only the argument checks run
    k.max_coeffs, k.lagrange_log_n, k.power, k._h = 100, 3, 6, ctypes.c_void_p(1)
    try:
        with pytest.raises(ValueError, match="basis 'evaluation' is unknown"):
            k.commit([1, 2, 3], basis="evaluation")
        with pytest.raises(ValueError, match="value 1 is not in 0 .. r - 1"):
            k.commit([0, R])
        with pytest.raises(ValueError, match="value 0 is not in 0 .. r - 1"):
            k.commit([-1])
        with pytest.raises(ValueError, match="rows of 32 bytes"):
            k.commit(bytes(33))
        with pytest.raises(ValueError, match="at least one coefficient"):
            k.commit([])
        with pytest.raises(ValueError, match="one length"):
            k.commit([[1, 2], [3]])
        with pytest.raises(ValueError, match="n = 101 exceeds max_coeffs = 100"):
            k.commit([1] * 101)
        with pytest.raises(ValueError, match="n = 4, the Lagrange level holds 8 points"):
            k.commit([1] * 4, basis="lagrange")
        with pytest.raises(ValueError, match="2 values for 1 polynomials"):
            k.open([1, 2, 3], [5, 6])
        with pytest.raises(ValueError, match="zs: value 0 is not in 0 .. r - 1"):
            k.open([1, 2, 3], [R])
        with pytest.raises(ValueError, match="n = 101 exceeds max_coeffs = 100"):
            k.open(np.zeros((2, 101 * 32), dtype=np.uint8), [1, 2])
        with pytest.raises(ValueError, match="points of 64 bytes"):
            k.verify(bytes(63), [1], [1], bytes(64))
        with pytest.raises(ValueError, match="one of each per opening"):
            k.verify(bytes(128), [1], [1, 2], bytes(128))
        with pytest.raises(ValueError, match="ys: value 0 is not in"):
            k.verify(bytes(64), [1], [1 << 256], bytes(64))
        with pytest.raises(ValueError, match="scalars: values in 1 .. 2\\^128 - 1"):
            k.verify_batch(bytes(64), [1], [1], bytes(64), scalars=[0])
        with pytest.raises(ValueError, match="scalars: values in 1 .. 2\\^128 - 1"):
            k.verify_batch(bytes(64), [1], [1], bytes(64), scalars=[1 << 128])
        with pytest.raises(ValueError, match="scalars: 1 x 16 bytes expected"):
            k.verify_batch(bytes(64), [1], [1], bytes(64), scalars=bytes(32))
        with pytest.raises(ValueError, match="coeffs: value 2 is not in"):
            K.fr_poly_divide([1, 2, R + 5], 3)
        with pytest.raises(ValueError, match="z: value 0 is not in"):
            K.fr_poly_divide([1, 2], R)
        with pytest.raises(ValueError, match="at least one coefficient"):
            K.fr_poly_divide([], 3)
        k.lagrange_log_n = None
        with pytest.raises(ValueError, match="no Lagrange level"):
            k.commit([1] * 8, basis="lagrange")
        k._h = ctypes.c_void_p()
        with pytest.raises(L.ZkHipError, match="closed"):
            k.commit([1, 2, 3])
        with pytest.raises(L.ZkHipError, match="closed"):
            k.verify(bytes(64), [1], [1], bytes(64))
    finally:
        k._h = ctypes.c_void_p()                        # nothing for __del__ to destroy


def test_create_refuses_sizes_the_file_cannot_serve_before_any_library_call(monkeypatch):
    from rapidsnark_old_amd import lib as L, kzg as K, ptau as P

    def never(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(L, "load_library", never)
    f = P.PtauFile.__new__(P.PtauFile)                  # a header without a file behind it
    f.power, f.sections = 6, {2: (0, 0), 3: (0, 0)}
    with pytest.raises(ValueError, match="max_coeffs 128 is outside 1 .. 127"):
        K.Kzg(f, max_coeffs=128)
    with pytest.raises(ValueError, match="max_coeffs 0 is outside"):
        K.Kzg(f, max_coeffs=0)
    with pytest.raises(ValueError, match="lagrange_log_n 7 is outside 0 .. 6"):
        K.Kzg(f, lagrange_log_n=7)
    with pytest.raises(ValueError, match="needs a prepared file"):
        K.Kzg(f, lagrange_log_n=6)
    with pytest.raises(TypeError):
        K.Kzg("pot.ptau")
