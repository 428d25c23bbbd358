"""The running products over Fr without a device: the header declares the four entries with their exact prototypes and
documents the knob and the conventions, every export is bound and re-exported, and the Python side refuses bad shapes and
values out of range before any library call."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkhip.h")
ENTRIES = {"zk_fr_batch_inverse": 5, "zk_fr_prefix_product": 5, "zk_fr_grand_product": 6, "zk_plonk_permutation_product": 10}
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def test_header_declares_the_entries():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    for decl in ("int zk_fr_batch_inverse(uint8_t *out, const uint8_t *in, uint64_t n, uint64_t *zeros, int32_t device);",
                 "int zk_fr_prefix_product(uint8_t *out, const uint8_t *in, uint64_t n, uint32_t flags, int32_t device);",
                 "int zk_fr_grand_product(uint8_t *z, uint8_t last[32], const uint8_t *num, const uint8_t *den, uint64_t n, int32_t device);",
                 "int zk_plonk_permutation_product(uint8_t *z, uint8_t last[32], const uint8_t *wires, const uint8_t *sigmas, uint32_t cols, "
                 "uint32_t log_n, const uint8_t *shifts, const uint8_t beta[32], const uint8_t gamma[32], int32_t device);"):
        assert decl in flat, decl
    assert "#define ZK_SCAN_EXCLUSIVE 1u" in text
    section = text[text.index("Grand products and batch inversion over Fr"):]
    for words in ("ZKHIP_SCAN_SEG", "STANDARD form", "NOT checked", "ZKHIP_SCAN_SEG: a number of elements per lane from 1 to 4096 expected",
                  "zk_fr_grand_product: denominator 5 is zero", "zk_plonk_permutation_product: row 5 has a zero denominator"):
        assert words in section, words


def test_every_export_is_bound_and_re_exported():
    from rapidsnark_old_amd import lib as L
    import rapidsnark_old_amd as zk
    lib = L.load_library()
    for name, nargs in ENTRIES.items():
        assert name in L.EXPORTS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert L.ZK_SCAN_EXCLUSIVE == 1
    for name in ("fr_batch_inverse", "fr_prefix_product", "fr_grand_product", "plonk_permutation_product"):
        assert getattr(zk, name) is getattr(zk.frscan, name), name


def test_python_refuses_bad_arguments_before_any_library_call(monkeypatch):
    from rapidsnark_old_amd import lib as L, frscan as F

    def never(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(L, "load_library", never)
    # values out of range, rows that are not 32 bytes
    for call in (lambda v: F.fr_batch_inverse(v), lambda v: F.fr_prefix_product(v), lambda v: F.fr_prefix_product(v, exclusive=True),
                 lambda v: F.fr_grand_product(v, [1, 1]), lambda v: F.fr_grand_product([1, 1], v)):
        with pytest.raises(ValueError, match="value 1 is not in 0 .. r - 1"):
            call([0, R])
        with pytest.raises(ValueError, match="value 0 is not in 0 .. r - 1"):
            call([-1, 5])
    with pytest.raises(ValueError, match="values: rows of 32 bytes"):
        F.fr_batch_inverse(bytes(33))
    with pytest.raises(ValueError, match="values: rows of 32 bytes"):
        F.fr_prefix_product(np.zeros(31, dtype=np.uint8))
    with pytest.raises(ValueError, match="den: rows of 32 bytes"):
        F.fr_grand_product(bytes(64), bytes(65))
    with pytest.raises(ValueError, match="2 numerators, 3 denominators"):
        F.fr_grand_product([1, 2], [1, 2, 3])
    # the permutation entry
    w = [[1, 2, 3, 4]] * 3
    with pytest.raises(ValueError, match="wires is 3 x 4, sigmas is 2 x 4"):
        F.plonk_permutation_product(w, w[:2], [1, 2, 3], 5, 7)
    with pytest.raises(ValueError, match="wires is 3 x 4, sigmas is 3 x 8"):
        F.plonk_permutation_product(w, [[1] * 8] * 3, [1, 2, 3], 5, 7)
    with pytest.raises(ValueError, match="wires is 3 x 4, sigmas is 3 x 8"):
        F.plonk_permutation_product(np.zeros((3, 4 * 32), dtype=np.uint8), np.zeros((3, 8 * 32), dtype=np.uint8), [1, 2, 3], 5, 7)
    with pytest.raises(ValueError, match="the columns must have one length"):
        F.plonk_permutation_product([[1, 2], [1]], [[1, 2], [1, 2]], [1, 2], 5, 7)
    with pytest.raises(ValueError, match="n = 3 is not a power of two"):
        F.plonk_permutation_product([[1, 2, 3]], [[1, 2, 3]], [1], 5, 7)
    with pytest.raises(ValueError, match="n = 0 is not a power of two"):
        F.plonk_permutation_product([[]], [[]], [1], 5, 7)
    with pytest.raises(ValueError, match="cols 0 is outside 1 .. 8"):
        F.plonk_permutation_product([], [], [], 5, 7)
    with pytest.raises(ValueError, match="cols 9 is outside 1 .. 8"):
        F.plonk_permutation_product([[1, 2]] * 9, [[1, 2]] * 9, list(range(1, 10)), 5, 7)
    with pytest.raises(ValueError, match="shifts: 2 values for 3 columns"):
        F.plonk_permutation_product(w, w, [1, 2], 5, 7)
    with pytest.raises(ValueError, match="a list of columns expected"):
        F.plonk_permutation_product([1, 2, 3, 4], w, [1, 2, 3], 5, 7)
    with pytest.raises(ValueError, match=r"wires\[1\]: value 2 is not in 0 .. r - 1"):
        F.plonk_permutation_product([[1, 2, 3, 4], [1, 2, R, 4]], w[:2], [1, 2], 5, 7)
    with pytest.raises(ValueError, match=r"sigmas\[0\]: value 0 is not in"):
        F.plonk_permutation_product(w[:1], [[-1, 2, 3, 4]], [1], 5, 7)
    with pytest.raises(ValueError, match="shifts: value 1 is not in"):
        F.plonk_permutation_product(w[:2], w[:2], [1, R], 5, 7)
    with pytest.raises(ValueError, match="beta: value 0 is not in"):
        F.plonk_permutation_product(w, w, [1, 2, 3], R, 7)
    with pytest.raises(ValueError, match="gamma: value 0 is not in"):
        F.plonk_permutation_product(w, w, [1, 2, 3], 5, -1)
    with pytest.raises(ValueError, match="beta: one value expected"):
        F.plonk_permutation_product(w, w, [1, 2, 3], [5, 6], 7)
    # nothing to do: no library call either
    out, zeros = F.fr_batch_inverse([])
    assert out.size == 0 and zeros == 0 and F.fr_prefix_product([]).size == 0
    z, last = F.fr_grand_product([], [])
    assert z.size == 0 and last == 1
