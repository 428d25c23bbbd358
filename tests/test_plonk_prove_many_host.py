"""The PLONK prover's many-call without a device: the header declares the entries, the statuses and the plan; the ctypes struct
has the compiled layout; the entries are bound and PlonkProver has the methods; Python refuses lengths and mismatches between
witnesses, publics and blinds before any library call; the C entries refuse what needs no device; and
tools/plonk_many_host_test.cpp (csrc/plonk_many_plan.hpp alone: the chunks, the width rule and its knob, both limits at their
edges with their messages, slots that do not overlap) builds for the host under the address and undefined-behaviour sanitizers
and exits 0."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "zkhip.h")
PLAN = ["size", "batch", "table_batch", "window_bits", "table_rows", "reserved", "table_bytes", "slot_bytes", "msm_bytes", "last_chunks",
        "last_multiplications", "last_launches", "last_drains", "last_refused", "reserved2"]


def test_header_declares_the_entries():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    for decl in ("int zk_plonk_prove_many(zk_plonk_prover *p, uint64_t m, uint8_t *proofs, uint32_t *status, const uint8_t *witnesses, const uint8_t *publics, "
                 "const uint8_t *blinds);",
                 "int zk_plonk_prove_r1cs_many(zk_plonk_prover *p, uint64_t m, uint8_t *proofs, uint32_t *status, const uint8_t *wtns, uint32_t nVars, "
                 "const uint8_t *blinds);",
                 "int zk_plonk_prover_commit_many(zk_plonk_prover *p, uint8_t *out, const uint8_t *coeffs, uint64_t k);",
                 "int zk_plonk_prover_many_info(zk_plonk_prover *p, zk_plonk_prover_many_plan *plan);",
                 "#define ZK_PLONK_MANY_MAX_BATCH 64", "#define ZK_PLONK_MANY_MADE 0", "#define ZK_PLONK_MANY_ZERO_DENOMINATOR 1", "#define ZK_PLONK_MANY_COPIES 2",
                 "#define ZK_PLONK_MANY_GATES 3", "#define ZK_PLONK_MANY_NOT_BELOW_R 4"):
        assert decl in flat, decl
    assert flat.index("int zk_plonk_prove(") < flat.index("int zk_plonk_prove_many(") < flat.index("int zk_plonk_verify(")
    section = re.sub(r"[\s*]+", " ", text[text.index("MANY WITNESSES A CALL"):text.index("int zk_plonk_prover_many_info")])
    for words in ("ZKHIP_PLONK_PROVE_BATCH: a number of proofs from 1 to 64 expected", "four multiplications a chunk whatever it holds",
                  "does not take the others with it", "left untouched", "zk_plonk_prove_many: proof 3: the copy constraints do not hold",
                  "zk_plonk_prove_many: proof 3: witness 5 is not below r", "m = 0 is accepted and touches no device", "FOR TESTS",
                  "3 x 64 x 1048582 scalars x 13 windows = 2617260672 >= 2^31 table rows; ZKHIP_PLONK_PROVE_BATCH=52 would fit",
                  "zk_plonk_prover_commit_many: vector 2 coefficient 5 is not below r", "witness has 5 values, the r1cs 7 wires",
                  "zk_plonk_prove_r1cs_many: the prover was not made from an r1cs (zk_plonk_prover_create_r1cs)"):
        assert words in section, words


def test_ctypes_struct_has_the_c_layout(tmp_path):
    from rapidsnark_old_amd import lib as L
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkhip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(zk_plonk_prover_many_plan));\n'
                   + "".join('    printf(" %%zu", offsetof(zk_plonk_prover_many_plan, %s));\n' % f for f in PLAN)
                   + '    printf(" %zu\\n", sizeof(zk_plonk_prover_plan));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert [name for name, _ in L.zk_plonk_prover_many_plan._fields_] == PLAN
    assert got[:-1] == [ctypes.sizeof(L.zk_plonk_prover_many_plan)] + [getattr(L.zk_plonk_prover_many_plan, f).offset for f in PLAN]
    assert got[0] == 72 and got[-1] == ctypes.sizeof(L.zk_plonk_prover_plan)          # and the lone prover's plan is what it was


def test_the_entries_are_bound():
    from rapidsnark_old_amd import lib as L
    import rapidsnark_old_amd as zk
    lib = L.load_library()
    for name, nargs in (("zk_plonk_prove_many", 7), ("zk_plonk_prove_r1cs_many", 7), ("zk_plonk_prover_commit_many", 4), ("zk_plonk_prover_many_info", 2)):
        assert name in L.EXPORTS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    for name in ("prove_many", "prove_r1cs_many", "commit_many", "many_info"):
        assert hasattr(zk.PlonkProver, name), name


class _NoDevice:
    """PlonkProver's argument handling without the object: no handle is ever asked for"""
    n, n_witness, n_public, r1cs, device = 8, 5, 2, None, 0
    _h = True

    def _handle(self):
        raise AssertionError("a library call was about to be made")


def test_python_refuses_bad_arguments_before_the_call():
    import rapidsnark_old_amd as zk
    fake = _NoDevice()
    fake._many_blinds = lambda b, m: zk.PlonkProver._many_blinds(fake, b, m)
    many = lambda *a: zk.PlonkProver.prove_many(fake, *a)        # noqa: E731
    w, pub, bl = [1, 2, 3, 4, 5], [2, 3], list(range(11))
    with pytest.raises(ValueError, match="^witnesses\\[1\\]: 4 values, n_witness = 5 expected$"):
        many([w, w[:4]], [pub, pub])
    with pytest.raises(ValueError, match="^publics: 1 rows for 2 witnesses$"):
        many([w, w], [pub])
    with pytest.raises(ValueError, match="^publics\\[1\\]: 3 values, n_public = 2 expected$"):
        many([w, w], [pub, pub + [1]])
    with pytest.raises(ValueError, match="^blinds: 1 rows for 2 witnesses$"):
        many([w, w], [pub, pub], [bl])
    with pytest.raises(ValueError, match="^blinds\\[1\\]: 10 values, 11 expected$"):
        many([w, w], [pub, pub], [bl, bl[:10]])
    with pytest.raises(ValueError, match="^blinds: 352 bytes, 2 rows of 11 scalars expected$"):
        many([w, w], [pub, pub], bytes(352))
    with pytest.raises(ValueError, match="^witnesses\\[0\\]: value 2 is not in 0 .. r - 1$"):
        many([[1, 2, 1 << 256, 4, 5]], [pub])                    # what does not fit 32 bytes; a value from r on is the library's to refuse
    with pytest.raises(AssertionError, match="a library call was about to be made"):
        many([w, w], [pub, pub], [bl, bl])                       # well-formed: the call would be made
    with pytest.raises(AssertionError, match="a library call was about to be made"):
        many([w, w])                                             # publics from the witnesses
    with pytest.raises(zk.ZkHipError, match="^zk_plonk_prove_r1cs_many: the prover was not made from an r1cs"):
        zk.PlonkProver.prove_r1cs_many(fake, [bytes(160)])
    commit = lambda c: zk.PlonkProver.commit_many(fake, c)       # noqa: E731
    with pytest.raises(ValueError, match="^coeffs: at least one polynomial expected$"):
        commit([])
    with pytest.raises(ValueError, match="^coeffs\\[1\\]: 15 coefficients, 1 .. n \\+ 6 = 14 expected$"):
        commit([[1], [1] * 15])
    with pytest.raises(ValueError, match="^coeffs\\[0\\]: 0 coefficients, 1 .. n \\+ 6 = 14 expected$"):
        commit([[]])


def test_c_entries_refuse_what_needs_no_device(monkeypatch):
    from rapidsnark_old_amd import lib as L
    lib = L.load_library()
    P = lambda a: ctypes.c_void_p(a.ctypes.data)         # noqa: E731
    buf, st = np.zeros(768, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    err = lambda: lib.zk_last_error().decode()           # noqa: E731
    assert lib.zk_plonk_prove_many(None, 1, P(buf), P(st), P(buf), P(buf), None) == 1 and err() == "null argument"
    assert lib.zk_plonk_prove_many(None, 0, None, None, None, None, None) == 1 and err() == "null argument"
    assert lib.zk_plonk_prove_r1cs_many(None, 1, P(buf), P(st), P(buf), 3, None) == 1 and err() == "null argument"
    assert lib.zk_plonk_prover_commit_many(None, P(buf), P(buf), 1) == 1 and err() == "null argument"
    plan = L.zk_plonk_prover_many_plan()
    plan.size = ctypes.sizeof(plan)
    assert lib.zk_plonk_prover_many_info(None, ctypes.byref(plan)) == 1 and err() == "null argument"
    assert st[0] == 0 and not buf.any()


def test_the_host_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "plonk_many_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "rapidsnark-old_amd", "csrc"), os.path.join(ROOT, "tools", "plonk_many_host_test.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if k != "ZKHIP_PLONK_PROVE_BATCH"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "plonk_many host checks OK", r.stdout + r.stderr
