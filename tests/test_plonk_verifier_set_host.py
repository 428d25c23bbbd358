"""The PLONK key-set verifier without a device: the header declares the entries, the plan and the report and says what is
sound and what is not; the ctypes structs have the compiled layout; the entries are bound and PlonkVerifierSet has the
methods; Python refuses a key_of of the wrong length, a publics row of the wrong width for its key and scalars of the wrong
shape before any call; the C entries refuse null before a device is touched; and tools/plonk_set_host_test.cpp
(csrc/plonk_set_plan.hpp alone: the order by key, the ragged offsets, groups, segments and the fold's ranges against a plain
restatement of the rules) builds for the host under the address and undefined-behaviour sanitizers and exits 0."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "zkhip.h")
REPORT = ["size", "group", "launches", "chunks", "groups", "groups_failed", "segments", "proofs_rechecked", "malformed"]
PLAN = ["size", "n_keys", "max_n_public", "device_bytes", "chunk", "last_launches", "last_chunks"]


def test_header_declares_the_entries():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    for decl in ("typedef struct zk_plonk_verifier_set zk_plonk_verifier_set;",
                 "int zk_plonk_verifier_set_create(zk_plonk_verifier_set **out, const zk_plonk_vkey *const *vks, uint32_t n_keys, int32_t device);",
                 "void zk_plonk_verifier_set_destroy(zk_plonk_verifier_set *set);",
                 "typedef struct zk_plonk_verifier_set_plan { uint32_t size; uint32_t n_keys; uint64_t max_n_public; uint64_t device_bytes; uint64_t chunk; "
                 "uint32_t last_launches; uint32_t last_chunks; } zk_plonk_verifier_set_plan;",
                 "int zk_plonk_verifier_set_info(zk_plonk_verifier_set *set, zk_plonk_verifier_set_plan *plan);",
                 "int zk_plonk_verifier_set_verify(zk_plonk_verifier_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, "
                 "uint64_t publics_bytes, uint64_t m, uint8_t *verdict);",
                 "typedef struct { uint32_t size; uint32_t group; uint32_t launches, chunks; uint64_t groups, groups_failed; uint64_t segments; "
                 "uint64_t proofs_rechecked, malformed; } zk_plonk_set_batch_report;",
                 "int zk_plonk_verifier_set_verify_batch(zk_plonk_verifier_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, "
                 "uint64_t publics_bytes, uint64_t m, const uint8_t *scalars16, uint8_t *verdict, zk_plonk_set_batch_report *report );",
                 "int zk_plonk_verifier_set_batch_sums(zk_plonk_verifier_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, "
                 "uint64_t publics_bytes, uint64_t m, const uint8_t *scalars16, uint8_t *sums, uint64_t sums_cap, uint64_t *n_groups);"):
        assert decl in flat, decl
    assert flat.index("int zk_plonk_verifier_batch_sums(") < flat.index("typedef struct zk_plonk_verifier_set zk_plonk_verifier_set;")
    section = text[text.index("A verifier over a KEY SET"):text.index("PLONK from an R1CS")]
    for words in ("COPIES the keys and borrows nothing", "zk_plonk_verifier_set_create: key 3's [tau]G2 is not key 0's",
                  "zk_plonk_verifier_set_create: n_keys 0 is outside 1 .. 65536", "zk_plonk_verifier_set_create: key 3: log_n 2 is outside 3 .. 25",
                  "zk_plonk_verifier_set_create: the keys' [tau]G2 is not a point of the twist in the subgroup",
                  "zk_plonk_verifier_set_verify: key_of[5] = 9, the set holds 4 keys",
                  "zk_plonk_verifier_set_verify: publics_bytes: 640 expected (20 values of 32 bytes), 608 given",
                  "zk_plonk_verifier_set_verify: m is not below 2^31", "INVALID, not an error", "RAGGED", "ORDERED BY KEY",
                  "Four launches a chunk", "NO limit on the keys of a group", "a group never straddles a chunk",
                  "e(L, G2) e(-W, [tau]G2) = 1", "FOR TESTS ONLY", "getrandom()", "zk_plonk_verifier_set_verify_batch: scalar 3 is zero",
                  "can predict before fixing the proofs are unsound", "THE TWO MAY STAND UNDER TWO DIFFERENT KEYS",
                  "Never pass constants, counters or a seeded generator", "at most 1 / (2^128 - 1) a group", "No pairing is run",
                  "zk_plonk_verifier_set_batch_sums: sums_cap 2 is below the call's 3 groups"):
        assert re.sub(r"\s+", " ", words) in re.sub(r"[\s*]+", " ", section), words


def test_ctypes_structs_have_the_c_layout(tmp_path):
    from rapidsnark_old_amd import lib as L
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkhip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(zk_plonk_set_batch_report));\n'
                   + "".join('    printf(" %%zu", offsetof(zk_plonk_set_batch_report, %s));\n' % f for f in REPORT)
                   + '    printf(" %zu", sizeof(zk_plonk_verifier_set_plan));\n'
                   + "".join('    printf(" %%zu", offsetof(zk_plonk_verifier_set_plan, %s));\n' % f for f in PLAN)
                   + '    printf("\\n");\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert [name for name, _ in L.zk_plonk_set_batch_report._fields_] == REPORT
    assert [name for name, _ in L.zk_plonk_verifier_set_plan._fields_] == PLAN
    assert got == ([ctypes.sizeof(L.zk_plonk_set_batch_report)] + [getattr(L.zk_plonk_set_batch_report, f).offset for f in REPORT]
                   + [ctypes.sizeof(L.zk_plonk_verifier_set_plan)] + [getattr(L.zk_plonk_verifier_set_plan, f).offset for f in PLAN])
    assert got[0] == 56 and got[len(REPORT) + 1] == 40


def test_the_entries_are_bound():
    from rapidsnark_old_amd import lib as L
    import rapidsnark_old_amd as zk
    lib = L.load_library()
    for name, nargs in (("zk_plonk_verifier_set_create", 4), ("zk_plonk_verifier_set_destroy", 1), ("zk_plonk_verifier_set_info", 2),
                        ("zk_plonk_verifier_set_verify", 7), ("zk_plonk_verifier_set_verify_batch", 9), ("zk_plonk_verifier_set_batch_sums", 10)):
        assert name in L.EXPORTS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    for name in ("verify", "verify_batch", "batch_sums", "info", "close", "__enter__", "__exit__"):
        assert hasattr(zk.PlonkVerifierSet, name), name


class _NoDevice:
    """PlonkVerifierSet's argument handling without the object: no handle is ever asked for"""
    n_public = [2, 16, 0, 2, 2]

    def _handle(self):
        raise AssertionError("a library call was about to be made")


def test_python_refuses_bad_arguments_before_the_call():
    import rapidsnark_old_amd as zk
    fake = _NoDevice()
    fake._inputs = lambda p, k, q: zk.PlonkVerifierSet._inputs(fake, p, k, q)
    proofs = np.zeros((3, 768), dtype=np.uint8)
    rows = [[1, 2], [], list(range(16))]
    a, ko, pb, m = fake._inputs(proofs, [0, 2, 1], rows)
    assert m == 3 and ko.dtype == np.uint32 and list(ko) == [0, 2, 1] and pb.dtype == np.uint8 and pb.size == 18 * 32
    assert pb.tobytes() == b"".join(int(v).to_bytes(32, "little") for row in rows for v in row)
    assert fake._inputs(proofs, [0, 2, 1], pb.tobytes())[2].tobytes() == pb.tobytes()          # the flat ragged bytes
    assert fake._inputs(proofs, [2, 2, 2], None)[2].size == 0
    calls = [lambda *args: zk.PlonkVerifierSet.verify(fake, *args), lambda *args: zk.PlonkVerifierSet.verify_batch(fake, *args),
             lambda *args: zk.PlonkVerifierSet.batch_sums(fake, *args, [1, 2, 3])]
    for call in calls:
        with pytest.raises(ValueError, match="^key_of: 2 entries for 3 proofs$"):
            call(proofs, [0, 2], rows)
        with pytest.raises(ValueError, match="^key_of\\[1\\] = 5, the set holds 5 keys$"):
            call(proofs, [0, 5, 1], rows)
        with pytest.raises(ValueError, match="^publics\\[1\\]: 0 values, n_public = 2 expected for key 3$"):
            call(proofs, [0, 3, 1], rows)
        with pytest.raises(ValueError, match="^publics\\[2\\]: 16 values, n_public = 0 expected for key 2$"):
            call(proofs, [0, 2, 2], rows)
        with pytest.raises(ValueError, match="^publics: 2 rows for 3 proofs$"):
            call(proofs, [0, 2, 1], rows[:2])
        with pytest.raises(ValueError, match="^publics: 544 bytes, 576 expected \\(18 values of 32 bytes\\)$"):
            call(proofs, [0, 2, 1], pb.tobytes()[:-32])
        with pytest.raises(ValueError, match="^publics: 3 rows expected"):
            call(proofs, [0, 2, 1], None)
        with pytest.raises(ValueError, match="^proofs: a uint8 array of m rows of 768 bytes expected$"):
            call(np.zeros((3, 767), dtype=np.uint8), [0, 2, 1], rows)
    for call in (zk.PlonkVerifierSet.verify_batch, zk.PlonkVerifierSet.batch_sums):
        with pytest.raises(ValueError, match="^scalars: 2 values for 3 proofs$"):
            call(fake, proofs, [0, 2, 1], rows, [1, 2])
        with pytest.raises(ValueError, match="^scalars\\[2\\] is zero$"):
            call(fake, proofs, [0, 2, 1], rows, [1, 2, 0])
        with pytest.raises(ValueError, match="^scalars\\[0\\] is not below 2\\^128$"):
            call(fake, proofs, [0, 2, 1], rows, [1 << 128, 2, 3])
        with pytest.raises(ValueError, match="^scalars: 47 bytes, 3 scalars of 16 bytes expected$"):
            call(fake, proofs, [0, 2, 1], rows, bytes(47))
    with pytest.raises(ValueError, match="^scalars: 3 values expected$"):
        zk.PlonkVerifierSet.batch_sums(fake, proofs, [0, 2, 1], rows, None)
    with pytest.raises(TypeError, match="^vkeys\\[0\\]: a PlonkVKey expected"):
        zk.PlonkVerifierSet([object()])
    with pytest.raises(ValueError, match="^vkeys: 0 keys, 1 to 65536 expected$"):
        zk.PlonkVerifierSet([])


def test_c_entries_refuse_null_before_a_device_is_touched():
    from rapidsnark_old_amd import lib as L
    lib = L.load_library()
    P = lambda a: ctypes.c_void_p(a.ctypes.data)         # noqa: E731
    buf, out = np.zeros(768, dtype=np.uint8), np.zeros(128, dtype=np.uint8)
    ko = np.zeros(1, dtype=np.uint32)
    rep = L.zk_plonk_set_batch_report()
    rep.size = ctypes.sizeof(rep)
    n = ctypes.c_uint64(7)
    h = ctypes.c_void_p(1)
    err = lambda: lib.zk_last_error().decode()           # noqa: E731
    assert lib.zk_plonk_verifier_set_create(None, None, 1, -1) == 1 and err() == "null argument"
    assert lib.zk_plonk_verifier_set_create(ctypes.byref(h), None, 1, -1) == 1 and err() == "null argument" and not h.value
    vk = L.zk_plonk_vkey()
    ptrs = (ctypes.POINTER(L.zk_plonk_vkey) * 2)(ctypes.pointer(vk), None)
    assert lib.zk_plonk_verifier_set_create(ctypes.byref(h), ptrs, 0, -1) == 1 and err() == "zk_plonk_verifier_set_create: n_keys 0 is outside 1 .. 65536"
    assert lib.zk_plonk_verifier_set_create(ctypes.byref(h), ptrs, 65537, -1) == 1 and err() == "zk_plonk_verifier_set_create: n_keys 65537 is outside 1 .. 65536"
    assert lib.zk_plonk_verifier_set_create(ctypes.byref(h), ptrs, 2, -1) == 1 and err() == "zk_plonk_verifier_set_create: key 0: vk->size is not sizeof(zk_plonk_vkey)"
    vk.size, vk.log_n = ctypes.sizeof(vk), 2
    assert lib.zk_plonk_verifier_set_create(ctypes.byref(h), ptrs, 2, -1) == 1 and err() == "zk_plonk_verifier_set_create: key 0: log_n 2 is outside 3 .. 25"
    vk.log_n, vk.n_public = 3, 9
    assert lib.zk_plonk_verifier_set_create(ctypes.byref(h), ptrs, 2, -1) == 1 and err() == "zk_plonk_verifier_set_create: key 0: n_public 9 exceeds n = 8"
    vk.n_public = 2
    ctypes.memset(vk.k1, 0xFF, 32)
    assert lib.zk_plonk_verifier_set_create(ctypes.byref(h), ptrs, 2, -1) == 1 and err() == "zk_plonk_verifier_set_create: key 0: k1 is not below r"
    ctypes.memset(vk.k1, 0, 32)
    vk.qo[0] = 1
    assert lib.zk_plonk_verifier_set_create(ctypes.byref(h), ptrs, 2, -1) == 1
    assert err() == "zk_plonk_verifier_set_create: key 0: a commitment of the key is not a point of the curve"
    vk.qo[0] = 0
    assert lib.zk_plonk_verifier_set_create(ctypes.byref(h), ptrs, 2, -1) == 1 and err() == "zk_plonk_verifier_set_create: key 1 is null"
    other = L.zk_plonk_vkey.from_buffer_copy(bytes(vk))
    other.tau_g2[5] = 1
    ptrs[1] = ctypes.pointer(other)
    assert lib.zk_plonk_verifier_set_create(ctypes.byref(h), ptrs, 2, -1) == 1 and err() == "zk_plonk_verifier_set_create: key 1's [tau]G2 is not key 0's"
    assert lib.zk_plonk_verifier_set_verify(None, P(buf), P(ko), P(buf), 0, 1, P(out)) == 1 and err() == "null argument"
    assert lib.zk_plonk_verifier_set_verify_batch(None, P(buf), P(ko), P(buf), 0, 1, None, P(out), ctypes.byref(rep)) == 1 and err() == "null argument"
    assert lib.zk_plonk_verifier_set_batch_sums(None, P(buf), P(ko), P(buf), 0, 1, P(buf), P(out), 1, ctypes.byref(n)) == 1 and err() == "null argument"
    assert n.value == 0
    assert lib.zk_plonk_verifier_set_batch_sums(None, P(buf), P(ko), P(buf), 0, 1, P(buf), P(out), 1, None) == 1 and err() == "null argument"
    plan = L.zk_plonk_verifier_set_plan()
    assert lib.zk_plonk_verifier_set_info(None, ctypes.byref(plan)) == 1 and err() == "null argument"
    lib.zk_plonk_verifier_set_destroy(None)


def test_the_host_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "plonk_set_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "rapidsnark-old_amd", "csrc"), os.path.join(ROOT, "tools", "plonk_set_host_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "plonk_set host checks OK", r.stdout + r.stderr
