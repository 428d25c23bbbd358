"""PLONK batch verification without a device: the header declares the two entries and the report and says what is sound and
what is not; the report's ctypes layout is the compiled one; the entries are bound and PlonkVerifier has the methods;
Python refuses bad scalars before any call; the C entries refuse null before a device is touched; and
tools/plonk_batch_host_test.cpp (csrc/plonk_batch_dev.hpp's per-proof products against plonk_transcript.hpp's scalars, the
arithmetic of chunks and groups) builds for the host under the address and undefined-behaviour sanitizers and exits 0."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "zkhip.h")
FIELDS = ["size", "group", "groups", "groups_failed", "proofs_rechecked", "malformed", "launches", "chunks"]


def test_header_declares_the_entries():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    for decl in ("typedef struct { uint32_t size; uint32_t group; uint64_t groups, groups_failed; uint64_t proofs_rechecked, malformed; "
                 "uint32_t launches, chunks; } zk_plonk_batch_report;",
                 "int zk_plonk_verifier_verify_batch(zk_plonk_verifier *v, const uint8_t *proofs, const uint8_t *publics, uint64_t m, "
                 "const uint8_t *scalars16, uint8_t *verdict, zk_plonk_batch_report *report );",
                 "int zk_plonk_verifier_batch_sums(zk_plonk_verifier *v, const uint8_t *proofs, const uint8_t *publics, uint64_t m, "
                 "const uint8_t *scalars16, uint8_t *sums, uint64_t sums_cap, uint64_t *n_groups);"):
        assert decl in flat, decl
    assert flat.index("int zk_plonk_verifier_challenges(") < flat.index("} zk_plonk_batch_report;") < flat.index("int zk_plonk_verifier_verify_batch(")
    section = text[text.index("PLONK prover and verifier"):text.index("PLONK from an R1CS")]
    for words in ("ZKHIP_PLONK_VERIFY_GROUP: a number of proofs from 1 to 2^20 expected", "zk_plonk_verifier_verify_batch: scalar 3 is zero",
                  "zk_plonk_verifier_verify_batch: m is not below 2^31", "FOR TESTS ONLY", "getrandom()", "redrawn while zero",
                  "at most one of the 2^128 - 1 values of its scalar", "can predict before fixing the proofs are unsound",
                  "Never pass constants, counters or a seeded generator", "e(L, G2) e(-W, [tau]G2) = 1", "a group never straddles a chunk",
                  "many invalid proofs", "last_launches = report->launches", "No pairing is run"):
        assert re.sub(r"\s+", " ", words) in re.sub(r"[\s*]+", " ", section), words
    # the plan keeps its layout
    assert "uint32_t last_chunks; /* chunks of the last call with m > 0: ceil(m / min(m, chunk)) */ } zk_plonk_verifier_plan;" in re.sub(r"\s+", " ", text)


def test_ctypes_report_has_the_c_layout(tmp_path):
    from rapidsnark_old_amd import lib as L
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkhip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(zk_plonk_batch_report));\n'
                   + "".join('    printf(" %%zu", offsetof(zk_plonk_batch_report, %s));\n' % f for f in FIELDS)
                   + '    printf(" %zu\\n", sizeof(zk_plonk_verifier_plan));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert [name for name, _ in L.zk_plonk_batch_report._fields_] == FIELDS
    assert got == [ctypes.sizeof(L.zk_plonk_batch_report)] + [getattr(L.zk_plonk_batch_report, f).offset for f in FIELDS] + [40]
    assert got[0] == 48


def test_the_entries_are_bound():
    from rapidsnark_old_amd import lib as L
    import rapidsnark_old_amd as zk
    lib = L.load_library()
    for name, nargs in (("zk_plonk_verifier_verify_batch", 7), ("zk_plonk_verifier_batch_sums", 8)):
        assert name in L.EXPORTS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    for name in ("verify_batch", "batch_sums", "verify", "challenges", "info"):
        assert hasattr(zk.PlonkVerifier, name), name


class _NoDevice:
    """PlonkVerifier's argument handling without the object: no handle is ever asked for"""
    n_public = 2


def test_python_refuses_bad_scalars_before_the_call():
    import rapidsnark_old_amd as zk
    check = zk.PlonkVerifier._batch_scalars
    assert check(None, 3) is None
    good = check([1, (1 << 128) - 1, 7], 3)
    assert good.dtype == np.uint8 and good.tobytes() == (1).to_bytes(16, "little") + b"\xff" * 16 + (7).to_bytes(16, "little")
    assert check(good.tobytes(), 3).tobytes() == good.tobytes() and check(good, 3).tobytes() == good.tobytes()
    with pytest.raises(ValueError, match="^scalars\\[1\\] is not below 2\\^128$"):
        check([1, 1 << 128, 2], 3)
    with pytest.raises(ValueError, match="^scalars\\[0\\] is not below 2\\^128$"):
        check([-1, 1, 2], 3)
    with pytest.raises(ValueError, match="^scalars\\[2\\] is zero$"):
        check([1, 2, 0], 3)
    with pytest.raises(ValueError, match="^scalars\\[1\\] is zero$"):
        check((5).to_bytes(16, "little") + bytes(16), 2)
    with pytest.raises(ValueError, match="^scalars: 2 values for 3 proofs$"):
        check([1, 2], 3)
    with pytest.raises(ValueError, match="^scalars: 33 bytes, 2 scalars of 16 bytes expected$"):
        check(bytes(33), 2)
    # through the methods: the checks come before the object is asked for its handle
    fake = _NoDevice()
    proofs = np.zeros((2, 768), dtype=np.uint8)
    fake._inputs = lambda p, q: zk.PlonkVerifier._inputs(fake, p, q)
    fake._batch_scalars = check
    for call in (zk.PlonkVerifier.verify_batch, zk.PlonkVerifier.batch_sums):
        with pytest.raises(ValueError, match="^scalars\\[1\\] is zero$"):
            call(fake, proofs, [[1, 2], [3, 4]], [9, 0])
        with pytest.raises(ValueError, match="^scalars: 3 values for 2 proofs$"):
            call(fake, proofs, [[1, 2], [3, 4]], [9, 8, 7])
    with pytest.raises(ValueError, match="^scalars: 2 values expected$"):
        zk.PlonkVerifier.batch_sums(fake, proofs, [[1, 2], [3, 4]], None)


def test_c_entries_refuse_null_before_a_device_is_touched():
    from rapidsnark_old_amd import lib as L
    lib = L.load_library()
    P = lambda a: ctypes.c_void_p(a.ctypes.data)         # noqa: E731
    buf, out = np.zeros(768, dtype=np.uint8), np.zeros(128, dtype=np.uint8)
    rep = L.zk_plonk_batch_report()
    rep.size = ctypes.sizeof(rep)
    n = ctypes.c_uint64(7)
    assert lib.zk_plonk_verifier_verify_batch(None, P(buf), P(buf), 1, None, P(out), ctypes.byref(rep)) == 1 and lib.zk_last_error().decode() == "null argument"
    assert lib.zk_plonk_verifier_verify_batch(None, P(buf), P(buf), 1, None, P(out), None) == 1 and lib.zk_last_error().decode() == "null argument"
    assert lib.zk_plonk_verifier_batch_sums(None, P(buf), P(buf), 1, P(buf), P(out), 1, ctypes.byref(n)) == 1 and lib.zk_last_error().decode() == "null argument"
    assert n.value == 0
    assert lib.zk_plonk_verifier_batch_sums(None, P(buf), P(buf), 1, P(buf), P(out), 1, None) == 1 and lib.zk_last_error().decode() == "null argument"


def test_the_host_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "plonk_batch_host_test")
    subprocess.check_call(["hipcc", "--offload-host-only", "-std=c++17", "-O1", "-g", "-x", "hip", os.path.join(ROOT, "tools", "plonk_batch_host_test.cpp"),
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "plonk_batch host checks OK", r.stdout + r.stderr
