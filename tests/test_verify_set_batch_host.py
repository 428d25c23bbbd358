"""zk_vkey_set_verify_batch without a device: the header declares the entry and its report, the ctypes struct has the C
layout (a C program prints sizeof and the offsets), the export is bound, VerificationKeySet.verify_batch refuses bad
arguments before any library call, and the host code the two batch entries share passes its own program's checks."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkhip.h")
FIELDS = ["size", "group", "group_keys", "launches", "groups", "groups_failed", "segments", "proofs_rechecked", "malformed"]


def test_header_declares_the_entry_and_the_report():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    assert ("int zk_vkey_set_verify_batch(zk_vkey_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, "
            "uint64_t publics_bytes, uint64_t n, const uint8_t *scalars16 , uint8_t *verdict, zk_vkey_set_batch_report *report );") in flat
    assert "} zk_vkey_set_batch_report;" in flat
    assert "uint32_t group, group_keys;" in flat and "uint64_t groups, groups_failed, segments;" in flat and "uint64_t proofs_rechecked, malformed;" in flat
    assert "ZKHIP_VERIFY_GROUP_KEYS" in text
    assert "Not here: random combination across keys" not in text
    # after the set's entries, and the set's plan keeps its fields
    assert flat.index("int zk_vkey_set_info(") < flat.index("int zk_vkey_set_verify_batch(")
    assert "uint64_t proofs_coop, proofs_lanes; /* totals since zk_vkey_set_create */" in re.sub(r"\s+", " ", text)


def test_ctypes_report_has_the_c_layout(tmp_path):
    from rapidsnark_old_amd import lib as L
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkhip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(zk_vkey_set_batch_report));\n'
                   + "".join('    printf(" %%zu", offsetof(zk_vkey_set_batch_report, %s));\n' % f for f in FIELDS)
                   + '    printf(" %zu %zu\\n", sizeof(zk_vkey_set_plan), sizeof(zk_vkey_batch_report));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert [name for name, _ in L.zk_vkey_set_batch_report._fields_] == FIELDS
    assert got == [ctypes.sizeof(L.zk_vkey_set_batch_report)] + [getattr(L.zk_vkey_set_batch_report, f).offset for f in FIELDS] + [40, 48]
    assert got[0] == 56


def test_shared_host_code_under_the_sanitizers(tmp_path):
    """csrc/hostutil.hpp and csrc/verify_batch_host.hpp alone, in a program of its own (tools/verify_batch_host_test.cpp): the
    strict reading of the group switches and the lax one of the chunk sizes, the on/off switch, the pick of the first bad
    point, 4096 drawn scalars (none zero, no two equal), the refusal of a zero scalar, the report's size, and ChunkPlan
    against a restatement of the grouping rule on the key_of layouts of the device tests."""
    exe = str(tmp_path / "verify_batch_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "rapidsnark-old_amd", "csrc"), os.path.join(ROOT, "tools", "verify_batch_host_test.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("ZKHIP_")}
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "OK: env_number, scalars, report size and ChunkPlan" in out.stdout, out.stdout + out.stderr


def test_the_export_is_bound():
    from rapidsnark_old_amd import lib as L
    assert "zk_vkey_set_verify_batch" in L.EXPORTS
    lib = L.load_library()
    args = lib.zk_vkey_set_verify_batch.argtypes
    assert len(args) == 9 and args[4:6] == [ctypes.c_uint64, ctypes.c_uint64] and args[-1]._type_ is L.zk_vkey_set_batch_report


def test_python_refuses_bad_arguments_before_any_library_call(monkeypatch):
    from rapidsnark_old_amd import lib as L, verify as V

    def never(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(L, "load_library", never)
    ks = V.VerificationKeySet.__new__(V.VerificationKeySet)   # a set object without a device: only the argument checks run
    ks.keys, ks.n_public, ks._h = [None] * 3, np.array([1, 0, 3], dtype=np.int64), ctypes.c_void_p(1)
    try:
        with pytest.raises(ValueError, match="multiple of 256"):
            ks.verify_batch(bytes(255), [0], bytes(32))
        with pytest.raises(ValueError, match="key_of: 2 indices expected"):
            ks.verify_batch(bytes(512), [0], bytes(32))
        with pytest.raises(ValueError, match="integers expected"):
            ks.verify_batch(bytes(512), [0.0, 1.0], bytes(32))
        with pytest.raises(ValueError, match=r"key_of\[1\] = 3: the set holds 3 keys"):
            ks.verify_batch(bytes(512), [0, 3], bytes(32))
        with pytest.raises(ValueError, match=r"key_of\[0\] = -1"):
            ks.verify_batch(bytes(512), np.array([-1, 0]), bytes(32))
        with pytest.raises(ValueError, match="publics: 128 bytes expected .* got 96"):   # the ragged total: 1 + 0 + 3 signals
            ks.verify_batch(bytes(768), (0, 1, 2), bytes(96))
        with pytest.raises(ValueError, match="publics: 0 bytes expected"):
            ks.verify_batch(bytes(256), [1], bytes(32))
        with pytest.raises(ValueError, match="scalars: 3 proofs x 16 bytes expected, got 47"):
            ks.verify_batch(bytes(768), [0, 1, 2], bytes(128), scalars=bytes(47))
        with pytest.raises(ValueError, match="scalars"):
            ks.verify_batch(bytes(768), [0, 1, 2], bytes(128), scalars=bytes(64))
        ks._h = ctypes.c_void_p()
        with pytest.raises(L.ZkHipError, match="closed"):
            ks.verify_batch(bytes(256), [1])
    finally:
        ks._h, ks.keys = ctypes.c_void_p(), []          # nothing for __del__ to destroy
