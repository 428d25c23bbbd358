"""zk_vkey_verify_batch without a device: the header declares the entry and its report, the ctypes struct has the C layout
(a C program prints sizeof and the offsets), the export is bound, and VerificationKey.verify_batch refuses bad arguments
before any library call."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkhip.h")
FIELDS = ["size", "group", "groups", "groups_failed", "proofs_rechecked", "malformed", "launches", "reserved"]


def test_header_declares_the_entry_and_the_report():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    assert ("int zk_vkey_verify_batch(zk_vkey *vk, const uint8_t *proofs, const uint8_t *publics, uint64_t n, "
            "const uint8_t *scalars16, uint8_t *verdict, zk_vkey_batch_report *report );") in flat
    assert "} zk_vkey_batch_report;" in flat and "#define ZK_VERIFY_PATH_BATCH 2" in text
    assert "ZKHIP_VERIFY_GROUP" in text and "FOR TESTS ONLY" in text and "unsound" in text
    # zk_vkey_plan is what it was
    assert "uint64_t proofs_coop, proofs_lanes;" in text


def test_ctypes_report_has_the_c_layout(tmp_path):
    from rapidsnark_old_amd import lib as L
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkhip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(zk_vkey_batch_report));\n'
                   + "".join('    printf(" %%zu", offsetof(zk_vkey_batch_report, %s));\n' % f for f in FIELDS)
                   + '    printf(" %zu\\n", sizeof(zk_vkey_plan));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert [name for name, _ in L.zk_vkey_batch_report._fields_] == FIELDS
    assert got == [ctypes.sizeof(L.zk_vkey_batch_report)] + [getattr(L.zk_vkey_batch_report, f).offset for f in FIELDS] + [32]
    assert got[0] == 48


def test_the_export_is_bound():
    from rapidsnark_old_amd import lib as L
    assert "zk_vkey_verify_batch" in L.EXPORTS and L.ZK_VERIFY_PATH_BATCH == 2
    lib = L.load_library()
    assert lib.zk_vkey_verify_batch.argtypes[-1]._type_ is L.zk_vkey_batch_report and len(lib.zk_vkey_verify_batch.argtypes) == 7


def test_python_refuses_bad_arguments_before_any_library_call(monkeypatch):
    from rapidsnark_old_amd import lib as L, verify as V

    def never(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(L, "load_library", never)
    vk = V.VerificationKey.__new__(V.VerificationKey)   # a key object without a device: only the argument checks run
    vk.n_public, vk._h = 2, ctypes.c_void_p(1)
    try:
        with pytest.raises(ValueError, match="multiple of 256"):
            vk.verify_batch(bytes(255), bytes(64))
        with pytest.raises(ValueError, match="publics"):
            vk.verify_batch(bytes(512), bytes(64))
        with pytest.raises(ValueError, match="scalars"):
            vk.verify_batch(bytes(512), bytes(128), scalars=bytes(31))
        with pytest.raises(ValueError, match="scalars"):
            vk.verify_batch(bytes(512), bytes(128), scalars=bytes(48))
        vk._h = ctypes.c_void_p()
        with pytest.raises(L.ZkHipError, match="closed"):
            vk.verify_batch(bytes(512), bytes(128))
    finally:
        vk._h = ctypes.c_void_p()                       # nothing for __del__ to destroy
