"""zk_vkey_set_* without a device: the header declares the four entries and the plan, the ctypes struct has the C layout (a C
program prints sizeof and the offsets), the exports are bound, and VerificationKeySet refuses bad arguments before any
library call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkhip.h")
FIELDS = ["size", "n_keys", "last_path", "last_launches", "last_waves_padded", "proofs_coop", "proofs_lanes"]


def test_header_declares_the_entries_and_the_plan():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    assert "typedef struct zk_vkey_set zk_vkey_set;" in flat
    assert "int zk_vkey_set_create(zk_vkey_set **out, zk_vkey *const *keys, uint32_t n_keys);" in flat
    assert "void zk_vkey_set_destroy(zk_vkey_set *set);" in flat
    assert ("int zk_vkey_set_verify(zk_vkey_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, "
            "uint64_t publics_bytes, uint64_t n, uint8_t *verdict);") in flat
    assert "int zk_vkey_set_info(zk_vkey_set *set, zk_vkey_set_plan *plan);" in flat
    assert "} zk_vkey_set_plan;" in flat
    # after the zk_vkey_verify_batch block, and that block and zk_vkey_plan are what they were
    assert flat.index("int zk_vkey_verify_batch(") < flat.index("typedef struct zk_vkey_set zk_vkey_set;")
    assert "uint64_t proofs_coop, proofs_lanes;" in text and "} zk_vkey_batch_report;" in flat


def test_ctypes_plan_has_the_c_layout(tmp_path):
    from rapidsnark_old_amd import lib as L
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkhip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(zk_vkey_set_plan));\n'
                   + "".join('    printf(" %%zu", offsetof(zk_vkey_set_plan, %s));\n' % f for f in FIELDS)
                   + '    printf(" %zu %zu\\n", sizeof(zk_vkey_plan), sizeof(zk_vkey_batch_report));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert [name for name, _ in L.zk_vkey_set_plan._fields_] == FIELDS
    assert got == [ctypes.sizeof(L.zk_vkey_set_plan)] + [getattr(L.zk_vkey_set_plan, f).offset for f in FIELDS] + [32, 48]
    assert got[0] == 40


def test_the_exports_are_bound():
    from rapidsnark_old_amd import lib as L
    import rapidsnark_old_amd as zk
    assert zk.VerificationKeySet is zk.verify.VerificationKeySet
    for name in ("zk_vkey_set_create", "zk_vkey_set_destroy", "zk_vkey_set_verify", "zk_vkey_set_info"):
        assert name in L.EXPORTS
    lib = L.load_library()
    assert len(lib.zk_vkey_set_create.argtypes) == 3 and lib.zk_vkey_set_create.argtypes[2] is ctypes.c_uint32
    assert lib.zk_vkey_set_destroy.restype is None and len(lib.zk_vkey_set_destroy.argtypes) == 1
    assert len(lib.zk_vkey_set_verify.argtypes) == 7 and lib.zk_vkey_set_verify.argtypes[4:6] == [ctypes.c_uint64, ctypes.c_uint64]
    assert lib.zk_vkey_set_info.argtypes[-1]._type_ is L.zk_vkey_set_plan


FAKES = []


def fake_key(V, n_public, device=-1, handle=1):
    vk = V.VerificationKey.__new__(V.VerificationKey)   # a key object without a device: only the argument checks run
    vk.n_public, vk.device, vk._h = n_public, device, ctypes.c_void_p(handle)
    FAKES.append(vk)                                    # its handle is taken back below: nothing for __del__ to destroy
    return vk


def test_python_refuses_bad_arguments_before_any_library_call(monkeypatch):
    from rapidsnark_old_amd import lib as L, verify as V

    def never(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(L, "load_library", never)
    keys = [fake_key(V, 1), fake_key(V, 0), fake_key(V, 3)]
    ks = V.VerificationKeySet.__new__(V.VerificationKeySet)
    ks.keys, ks.n_public, ks._h = keys, np.array([1, 0, 3], dtype=np.int64), ctypes.c_void_p(1)
    try:
        with pytest.raises(ValueError, match="at least one key"):
            V.VerificationKeySet([])
        with pytest.raises(ValueError, match="one device; these are on devices 0, 2"):
            V.VerificationKeySet([fake_key(V, 1, device=0), fake_key(V, 1, device=2), fake_key(V, 1, device=0)])
        with pytest.raises(ValueError, match="key 1 is closed"):
            V.VerificationKeySet([fake_key(V, 1), fake_key(V, 1, handle=None)])
        with pytest.raises(ValueError, match="key 0 is not a VerificationKey"):
            V.VerificationKeySet([object()])
        with pytest.raises(ValueError, match="multiple of 256"):
            ks.verify(bytes(255), [0], bytes(32))
        with pytest.raises(ValueError, match="key_of: 2 indices expected"):
            ks.verify(bytes(512), [0], bytes(32))
        with pytest.raises(ValueError, match="key_of: 2 indices expected"):
            ks.verify(bytes(512), [[0, 1]], bytes(32))
        with pytest.raises(ValueError, match="integers expected"):
            ks.verify(bytes(512), [0.0, 1.0], bytes(32))
        with pytest.raises(ValueError, match=r"key_of\[1\] = 3: the set holds 3 keys"):
            ks.verify(bytes(512), [0, 3], bytes(32))
        with pytest.raises(ValueError, match=r"key_of\[0\] = -1"):
            ks.verify(bytes(512), np.array([-1, 0]), bytes(32))
        with pytest.raises(ValueError, match="publics: 128 bytes expected .* got 96"):   # the ragged total: 1 + 0 + 3 signals
            ks.verify(bytes(768), (0, 1, 2), bytes(96))
        with pytest.raises(ValueError, match="publics: 0 bytes expected"):
            ks.verify(bytes(256), [1], bytes(32))
        ks._h = ctypes.c_void_p()
        with pytest.raises(L.ZkHipError, match="closed"):
            ks.verify(bytes(256), [1])
        with pytest.raises(L.ZkHipError, match="closed"):
            ks.info()
    finally:
        ks._h = ctypes.c_void_p()                       # nothing for __del__ to destroy
        for k in FAKES:
            k._h = ctypes.c_void_p()
        del FAKES[:]
