"""The cooperative pairing path's host-checkable parts (csrc/pairing_coop.hpp): the lane-to-coefficient map of the sliced Fq12
product against pairing.hpp's f12_mul / f12_sqr / f12_mul_line on random elements, and the reading of
ZKHIP_VERIFY_COOP_MAX / ZKHIP_PAIRING_COOP_MAX.  tools/pairing_coop_host_test.cpp is built for the host and run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sliced_fq12_products_equal_the_tower_forms_and_thresholds_parse(tmp_path):
    exe = str(tmp_path / "pairing_coop_host_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rapidsnark-old_amd", "csrc"),
                           os.path.join(ROOT, "tools", "pairing_coop_host_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "OK: sliced product" in out.stdout, out.stdout + out.stderr


def test_new_exports_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    for needle in ("#define ZK_VERIFY_PATH_LANES 0", "#define ZK_VERIFY_PATH_COOP  1", "int zk_vkey_info(zk_vkey *vk, zk_vkey_plan *plan);",
                   "int zk_pairing_last_path(void);"):
        assert needle in text, needle
    from rapidsnark_old_amd import lib as L
    assert "zk_vkey_info" in L.EXPORTS and "zk_pairing_last_path" in L.EXPORTS
    import ctypes
    assert ctypes.sizeof(L.zk_vkey_plan) == 32
