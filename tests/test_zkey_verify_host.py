"""`zkeyverify`'s argument and file errors, the shapes of the three files that must agree (found on the host: INVALID, exit
1, no device), the memory estimate (zk_zkey_verify_sizes) and the refused check scalars: none of it touches a device.  The
.ptau files are tests/test_ptau_prepare_host.py's, written with oracle.bn254; the keys are the committed golden key of
r1cs_n8 and variants of it written with oracle.groth16_ref."""
import copy
import os
import random
import subprocess

import pytest

from conftest import ROOT, golden_bytes, golden_path

from oracle import groth16_ref as g
from rapidsnark_old_amd import r1cs as R, zkverify as V
from test_ptau_prepare_host import LAG, ptau_bytes

RM = g.R_MOD
ZKEYVERIFY = os.path.join(ROOT, "rapidsnark-old_amd", "zkeyverify")
USAGE = "Usage: zkeyverify <circuit.r1cs> <pot.ptau> <circuit.zkey>"


def circuits():
    """r1cs_n8 and r1cs_n64 of oracle/gen_golden.py (the same seeded calls)"""
    rng = random.Random(7)
    return {name: g.random_r1cs(rng, *args)[0] for name, args in (("r1cs_n8", (5, 1)), ("r1cs_n64", (50, 3)))}


CIRC = circuits()


def r1cs_bytes(c, A=None):
    return R.write_r1cs_rows(A if A is not None else c.A, c.B, c.C, c.nVars, c.nPublic)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("zkv")
    out = {}

    def put(name, data):
        out[name] = str(d / name)
        with open(out[name], "wb") as f:
            f.write(data)

    put("c.r1cs", r1cs_bytes(CIRC["r1cs_n8"]))
    put("p3.ptau", ptau_bytes(3))                                   # the domain of r1cs_n8 is 8
    put("p2.ptau", ptau_bytes(2))
    put("p3_unprepared.ptau", ptau_bytes(3, drop=LAG))
    key = golden_bytes("r1cs_n8", "circuit.zkey")
    put("c.zkey", key)
    zk = g.read_zkey(key)
    assert (zk.nVars, zk.nPublic, zk.domainSize) == (CIRC["r1cs_n8"].nVars, 1, 8)
    v = copy.deepcopy(zk)                                            # one more wire, with a point in every per-wire section
    v.nVars += 1
    for sec in (v.A, v.B1, v.B2, v.C):
        sec.append(sec[-1])
    put("nvars.zkey", g.write_zkey(v))
    v = copy.deepcopy(zk)                                            # one more public signal: IC grows, C shrinks
    v.nPublic += 1
    v.IC.append(v.C.pop(0))
    put("npublic.zkey", g.write_zkey(v))
    v = copy.deepcopy(zk)                                            # half the domain: 5 constraints + 1 + 1 rows do not fit 4
    v.domainSize //= 2
    v.H = v.H[:4]
    put("domain.zkey", g.write_zkey(v))
    return out


def run(*args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([ZKEYVERIFY, *args], capture_output=True, text=True, timeout=120, env=e)


def test_usage_and_argument_count(files):
    a = (files["c.r1cs"], files["p3.ptau"], files["c.zkey"])
    for argv in ((), a[:1], a[:2], a + a[:1]):
        res = run(*argv)
        assert res.returncode == 255 and USAGE in res.stderr and res.stdout == ""


@pytest.mark.parametrize("which", [0, 1, 2])
def test_missing_truncated_and_wrong_magic_files(files, tmp_path, which):
    good = [files["c.r1cs"], files["p3.ptau"], files["c.zkey"]]
    with open(good[which], "rb") as f:
        data = f.read()
    bad = str(tmp_path / "bad")
    for make in ("missing", "truncated", "short", "magic"):
        if make == "missing":
            if os.path.exists(bad):
                os.remove(bad)
        else:
            with open(bad, "wb") as f:
                f.write({"truncated": data[:len(data) - 40], "short": data[:30], "magic": b"wtns" + data[4:]}[make])
        argv = list(good)
        argv[which] = bad
        res = run(*argv)
        assert res.returncode == 255 and res.stdout == "" and res.stderr.strip(), (make, res.stdout, res.stderr)
        if make == "magic":
            assert "Invalid file type" in res.stderr


@pytest.mark.parametrize("ptau,zkey,line", [
    ("p3.ptau", "nvars.zkey", "INVALID: nVars: the key has 10 wires, the circuit 9"),
    ("p3.ptau", "npublic.zkey", "INVALID: nPublic: the key has 2 public signals, the circuit 1"),
    ("p3.ptau", "domain.zkey", "INVALID: domain: the key has a domain of 4"),
    ("p3_unprepared.ptau", "c.zkey", "INVALID: ptau: the file is not prepared for phase 2"),
    ("p2.ptau", "c.zkey", "INVALID: ptau: the file holds 2^2 and the circuit needs 2^3"),
])
def test_shapes_that_disagree_are_invalid_without_a_device(files, ptau, zkey, line):
    assert CIRC["r1cs_n8"].nVars == 9
    # no device may be touched: one that does not exist is named, and the verdict still comes
    res = run(files["c.r1cs"], files[ptau], files[zkey], env={"ZKHIP_DEVICE": "9999", "HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""})
    assert res.returncode == 1 and res.stderr == "", (res.stdout, res.stderr)
    lines = res.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith(line), res.stdout
    rep = V.zkey_verify(files["c.r1cs"], files[ptau], files[zkey], s=5, device=9999)
    assert rep.verdict == 1 and not rep.ok and not rep.failed and len(rep.shape_failed) == 1


def test_two_shapes_at_once_report_both(files):
    res = run(files["c.r1cs"], files["p2.ptau"], files["nvars.zkey"], env={"ZKHIP_DEVICE": "9999"})
    assert res.returncode == 1
    assert [ln.split(":")[1].strip() for ln in res.stdout.splitlines()] == ["nVars", "ptau"]
    assert V.zkey_verify(files["c.r1cs"], files["p2.ptau"], files["nvars.zkey"], device=9999).shape_failed == {"nVars", "ptau_power"}


def test_sizes_grow_with_the_terms_and_the_domain(files, tmp_path):
    c8, c64 = CIRC["r1cs_n8"], CIRC["r1cs_n64"]
    z8 = V.zkey_verify_sizes(files["c.r1cs"], files["p3.ptau"], files["c.zkey"])
    assert z8["log_domain"] == 3 and z8["shape_failed"] == set() and z8["chunk_points"] == 9 and 0 < z8["device_bytes"] < 1 << 32
    A = [dict(row) for row in c8.A]
    for row in A:                                                    # more terms, the same rows and wires
        for s in range(c8.nVars):
            row.setdefault(s, 3)
    more = V.zkey_verify_sizes(r1cs_bytes(c8, A), files["p3.ptau"], files["c.zkey"])
    assert more["log_domain"] == 3 and more["device_bytes"] > z8["device_bytes"]
    z64 = V.zkey_verify_sizes(r1cs_bytes(c64), files["p3.ptau"], golden_path("r1cs_n64", "circuit.zkey"))
    assert z64["log_domain"] == 6 and z64["shape_failed"] == {"ptau_power"} and z64["device_bytes"] > more["device_bytes"]


def test_sizes_follow_the_chunk_variable(files, monkeypatch):
    monkeypatch.setenv("ZKHIP_ZKEY_VERIFY_CHUNK", "4")
    assert V.zkey_verify_sizes(files["c.r1cs"], files["p3.ptau"], files["c.zkey"])["chunk_points"] == 4
    monkeypatch.setenv("ZKHIP_ZKEY_VERIFY_CHUNK", "0")
    with pytest.raises(V.L.ZkHipError, match="ZKHIP_ZKEY_VERIFY_CHUNK"):
        V.zkey_verify_sizes(files["c.r1cs"], files["p3.ptau"], files["c.zkey"])


def test_files_that_are_not_what_they_claim_are_errors_in_python(files):
    with open(files["c.zkey"], "rb") as f:
        key = f.read()
    with pytest.raises(ValueError):
        V.zkey_verify_sizes(files["c.r1cs"], files["p3.ptau"], key[:len(key) - 40])
    with pytest.raises(ValueError, match="not a zkey file"):
        V.zkey_verify_sizes(files["c.r1cs"], files["p3.ptau"], b"ptau" + key[4:])
    with pytest.raises(V.L.ZkHipError, match="ptau section 12 is short"):
        V.zkey_verify_sizes(files["c.r1cs"], ptau_bytes(3, short=(12, 64)), files["c.zkey"])


@pytest.mark.parametrize("scalar", [0, 1, RM, RM + 5])
def test_the_test_scalar_is_refused(files, scalar):
    res = run(files["c.r1cs"], files["p3.ptau"], files["c.zkey"], env={"ZKHIP_ZKEY_VERIFY_SCALAR": str(scalar)})
    assert res.returncode == 255 and res.stdout == "" and "ZKHIP_ZKEY_VERIFY_SCALAR: a decimal number from 2 to r - 1 expected" in res.stderr
    with pytest.raises(ValueError, match="at least 2 and below r"):
        V.zkey_verify(files["c.r1cs"], files["p3.ptau"], files["c.zkey"], s=scalar)
    # the library itself refuses it too, before any device
    import ctypes as C
    lib = V.L.load_library()
    rep = V.L.zk_zkey_verify_report()
    rep.size = C.sizeof(rep)

    def fn(rv, pv, zv):
        ss = V.L._scalar32(scalar)
        return lib.zk_zkey_verify(C.byref(rv), C.byref(pv), C.byref(zv), V.L._ptr(ss), 9999, C.byref(rep))
    assert V._call(files["c.r1cs"], files["p3.ptau"], files["c.zkey"], fn) != 0
    assert b"at least 2 and below r" in lib.zk_last_error()


@pytest.mark.parametrize("scalar", ["12x", "-3", ""])
def test_a_scalar_that_is_no_number_is_refused(files, scalar):
    res = run(files["c.r1cs"], files["p3.ptau"], files["c.zkey"], env={"ZKHIP_ZKEY_VERIFY_SCALAR": scalar})
    assert res.returncode == 255 and "ZKHIP_ZKEY_VERIFY_SCALAR" in res.stderr
