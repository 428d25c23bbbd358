"""The host half of the phase-2 contribution, none of which touches a device: the schedule zk_g1_scale_plan makes of a
scalar (the endomorphism split and its joint signed-digit recoding) against Python integers, and `zkeycontribute`'s
argument and file errors, every one of them refused before any device call."""
import math
import os
import random
import struct
import subprocess

import pytest

from conftest import ROOT, golden_bytes

from oracle import bn254 as bn
from rapidsnark_old_amd import lib as L

RM, QM = bn.R_MOD, bn.Q_MOD
BETA = 2203960485148121921418603742825762020974279258880205651966
LAMBDA = 4407920970296243842393367215006156084916469457145843978461
ZKEYCONTRIBUTE = os.path.join(ROOT, "rapidsnark-old_amd", "zkeycontribute")
PLAN_MAX = 130                                         # ZK_SCALE_PLAN_MAX of include/zkhip.h


def lattice_basis():
    """the reduced basis of {(a, b): a + b lambda = 0 mod r}: the extended Euclid on (r, lambda), stopped around sqrt(r)"""
    rows, (r0, t0), (r1, t1) = [], (RM, 0), (LAMBDA, 1)
    while r1:
        q = r0 // r1
        (r0, t0), (r1, t1) = (r1, t1), (r0 - q * r1, t0 - q * t1)
        rows.append((r0, -t0))
    i = next(j for j, (rr, _) in enumerate(rows) if rr < math.isqrt(RM))
    v1 = rows[i]
    v2 = min(rows[i - 1], rows[i + 1], key=lambda v: v[0] ** 2 + v[1] ** 2)
    return v1, v2


def edge_scalars():
    """the scalars at which the split or the recoding can go wrong"""
    out = [0, 1, 2, 3, RM - 1, RM - 2, LAMBDA, LAMBDA + 1, LAMBDA - 1, RM - LAMBDA, LAMBDA * LAMBDA % RM, (RM + 1) // 2, (RM - 1) // 2,
           1 << 127, (1 << 128) + 1, (1 << 128) - 1]
    for v in lattice_basis():
        for x in v:
            out += [x % RM, -x % RM]
    return out


def test_the_constants():
    assert pow(BETA, 3, QM) == 1 and BETA != 1
    assert (LAMBDA * LAMBDA + LAMBDA + 1) % RM == 0
    lam_g = bn.G1.mul(bn.G1.gen, LAMBDA)                # phi(x, y) = (beta x, y) = lambda (x, y)
    assert lam_g == (BETA * bn.G1.gen[0] % QM, bn.G1.gen[1])
    for a, b in lattice_basis():
        assert (a + b * LAMBDA) % RM == 0 and abs(a) < 1 << 128 and abs(b) < 1 << 128


def check_plan(k):
    dp, dphi = L.g1_scale_plan(k)
    assert len(dp) == len(dphi) <= PLAN_MAX
    assert all(d in (-1, 0, 1) for d in dp + dphi)
    assert sum((a + LAMBDA * b) << i for i, (a, b) in enumerate(zip(dp, dphi))) % RM == k
    if dp:
        assert dp[-1] or dphi[-1]                       # the top column is not empty: no doubling of infinity is scheduled
    return dp, dphi


@pytest.mark.parametrize("k", edge_scalars())
def test_plan_of_edge_scalars(k):
    check_plan(k)


def test_plan_of_zero_is_empty_and_of_one_is_one_column():
    assert L.g1_scale_plan(0) == ([], [])
    assert L.g1_scale_plan(1) == ([1], [0])
    assert L.g1_scale_plan(LAMBDA) == ([0], [1])
    assert L.g1_scale_plan(RM - 1) == ([-1], [0])


def test_plan_of_random_scalars_halves_the_length():
    rng = random.Random(20261017)
    longest, filled = 0, 0
    for _ in range(1000):
        dp, dphi = check_plan(rng.randrange(RM))
        longest = max(longest, len(dp))
        filled += sum(1 for a, b in zip(dp, dphi) if a or b)
    assert longest <= 128                               # |k1|, |k2| < 2^127 and a joint sparse form is one digit longer
    assert filled < 1000 * 70                           # about half of ~127 columns are empty (the form's density is 1/2)


def test_plan_refuses_r_and_a_short_buffer():
    import ctypes as C
    with pytest.raises(L.ZkHipError, match="not below r"):
        L.g1_scale_plan(RM)
    with pytest.raises(L.ZkHipError, match="not below r"):
        L.g1_scale_plan((1 << 256) - 1)
    lib = L.load_library()
    a, b, n = (C.c_int8 * 4)(), (C.c_int8 * 4)(), C.c_uint32(0)
    k = (C.c_uint8 * 32)(*(RM - 12345).to_bytes(32, "little"))
    assert lib.zk_g1_scale_plan(C.cast(k, C.c_void_p), a, b, 4, C.byref(n)) != 0
    assert n.value > 4 and b"room for 4" in lib.zk_last_error()


# ---------------------------------------------------------------- zkeycontribute: arguments and files
def run(*args, scalar="12345"):
    env = dict(os.environ)
    env.pop("ZKHIP_CONTRIB_SCALAR", None)
    if scalar is not None:
        env["ZKHIP_CONTRIB_SCALAR"] = scalar
    return subprocess.run([ZKEYCONTRIBUTE, *args], capture_output=True, text=True, timeout=120, env=env)


def sections_of(data):
    (n,) = struct.unpack_from("<I", data, 8)
    at, out = 12, []
    for _ in range(n):
        sid, size = struct.unpack_from("<IQ", data, at)
        out.append((sid, data[at + 12:at + 12 + size]))
        at += 12 + size
    return out


def binfile(magic, version, secs):
    out = [magic, struct.pack("<II", version, len(secs))]
    for sid, payload in secs:
        out += [struct.pack("<IQ", sid, len(payload)), payload]
    return b"".join(out)


def test_zkeycontribute_arguments_and_file_errors(tmp_path):
    good = golden_bytes("r1cs_n8", "circuit.zkey")
    secs = sections_of(good)
    assert [sid for sid, _ in secs] == list(range(1, 11))
    ip, op, vp = str(tmp_path / "in.zkey"), str(tmp_path / "out.zkey"), str(tmp_path / "vk.json")
    for argv in ((), (ip,), (ip, op, vp, vp)):
        res = run(*argv)
        assert res.returncode == 255 and "Usage: zkeycontribute" in res.stderr
    res = run(ip, op)
    assert res.returncode == 255 and res.stderr.strip() and "HIP" not in res.stderr            # no such input
    assert os.listdir(str(tmp_path)) == []

    def with_section(sid, f):
        return binfile(b"zkey", 1, [(s, f(p) if s == sid else p) for s, p in secs])

    sec2 = dict(secs)[2]
    other_q = sec2[:4] + RM.to_bytes(32, "little") + sec2[36:]
    n_h = len(dict(secs)[9])
    cases = [(b"ptau" + good[4:], "Invalid file type. It should be zkey and it us ptau"),
             (b"r1cs" + good[4:], "Invalid file type. It should be zkey and it us r1cs"),
             (good[:4] + struct.pack("<I", 2) + good[8:], "Invalid version"),
             (good[:-100], "Unexpected end of file"),
             (with_section(9, lambda p: p[:-64]), "zkey section 9 is short: %d bytes, the header implies %d" % (n_h - 64, n_h)),
             (with_section(8, lambda p: p[:-1]), "zkey section 8 is short"),
             (with_section(5, lambda p: p + bytes(64)), "zkey section 5 is long"),
             (with_section(4, lambda p: p[:-44]), "zkey section 4 is short"),
             (with_section(2, lambda p: p[:-128]), "Invalid section size"),
             (binfile(b"zkey", 1, [(s, p) for s, p in secs if s != 9]), "zkey has no section 9"),
             (binfile(b"zkey", 1, [(s, p) for s, p in secs if s != 10]), "zkey has no section 10"),
             (with_section(1, lambda p: struct.pack("<I", 2)), "zkey file is not groth16"),
             (with_section(2, lambda p: other_q), "zkey curve not supported"),
             (with_section(2, lambda p: p[:-128] + bytes(127) + b"\x01"), "vk_delta_2 is not a point of the curve"),
             (with_section(2, lambda p: p[:-192] + bytes(64) + p[-128:]), "vk_delta_1 is not a point of the curve")]
    for data, msg in cases:
        with open(ip, "wb") as f:
            f.write(data)
        for extra in ((), (vp,)):
            res = run(ip, op, *extra)
            assert res.returncode == 255 and msg in res.stderr, (msg, res.stderr)
            assert "HIP" not in res.stderr, res.stderr
            assert sorted(os.listdir(str(tmp_path))) == ["in.zkey"], msg

    with open(ip, "wb") as f:
        f.write(good)
    for scalar in ("0", str(RM), str(RM + 5), "12x", "", "-3", "0x10", "9" * 90):
        res = run(ip, op, vp, scalar=scalar)
        assert res.returncode == 255 and "ZKHIP_CONTRIB_SCALAR is not a decimal number d with 0 < d < r" in res.stderr, (scalar, res.stderr)
        assert scalar == "" or len(scalar) < 4 or scalar not in res.stderr          # the value is not echoed
        assert sorted(os.listdir(str(tmp_path))) == ["in.zkey"], scalar
    res = run(ip, ip)
    assert res.returncode == 255 and "the same file" in res.stderr
    os.link(ip, op)                                                          # another name of the same file
    res = run(ip, op)
    assert res.returncode == 255 and "the same file" in res.stderr
    with open(ip, "rb") as f:
        assert f.read() == good


def test_python_zkey_contribute_refuses_before_the_device(tmp_path):
    from rapidsnark_old_amd import zkey_contribute
    good = golden_bytes("r1cs_n8", "circuit.zkey")
    secs = sections_of(good)
    ip, op = str(tmp_path / "in.zkey"), str(tmp_path / "out.zkey")
    with open(ip, "wb") as f:
        f.write(good)
    for d in (0, RM, -1):
        with pytest.raises(ValueError, match="0 < d < r"):
            zkey_contribute(ip, op, d=d)
    with pytest.raises(ValueError, match="the same file"):
        zkey_contribute(ip, ip, d=5)
    short = str(tmp_path / "short.zkey")
    with open(short, "wb") as f:
        f.write(binfile(b"zkey", 1, [(s, p[:-64] if s == 9 else p) for s, p in secs]))
    with pytest.raises(ValueError, match="zkey section 9 is short"):
        zkey_contribute(short, op, d=5)
    with open(short, "wb") as f:
        f.write(b"ptau" + good[4:])
    with pytest.raises(ValueError, match="not a zkey file"):
        zkey_contribute(short, op, d=5)
    assert sorted(os.listdir(str(tmp_path))) == ["in.zkey", "short.zkey"]


# ---------------------------------------------------------------- zkeycontribute: the exact exit code, stdout and stderr
def exact_case(name, d):
    """-> (argv, ZKHIP_CONTRIB_SCALAR) of one refusal; the files are written into d, which is the program's directory"""
    secs = sections_of(golden_bytes("r1cs_n8", "circuit.zkey"))
    patch = lambda sid, f: binfile(b"zkey", 1, [(s, f(p) if s == sid else p) for s, p in secs])
    without = lambda sid: binfile(b"zkey", 1, [(s, p) for s, p in secs if s != sid])
    data = {"usage": None,
            "nPublic_exceeds_nVars": patch(2, lambda p: p[:76] + p[72:76] + p[80:]),        # nPublic := nVars
            "section_4_without_count": patch(4, lambda p: p[:2]),
            "section_3_long": patch(3, lambda p: p + bytes(64)),
            "section_6_short": patch(6, lambda p: p[:-64]),
            "section_7_long": patch(7, lambda p: p + bytes(128)),
            "no_section_1": without(1),
            "no_section_4": without(4)}.get(name, binfile(b"zkey", 1, secs))
    if data is not None:
        with open(os.path.join(d, "in.zkey"), "wb") as f:
            f.write(data)
    argv = {"usage": (), "out_directory_missing": ("in.zkey", "nowhere/out.zkey"),
            "vk_directory_missing": ("in.zkey", "out.zkey", "nowhere/vk.json")}.get(name, ("in.zkey", "out.zkey"))
    scalar = {"scalar_2p256": str(1 << 256), "scalar_r": str(RM), "scalar_zero": "0", "scalar_empty": "", "scalar_leading_space": " 5"}.get(name, "12345")
    return argv, scalar


BAD_SCALAR = "ZKHIP_CONTRIB_SCALAR is not a decimal number d with 0 < d < r\n"
EXACT = {      # what the programs of the commit before the host helpers were shared printed: (exit code, stdout, stderr)
    "usage": (255, "", "Invalid number of parameters:\nUsage: zkeycontribute <in.zkey> <out.zkey> [verification_key.json]\n"),
    "nPublic_exceeds_nVars": (255, "", "zkey header: nPublic + 1 exceeds nVars\n"),
    "section_4_without_count": (255, "", "zkey section 4 is short: it has no record count\n"),
    "section_3_long": (255, "", "zkey section 3 is long: 192 bytes, the header implies 128\n"),
    "section_6_short": (255, "", "zkey section 6 is short: 512 bytes, the header implies 576\n"),
    "section_7_long": (255, "", "zkey section 7 is long: 1280 bytes, the header implies 1152\n"),
    "no_section_1": (255, "", "zkey has no section 1\n"),
    "no_section_4": (255, "", "zkey has no section 4\n"),
    "out_directory_missing": (255, "", "cannot write nowhere/out.zkey\n"),
    "vk_directory_missing": (255, "", "cannot write nowhere/vk.json\n"),
    "scalar_2p256": (255, "", BAD_SCALAR),
    "scalar_r": (255, "", BAD_SCALAR),
    "scalar_zero": (255, "", BAD_SCALAR),
    "scalar_empty": (255, "", BAD_SCALAR),
    "scalar_leading_space": (255, "", BAD_SCALAR),
}


@pytest.mark.parametrize("name", sorted(EXACT))
def test_zkeycontribute_exact_refusals_before_the_device(name, tmp_path):
    argv, scalar = exact_case(name, str(tmp_path))
    res = subprocess.run([ZKEYCONTRIBUTE, *argv], capture_output=True, text=True, timeout=120, cwd=str(tmp_path),
                         env=dict(os.environ, ZKHIP_CONTRIB_SCALAR=scalar))
    assert (res.returncode, res.stdout, res.stderr) == EXACT[name]
    assert sorted(os.listdir(str(tmp_path))) == ([] if name == "usage" else ["in.zkey"])
