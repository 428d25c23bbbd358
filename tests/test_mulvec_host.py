"""The host half of the Powers of Tau contribution, none of which touches a device: the split zk_glv_split makes of a scalar
(the code every lane of zk_g*_mul_vec runs) against Python integers, `ptaunew` / ptau_new, `ptaucontribute`'s argument and
file errors, every one of them refused before any device call, and zk_ptau_contribute_sizes."""
import os
import random
import struct
import subprocess

import pytest

from conftest import ROOT

from oracle import bn254 as bn
from rapidsnark_old_amd import lib as L, ptau as P, synth
from test_ptau_prepare_host import LAG, ptau_bytes
from test_zkey_contribute_host import LAMBDA, lattice_basis, sections_of

RM, QM = bn.R_MOD, bn.Q_MOD
BIN = os.path.join(ROOT, "rapidsnark-old_amd")
PTAUNEW, PTAUCONTRIBUTE = os.path.join(BIN, "ptaunew"), os.path.join(BIN, "ptaucontribute")


def split_edge_scalars():
    """the scalars at which the split can go wrong: the ends of the range, around +-lambda, powers of two around the halves'
    length, the entries A, B, C of the reduced basis v1 = (A, -B), v2 = (C, A), and fractions of r"""
    (a, mb), (c, a2) = lattice_basis()
    assert a == a2 and mb < 0 and a * a - mb * c == RM
    out = [0, 1, 2, RM - 1, RM - 2]
    out += [s * LAMBDA % RM for s in (1, -1)] + [(s * LAMBDA + t) % RM for s in (1, -1) for t in (1, -1)] + [LAMBDA * LAMBDA % RM]
    out += [(1 << 127) - 1, 1 << 127, 1 << 128, 1 << 253, a, -mb, c, RM // 2, RM // 2 + 1, RM // 3]
    return out


def check_split(k):
    k1, k2 = L.glv_split(k)
    assert 0 <= k1 < 1 << 128 and 0 <= k2 < 1 << 128, k
    assert (k1 + k2 * LAMBDA - k) % RM == 0, k
    return k1, k2


@pytest.mark.parametrize("k", split_edge_scalars())
def test_split_of_edge_scalars(k):
    check_split(k)


def test_split_of_zero_is_a_lattice_vector():
    (a, mb), (c, _) = lattice_basis()
    assert L.glv_split(0) == (c - a, a - mb)            # v2 - v1 = (C - A, A + B)


def test_split_of_random_scalars():
    rng = random.Random(20261018)
    low = 1 << 128
    for _ in range(20000):
        low = min(low, *check_split(rng.randrange(RM)))
    assert low > 0                                       # the bound of csrc/glv.hpp: both halves are strictly positive


def test_split_refuses_r():
    for k in (RM, RM + 1, (1 << 256) - 1):
        with pytest.raises(L.ZkHipError, match="not below r"):
            L.glv_split(k)


# ---------------------------------------------------------------- ptaunew / ptau_new
def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("power", [1, 3])
def test_ptaunew_writes_generators(tmp_path, power):
    cli, py = str(tmp_path / "cli.ptau"), str(tmp_path / "py.ptau")
    res = subprocess.run([PTAUNEW, str(power), cli], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout == "", res.stderr
    P.ptau_new(power, py)
    data = read(cli)
    assert data == read(py)
    assert sorted(os.listdir(str(tmp_path))) == ["cli.ptau", "py.ptau"]
    assert data[:8] == b"ptau" + struct.pack("<I", 1)
    secs = sections_of(data)
    assert [sid for sid, _ in secs] == [1, 2, 3, 4, 5, 6, 7]
    s = dict(secs)
    assert s[1] == struct.pack("<I", 32) + QM.to_bytes(32, "little") + struct.pack("<II", power, power)
    n = 1 << power
    g1, g2 = synth.g1_gen_bytes(), synth.g2_gen_bytes()
    assert g1 == bn.g1_to_bytes(bn.G1.gen) and g2 == bn.g2_to_bytes(bn.G2.gen)
    assert s[2] == g1 * (2 * n - 1) and s[3] == g2 * n and s[4] == g1 * n and s[5] == g1 * n and s[6] == g2
    assert s[7] == bytes(4)
    f = P.PtauFile(cli)
    assert (f.power, f.ceremony_power, f.prepared) == (power, power, False)
    f.close()


@pytest.mark.parametrize("argv", [("0",), ("29",), ("-1",), ("3x",), ("",), ("4294967297",)])
def test_ptaunew_refuses_other_powers(tmp_path, argv):
    res = subprocess.run([PTAUNEW, *argv, str(tmp_path / "out.ptau")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 255 and "the power must be a number from 1 to 28" in res.stderr and res.stdout == ""
    assert os.listdir(str(tmp_path)) == []


def test_ptaunew_arguments(tmp_path):
    for argv in ((), ("3",), ("3", str(tmp_path / "a"), "b")):
        res = subprocess.run([PTAUNEW, *argv], capture_output=True, text=True, timeout=120)
        assert res.returncode == 255 and "Usage: ptaunew <power> <out.ptau>" in res.stderr
    res = subprocess.run([PTAUNEW, "2", str(tmp_path / "nowhere" / "out.ptau")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 255 and "cannot write" in res.stderr
    assert os.listdir(str(tmp_path)) == []
    for power in (0, 29):
        with pytest.raises(ValueError, match="power"):
            P.ptau_new(power, str(tmp_path / "py.ptau"))
    assert os.listdir(str(tmp_path)) == []


# ---------------------------------------------------------------- ptaucontribute: arguments and files
def contribute(*args, scalars="5,6,7"):
    env = dict(os.environ)
    env.pop("ZKHIP_PTAU_CONTRIB_SCALARS", None)
    if scalars is not None:
        env["ZKHIP_PTAU_CONTRIB_SCALARS"] = scalars
    return subprocess.run([PTAUCONTRIBUTE, *args], capture_output=True, text=True, timeout=120, env=env)


@pytest.fixture(scope="module")
def good():
    return ptau_bytes(2, drop=LAG)


def test_ptaucontribute_arguments_and_file_errors(tmp_path, good):
    ip, op = str(tmp_path / "in.ptau"), str(tmp_path / "out.ptau")
    for argv in ((), (ip,), (ip, op, op)):
        res = contribute(*argv)
        assert res.returncode == 255 and "Usage: ptaucontribute <in.ptau> <out.ptau>" in res.stderr
    res = contribute(ip, op)
    assert res.returncode == 255 and res.stderr.strip() and "HIP" not in res.stderr            # no such input
    assert os.listdir(str(tmp_path)) == []
    cases = [(b"zkey" + good[4:], "Invalid file type"),
             (good[:-100], ""),                                                  # truncated: the last section runs past the end
             (good[:40], ""),
             (ptau_bytes(2, drop=LAG, q=RM), "ptau curve not supported"),
             (ptau_bytes(2, drop=LAG, n8=48), "only 256-bit fields"),
             (ptau_bytes(2, drop=LAG, header_power=0), "power 0 is not supported"),
             (ptau_bytes(2, drop=LAG, header_power=29), "power 29 is not supported"),
             (ptau_bytes(2, drop=LAG, short=(3, 1)), "ptau section 3 is short: 511 bytes, power 2 needs 512"),
             (ptau_bytes(2, drop=LAG, short=(2, 64)), "ptau section 2 is short: 384 bytes, power 2 needs 448"),
             (ptau_bytes(2, drop=LAG, short=(6, 1)), "ptau section 6 is short: 127 bytes, power 2 needs 128"),
             (ptau_bytes(2), "contribute before `ptauprepare`"),                    # a prepared input
             (ptau_bytes(2, drop=(12, 13, 15)), "contribute before `ptauprepare`")]
    cases += [(ptau_bytes(2, drop=LAG + (sid,)), "ptau has no section %d" % sid) for sid in (2, 3, 4, 5, 6)]
    for data, msg in cases:
        with open(ip, "wb") as f:
            f.write(data)
        res = contribute(ip, op)
        assert res.returncode == 255 and res.stdout == "" and res.stderr.strip() and msg in res.stderr, (msg, res.stderr)
        assert "HIP" not in res.stderr, res.stderr
        assert sorted(os.listdir(str(tmp_path))) == ["in.ptau"], msg

    with open(ip, "wb") as f:
        f.write(good)
    for scalars in ("", "5", "5,6", "5,6,7,8", "0,6,7", "5,0,7", "5,6,0", "5,6,%d" % RM, "%d,6,7" % (RM + 5), "5,6x,7", "5, 6,7", "-5,6,7",
                    "0x10,6,7", "5,6," + "9" * 90, ",,"):
        res = contribute(ip, op, scalars=scalars)
        assert res.returncode == 255 and "ZKHIP_PTAU_CONTRIB_SCALARS is not three decimal numbers" in res.stderr, (scalars, res.stderr)
        assert len(scalars) < 8 or scalars not in res.stderr                       # the values are not echoed
        assert sorted(os.listdir(str(tmp_path))) == ["in.ptau"], scalars
    res = contribute(ip, ip)
    assert res.returncode == 255 and "the same file" in res.stderr
    os.link(ip, op)                                                                # another name of the same file
    res = contribute(ip, op)
    assert res.returncode == 255 and "the same file" in res.stderr
    assert read(ip) == good


def test_python_ptau_contribute_refuses_before_the_device(tmp_path, good):
    ip, op = str(tmp_path / "in.ptau"), str(tmp_path / "out.ptau")
    with open(ip, "wb") as f:
        f.write(good)
    for bad in ((0, 6, 7), (5, RM, 7), (5, 6, -1)):
        with pytest.raises(ValueError, match="0 < s < r"):
            P.ptau_contribute(ip, op, *bad)
    with pytest.raises(ValueError, match="the same file"):
        P.ptau_contribute(ip, ip, 5, 6, 7)
    other = str(tmp_path / "other.ptau")
    for data, exc, msg in ((ptau_bytes(2, drop=LAG, short=(5, 64)), L.ZkHipError, "ptau section 5 is short: 192 bytes, power 2 needs 256"),
                           (ptau_bytes(2), L.ZkHipError, "contribute before `ptauprepare`"),
                           (b"zkey" + good[4:], ValueError, "not a ptau file")):
        with open(other, "wb") as f:
            f.write(data)
        with pytest.raises(exc, match=msg):
            P.ptau_contribute(other, op, 5, 6, 7)
    assert sorted(os.listdir(str(tmp_path))) == ["in.ptau", "other.ptau"]


# ---------------------------------------------------------------- zk_ptau_contribute_sizes
def test_contribute_sizes_of_power_3(monkeypatch):
    monkeypatch.delenv("ZKHIP_PTAU_CONTRIB_CHUNK", raising=False)
    z = P.ptau_contribute_sizes(ptau_bytes(3, drop=LAG))
    assert (z["tau_g1_bytes"], z["tau_g2_bytes"], z["alpha_tau_g1_bytes"], z["beta_tau_g1_bytes"], z["beta_g2_bytes"]) == (15 * 64, 8 * 128, 8 * 64, 8 * 64, 128)
    assert z["chunk_points"] == 15                      # section 2 in one chunk
    # two buffer sets of a chunk each (points, XYZZ, the normalisation's prefix row, a page) and the table of squarings
    # with the factor, a page of slack; the groups run one after the other
    g1_need = 2 * (15 * (64 + 128 + 32) + 4096) + 65 * 32 + 4096
    g2_need = 2 * (8 * (128 + 256 + 64) + 4096) + 65 * 32 + 4096
    assert z["device_bytes"] == max(g1_need, g2_need)
    monkeypatch.setenv("ZKHIP_PTAU_CONTRIB_CHUNK", "4")
    assert P.ptau_contribute_sizes(ptau_bytes(3, drop=LAG))["chunk_points"] == 4
    monkeypatch.setenv("ZKHIP_PTAU_CONTRIB_CHUNK", "0")
    with pytest.raises(L.ZkHipError, match="ZKHIP_PTAU_CONTRIB_CHUNK"):
        P.ptau_contribute_sizes(ptau_bytes(3, drop=LAG))


@pytest.mark.parametrize("args,msg", [
    (dict(short=(4, 64)), r"section 4 is short: 192 bytes, power 2 needs 256"),
    (dict(drop=LAG + (5,)), "no section 5"),
    (dict(drop=()), "contribute before `ptauprepare`"),
    (dict(header_power=0), "power 0 is not supported"),
    (dict(header_power=29), "power 29 is not supported"),
])
def test_contribute_sizes_refuses_bad_files(args, msg):
    args = dict({"drop": LAG}, **args)
    with pytest.raises(L.ZkHipError, match=msg):
        P.ptau_contribute_sizes(ptau_bytes(2, **args))
