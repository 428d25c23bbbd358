"""`ptaucheck`'s argument and file errors, PtauFile.file_view, the size check of the .ptau check (zk_ptau_check_sizes: host
only) and the fixture of twist points outside the subgroup: none of it touches a device.  The .ptau files are
tests/test_ptau_prepare_host.py's, written with oracle.bn254."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT, golden_path

from oracle import bn254 as bn
from rapidsnark_old_amd import ptau as P
from rapidsnark_old_amd.lib import ZkHipError
from test_ptau_prepare_host import LAG, ptau_bytes

RM, QM = bn.R_MOD, bn.Q_MOD
PTAUCHECK = os.path.join(ROOT, "rapidsnark-old_amd", "ptaucheck")


@pytest.fixture(scope="module")
def files():
    return {(power, prepared): ptau_bytes(power, drop=() if prepared else LAG) for power in (1, 2, 3) for prepared in (False, True)}


def run(*args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([PTAUCHECK, *args], capture_output=True, text=True, timeout=120, env=e)


def write(tmp_path, data):
    p = str(tmp_path / "in.ptau")
    with open(p, "wb") as f:
        f.write(data)
    return p


def test_arguments_and_a_missing_file(tmp_path):
    ip = str(tmp_path / "in.ptau")
    for argv in ((), (ip, ip)):
        res = run(*argv)
        assert res.returncode == 255 and "Usage: ptaucheck <file.ptau>" in res.stderr and res.stdout == ""
    res = run(ip)
    assert res.returncode == 255 and res.stderr.strip() and res.stdout == ""


def test_file_errors_leave_with_255(tmp_path, files):
    good = files[(2, True)]
    cases = [(b"zkey" + good[4:], "Invalid file type"),
             (good[:len(good) - 100], ""),                                   # truncated: the last section runs past the end
             (good[:40], ""),
             (ptau_bytes(2, q=RM), "ptau curve not supported"),
             (ptau_bytes(2, n8=48), "only 256-bit fields"),
             (ptau_bytes(2, header_power=0), "power 0 is not supported"),
             (ptau_bytes(2, drop=LAG, header_power=29), "power 29 is not supported"),
             (ptau_bytes(2, header_power=28), "power 28 is not supported"),    # a prepared file stops at 27
             (ptau_bytes(2, short=(3, 1)), "ptau section 3 is short: 511 bytes, power 2 needs 512"),
             (ptau_bytes(2, short=(2, 64)), "ptau section 2 is short: 384 bytes, power 2 needs 448"),
             (ptau_bytes(2, short=(13, 128)), "ptau section 13 is short: 768 bytes, power 2 needs 896"),
             (ptau_bytes(2, drop=(15,)), "only some of the Lagrange sections 12 to 15 (section 15 is missing)"),
             (ptau_bytes(2, drop=(12, 14)), "only some of the Lagrange sections 12 to 15 (section 12 is missing)")]
    cases += [(ptau_bytes(2, drop=LAG + (sid,)), "ptau has no section %d" % sid) for sid in (2, 3, 4, 5, 6)]
    cases += [(ptau_bytes(2, drop=(sid,)), "ptau has no section %d" % sid) for sid in (2, 6)]
    for data, msg in cases:
        res = run(write(tmp_path, data))
        assert res.returncode == 255 and res.stdout == "" and res.stderr.strip() and msg in res.stderr, (msg, res.stderr)


@pytest.mark.parametrize("scalar", ["0", "1", str(RM), str(RM + 5), "12x", "-3", ""])
def test_the_test_scalar_is_refused_before_the_device(tmp_path, files, scalar):
    res = run(write(tmp_path, files[(1, True)]), env={"ZKHIP_PTAU_CHECK_SCALAR": scalar})
    assert res.returncode == 255 and res.stdout == "" and "ZKHIP_PTAU_CHECK_SCALAR" in res.stderr


@pytest.mark.parametrize("power", [1, 2, 3])
def test_sizes_of_good_files(files, power):
    n = 1 << power
    z = P.ptau_check_sizes(files[(power, False)])
    assert (z["prepared"], z["chunk_points"]) == (0, n)                       # the largest range is a whole row of sections 3 to 5
    z1 = P.ptau_check_sizes(files[(power, True)])
    assert (z1["prepared"], z1["chunk_points"]) == (1, 2 * n)                 # level power + 1 of section 12
    assert 0 < z["device_bytes"] <= z1["device_bytes"] < 1 << 32


def test_sizes_follow_the_chunk_variable(files, monkeypatch):
    monkeypatch.setenv("ZKHIP_PTAU_CHUNK", "3")
    assert P.ptau_check_sizes(files[(3, True)])["chunk_points"] == 3
    monkeypatch.setenv("ZKHIP_PTAU_CHUNK", "0")
    with pytest.raises(ZkHipError, match="ZKHIP_PTAU_CHUNK"):
        P.ptau_check_sizes(files[(3, True)])


@pytest.mark.parametrize("args,msg", [
    (dict(short=(5, 64)), r"section 5 is short: 192 bytes, power 2 needs 256"),
    (dict(short=(6, 1)), r"section 6 is short: 127 bytes, power 2 needs 128"),
    (dict(short=(12, 64)), r"section 12 is short: 896 bytes, power 2 needs 960"),
    (dict(drop=(4,)), "no section 4"),
    (dict(drop=(13,)), "only some of the Lagrange sections"),
    (dict(header_power=0), "power 0 is not supported"),
    (dict(header_power=28), "power 28 is not supported"),
])
def test_sizes_refuses_bad_files(args, msg):
    with pytest.raises(ZkHipError, match=msg):
        P.ptau_check_sizes(ptau_bytes(2, **args))
    with pytest.raises(ZkHipError, match=msg):                               # the check itself refuses them too, before any device
        P.ptau_check(ptau_bytes(2, **args), s=5)


def test_the_file_view(files):
    f = P.PtauFile(files[(2, True)])
    v = f.file_view()
    assert v.power == 2
    assert [int(v.sec_bytes[k]) for k in range(16)] == [0, 0, 7 * 64, 4 * 128, 4 * 64, 4 * 64, 128, 0, 0, 0, 0, 0, 15 * 64, 7 * 128, 7 * 64, 7 * 64]
    assert all((v.sec[k] is not None) == (k in (2, 3, 4, 5, 6, 12, 13, 14, 15)) for k in range(16))
    assert v.sec[3] == f.section(3).ctypes.data and v.sec[15] == f.section(15).ctypes.data
    u = P.PtauFile(files[(2, False)]).file_view()
    assert all(u.sec[k] is None and u.sec_bytes[k] == 0 for k in LAG)


def test_the_fixture_generator_reproduces_the_committed_fixture(tmp_path):
    out = str(tmp_path / "points.json")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_g2_cofactor_points.py"), out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    with open(out, "rb") as f, open(golden_path("g2_cofactor_points.json"), "rb") as g:
        assert f.read() == g.read()


def test_the_fixture_holds_what_it_says():
    """every point is on the twist; the cofactor points have their prime orders, whose product is 2q - r; nothing is in the
    order-r subgroup"""
    from conftest import golden_json
    d = golden_json("g2_cofactor_points.json")
    dec = lambda p: ((int(p["x"][0]), int(p["x"][1])), (int(p["y"][0]), int(p["y"][1])))
    prod = 1
    for p in d["cofactor"]:
        Pt, l = dec(p), int(p["order"])
        prod *= l
        assert bn.G2.is_on_curve(Pt) and bn.G2.mul(Pt, l) is None and bn.G2.mul(Pt, RM) is not None
    assert len(d["cofactor"]) == 4 and prod == 2 * QM - RM == int(d["h2"])
    assert len(d["outside"]) == 8
    for p in d["outside"]:
        assert bn.G2.is_on_curve(dec(p)) and bn.G2.mul(dec(p), RM) is not None
