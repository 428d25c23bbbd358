"""`ptauprepare`'s argument and file errors, PtauFile.prepared / powers_view and the size check of the phase-2 preparation
(zk_ptau_prepare_sizes: host only), none of which touches a device.  The .ptau files are written here with oracle.bn254."""
import os
import struct
import subprocess

import pytest

from conftest import ROOT

from oracle import bn254 as bn
from rapidsnark_old_amd import ptau as P
from rapidsnark_old_amd.lib import ZkHipError

RM, QM = bn.R_MOD, bn.Q_MOD
PTAUPREPARE = os.path.join(ROOT, "rapidsnark-old_amd", "ptauprepare")
TAU, ALPHA, BETA = 1234567, 89101112, 13141516


def lagrange(tau, n, zero_top=False):
    """L_j^(n)(tau) = 1/n sum_k tau^k w^-jk, the top power left out on request"""
    w = bn.fr_root(n.bit_length() - 1)
    winv, ninv = pow(w, -1, RM), pow(n, -1, RM)
    kmax = n - 1 if zero_top else n
    return [sum(pow(tau, k, RM) * pow(winv, j * k, RM) for k in range(kmax)) * ninv % RM for j in range(n)]


def g1(x):
    return bn.g1_to_bytes(bn.G1.mul(bn.G1.gen, x % RM))


def g2(x):
    return bn.g2_to_bytes(bn.G2.mul(bn.G2.gen, x % RM))


def ptau_bytes(power, drop=(), short=None, q=QM, n8=32, magic=b"ptau", header_power=None):
    """a prepared .ptau of `power` from (TAU, ALPHA, BETA), as tests/test_ptau_host.py's; drop: section ids left out;
    short: (section, bytes cut off); header_power: the power the header claims"""
    n = 1 << power
    levels = lambda top, zt: [lagrange(TAU, 1 << p, zero_top=(zt and p == top)) for p in range(top + 1)]
    l12 = [x for lvl in levels(power + 1, True) for x in lvl]
    l13 = [x for lvl in levels(power, False) for x in lvl]
    hp = power if header_power is None else header_power
    secs = {
        1: struct.pack("<I", n8) + q.to_bytes(n8, "little") + struct.pack("<II", hp, hp),
        2: b"".join(g1(pow(TAU, i, RM)) for i in range(2 * n - 1)),
        3: b"".join(g2(pow(TAU, i, RM)) for i in range(n)),
        4: b"".join(g1(ALPHA * pow(TAU, i, RM)) for i in range(n)),
        5: b"".join(g1(BETA * pow(TAU, i, RM)) for i in range(n)),
        6: g2(BETA),
        7: struct.pack("<I", 0),
        12: b"".join(g1(x) for x in l12),
        13: b"".join(g2(x) for x in l13),
        14: b"".join(g1(ALPHA * x) for x in l13),
        15: b"".join(g1(BETA * x) for x in l13),
    }
    if short:
        sid, cut = short
        secs[sid] = secs[sid][:-cut]
    out = [magic, struct.pack("<II", 1, len(secs) - len(drop))]
    for sid, payload in secs.items():
        if sid not in drop:
            out += [struct.pack("<IQ", sid, len(payload)), payload]
    return b"".join(out)


LAG = (12, 13, 14, 15)


def test_prepared_and_the_powers_view():
    assert P.PtauFile(ptau_bytes(1)).prepared
    assert not P.PtauFile(ptau_bytes(1, drop=(14,))).prepared
    f = P.PtauFile(ptau_bytes(2, drop=LAG))
    assert not f.prepared
    v = f.powers_view()
    assert (v.power, v.tau_g1_bytes, v.tau_g2_bytes, v.alpha_tau_g1_bytes, v.beta_tau_g1_bytes) == (2, 7 * 64, 4 * 128, 4 * 64, 4 * 64)
    assert v.tau_g1 == f.section(2).ctypes.data and v.beta_tau_g1 == f.section(5).ctypes.data
    assert not P.PtauFile(ptau_bytes(1, drop=LAG + (3,))).powers_view().tau_g2


def test_sizes_of_power_2():
    z = P.prepare_sizes(ptau_bytes(2, drop=LAG))
    assert z["lagrange_g1_bytes"] == 15 * 64                    # levels 0 .. 3
    assert (z["lagrange_g2_bytes"], z["lagrange_alpha_g1_bytes"], z["lagrange_beta_g1_bytes"]) == (7 * 128, 7 * 64, 7 * 64)
    # the powers, two XYZZ rows + an affine row + a prefix row of the top level, the twiddles and 1/2^p, a page of slack:
    # the same for section 2 (7 powers, top level 2^3, 32-byte field) and section 3 (4 powers, top level 2^2, 64-byte field)
    g1_need = 7 * 64 + 8 * (2 * 128 + 64 + 32) + (4 * 32 + 29 * 32) + 4096
    g2_need = 4 * 128 + 4 * (2 * 256 + 128 + 64) + (2 * 32 + 29 * 32) + 4096
    assert z["device_bytes"] == max(g1_need, g2_need)
    assert P.prepare_sizes(ptau_bytes(2))["lagrange_g1_bytes"] == 15 * 64      # the sizes call does not mind sections 12 to 15


@pytest.mark.parametrize("args,msg", [
    (dict(short=(2, 64)), r"section 2 is short: 384 bytes, power 2 needs 448"),
    (dict(short=(4, 64)), r"section 4 is short: 192 bytes, power 2 needs 256"),
    (dict(short=(3, 1)), r"section 3 is short: 511 bytes, power 2 needs 512"),
    (dict(drop=LAG + (2,)), "no section 2"),
    (dict(drop=LAG + (3,)), "no section 3"),
    (dict(header_power=28), "power 28 is not supported"),
    (dict(header_power=0), "power 0 is not supported"),
])
def test_sizes_refuses_bad_files(args, msg):
    args = dict(args)
    args.setdefault("drop", LAG)
    with pytest.raises(ZkHipError, match=msg):
        P.prepare_sizes(ptau_bytes(2, **args))


def test_prepare_phase2_refuses_a_prepared_file_without_a_device(tmp_path):
    dst = str(tmp_path / "o.ptau")
    with pytest.raises(ValueError, match="already prepared for phase 2"):
        P.prepare_phase2(ptau_bytes(1), dst)
    with pytest.raises(ZkHipError, match="section 5 is short"):
        P.prepare_phase2(ptau_bytes(1, drop=LAG, short=(5, 64)), dst)
    assert os.listdir(str(tmp_path)) == []


def run(*args):
    return subprocess.run([PTAUPREPARE, *args], capture_output=True, text=True, timeout=120)


def test_ptauprepare_arguments_and_file_errors(tmp_path):
    ip, op = str(tmp_path / "in.ptau"), str(tmp_path / "out.ptau")
    for argv in ((), (ip,), (ip, op, op)):
        res = run(*argv)
        assert res.returncode == 255 and "Usage: ptauprepare" in res.stderr
    res = run(ip, op)
    assert res.returncode == 255 and res.stderr.strip()                      # no such input
    unprepared = ptau_bytes(2, drop=LAG)
    cases = [(ptau_bytes(2), "already prepared for phase 2"),
             (ptau_bytes(2, drop=LAG, q=RM), "ptau curve not supported"),
             (ptau_bytes(2, drop=LAG, n8=48), "only 256-bit fields"),
             (b"zkey" + unprepared[4:], "Invalid file type"),
             (ptau_bytes(2, drop=LAG, short=(2, 64)), "section 2 is short"),
             (ptau_bytes(2, drop=LAG, short=(4, 128)), "section 4 is short"),
             (ptau_bytes(2, drop=LAG + (2,)), "no section 2"),
             (ptau_bytes(2, drop=LAG + (3,)), "no section 3"),
             (ptau_bytes(2, drop=LAG + (5,)), "no section 5"),
             (ptau_bytes(2, drop=LAG + (6,)), "no section 6"),
             (ptau_bytes(2, drop=LAG, header_power=28), "power 28 is not supported")]
    for data, msg in cases:
        with open(ip, "wb") as f:
            f.write(data)
        res = run(ip, op)
        assert res.returncode == 255 and msg in res.stderr, (msg, res.stderr)
        assert sorted(os.listdir(str(tmp_path))) == ["in.ptau"], msg
    with open(ip, "wb") as f:
        f.write(unprepared)
    res = run(ip, ip)
    assert res.returncode == 255 and "the same file" in res.stderr
    os.link(ip, op)                                                          # another name of the same file
    res = run(ip, op)
    assert res.returncode == 255 and "the same file" in res.stderr
    with open(ip, "rb") as f:
        assert f.read() == unprepared


# ---------------------------------------------------------------- ptauprepare: the exact exit code, stdout and stderr
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


@pytest.fixture(scope="module")
def unprepared_sections():
    return sections_of(ptau_bytes(1, drop=LAG))


def exact_case(name, d, secs):
    """-> argv of one refusal; the file is written into d, which is the program's directory"""
    patch = lambda sid, f: binfile(b"ptau", 1, [(s, f(p) if s == sid else p) for s, p in secs])
    data = {"usage": None,
            "already_prepared": binfile(b"ptau", 1, secs + [(s, bytes(64)) for s in LAG]),     # sections 12 to 15 are not read
            "no_section_4": binfile(b"ptau", 1, [(s, p) for s, p in secs if s != 4]),
            "section_6_short": patch(6, lambda p: p[:64]),
            "beta_g2_off_the_curve": patch(6, lambda p: p[:96] + (5).to_bytes(32, "little")),
            "beta_g1_at_infinity": patch(5, lambda p: bytes(64) + p[64:]),
            "version_2": binfile(b"ptau", 2, secs)}.get(name, binfile(b"ptau", 1, secs))
    if data is not None:
        with open(os.path.join(d, "in.ptau"), "wb") as f:
            f.write(data)
    return {"usage": (), "out_directory_missing": ("in.ptau", "nowhere/out.ptau"), "input_missing": ("other.ptau", "out.ptau")}.get(name, ("in.ptau", "out.ptau"))


EXACT = {      # what the programs of the commit before the host helpers were shared printed: (exit code, stdout, stderr)
    "usage": (255, "", "Invalid number of parameters:\nUsage: ptauprepare <in.ptau> <out.ptau>\n"),
    "already_prepared": (255, "", "the ptau file is already prepared for phase 2 (it has sections 12 to 15)\n"),
    "no_section_4": (255, "", "ptau has no section 4\n"),
    "section_6_short": (255, "", "ptau section 6 is short\n"),
    "beta_g2_off_the_curve": (255, "", "ptau betaG2 is not a point of the curve\n"),
    "beta_g1_at_infinity": (255, "", "ptau betaTauG1[0] is not a point of the curve\n"),
    "version_2": (255, "", "Invalid version. It should be <=1 and it us 2\n"),
    "out_directory_missing": (255, "", "cannot write nowhere/out.ptau\n"),
    "input_missing": (255, "", "open: No such file or directory\n"),
}


@pytest.mark.parametrize("name", sorted(EXACT))
def test_ptauprepare_exact_refusals_before_the_device(name, tmp_path, unprepared_sections):
    argv = exact_case(name, str(tmp_path), unprepared_sections)
    res = subprocess.run([PTAUPREPARE, *argv], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert (res.returncode, res.stdout, res.stderr) == EXACT[name]
    assert sorted(os.listdir(str(tmp_path))) == ([] if name == "usage" else ["in.ptau"])
