"""The .ptau reader (rapidsnark_old_amd.ptau), the setup's size and file checks (zk_groth16_setup_sizes: host only) and
`zkeynew`'s argument and file errors, none of which touches a device.  The .ptau files are written here with oracle.bn254."""
import os
import struct
import subprocess

import pytest

from conftest import ROOT

from oracle import bn254 as bn, groth16_ref as g
from rapidsnark_old_amd import ptau as P, r1cs as R
from rapidsnark_old_amd.lib import ZkHipError

RM, QM = bn.R_MOD, bn.Q_MOD
ZKEYNEW = os.path.join(ROOT, "rapidsnark-old_amd", "zkeynew")
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


def ptau_bytes(power, drop=(), short=None, q=QM, n8=32, magic=b"ptau", alpha1=None):
    """a prepared .ptau of `power` from (TAU, ALPHA, BETA); drop: section ids left out; short: (section, bytes cut off)"""
    n = 1 << power
    levels = lambda top, zt: [lagrange(TAU, 1 << p, zero_top=(zt and p == top)) for p in range(top + 1)]
    l12 = [x for lvl in levels(power + 1, True) for x in lvl]
    l13 = [x for lvl in levels(power, False) for x in lvl]
    secs = {
        1: struct.pack("<I", n8) + q.to_bytes(n8, "little") + struct.pack("<II", power, power),
        2: b"".join(g1(pow(TAU, i, RM)) for i in range(2 * n - 1)),
        3: b"".join(g2(pow(TAU, i, RM)) for i in range(n)),
        4: alpha1 if alpha1 is not None else b"".join(g1(ALPHA * pow(TAU, i, RM)) for i in range(n)),
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


@pytest.fixture(scope="module")
def p2():
    return ptau_bytes(2)


def circuit(n_constraints):
    """n_constraints copies of multiplier2's constraint (nPublic 1): 2^k >= n_constraints + 2"""
    return R.write_r1cs_rows([{2: 1}] * n_constraints, [{3: 1}] * n_constraints, [{1: 1}] * n_constraints, 4, 1)


def test_reader_header_and_levels(p2):
    f = P.PtauFile(p2)
    assert (f.n8, f.q, f.power, f.ceremony_power, f.prepared) == (32, QM, 2, 2, True)
    for p in range(4):
        assert bytes(f.level(12, p)) == b"".join(g1(x) for x in lagrange(TAU, 1 << p, zero_top=(p == 3)))
    for p in range(3):
        assert bytes(f.level(13, p)) == b"".join(g2(x) for x in lagrange(TAU, 1 << p))
        assert bytes(f.level(15, p)) == b"".join(g1(BETA * x) for x in lagrange(TAU, 1 << p))
    with pytest.raises(ValueError, match="short"):
        f.level(13, 3)
    # level k of the Lagrange sections is what groth16_ref's setup evaluates: L_j(tau) of the domain 2^k
    assert bytes(f.level(12, 2)) == b"".join(g1(x) for x in g._lagrange_at(TAU, 4))
    assert bytes(f.point(4, 0, 64)) == g1(ALPHA) and bytes(f.point(6, 0, 128)) == g2(BETA)


def test_reader_refuses_other_files(p2, tmp_path):
    with pytest.raises(ValueError, match="not a ptau"):
        P.PtauFile(b"zkey" + p2[4:])
    with pytest.raises(ValueError, match="n8"):
        P.PtauFile(ptau_bytes(1, n8=48, q=QM))
    with pytest.raises(ValueError, match="curve not supported"):
        P.PtauFile(ptau_bytes(1, q=RM))
    with pytest.raises(ValueError, match="truncated"):
        P.PtauFile(p2[:-10])
    path = tmp_path / "p.ptau"
    path.write_bytes(p2)
    f = P.PtauFile(str(path))                      # a path is mapped, not read
    assert f.power == 2 and bytes(f.level(14, 1)) == p2_level(p2, 14, 1)
    f.close()


def p2_level(data, sid, p):
    return bytes(P.PtauFile(data).level(sid, p))


@pytest.mark.parametrize("args,msg", [
    (dict(drop=(12,)), "not prepared for phase 2"),
    (dict(drop=(12, 13, 14, 15)), "not prepared for phase 2"),
    (dict(short=(12, 64)), "section 12 is short"),
    (dict(short=(13, 1)), "section 13 is short"),
    (dict(short=(15, 64)), "section 15 is short"),
])
def test_setup_sizes_refuses_bad_ptau(tmp_path, args, msg):
    with pytest.raises(ZkHipError, match=msg):
        P.setup_sizes(circuit(1), ptau_bytes(2, **args))


def test_setup_sizes_of_a_circuit(p2):
    assert P.setup_sizes(circuit(1), p2) == {"nVars": 4, "nPublic": 1, "domainSize": 4, "log_domain": 2, "nCoefs": 4}
    assert P.setup_sizes(circuit(2), p2)["domainSize"] == 4          # 2 + 1 + 1 rows
    with pytest.raises(ZkHipError, match=r"needs 2\^3 and the ptau file holds 2\^2"):
        P.setup_sizes(circuit(3), p2)
    with pytest.raises(ZkHipError, match="fewer than the constant wire"):
        P.setup_sizes(R.write_r1cs_rows([{0: 1}], [{0: 1}], [{0: 1}], 2, 3), p2)


def test_setup_sizes_refuses_more_than_2p27(p2):
    """a header claiming 2^27 constraints: refused from the sizes alone, before the constraints are walked"""
    from rapidsnark_old_amd import lib as L
    import ctypes as C
    f = P.PtauFile(p2)
    pv = f.view()
    pv.power = 28
    rv = L.zk_r1cs_view(4, 1, 0, 2, 1 << 27, None, 0)
    s = L.zk_setup_sizes()
    assert L.load_library().zk_groth16_setup_sizes(C.byref(rv), C.byref(pv), C.byref(s)) != 0
    assert "more than 2^27" in L.load_library().zk_last_error().decode()


def run_zkeynew(*args):
    return subprocess.run([ZKEYNEW, *args], capture_output=True, text=True, timeout=120)


def test_zkeynew_arguments_and_file_errors(p2, tmp_path):
    rp, pp, zp, vp = (str(tmp_path / x) for x in ("c.r1cs", "p.ptau", "c.zkey", "vk.json"))
    with open(rp, "wb") as f:
        f.write(circuit(3))
    res = run_zkeynew(rp, pp)
    assert res.returncode == 255 and "Usage: zkeynew" in res.stderr
    res = run_zkeynew(rp, pp, zp)
    assert res.returncode == 255 and res.stderr.strip()                      # no such ptau
    cases = [(ptau_bytes(2), "needs 2^3 and the ptau file holds 2^2"),
             (ptau_bytes(3, drop=(13,)), "not prepared for phase 2"),
             (ptau_bytes(3, short=(14, 64)), "section 14 is short"),
             (ptau_bytes(2, q=RM), "ptau curve not supported"),
             (b"zkey" + ptau_bytes(2)[4:], "Invalid file type"),
             (ptau_bytes(2, alpha1=g1(ALPHA)[:32] + (5).to_bytes(32, "little") + bytes(64 * 3)), "alphaTauG1[0] is not a point")]
    for data, msg in cases:
        with open(pp, "wb") as f:
            f.write(data)
        res = run_zkeynew(rp, pp, zp, vp)
        assert res.returncode == 255 and msg in res.stderr, (msg, res.stderr)
        assert not os.path.exists(zp) and not os.path.exists(vp)
        assert not [x for x in os.listdir(str(tmp_path)) if x.endswith(".partial")]
    with open(rp, "wb") as f:
        f.write(b"r1cs" + struct.pack("<II", 1, 0))
    res = run_zkeynew(rp, pp, zp)
    assert res.returncode == 255 and not os.path.exists(zp)


# ---------------------------------------------------------------- zkeynew: the exact exit code, stdout and stderr
def exact_case(name, d, ptau):
    """-> argv of one refusal; the files are written into d, which is the program's directory"""
    r1cs = circuit(1)
    head = 12 + 12                                    # section 1 leads the file: n8, the prime, the counts
    if name == "r1cs_other_prime":
        r1cs = r1cs[:head + 4] + QM.to_bytes(32, "little") + r1cs[head + 36:]
    elif name == "r1cs_n8_48":
        r1cs = r1cs[:head] + struct.pack("<I", 48) + r1cs[head + 4:]
    elif name == "r1cs_custom_gates":
        r1cs = r1cs[:8] + struct.pack("<I", 4) + r1cs[12:] + struct.pack("<IQ", 5, 4) + bytes(4)
    elif name == "r1cs_is_a_ptau":
        r1cs = ptau
    elif name == "ptau_version_2":
        ptau = ptau[:4] + struct.pack("<I", 2) + ptau[8:]
    elif name == "ptau_cut_in_the_table":
        ptau = ptau[:30]
    for fname, data in (("c.r1cs", r1cs), ("p.ptau", ptau)):
        if name != "ptau_missing" or fname != "p.ptau":
            with open(os.path.join(d, fname), "wb") as f:
                f.write(data)
    return () if name == "usage" else ("c.r1cs", "p.ptau", "c.zkey", "vk.json")


EXACT = {      # what the programs of the commit before the host helpers were shared printed: (exit code, stdout, stderr)
    "usage": (255, "", "Invalid number of parameters:\nUsage: zkeynew <circuit.r1cs> <pot.ptau> <circuit.zkey> [verification_key.json]\n"),
    "r1cs_other_prime": (255, "", "r1cs curve not supported\n"),
    "r1cs_n8_48": (255, "", "r1cs: only 256-bit fields are supported\n"),
    "r1cs_custom_gates": (255, "", "r1cs custom gates are not supported: Groth16 cannot use them\n"),
    "r1cs_is_a_ptau": (255, "", "Invalid file type. It should be r1cs and it us ptau\n"),
    "ptau_version_2": (255, "", "Invalid version. It should be <=1 and it us 2\n"),
    "ptau_cut_in_the_table": (255, "", "Unexpected end of file\n"),
    "ptau_missing": (255, "", "open: No such file or directory\n"),
}


@pytest.mark.parametrize("name", sorted(EXACT))
def test_zkeynew_exact_refusals_before_the_device(name, tmp_path, p2):
    argv = exact_case(name, str(tmp_path), p2)
    res = subprocess.run([ZKEYNEW, *argv], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert (res.returncode, res.stdout, res.stderr) == EXACT[name]
    assert not [x for x in os.listdir(str(tmp_path)) if x not in ("c.r1cs", "p.ptau")]
