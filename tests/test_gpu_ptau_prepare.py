"""Phase-2 preparation of a .ptau on the GPU (zk_g1_lagrange / zk_g2_lagrange, zk_ptau_prepare, ptau.prepare_phase2,
`ptauprepare`): the inverse DFT over points against a big-integer one written here, whole files against files made on the
CPU and against write_trapdoor_ptau's own Lagrange sections (an inverse NTT in Fr, then fixed-base multiplications: another
route to the same bytes), and through `zkeynew` and a proof.  Every comparison is byte for byte: the affine form of a point
is unique."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from oracle import bn254 as bn, groth16_ref as g, pairing
from rapidsnark_old_amd import ptau as P, r1cs as R

pytestmark = pytest.mark.gpu
RM, QM = bn.R_MOD, bn.Q_MOD
BIN = os.path.join(ROOT, "rapidsnark-old_amd")
TAU, ALPHA, BETA = 1234567, 89101112, 13141516
TOXIC3 = (0x1234567 * 0x89ABCDEF + 17, 0xA1FA << 200 | 99, 0xBE7A << 180 | 7)
LAG = (12, 13, 14, 15)
GROUPS = {"g1": (bn.G1, bn.g1_to_bytes, 64), "g2": (bn.G2, bn.g2_to_bytes, 128)}


# ---------------------------------------------------------------- the operators against the big-integer oracle
def idft_points(E, pts):
    """radix-2 decimation-in-frequency inverse DFT over curve points: out_j = (1/n) sum_k w^(-jk) P_k, natural order"""
    n = len(pts)
    p = n.bit_length() - 1
    x = list(pts)
    winv = pow(bn.fr_root(p), -1, RM) if p else 1
    half = n // 2
    while half >= 1:
        step = n // (2 * half)
        for lo0 in range(0, n, 2 * half):
            for j in range(half):
                a, b = x[lo0 + j], x[lo0 + j + half]
                x[lo0 + j] = E.add(a, b)
                x[lo0 + j + half] = E.mul(E.sub(a, b), pow(winv, j * step, RM))
        half //= 2
    ninv = pow(n, -1, RM)
    rev = lambda i: int(format(i, "0%db" % p)[::-1], 2) if p else 0
    return [E.mul(x[rev(j)], ninv) for j in range(n)]


def run_op(zk, group, pts, log_n):
    E, to_bytes, nb = GROUPS[group]
    fn = zk.g1_lagrange if group == "g1" else zk.g2_lagrange
    got = fn(b"".join(to_bytes(q) for q in pts), log_n)
    n = 1 << log_n
    padded = (list(pts) + [None] * n)[:n]
    want = b"".join(to_bytes(q) for q in idft_points(E, padded))
    assert got.size == n * nb
    assert got.tobytes() == want
    return padded


@pytest.mark.parametrize("group", ["g1", "g2"])
@pytest.mark.parametrize("log_n", range(7))
def test_operator_on_arbitrary_points(zk, group, log_n):
    E = GROUPS[group][0]
    rng = random.Random(1000 * log_n + len(group))
    run_op(zk, group, [E.mul(E.gen, rng.randrange(1, RM)) for _ in range(1 << log_n)], log_n)


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_operator_special_inputs(zk, group):
    E = GROUPS[group][0]
    rng = random.Random(group)
    rnd = lambda: E.mul(E.gen, rng.randrange(1, RM))
    Pt = rnd()
    run_op(zk, group, [rnd() for _ in range(5)], 3)                        # n_points < 2^log_n: the rest is infinity
    run_op(zk, group, [rnd() for _ in range(11)], 3)                       # n_points > 2^log_n: the rest is not read
    run_op(zk, group, [], 2)                                               # nothing but infinity
    run_op(zk, group, [None, rnd(), None, None, rnd(), None, rnd(), rnd()], 3)      # inputs at infinity
    run_op(zk, group, [Pt] * 8, 3)                                         # a = b in every butterfly of the first stage
    run_op(zk, group, [Pt, E.neg(Pt)] * 4, 3)                              # P beside -P: a = -b in the last stages
    run_op(zk, group, [Pt, Pt, E.neg(Pt), E.neg(Pt), rnd(), None, Pt, E.dbl(Pt)], 3)
    run_op(zk, group, [Pt] * 16, 4)


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_operator_names_a_point_off_the_curve(zk, group):
    E, to_bytes, nb = GROUPS[group]
    pts = bytearray(b"".join(to_bytes(E.mul(E.gen, k + 2)) for k in range(8)))
    pts[5 * nb + 3] ^= 1
    pts[6 * nb + 40] ^= 1
    fn = zk.g1_lagrange if group == "g1" else zk.g2_lagrange
    with pytest.raises(zk.ZkHipError, match="point 5 is not on the curve"):
        fn(bytes(pts), 3)
    bad = bytearray(b"".join(to_bytes(E.mul(E.gen, k + 2)) for k in range(2)))
    bad[nb:nb + 32] = (QM + 1).to_bytes(32, "little")                       # a coordinate that is not below q
    with pytest.raises(zk.ZkHipError, match="point 1 is not on the curve"):
        fn(bytes(bad), 1)


# ---------------------------------------------------------------- tiny whole files made on the CPU
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


def ptau_bytes(power, drop=()):
    """a prepared .ptau of `power` from (TAU, ALPHA, BETA), as tests/test_ptau_host.py's; drop: section ids left out"""
    n = 1 << power
    levels = lambda top, zt: [lagrange(TAU, 1 << p, zero_top=(zt and p == top)) for p in range(top + 1)]
    l12 = [x for lvl in levels(power + 1, True) for x in lvl]
    l13 = [x for lvl in levels(power, False) for x in lvl]
    secs = {
        1: struct.pack("<I", 32) + QM.to_bytes(32, "little") + struct.pack("<II", power, power),
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
    out = [b"ptau", struct.pack("<II", 1, len(secs) - len(drop))]
    for sid, payload in secs.items():
        if sid not in drop:
            out += [struct.pack("<IQ", sid, len(payload)), payload]
    return b"".join(out)


def sections(path_or_bytes):
    f = P.PtauFile(path_or_bytes)
    out = {sid: bytes(f.section(sid)) for sid in f.sections}
    order = [sid for _, sid in sorted((pos, sid) for sid, (pos, _) in f.sections.items())]
    f.close()
    return out, order


def without_lagrange(src, dst):
    """the file at src with sections 12 to 15 left out (and a section the preparation must not copy)"""
    secs, order = sections(src)
    keep = [sid for sid in order if sid not in LAG]
    with open(dst, "wb") as f:
        f.write(b"ptau" + struct.pack("<II", 1, len(keep)))
        for sid in keep:
            f.write(struct.pack("<IQ", sid, len(secs[sid])) + secs[sid])


@pytest.mark.parametrize("power", [1, 2, 3])
def test_tiny_files_equal_the_cpu_made_sections(zk, tmp_path, power):
    want, _ = sections(ptau_bytes(power))
    src = ptau_bytes(power, drop=LAG)
    dst = str(tmp_path / "out.ptau")
    zk.prepare_phase2(src, dst)
    got, order = sections(dst)
    assert order == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    for sid in range(1, 8):
        assert got[sid] == want[sid], sid
    for sid in LAG:
        assert got[sid] == want[sid], sid
    assert sorted(os.listdir(str(tmp_path))) == ["out.ptau"]
    assert P.PtauFile(dst).prepared


def test_sections_are_copied_in_the_input_order_and_others_dropped(zk, tmp_path):
    secs, _ = sections(ptau_bytes(1))
    order = [1, 7, 6, 99, 5, 4, 3, 2]
    secs[99] = b"not copied"
    data = b"ptau" + struct.pack("<II", 1, len(order)) + b"".join(struct.pack("<IQ", s, len(secs[s])) + secs[s] for s in order)
    dst = str(tmp_path / "out.ptau")
    zk.prepare_phase2(data, dst)
    got, got_order = sections(dst)
    assert got_order == [1, 7, 6, 5, 4, 3, 2, 12, 13, 14, 15]
    assert all(got[s] == secs[s] for s in got_order)


# ---------------------------------------------------------------- trapdoor files: degenerate tau, sizes
def count_infinity(data, nb):
    a = np.frombuffer(data, dtype=np.uint8).reshape(-1, nb)
    return int((a.max(axis=1) == 0).sum())


def prepare_and_compare(zk, tmp_path, power, toxic, runs=1):
    full, bare, out = (str(tmp_path / x) for x in ("full.ptau", "bare.ptau", "out.ptau"))
    zk.write_trapdoor_ptau(power, *toxic, full)
    zk.write_trapdoor_ptau(power, *toxic, bare, prepared=False)
    want, _ = sections(full)
    src, src_order = sections(bare)
    assert src_order == [1, 2, 3, 4, 5, 6, 7] and all(src[s] == want[s] for s in src_order)
    first = None
    for _ in range(runs):
        zk.prepare_phase2(bare, out)
        got, order = sections(out)
        assert order == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
        for sid in order:
            assert got[sid] == want[sid], sid
        with open(out, "rb") as f:
            data = f.read()
        assert first is None or data == first
        first = data
        os.remove(out)
    return want


@pytest.mark.parametrize("tau", ["one", "root8"])
def test_degenerate_tau_reaches_doubling_and_cancellation(zk, tmp_path, tau):
    """tau = 1: every power is the same point (a = b in every butterfly: doublings, and differences at infinity); tau an
    8th root of unity: the powers repeat with period 8 and P meets -P.  Most Lagrange points are then infinity."""
    t = 1 if tau == "one" else bn.fr_root(3)
    want = prepare_and_compare(zk, tmp_path, 5, (t, TOXIC3[1], TOXIC3[2]))
    assert count_infinity(want[12], 64) >= 22
    assert count_infinity(want[13], 128) >= 10 and count_infinity(want[14], 64) >= 10 and count_infinity(want[15], 64) >= 10


@pytest.mark.parametrize("power", [1, 2, 9, 12, 16])
def test_sizes_equal_the_trapdoor_route_and_repeat(zk, tmp_path, power):
    prepare_and_compare(zk, tmp_path, power, TOXIC3, runs=2)


# ---------------------------------------------------------------- the chain through the binaries
def test_cli_chain_ptauprepare_zkeynew_prover(zk, tmp_path):
    c, w = g.random_r1cs(random.Random(7), 5, 1)                           # oracle/gen_golden.py's r1cs_n8
    rp = str(tmp_path / "c.r1cs")
    with open(rp, "wb") as f:
        f.write(R.write_r1cs_rows(c.A, c.B, c.C, c.nVars, c.nPublic))
    full, bare, out = (str(tmp_path / x) for x in ("full.ptau", "bare.ptau", "out.ptau"))
    zk.write_trapdoor_ptau(9, *TOXIC3, full)
    zk.write_trapdoor_ptau(9, *TOXIC3, bare, prepared=False)
    res = subprocess.run([os.path.join(BIN, "zkeynew"), rp, bare, str(tmp_path / "no.zkey")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 255 and "not prepared for phase 2" in res.stderr
    res = subprocess.run([os.path.join(BIN, "ptauprepare"), bare, out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    assert not os.path.exists(out + ".partial")
    keys = []
    for pp, name in ((out, "a.zkey"), (full, "b.zkey")):
        zp = str(tmp_path / name)
        res = subprocess.run([os.path.join(BIN, "zkeynew"), rp, pp, zp], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr
        with open(zp, "rb") as f:
            keys.append(f.read())
    assert keys[0] == keys[1]
    ozk, trap = g.setup(c, (*TOXIC3, 1, 1))
    r, s = 0xC0FFEE, (1 << 200) + 12345
    p = zk.Prover(str(tmp_path / "a.zkey"), device=0)
    proof = p.prove(g.write_wtns(w), r=r, s=s)
    p.close()
    pts = (bn.g1_from_bytes(proof[:64]), bn.g2_from_bytes(proof[64:192]), bn.g1_from_bytes(proof[192:]))
    vk = {"alpha1": ozk.alpha1, "beta2": ozk.beta2, "gamma2": ozk.gamma2, "delta2": ozk.delta2, "IC": ozk.IC}
    assert pairing.groth16_verify(vk, w[1:c.nPublic + 1], pts)
    assert g.trapdoor_check(trap, c.nPublic, w, r, s, pts)


# ---------------------------------------------------------------- errors on the device path
def test_a_point_off_the_curve_names_its_section_and_index(zk, tmp_path):
    bare, bad, out = (str(tmp_path / x) for x in ("bare.ptau", "bad.ptau", "out.ptau"))
    zk.write_trapdoor_ptau(4, *TOXIC3, bare, prepared=False)
    f = P.PtauFile(bare)
    pos, _ = f.sections[3]
    f.close()
    with open(bare, "rb") as fh:
        data = bytearray(fh.read())
    data[pos + 11 * 128 + 70] ^= 4                                         # one coordinate of point 11 of section 3
    with open(bad, "wb") as fh:
        fh.write(data)
    res = subprocess.run([os.path.join(BIN, "ptauprepare"), bad, out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 255 and "section 3: point 11 is not on the curve" in res.stderr, res.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["bad.ptau", "bare.ptau"]
    with pytest.raises(zk.ZkHipError, match="section 3: point 11 is not on the curve"):
        zk.prepare_phase2(bad, out)
    assert sorted(os.listdir(str(tmp_path))) == ["bad.ptau", "bare.ptau"]
