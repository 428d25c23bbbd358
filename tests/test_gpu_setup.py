"""Groth16 setup on the GPU (zk_groth16_setup, rapidsnark_old_amd.groth16_setup, `zkeynew`): keys from a .r1cs and a
trapdoor .ptau against the Python oracle (oracle/groth16_ref.py), against zkgen's own keys, and through proofs."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from oracle import bn254 as bn, groth16_ref as g, pairing
from rapidsnark_old_amd import r1cs as R, synth, zkgen

pytestmark = pytest.mark.gpu
RM = g.R_MOD
BIN = os.path.join(ROOT, "rapidsnark-old_amd")
G1, G2 = synth.g1_gen_bytes(), synth.g2_gen_bytes()
TOXIC3 = (0x1234567 * 0x89ABCDEF + 17, 0xA1FA << 200 | 99, 0xBE7A << 180 | 7)        # tau, alpha, beta of the small ptaus


def items(row):
    return list(row.items()) if isinstance(row, dict) else list(row)


def merged(rows):
    out = []
    for row in rows:
        d = {}
        for s, v in items(row):
            d[s] = (d.get(s, 0) + v) % RM
        out.append({s: v for s, v in d.items() if v})
    return out


def golden_circuits():
    """multiplier2 and the random circuits of oracle/gen_golden.py (same seeded calls), with their witnesses"""
    out = {"multiplier2": (g.multiplier2_r1cs(), [1, 33, 3, 11])}
    rng = random.Random(7)
    for name, args in (("r1cs_n8", (5, 1)), ("r1cs_n64", (50, 3)), ("r1cs_nopub", (10, 0)), ("r1cs_n256", (200, 2))):
        out[name] = g.random_r1cs(rng, *args)
    return out


GOLD = golden_circuits()


@pytest.fixture(scope="module")
def small_ptau(zk, tmp_path_factory):
    """power 9 (> k of every golden circuit) and power 8 (= k of r1cs_n256), both from TOXIC3"""
    d = tmp_path_factory.mktemp("ptau")
    paths = {}
    for power in (9, 8):
        paths[power] = str(d / ("p%d.ptau" % power))
        zk.write_trapdoor_ptau(power, *TOXIC3, paths[power])
    return paths


def r1cs_file(tmp_path, c, name="c.r1cs"):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(R.write_r1cs_rows(c.A, c.B, c.C, c.nVars, c.nPublic))
    return p


def write_key(key, path):
    zkgen.write_zkey(key, path)
    with open(path, "rb") as f:
        return f.read()


def oracle_vk(ozk):
    return {"alpha1": ozk.alpha1, "beta2": ozk.beta2, "gamma2": ozk.gamma2, "delta2": ozk.delta2, "IC": ozk.IC}


def prove_and_verify(zk, zkey_path, ozk, trap, c, w, r=0xC0FFEE, s=(1 << 200) + 12345):
    p = zk.Prover(zkey_path, device=0)
    proof = p.prove(g.write_wtns(w), r=r, s=s)
    p.close()
    pts = (bn.g1_from_bytes(proof[:64]), bn.g2_from_bytes(proof[64:192]), bn.g1_from_bytes(proof[192:]))
    assert pairing.groth16_verify(oracle_vk(ozk), w[1:c.nPublic + 1], pts)
    assert g.trapdoor_check(trap, c.nPublic, w, r, s, pts)
    return proof


@pytest.mark.parametrize("name", sorted(GOLD))
def test_golden_circuits_equal_the_oracle_and_prove(zk, small_ptau, tmp_path, name):
    c, w = GOLD[name]
    rp = r1cs_file(tmp_path, c)
    key = zk.groth16_setup(rp, small_ptau[9], device=0)
    got = g.read_zkey(write_key(key, str(tmp_path / "k.zkey")))
    ozk, trap = g.setup(c, (*TOXIC3, 1, 1))
    assert (got.nVars, got.nPublic, got.domainSize) == (ozk.nVars, ozk.nPublic, ozk.domainSize)
    for name_ in ("alpha1", "beta1", "beta2", "gamma2", "delta1", "delta2", "IC", "A", "B1", "B2", "C", "H"):
        assert getattr(got, name_) == getattr(ozk, name_), name_
    assert sorted(got.coefs) == sorted(ozk.coefs)
    prove_and_verify(zk, str(tmp_path / "k.zkey"), ozk, trap, c, w)
    ck = zk.R1cs(rp, device=0)
    assert ck.match_zkey(str(tmp_path / "k.zkey")) == (0, None)
    ck.close()


def test_power_equal_to_k_truncates_only_h(zk, small_ptau, tmp_path):
    c, w = GOLD["r1cs_n256"]                                     # 200 + 2 + 1 rows: k = 8
    key = zk.groth16_setup(r1cs_file(tmp_path, c), small_ptau[8], device=0)
    ozk, trap = g.setup(c, (*TOXIC3, 1, 1))
    got = g.read_zkey(write_key(key, str(tmp_path / "k.zkey")))
    for name_ in ("IC", "A", "B1", "B2", "C"):
        assert getattr(got, name_) == getattr(ozk, name_), name_
    pf = zk.PtauFile(small_ptau[8])
    top = np.asarray(pf.level(12, 9)).reshape(-1, 64)
    assert np.array_equal(np.asarray(key["pointsH"]).reshape(-1, 64), top[1::2])
    pf.close()
    assert got.H != ozk.H
    prove_and_verify(zk, str(tmp_path / "k.zkey"), ozk, trap, c, w)


def test_cli_chain_zkeynew_prover_and_verification_key(zk, small_ptau, tmp_path):
    c, w = GOLD["r1cs_n64"]
    rp = r1cs_file(tmp_path, c)
    zp, vkp = str(tmp_path / "c.zkey"), str(tmp_path / "vk.json")
    res = subprocess.run([os.path.join(BIN, "zkeynew"), rp, small_ptau[9], zp, vkp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    key = zk.groth16_setup(rp, small_ptau[9], device=0)
    with open(zp, "rb") as f:
        assert f.read() == write_key(key, str(tmp_path / "py.zkey"))
    with open(vkp) as f:
        assert json.load(f) == zkgen.verification_key(key)
    wt = tmp_path / "w.wtns"
    wt.write_bytes(g.write_wtns(w))
    out = [str(tmp_path / "proof.json"), str(tmp_path / "public.json")]
    res = subprocess.run([os.path.join(BIN, "prover"), zp, str(wt), *out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    pj = json.load(open(out[0]))
    pts = (tuple(int(x) for x in pj["pi_a"][:2]), tuple(tuple(int(x) for x in pj["pi_b"][i]) for i in range(2)), tuple(int(x) for x in pj["pi_c"][:2]))
    ozk, trap = g.setup(c, (*TOXIC3, 1, 1))
    assert pairing.groth16_verify(oracle_vk(ozk), w[1:c.nPublic + 1], pts)
    assert json.load(open(out[1])) == [str(x) for x in w[1:c.nPublic + 1]]


# ---------------------------------------------------------------- zkgen's circuits at 2^16 and 2^18
def fixed_points(zk, trap, n_pub, n):
    """A, B1, B2, IC, C, H of a zkgen key with gamma = delta = 1, by fixed-base multiplications of its trapdoor values"""
    K = np.asarray(trap["K"]).reshape(-1, 32)
    lag2 = np.frombuffer(zk.fr_ntt(zkgen._powers(trap["toxic"][0], 2 * n), inverse=True), dtype=np.uint8).reshape(-1, 32)   # L^(2n)(tau)
    rows = lambda a: np.ascontiguousarray(a).reshape(-1)
    return {"pointsA": zk.fixed_base_g1(G1, trap["At"]), "pointsB1": zk.fixed_base_g1(G1, trap["Bt"]), "pointsB2": zk.fixed_base_g2(G2, trap["Bt"]),
            "pointsIC": zk.fixed_base_g1(G1, rows(K[:n_pub + 1])), "pointsC": zk.fixed_base_g1(G1, rows(K[n_pub + 1:])),
            "pointsH": zk.fixed_base_g1(G1, rows(lag2[1::2]))}


@pytest.fixture(scope="module")
def zkgen_ptau(zk, tmp_path_factory):
    """one trapdoor ptau of power k + 1 per k: zkgen.generate draws (tau, alpha, beta) from (k, seed) alone, so the plain
    and the circuit_like key of one k share them"""
    d = tmp_path_factory.mktemp("zkgen_ptau")
    cache = {}

    def get(k, toxic):
        if k not in cache:
            cache[k] = (str(d / ("p%d.ptau" % (k + 1))), toxic[:3])
            zk.write_trapdoor_ptau(k + 1, *toxic[:3], cache[k][0])
        assert cache[k][1] == toxic[:3]
        return cache[k][0]
    return get


@pytest.mark.parametrize("k,circuit_like", [(16, False), (16, True), (18, False), (18, True)])
def test_zkgen_circuits_equal_their_trapdoor_tables(zk, zkgen_ptau, tmp_path, k, circuit_like):
    key = zkgen.generate(k, 2, seed=3, circuit_like=circuit_like)
    rp = str(tmp_path / "c.r1cs")
    zkgen.write_r1cs(key, rp)
    toxic = key["trap"]["toxic"]
    got = zk.groth16_setup(rp, zkgen_ptau(k, toxic), device=0)
    assert (got["nVars"], got["nPublic"], got["domainSize"]) == (key["nVars"], 2, 1 << k)
    want = fixed_points(zk, key["trap"], 2, 1 << k)
    for name in ("pointsA", "pointsB1", "pointsB2", "pointsIC", "pointsC", "pointsH"):
        assert np.array_equal(np.asarray(got[name]), want[name]), name
    if circuit_like:                                             # nVars != n and rows at infinity in A / B
        assert got["nVars"] != got["domainSize"]
        assert (np.asarray(got["pointsA"]).reshape(-1, 64).max(axis=1) == 0).any()
    # the same coefficient records as the key (a multiset; zkgen drops none that the .r1cs holds)
    dt = synth.COEF_DTYPE
    a = np.frombuffer(np.asarray(got["coefs"]).tobytes()[4:], dtype=dt)
    b = np.frombuffer(np.asarray(key["coefs"]).tobytes()[4:], dtype=dt)
    srt = lambda r: np.sort(np.frombuffer(r.tobytes(), dtype="V44"))
    assert a.size == got["nCoefs"] and np.array_equal(srt(a), srt(b))


# ---------------------------------------------------------------- shapes that break naive kernels
def shaped_circuit(kind, rng):
    """-> (A, B, C rows as lists with repeats allowed, nWires, nPublic)"""
    full = lambda: rng.randrange(RM // 2, RM)
    if kind == "long_column":
        m, nw, npub = 100000, 300, 2
        A = [[(0, 1 if i % 3 else RM - 1)] for i in range(m)]           # the constant wire: a column of 10^5 terms
        B = [[] for _ in range(m)]
        C = [[(100 + i % 150, 1)] for i in range(m)]
        for i in range(1000):
            A[i].append((5, full()))                                   # full-size and r - 1 coefficients
            B[i].append((6, RM - 1))
        base = 2000
        for j, L in enumerate((15, 16, 17, 31, 32, 33)):                # the segment-cut lengths in one column each
            for t in range(L):
                B[base + t].append((10 + j, rng.randrange(1, RM)))
                A[base + t].append((30 + j, 1 << (t * 7 % 250)))
            base += L
        A[7] += [(20, 5), (20, 5)]                                       # the same (constraint, wire) twice
        B[9] += [(21, 3), (21, RM - 3)]                                  # terms that cancel: B_21 = infinity
        # wires 250 .. 299 are in no matrix
        return A, B, C, nw, npub
    if kind == "no_public":
        m, nw = 40, 60
        A = [[(1 + i % 30, rng.randrange(RM)), (0, 1)] for i in range(m)]
        B = [[(2 + i % 20, RM - 1), (2 + i % 20, RM - 1)] for i in range(m)]
        C = [[(31 + i % 20, full())] for i in range(m)]
        A[3] += [(45, 7), (45, RM - 7)]
        return A, B, C, nw, 0
    if kind == "all_public":
        m, nw = 20, 9
        A = [[(i % 9, rng.randrange(RM))] for i in range(m)]
        B = [[((i + 4) % 9, 2)] for i in range(m)]
        C = [[((i + 1) % 9, RM - 1)] for i in range(m)]
        return A, B, C, nw, 8
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["long_column", "no_public", "all_public"])
def test_shapes_against_setup_scalars(zk, tmp_path, kind):
    A, B, C, nw, npub = shaped_circuit(kind, random.Random(kind))
    rp = str(tmp_path / "c.r1cs")
    with open(rp, "wb") as f:
        f.write(R.write_r1cs_rows(A, B, C, nw, npub))
    circ = g.R1CS(nw, npub, merged(A), merged(B), merged(C))
    trap = g.setup_scalars(circ, (*TOXIC3, 1, 1))
    n = trap["n"]
    pp = str(tmp_path / "p.ptau")
    zk.write_trapdoor_ptau(n.bit_length(), *TOXIC3, pp)              # power k + 1
    got = zk.groth16_setup(rp, pp, device=0)
    assert (got["nVars"], got["nPublic"], got["domainSize"]) == (nw, npub, n)
    want = {"pointsA": zk.fixed_base_g1(G1, trap["At"]), "pointsB1": zk.fixed_base_g1(G1, trap["Bt"]),
            "pointsB2": zk.fixed_base_g2(G2, trap["Bt"]), "pointsIC": zk.fixed_base_g1(G1, trap["K"][:npub + 1])}
    if nw > npub + 1:
        want["pointsC"] = zk.fixed_base_g1(G1, trap["K"][npub + 1:])
    else:
        assert got["pointsC"].size == 0
    for name, v in want.items():
        assert np.array_equal(np.asarray(got[name]), v), name
    if kind == "long_column":
        assert not np.asarray(got["pointsB1"]).reshape(-1, 64)[21].any() and not np.asarray(got["pointsB2"]).reshape(-1, 128)[21].any()
        assert not np.asarray(got["pointsA"]).reshape(-1, 64)[250:].any()
    pn = sum(len(r) for r in A) + npub + 1 + sum(len(r) for r in B)
    assert got["nCoefs"] == pn


def test_base_tables_of_infinity_points(zk, tmp_path):
    """tau = 1: L_j(1) = 0 for every j > 0 of every level, so all the base points but index 0 are the all-zero infinity
    encoding and every term outside constraint 0 (the public-input rows included) multiplies infinity, at every bit
    length.  What is left is row 0: table entry s is (its coefficient of wire s) times G, alpha G or beta G.
    (oracle.groth16_ref.setup_scalars cannot serve: its _lagrange_at inverts tau - w^j, which is zero here.)"""
    rng = random.Random("infinity bases")
    _, alpha, beta = TOXIC3
    m, nw, npub = 6, 10, 2
    full = lambda: rng.randrange(RM // 2, RM)
    A = [[(0, 1), (3, RM - 1), (5, full())]] + [[(rng.randrange(nw), c)] for c in (1, RM - 1, full(), 2, 1 << 100)]
    B = [[(1, RM - 1), (4, full()), (7, 1)]] + [[(rng.randrange(nw), c)] for c in (full(), 1, RM - 1, 3, RM - 2)]
    C = [[(2, full()), (5, 1), (9, RM - 1)]] + [[(rng.randrange(nw), c)] for c in (RM - 1, full(), 1, 5, 1 << 200)]
    assert (len(A), len(B), len(C)) == (m, m, m)
    rp, pp = str(tmp_path / "c.r1cs"), str(tmp_path / "p.ptau")
    with open(rp, "wb") as f:
        f.write(R.write_r1cs_rows(A, B, C, nw, npub))
    zk.write_trapdoor_ptau(5, 1, alpha, beta, pp)                     # domain 16: power k + 1
    pf = zk.PtauFile(pp)
    lvl = np.asarray(pf.level(12, 4)).reshape(-1, 64).copy()
    pf.close()
    assert lvl[0].any() and not lvl[1:].any()
    got = zk.groth16_setup(rp, pp, device=0)
    assert (got["nVars"], got["nPublic"], got["domainSize"]) == (nw, npub, 16)
    row0 = lambda M: [dict(M[0]).get(s, 0) for s in range(nw)]
    a0, b0, c0 = row0(A), row0(B), row0(C)
    K = [(beta * a + alpha * b + c) % RM for a, b, c in zip(a0, b0, c0)]
    want = {"pointsA": zk.fixed_base_g1(G1, a0), "pointsB1": zk.fixed_base_g1(G1, b0), "pointsB2": zk.fixed_base_g2(G2, b0),
            "pointsIC": zk.fixed_base_g1(G1, K[:npub + 1]), "pointsC": zk.fixed_base_g1(G1, K[npub + 1:]),
            "pointsH": np.zeros(16 * 64, dtype=np.uint8)}
    for name, v in want.items():
        assert np.array_equal(np.asarray(got[name]).reshape(-1), v), name
    assert np.asarray(got["pointsA"]).reshape(-1, 64)[[0, 3, 5]].any(axis=1).all()      # row 0 is there: not everything vanished


# ---------------------------------------------------------------- errors
def test_errors_through_the_abi_and_the_cli(zk, small_ptau, tmp_path):
    c, _ = GOLD["r1cs_n8"]
    for rows, msg in (((c.A[:-1] + [{c.nVars + 3: 1}], c.B, c.C), "wire id >= nWires"),
                      ((c.A, c.B[:-1] + [{1: RM}], c.C), "coefficient >= r")):
        rp = str(tmp_path / "bad.r1cs")
        with open(rp, "wb") as f:
            f.write(R.write_r1cs_rows(*rows, c.nVars, c.nPublic))
        with pytest.raises(zk.ZkHipError, match=msg):
            zk.groth16_setup(rp, small_ptau[9], device=0)
        zp = str(tmp_path / "bad.zkey")
        res = subprocess.run([os.path.join(BIN, "zkeynew"), rp, small_ptau[9], zp, str(tmp_path / "vk.json")], capture_output=True, text=True,
                             timeout=300)
        assert res.returncode == 255 and msg in res.stderr
        assert not os.path.exists(zp) and not os.path.exists(str(tmp_path / "vk.json"))
