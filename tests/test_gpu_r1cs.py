"""The R1CS witness check on the GPU (zk_r1cs_*, rapidsnark_old_amd.R1cs, `wtnscheck`, `prover` with ZKHIP_R1CS).  Every
expected result is computed here in Python from the rows (oracle.groth16_ref.R1CS style: {wire: value} or [(wire, value)])."""
import os
import random
import subprocess
import threading

import numpy as np
import pytest

from conftest import CIRCUITS, ROOT, golden_bytes, golden_json, golden_path

from oracle import groth16_ref as g
from rapidsnark_old_amd import r1cs as R

pytestmark = pytest.mark.gpu
RM = g.R_MOD
BIN = os.path.join(ROOT, "rapidsnark-old_amd")
SEG = 16                                                   # csrc/r1cs.hip: terms per lane


def items(row):
    return list(row.items()) if isinstance(row, dict) else list(row)


def dot(row, w):
    return sum(v * w[s] for s, v in items(row)) % RM


def expect(A, B, C, w):
    """(failed, first, (a, b, c) of first) from the rows"""
    bad = [i for i in range(len(A)) if (dot(A[i], w) * dot(B[i], w) - dot(C[i], w)) % RM]
    if not bad:
        return 0, None, None
    i = bad[0]
    return len(bad), i, (dot(A[i], w), dot(B[i], w), dot(C[i], w))


def values(w):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in w), dtype=np.uint8).copy()


def assert_report(rep, A, B, C, w):
    failed, first, abc = expect(A, B, C, w)
    assert (rep.failed, rep.first_failed) == (failed, first)
    if first is not None:
        assert (rep.a, rep.b, rep.c) == abc


def golden_circuits():
    """the five golden circuits' rows, regenerated from oracle/gen_golden.py's seeded calls"""
    out = {"multiplier2": (g.multiplier2_r1cs(), [1, 33, 3, 11])}
    rng = random.Random(7)
    for name, args in (("r1cs_n8", (5, 1)), ("r1cs_n64", (50, 3)), ("r1cs_nopub", (10, 0)), ("r1cs_n256", (200, 2))):
        out[name] = g.random_r1cs(rng, *args)
    return out


GOLD = golden_circuits()


def r1cs_bytes(c, **kw):
    return R.write_r1cs_rows(c.A, c.B, c.C, c.nVars, c.nPublic, **kw)


@pytest.mark.parametrize("name", CIRCUITS)
def test_golden_circuits_pass_and_match_their_keys(zk, name):
    c, w = GOLD[name]
    assert g.read_wtns(golden_bytes(name, "witness.wtns"))["witness"] == w
    ck = zk.R1cs(r1cs_bytes(c), device=0)
    rep = ck.check(golden_path(name, "witness.wtns"))
    assert rep.ok and rep.failed == 0 and rep.first_failed is None and rep.one_ok and rep.first_unreduced is None
    assert ck.match_zkey(golden_path(name, "circuit.zkey")) == (0, None)
    ck.close()


def test_multiplier2_wrong_output(zk):
    c, _ = GOLD["multiplier2"]
    ck = zk.R1cs(r1cs_bytes(c))
    rep = ck.check(values([1, 34, 3, 11]))
    assert not rep.ok and (rep.failed, rep.first_failed, rep.a, rep.b, rep.c) == (1, 0, 3, 11, 34)
    assert rep.one_ok and rep.first_unreduced is None


@pytest.mark.parametrize("logm", [10, 13, 16])
def test_perturbed_witnesses(zk, logm):
    rng = random.Random(1000 + logm)
    c, w = g.random_r1cs(rng, 1 << logm, 2)
    ck = zk.R1cs(r1cs_bytes(c))
    assert ck.check(values(w)).ok
    for k in (1, 2, 50):
        w2 = list(w)
        for i in rng.sample(range(1, len(w)), k):
            w2[i] = (w2[i] + rng.randrange(1, RM)) % RM
        rep = ck.check(values(w2))
        assert_report(rep, c.A, c.B, c.C, w2)
        assert rep.failed >= 1


LENGTHS = [0, 1, 7, 8, 9, SEG - 1, SEG, SEG + 1, 2 * SEG + 1, 254, 4096, 100000]


def long_row(n):
    return [(1 + (k % 5), RM - 1) for k in range(n)]      # coefficients r - 1, duplicate wire ids


@pytest.mark.parametrize("where", ["A", "B", "C"])
def test_long_and_skewed_rows_exact(zk, where):
    n_wires = 6
    w = [1] + [RM - 1] * (n_wires - 1)                     # witness values r - 1
    rows_sat, cases = ([], [], []), []
    for n in LENGTHS:
        v = dot(long_row(n), w)
        if where == "A":
            row = (long_row(n), [(0, 1)], [(0, v)])
        elif where == "B":
            row = ([(0, 1)], long_row(n), [(0, v)])
        else:
            row = ([(0, 1)], [(0, v)], long_row(n))
        cases.append(row)
        for k in range(3):
            rows_sat[k].append(row[k])
    # a linear constraint: empty A (a = 0), C sums to zero over duplicate wires
    rows_sat[0].append([])
    rows_sat[1].append([(1, 5)])
    rows_sat[2].append([(1, 1), (1, RM - 1)])
    ck = zk.R1cs(R.write_r1cs_rows(*rows_sat, n_wires, 1))
    rep = ck.check(values(w))
    assert rep.ok, rep
    ck.close()
    for n, row in zip(LENGTHS, cases):                     # unsatisfied: the constant side off by one
        A, B, C = [list(x) for x in row]
        if where == "C":
            B = [(0, (B[0][1] + 1) % RM)]
        else:
            C = [(0, (C[0][1] + 1) % RM)]
        ck = zk.R1cs(R.write_r1cs_rows([A, []], [B, [(2, 3)]], [C, [(3, 0)]], n_wires, 1))
        rep = ck.check(values(w))
        assert_report(rep, [A, []], [B, [(2, 3)]], [C, [(3, 0)]], w)
        assert rep.failed == 1 and rep.first_failed == 0, (n, rep)
        ck.close()


def test_edge_cases(zk):
    empty = R.write_r1cs_rows([], [], [], 3, 1)
    ck = zk.R1cs(empty)
    assert ck.check(values([1, 5, 6])).ok
    rep = ck.check(values([2, 5, 6]))
    assert not rep.ok and not rep.one_ok and rep.failed == 0
    rep = ck.check(values([1, 5, RM + 3]))
    assert not rep.ok and rep.first_unreduced == 2
    with pytest.raises(zk.ZkHipError, match="4 values"):
        ck.check(values([1, 5, 6, 7]))
    ck.close()
    c, w = GOLD["r1cs_n8"]
    A = [items(r) for r in c.A]
    A[3] = A[3] + [(c.nVars, 1)]
    with pytest.raises(zk.ZkHipError, match="constraint 3: wire id"):
        zk.R1cs(R.write_r1cs_rows(A, c.B, c.C, c.nVars, c.nPublic))
    B = [items(r) for r in c.B]
    B[2] = [(0, RM)]
    with pytest.raises(zk.ZkHipError, match="constraint 2: coefficient"):
        zk.R1cs(R.write_r1cs_rows(c.A, B, c.C, c.nVars, c.nPublic))
    with pytest.raises(ValueError, match="curve not supported"):
        zk.R1cs(R.write_r1cs_rows(c.A, c.B, c.C, c.nVars, c.nPublic, prime=RM + 2))
    ck = zk.R1cs(r1cs_bytes(c))
    with pytest.raises(zk.ZkHipError, match="values"):
        ck.check(golden_path("multiplier2", "witness.wtns"))
    # an unreduced witness value is still summed exactly: w + r gives the same constraint values as w
    w2 = list(w)
    w2[4] += RM
    rep = ck.check(values(w2))
    assert rep.first_unreduced == 4 and rep.failed == 0


def zkey_with_coef_changed(data, k):
    secs, pos = {}, 12
    for _ in range(int.from_bytes(data[8:12], "little")):
        sid, size = int.from_bytes(data[pos:pos + 4], "little"), int.from_bytes(data[pos + 4:pos + 12], "little")
        secs[sid] = pos + 12
        pos += 12 + size
    b = bytearray(data)
    at = secs[4] + 4 + 44 * k
    row = int.from_bytes(b[at + 4:at + 8], "little")
    b[at + 12] ^= 1
    return bytes(b), row


def test_match_zkey(zk):
    c, w = GOLD["r1cs_n64"]
    zkey = golden_bytes("r1cs_n64", "circuit.zkey")
    ck = zk.R1cs(r1cs_bytes(c))
    bad, row = zkey_with_coef_changed(zkey, 17)
    assert ck.match_zkey(bad) == (1, row)
    # A and B swapped in one row
    A, B = list(c.A), list(c.B)
    A[5], B[5] = c.B[5], c.A[5]
    assert zk.R1cs(R.write_r1cs_rows(A, B, c.C, c.nVars, c.nPublic)).match_zkey(zkey) == (1, 5)
    # an extra constraint
    m = len(c.A)
    n, first = zk.R1cs(R.write_r1cs_rows(c.A + [{0: 1}], c.B + [{0: 1}], c.C + [{0: 1}], c.nVars, c.nPublic)).match_zkey(zkey)
    assert n >= 1 and first == m
    # another nPublic
    with pytest.raises(zk.ZkHipError, match="nPublic"):
        zk.R1cs(R.write_r1cs_rows(c.A, c.B, c.C, c.nVars, c.nPublic + 1)).match_zkey(zkey)
    # A and C negated: the witness still holds, the key is another circuit's
    neg = lambda rows: [{s: (-v) % RM for s, v in r.items()} for r in rows]
    ckn = zk.R1cs(R.write_r1cs_rows(neg(c.A), c.B, neg(c.C), c.nVars, c.nPublic))
    assert ckn.check(values(w)).ok
    n, first = ckn.match_zkey(zkey)
    assert first == 0 and n == m


def test_check_dev_and_threads(zk):
    import torch
    c, w = g.random_r1cs(random.Random(5), 3000, 2)
    w2 = list(w)
    w2[100] = (w2[100] + 1) % RM
    ck = zk.R1cs(r1cs_bytes(c), device=0)
    host = ck.check(values(w2))
    assert_report(host, c.A, c.B, c.C, w2)
    d = torch.from_numpy(values(w2)).to("cuda:0")
    torch.cuda.synchronize()
    assert ck.check_dev(d.data_ptr(), len(w2)) == host
    other = zk.R1cs(r1cs_bytes(c), device=0)
    res, errs = [], []

    def work(obj, wt, n):
        try:
            for _ in range(n):
                res.append(obj.check(values(wt)))
        except Exception as e:      # noqa: BLE001
            errs.append(e)

    ths = [threading.Thread(target=work, args=(ck, w2, 8)), threading.Thread(target=work, args=(ck, w2, 8)),
           threading.Thread(target=work, args=(other, w2, 8))]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs and len(res) == 24 and all(r == host for r in res)


def test_large_zkgen_circuit(zk, tmp_path):
    from rapidsnark_old_amd import zkgen, synth
    key = zkgen.generate(18, 2, 0, circuit_like=True)
    zkgen.write_all(key, str(tmp_path))
    zkgen.write_r1cs(key, str(tmp_path / "circuit.r1cs"))
    ck = zk.R1cs(str(tmp_path / "circuit.r1cs"))
    assert ck.check(str(tmp_path / "witness.wtns")).ok
    assert ck.match_zkey(str(tmp_path / "circuit.zkey")) == (0, None)
    # one internal signal changed: the failing set from the key's own records
    m, n_in = key["nConstraints"], key["nInputs"]
    w = np.ascontiguousarray(key["witness"]).reshape(-1, 32).copy()
    wi = [int.from_bytes(bytes(r), "little") for r in w]
    s = 1 + n_in + 12345
    wi[s] = (wi[s] + 7) % RM
    w[s] = np.frombuffer(wi[s].to_bytes(32, "little"), dtype=np.uint8)
    rec = np.frombuffer(np.ascontiguousarray(key["coefs"]).tobytes()[4:], dtype=synth.COEF_DTYPE)
    rows = sorted(set(int(x) for x in rec["c"][(rec["s"] == s) & (rec["c"] < m)]) | {s - 1 - n_in})
    r2inv = pow(1 << 512, -1, RM)
    def row_val(mat, i):
        sel = rec[(rec["m"] == mat) & (rec["c"] == i)]
        return sum(int.from_bytes(bytes(t["v"]), "little") * r2inv * wi[int(t["s"])] for t in sel) % RM
    fails = [i for i in rows if (row_val(0, i) * row_val(1, i) - wi[1 + n_in + i]) % RM]
    rep = ck.check(w.reshape(-1))
    assert (rep.failed, rep.first_failed) == (len(fails), fails[0] if fails else None)


def run_bin(name, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([os.path.join(BIN, name), *args], capture_output=True, text=True, errors="replace", env=e, timeout=300)


def test_cli(tmp_path):
    c, _ = GOLD["multiplier2"]
    p = tmp_path / "m.r1cs"
    p.write_bytes(r1cs_bytes(c))
    r = run_bin("wtnscheck", str(p), golden_path("multiplier2", "witness.wtns"))
    assert r.returncode == 0, r.stderr
    bad = tmp_path / "bad.wtns"
    bad.write_bytes(g.write_wtns([1, 34, 3, 11]))
    r = run_bin("wtnscheck", str(p), str(bad))
    assert r.returncode == 1
    assert "constraint 0 fails: A.w = 3, B.w = 11, C.w = 34" in r.stdout and "1 of 1 constraints fail" in r.stdout
    # prover with the guard: the same proof.json; an invalid witness or another circuit: exit 255, no files
    name = "r1cs_n64"
    cn, _ = GOLD[name]
    pn = tmp_path / "n64.r1cs"
    pn.write_bytes(r1cs_bytes(cn))
    meta = golden_json(name, "meta.json")
    le = lambda x: int(x).to_bytes(32, "little").hex()
    env = {"ZKHIP_FIXED_R": le(meta["r"]), "ZKHIP_FIXED_S": le(meta["s"])}
    out = lambda tag: (str(tmp_path / ("p%s.json" % tag)), str(tmp_path / ("q%s.json" % tag)))
    r = run_bin("prover", golden_path(name, "circuit.zkey"), golden_path(name, "witness.wtns"), *out("0"), env=env)
    assert r.returncode == 0, r.stderr
    r = run_bin("prover", golden_path(name, "circuit.zkey"), golden_path(name, "witness.wtns"), *out("1"), env=dict(env, ZKHIP_R1CS=str(pn)))
    assert r.returncode == 0, r.stderr
    assert open(out("1")[0], "rb").read() == open(out("0")[0], "rb").read() == golden_bytes(name, "proof.json")
    wt = g.read_wtns(golden_bytes(name, "witness.wtns"))["witness"]
    wt[10] = (wt[10] + 1) % RM
    badw = tmp_path / "bad64.wtns"
    badw.write_bytes(g.write_wtns(wt))
    r = run_bin("prover", golden_path(name, "circuit.zkey"), str(badw), *out("2"), env=dict(env, ZKHIP_R1CS=str(pn)))
    assert r.returncode == 255 and "constraint" in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert not any(os.path.exists(f) for f in out("2"))
    r = run_bin("prover", golden_path("r1cs_n256", "circuit.zkey"), golden_path("r1cs_n256", "witness.wtns"), *out("3"),
                env=dict(env, ZKHIP_R1CS=str(pn)))
    assert r.returncode == 255 and "r1cs does not match the zkey" in r.stderr, r.stderr
    assert not any(os.path.exists(f) for f in out("3"))
