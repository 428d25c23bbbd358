"""The phase-2 contribution on the GPU: the one-scalar operator zk_g1_scale against two independent routes (the fixed-base
kernel on the discrete logs, the Python oracle) and against its own plain double-and-add, then zk_zkey_contribute /
zkey_contribute / `zkeycontribute` on keys whose trapdoor is known, through proofs and the pairing check."""
import importlib.util
import json
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import valid_key as vk
from oracle import bn254 as bn, groth16_ref as g, pairing
from rapidsnark_old_amd import r1cs as R, synth
from test_zkey_contribute_host import LAMBDA, edge_scalars, sections_of, binfile

pytestmark = pytest.mark.gpu
RM, QM = bn.R_MOD, bn.Q_MOD
BIN = os.path.join(ROOT, "rapidsnark-old_amd")
G1, G2 = synth.g1_gen_bytes(), synth.g2_gen_bytes()
_spec = importlib.util.spec_from_file_location("refcheck_verify", os.path.join(ROOT, "tools", "refcheck", "verify.py"))
verify = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(verify)


def logs_for(n, k, rng):
    """n discrete logs a_i: infinity at the first, a middle and the last place, 1, r - 1 and +-1/k (a_i k = +-1) among them"""
    a = [rng.randrange(1, RM) for _ in range(n)]
    special = [1, RM - 1] + ([pow(k, -1, RM), -pow(k, -1, RM) % RM] if k else [])
    for i, v in zip(range(1, n - 1), special):
        a[i] = v
    for i in {0, n // 2, n - 1} if n > 2 else ():
        a[i] = 0
    return a


def scaled(zk, a, k):
    """(k P_i as zk_g1_scale gives them, as the fixed-base kernel gives them from the logs) for P_i = a_i G"""
    pts = zk.fixed_base_g1(G1, a) if a else np.zeros(0, np.uint8)
    want = zk.fixed_base_g1(G1, [x * k % RM for x in a]) if a else np.zeros(0, np.uint8)
    return zk.g1_scale(pts, k), want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_operator_against_the_fixed_base_kernel(zk, n):
    rng = random.Random(500 + n)
    k = rng.randrange(1, RM)
    got, want = scaled(zk, logs_for(n, k, rng), k)
    assert got.shape == (64 * n,) and np.array_equal(got, want)


def test_operator_at_every_edge_scalar(zk, monkeypatch):
    """n = 65 (two waves, the second one lane wide): every scalar at which the split, the recoding or an addition meets a
    special case (k = 0: all infinity; small k, +-lambda, +-lambda +- 1: the accumulator meets +- the point it adds)"""
    rng = random.Random(65)
    for k in edge_scalars() + [LAMBDA - 2, 2 * LAMBDA % RM, (RM - LAMBDA - 1) % RM, 5, 7]:
        got, want = scaled(zk, logs_for(65, k, rng), k)
        assert np.array_equal(got, want), k
        if k == 0:
            assert not got.any()
    monkeypatch.setenv("ZKHIP_SCALE_PLAIN", "1")                 # the second route: the plain 254-bit double-and-add
    for k in (0, 1, RM - 1, LAMBDA, rng.randrange(RM)):
        got, want = scaled(zk, logs_for(65, k, rng), k)
        assert np.array_equal(got, want), k


def test_operator_against_the_python_oracle(zk):
    rng = random.Random(8)
    a = [rng.randrange(1, RM) for _ in range(8)]
    a[3] = 0
    pts = zk.fixed_base_g1(G1, a)
    for k in (rng.randrange(RM), LAMBDA + 1, RM - 2):
        want = b"".join(bn.g1_to_bytes(bn.G1.mul(bn.G1.mul(bn.G1.gen, x), k)) if x else bytes(64) for x in a)
        assert zk.g1_scale(pts, k).tobytes() == want, k


def test_operator_errors(zk):
    rng = random.Random(9)
    n = 70
    pts = zk.fixed_base_g1(G1, [rng.randrange(1, RM) for _ in range(n)])
    for k in (RM, RM + 1, (1 << 256) - 1):
        with pytest.raises(zk.ZkHipError, match="not below r"):
            zk.g1_scale(pts, k)
    for at in (0, n - 1):
        off = pts.copy()
        off[64 * at + 32] ^= 1                                    # y changed: off the curve
        with pytest.raises(zk.ZkHipError, match=r"zk_g1_scale: point %d is not on the curve" % at):
            zk.g1_scale(off, 3)
        big = pts.copy()
        big[64 * at:64 * at + 32] = np.frombuffer(QM.to_bytes(32, "little"), np.uint8)          # x = q: not below q
        with pytest.raises(zk.ZkHipError, match=r"point %d is not on the curve" % at):
            zk.g1_scale(big, 3)
    both = pts.copy()
    both[64 * 5 + 32] ^= 1
    both[64 * 40 + 32] ^= 1
    with pytest.raises(zk.ZkHipError, match="point 5 is"):          # the lowest failing index
        zk.g1_scale(both, 3)


def test_chunks_on_both_buffer_sets_name_the_lowest_bad_point(zk, monkeypatch):
    """13 points in chunks of 4: four chunks, the last of one point, so both buffer sets are used again and then drained"""
    rng = random.Random(13)
    pts = zk.fixed_base_g1(G1, [rng.randrange(1, RM) for _ in range(13)])
    whole = zk.g1_scale(pts, 3)                                     # one chunk
    monkeypatch.setenv("ZKHIP_SCALE_CHUNK", "4")
    # chunks 1 and 2, one per buffer set and both in flight; the last chunk alone, seen only in the final drain; chunks 2
    # and 3, both seen in the final drain, which runs oldest first
    for flipped, named in (((6, 9), 6), ((12,), 12), ((9, 12), 9)):
        off = pts.copy()
        for at in flipped:
            off[64 * at + 32] ^= 1
        with pytest.raises(zk.ZkHipError, match=r"zk_g1_scale: point %d is not on the curve" % named):
            zk.g1_scale(off, 3)
    assert np.array_equal(zk.g1_scale(pts, 3), whole)


# ---------------------------------------------------------------- the contribution on a key whose trapdoor is known
@pytest.fixture(scope="module")
def trapdoor_key(zk, tmp_path_factory):
    """a valid key over a 2^6 domain with its toxic waste, its file and its witness"""
    d = tmp_path_factory.mktemp("contrib")
    wl, wit, trap, w = vk.build(zk, 6, seed=1066)
    path = str(d / "in.zkey")
    with open(path, "wb") as f:
        f.write(vk.zkey_bytes(wl))
    return {"wl": wl, "wit": wit, "trap": trap, "w": w, "path": path, "dir": d}


D1 = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F0E1 % RM


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_chunk_borders_do_not_show_in_the_file(zk, trapdoor_key, monkeypatch):
    """62 points of section 8 and 64 of section 9 in chunks of 1, 7, 64 and one chunk: the same bytes"""
    d = trapdoor_key["dir"]
    files = []
    for chunk in (1, 7, 64, 10 ** 6):
        monkeypatch.setenv("ZKHIP_SCALE_CHUNK", str(chunk))
        out = str(d / ("chunk%d.zkey" % chunk))
        zk.zkey_contribute(trapdoor_key["path"], out, d=D1)
        files.append(read(out))
    assert all(f == files[0] for f in files[1:])
    monkeypatch.setenv("ZKHIP_SCALE_PLAIN", "1")
    monkeypatch.setenv("ZKHIP_SCALE_CHUNK", "7")
    out = str(d / "plain.zkey")
    zk.zkey_contribute(trapdoor_key["path"], out, d=D1)
    assert read(out) == files[0]


def test_contribution_on_a_trapdoor_key(zk, trapdoor_key):
    t, wl, trap, w = trapdoor_key, trapdoor_key["wl"], trapdoor_key["trap"], trapdoor_key["w"]
    out, vkp = str(t["dir"] / "out.zkey"), str(t["dir"] / "vk.json")
    zk.zkey_contribute(t["path"], out, d=D1, vk_path=vkp)
    assert not os.path.exists(out + ".partial")
    old, new = dict(sections_of(read(t["path"]))), dict(sections_of(read(out)))
    assert [s for s, _ in sections_of(read(out))] == list(range(1, 11)) and read(out)[:8] == read(t["path"])[:8]
    dinv = pow(D1, -1, RM)
    delta = trap["toxic"][4]
    assert new[8] == zk.fixed_base_g1(G1, [x * dinv % RM for x in trap["C"]]).tobytes()
    assert new[9] == zk.fixed_base_g1(G1, [x * dinv % RM for x in trap["Hs"]]).tobytes()
    assert new[2][:-192] == old[2][:-192]
    assert new[2][-192:-128] == zk.g1_mul(G1, delta * D1 % RM)
    assert new[2][-128:] == zk.g2_mul(G2, delta * D1 % RM)
    for sid in (1, 3, 4, 5, 6, 7, 10):
        assert new[sid] == old[sid], sid
    # a proof from the new key: the discrete logs of the old key's with delta d in delta's place
    r, s = 0x0123456789ABCDEF0123, (1 << 247) - 12345
    p = zk.Prover(out, device=0)
    proof = p.prove(vk.wtns_bytes(wl, t["wit"]), r=r, s=s)
    p.close()
    trap2 = dict(trap, toxic=trap["toxic"][:4] + (delta * D1 % RM,))
    a, b, c = vk.expected_proof_dlogs(trap2, wl["nPublic"], w, r, s)
    assert proof[0:64] == zk.g1_mul(G1, a)
    assert proof[64:192] == zk.g2_mul(G2, b)
    assert proof[192:256] == zk.g1_mul(G1, c)
    pts = (bn.g1_from_bytes(proof[:64]), bn.g2_from_bytes(proof[64:192]), bn.g1_from_bytes(proof[192:]))
    pub = w[1:wl["nPublic"] + 1]
    new_vk = verify.load_vk(vkp)
    assert new_vk == verify.vk_from_zkey(out)
    assert pairing.groth16_verify(new_vk, pub, pts)
    assert not pairing.groth16_verify(verify.vk_from_zkey(t["path"]), pub, pts)


def test_two_contributions_compose(zk, trapdoor_key):
    d = trapdoor_key["dir"]
    d2 = (RM - 1) // 3 + 77
    one, two, both = str(d / "c1.zkey"), str(d / "c2.zkey"), str(d / "c12.zkey")
    zk.zkey_contribute(trapdoor_key["path"], one, d=D1)
    zk.zkey_contribute(one, two, d=d2)
    zk.zkey_contribute(trapdoor_key["path"], both, d=D1 * d2 % RM)
    assert read(two) == read(both)


def test_a_drawn_scalar_differs_from_run_to_run(zk, trapdoor_key):
    d = trapdoor_key["dir"]
    outs = [str(d / "r1.zkey"), str(d / "r2.zkey")]
    for o in outs:
        zk.zkey_contribute(trapdoor_key["path"], o)
    a, b, old = (dict(sections_of(read(p)))[2][-192:] for p in outs + [trapdoor_key["path"]])
    assert a != b and a != old and b != old


def test_empty_section_8(zk, tmp_path):
    """every signal public: section 8 has no point, section 9 has two"""
    r1cs = g.R1CS(3, 2, [{1: 1}], [{1: 1}], [{2: 1}])            # x1 * x1 = x2, both public
    rng = random.Random(7)
    toxic = tuple(rng.randrange(1, RM) for _ in range(5))
    ozk, trap = g.setup(r1cs, toxic)
    assert ozk.C == []
    ip, op = str(tmp_path / "allpub.zkey"), str(tmp_path / "out.zkey")
    with open(ip, "wb") as f:
        f.write(g.write_zkey(ozk))
    zk.zkey_contribute(ip, op, d=D1)
    new = dict(sections_of(read(op)))
    assert new[8] == b""
    assert new[9] == zk.fixed_base_g1(G1, [x * pow(D1, -1, RM) % RM for x in trap["Hs"]]).tobytes()
    w = [1, 5, 25]
    p = zk.Prover(op, device=0)
    proof = p.prove(g.write_wtns(w), r=11, s=13)
    p.close()
    pts = (bn.g1_from_bytes(proof[:64]), bn.g2_from_bytes(proof[64:192]), bn.g1_from_bytes(proof[192:]))
    assert pairing.groth16_verify(verify.vk_from_zkey(op), w[1:3], pts)


# ---------------------------------------------------------------- the programs, one after another
TOXIC3 = (0x1234567 * 0x89ABCDEF + 17, 0xA1FA << 200 | 99, 0xBE7A << 180 | 7)


@pytest.fixture(scope="module")
def zkeynew_key(zk, tmp_path_factory):
    """`zkeynew`'s key (gamma = delta = 1) of a random circuit with 50 constraints and 3 public signals, and its witness"""
    d = tmp_path_factory.mktemp("chain")
    c, w = g.random_r1cs(random.Random(77), 50, 3)
    ptau, rp, zp = str(d / "p7.ptau"), str(d / "c.r1cs"), str(d / "c0.zkey")
    zk.write_trapdoor_ptau(7, *TOXIC3, ptau)
    with open(rp, "wb") as f:
        f.write(R.write_r1cs_rows(c.A, c.B, c.C, c.nVars, c.nPublic))
    res = subprocess.run([os.path.join(BIN, "zkeynew"), rp, ptau, zp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    wt = str(d / "w.wtns")
    with open(wt, "wb") as f:
        f.write(g.write_wtns(w))
    return {"dir": d, "zkey": zp, "wtns": wt, "c": c, "w": w}


def contribute_cli(args, scalar=None, chunk=None):
    env = dict(os.environ)
    for name, v in (("ZKHIP_CONTRIB_SCALAR", scalar), ("ZKHIP_SCALE_CHUNK", chunk)):
        env.pop(name, None)
        if v is not None:
            env[name] = str(v)
    return subprocess.run([os.path.join(BIN, "zkeycontribute"), *args], capture_output=True, text=True, timeout=300, env=env)


def prove_cli(d, zkey, wtns, tag):
    out = [str(d / (tag + "_proof.json")), str(d / (tag + "_public.json"))]
    res = subprocess.run([os.path.join(BIN, "prover"), zkey, wtns, *out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    return out


def test_cli_chain_zkeynew_zkeycontribute_prover(zk, zkeynew_key):
    k, d = zkeynew_key, zkeynew_key["dir"]
    z1, v1 = str(d / "c1.zkey"), str(d / "vk1.json")
    res = contribute_cli([k["zkey"], z1, v1], scalar=D1, chunk=33)
    assert res.returncode == 0, res.stderr
    assert str(D1) not in res.stderr + res.stdout and "%x" % D1 not in res.stderr + res.stdout
    assert sorted(p for p in os.listdir(str(d)) if "partial" in p) == []
    py = str(d / "py1.zkey")
    zk.zkey_contribute(k["zkey"], py, d=D1, vk_path=str(d / "pyvk1.json"))
    assert read(z1) == read(py)                                  # the program and the binding write the same key
    assert json.load(open(v1)) == json.load(open(str(d / "pyvk1.json")))
    new2 = dict(sections_of(read(z1)))[2]
    assert new2[-192:-128] == zk.g1_mul(G1, D1) and new2[-128:] == zk.g2_mul(G2, D1)          # delta was 1
    proof, public = prove_cli(d, z1, k["wtns"], "one")
    assert verify.verify_files(proof, public, v1)
    assert json.load(open(public)) == [str(x) for x in k["w"][1:k["c"].nPublic + 1]]
    # a second party, whose scalar nobody fixes
    z2, v2 = str(d / "c2.zkey"), str(d / "vk2.json")
    res = contribute_cli([z1, z2, v2])
    assert res.returncode == 0, res.stderr
    assert dict(sections_of(read(z2)))[2][-192:-128] != new2[-192:-128]
    proof2, public2 = prove_cli(d, z2, k["wtns"], "two")
    assert verify.verify_files(proof2, public2, v2)
    assert not verify.verify_files(proof2, public2, v1)


def test_cli_names_the_section_and_index_of_a_bad_point(zk, zkeynew_key):
    d = zkeynew_key["dir"]
    secs = sections_of(read(zkeynew_key["zkey"]))
    h = bytearray(dict(secs)[9])
    h[64 * 37 + 33] ^= 4
    bad, out, vkp = str(d / "bad.zkey"), str(d / "bad_out.zkey"), str(d / "bad_vk.json")
    with open(bad, "wb") as f:
        f.write(binfile(b"zkey", 1, [(s, bytes(h) if s == 9 else p) for s, p in secs]))
    for chunk in (None, 16):
        res = contribute_cli([bad, out, vkp], scalar=D1, chunk=chunk)
        assert res.returncode == 255 and "zkey section 9: point 37 is not on the curve" in res.stderr, res.stderr
        assert not [p for p in os.listdir(str(d)) if p.startswith("bad_")]
    with pytest.raises(zk.ZkHipError, match="zkey section 9: point 37"):
        zk.zkey_contribute(bad, out, d=D1)
    assert not [p for p in os.listdir(str(d)) if p.startswith("bad_")]
