"""The executables `plonkvkey <circuit.r1cs> <pot.ptau> <verification_key.json>` and `plonkverifier <verification_key.json>
<public.json> <proof.json>`: with `plonkprover` they close the chain of files, r1cs + ptau + wtns -> key, proof, publics ->
verdict.  Exit codes 0 / 1 (INVALID, saying malformed or failing equation) / 255 with exact texts."""
import json
import os
import subprocess

import pytest

import plonk_r1cs_instance as pr
from conftest import ROOT
from oracle import bn254 as bn

BIN = os.path.join(ROOT, "rapidsnark-old_amd")
TAU, ALPHA, BETA = 0x1F3A9C5E77D1B2A49E0C6F5D3B8A17264C9E0F1D2B3A4958, 0x2B7E151628AED2A6ABF7158809CF4F3C, 0x3243F6A8885A308D313198A2E0370734
FIELDS = ["protocol", "curve", "nPublic", "power", "k1", "k2", "Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3", "X_2", "w"]
OK_TEXT = "OK: the proof verifies\n"
EQUATION = "INVALID: the proof is well-formed but the pairing equation does not hold\n"
MALFORMED = "INVALID: the proof is malformed (a point off the curve, a coordinate that is not below q, or a value or public signal that is not below r)\n"


def run(prog, *args):
    return subprocess.run([os.path.join(BIN, prog), *args], capture_output=True, text=True, errors="replace", timeout=300)


def test_usage_and_missing_files(tmp_path):
    r = run("plonkvkey")
    assert r.returncode == 255 and r.stderr == "Invalid number of parameters:\nUsage: plonkvkey <circuit.r1cs> <pot.ptau> <verification_key.json>\n"
    r = run("plonkverifier", "a", "b")
    assert r.returncode == 255 and r.stderr == "Invalid number of parameters:\nUsage: plonkverifier <verification_key.json> <public.json> <proof.json>\n"
    r = run("plonkvkey", "/nonexistent.r1cs", "/nonexistent.ptau", str(tmp_path / "vk.json"))
    assert r.returncode == 255 and r.stderr.startswith("open") and not os.listdir(tmp_path)
    r = run("plonkverifier", "/nonexistent.json", "/nonexistent.json", "/nonexistent.json")
    assert r.returncode == 255 and r.stderr == "/nonexistent.json: cannot be opened\n" and r.stdout == ""


@pytest.fixture(scope="module")
def files(zk, tmp_path_factory):
    """the three programs in a row, once: key, proof and publics of proof_6, and the key of another circuit with two publics"""
    d = tmp_path_factory.mktemp("plonk_verifier_cli")
    c, other = pr.case("proof_6"), pr.case("proof_4")
    assert c.n_public == other.n_public == 2
    p = {k: str(d / k) for k in ("c.r1cs", "other.r1cs", "p8.ptau", "w.wtns", "vk.json", "other_vk.json", "proof.json", "public.json")}
    open(p["c.r1cs"], "wb").write(c.data)
    open(p["other.r1cs"], "wb").write(other.data)
    open(p["w.wtns"], "wb").write(c.wtns)
    zk.write_trapdoor_ptau(8, TAU, ALPHA, BETA, p["p8.ptau"], prepared=False)
    runs = [run("plonkvkey", p["c.r1cs"], p["p8.ptau"], p["vk.json"]), run("plonkvkey", p["other.r1cs"], p["p8.ptau"], p["other_vk.json"]),
            run("plonkprover", p["c.r1cs"], p["p8.ptau"], p["w.wtns"], p["proof.json"], p["public.json"])]
    return c, p, runs, d


def changed(files, name, change):
    """a copy of one of the JSON files with change(d) applied"""
    c, p, runs, d = files
    j = json.load(open(p[name]))
    j = change(j) or j
    path = str(d / ("changed_" + name))
    json.dump(j, open(path, "w"))
    return path


@pytest.mark.gpu
def test_key_proof_and_verdict_from_the_files(zk, files):
    c, p, runs, d = files
    for r in runs:
        assert r.returncode == 0 and r.stderr == "", r.stderr
    text = open(p["vk.json"]).read()
    key = json.loads(text)
    assert list(key) == FIELDS and (key["protocol"], key["curve"], key["nPublic"], key["power"], key["k1"], key["k2"]) == ("plonk", "bn128", 2, 6, "2", "3")
    assert key["w"] == str(bn.fr_root(6)) and key["X_2"][2] == ["1", "0"]
    assert [int(v) for pair in key["X_2"][:2] for v in pair] == [v for pair in bn.G2.mul(bn.G2_GEN, TAU) for v in pair]
    r = run("plonkverifier", p["vk.json"], p["public.json"], p["proof.json"])
    assert (r.returncode, r.stdout, r.stderr) == (0, OK_TEXT, "")
    # the key is the one the library makes, and Python reads and writes the same file
    vk = zk.PlonkVKey.from_json(text)
    with zk.Kzg.from_ptau(p["p8.ptau"], max_coeffs=64 + 6) as kzg, zk.PlonkProver.from_r1cs(kzg, p["c.r1cs"]) as prover:
        assert bytes(prover.vkey()._c) == bytes(vk._c)
    assert json.loads(vk.to_json()) == key
    again = str(d / "python_vk.json")
    open(again, "w").write(vk.to_json())
    r = run("plonkverifier", again, p["public.json"], p["proof.json"])
    assert (r.returncode, r.stdout) == (0, OK_TEXT)


@pytest.mark.gpu
def test_invalid_proofs_exit_1_saying_why(files):
    c, p, runs, d = files
    bad = changed(files, "proof.json", lambda j: j.update(eval_a=str((int(j["eval_a"]) + 1) % bn.R_MOD)))
    r = run("plonkverifier", p["vk.json"], p["public.json"], bad)
    assert (r.returncode, r.stdout, r.stderr) == (1, EQUATION, "")
    pub = changed(files, "public.json", lambda j: [j[1], j[0]])
    r = run("plonkverifier", p["vk.json"], pub, p["proof.json"])
    assert (r.returncode, r.stdout) == (1, EQUATION)
    off = changed(files, "proof.json", lambda j: j.update(Z=["1", "3", "1"]))            # 9 != 1 + 3
    r = run("plonkverifier", p["vk.json"], p["public.json"], off)
    assert (r.returncode, r.stdout, r.stderr) == (1, MALFORMED, "")
    big = changed(files, "proof.json", lambda j: j.update(eval_zw=str(bn.R_MOD)))
    r = run("plonkverifier", p["vk.json"], p["public.json"], big)
    assert (r.returncode, r.stdout) == (1, MALFORMED)
    r = run("plonkverifier", p["other_vk.json"], p["public.json"], p["proof.json"])      # a key for another circuit
    assert (r.returncode, r.stdout) == (1, EQUATION)
    # infinity (0 1 0) is a point, and a third coordinate is honoured
    inf = changed(files, "proof.json", lambda j: j.update(Wxiw=["0", "1", "0"]))
    r = run("plonkverifier", p["vk.json"], p["public.json"], inf)
    assert (r.returncode, r.stdout) == (1, EQUATION)
    z = 5
    scaled = changed(files, "proof.json", lambda j: j.update(A=[str(int(j["A"][0]) * z % bn.Q_MOD), str(int(j["A"][1]) * z % bn.Q_MOD), str(z)]))
    r = run("plonkverifier", p["vk.json"], p["public.json"], scaled)
    assert (r.returncode, r.stdout) == (0, OK_TEXT)


@pytest.mark.gpu
def test_what_the_files_are_refused_for(files):
    c, p, runs, d = files
    short = changed(files, "public.json", lambda j: j[:1])
    r = run("plonkverifier", p["vk.json"], short, p["proof.json"])
    assert r.returncode == 255 and r.stdout == "" and r.stderr == "the verification key is for 2 public signals, %s holds 1\n" % short
    for change, text in ((lambda j: j.update(w=str(bn.fr_root(7))), "%s: w is not this library's root of unity for power 6\n"),
                         (lambda j: j.update(protocol="groth16"), "%s: protocol \"groth16\" is not plonk\n"),
                         (lambda j: j.update(curve="bls12381"), "%s: curve \"bls12381\" is not bn128\n"),
                         (lambda j: j.pop("S3") and None, "%s: no \"S3\"\n"),
                         (lambda j: j.update(power=29), "%s: power 29 is outside 0 .. 28\n")):
        key = changed(files, "vk.json", change)
        r = run("plonkverifier", key, p["public.json"], p["proof.json"])
        assert (r.returncode, r.stdout, r.stderr) == (255, "", text % key)
    r = run("plonkverifier", p["vk.json"], p["public.json"], p["vk.json"])               # a key where a proof is expected
    assert r.returncode == 255 and r.stderr == "%s: no \"A\"\n" % p["vk.json"]
    r = run("plonkverifier", p["vk.json"], p["public.json"], "/nonexistent.json")
    assert r.returncode == 255 and r.stderr == "/nonexistent.json: cannot be opened\n"
