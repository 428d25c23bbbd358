"""The `plonkprover <circuit.r1cs> <pot.ptau> <witness.wtns> <proof.json> <public.json>` executable: a proof from the three
files that plonk_verify accepts under the key of the same compile, the public signals, and the exit codes (0, 1 for a witness
the prover refuses, 255 for errors; nothing is written unless the proof was made)."""
import json
import os
import subprocess

import pytest

import plonk_r1cs_instance as pr
from conftest import ROOT
from oracle import bn254 as bn
from oracle.groth16_ref import write_wtns

PROG = os.path.join(ROOT, "rapidsnark-old_amd", "plonkprover")
TAU, ALPHA, BETA = 0x1F3A9C5E77D1B2A49E0C6F5D3B8A17264C9E0F1D2B3A4958, 0x2B7E151628AED2A6ABF7158809CF4F3C, 0x3243F6A8885A308D313198A2E0370734
POINTS = ("A", "B", "C", "Z", "T1", "T2", "T3", "Wxi", "Wxiw")
EVALS = ("eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw")


def run(*args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([PROG, *args], capture_output=True, text=True, errors="replace", env=e, timeout=300)


def test_usage_and_missing_files(tmp_path):
    r = run()
    assert r.returncode == 255
    assert r.stderr == "Invalid number of parameters:\nUsage: plonkprover <circuit.r1cs> <pot.ptau> <witness.wtns> <proof.json> <public.json>\n"
    out = (str(tmp_path / "proof.json"), str(tmp_path / "public.json"))
    r = run("/nonexistent.r1cs", "/nonexistent.ptau", "/nonexistent.wtns", *out)
    assert r.returncode == 255 and r.stderr.startswith("open") and not os.listdir(tmp_path)


def proof_bytes(text):
    """proof.json -> the 768 bytes of a PlonkProof"""
    d = json.loads(text)
    assert list(d) == list(POINTS + EVALS) + ["protocol", "curve"] and d["protocol"] == "plonk" and d["curve"] == "bn128"
    out = b""
    for name in POINTS:
        x, y, z = (int(v) for v in d[name])
        assert z == 1, name
        out += (x * bn.MONT_R % bn.Q_MOD).to_bytes(32, "little") + (y * bn.MONT_R % bn.Q_MOD).to_bytes(32, "little")
    return out + b"".join(int(d[name]).to_bytes(32, "little") for name in EVALS)


@pytest.fixture(scope="module")
def files(zk, tmp_path_factory):
    d = tmp_path_factory.mktemp("plonk_cli")
    c = pr.case("proof_6")
    paths = {k: str(d / k) for k in ("c.r1cs", "p8.ptau", "w.wtns", "bad.wtns", "other.wtns")}
    open(paths["c.r1cs"], "wb").write(c.data)
    open(paths["w.wtns"], "wb").write(c.wtns)
    bad = list(c.witness)
    bad[-1] = (bad[-1] + 1) % bn.R_MOD
    open(paths["bad.wtns"], "wb").write(write_wtns(bad))
    open(paths["other.wtns"], "wb").write(write_wtns(c.witness[:-1]))
    zk.write_trapdoor_ptau(8, TAU, ALPHA, BETA, paths["p8.ptau"], prepared=False)
    return c, paths


@pytest.mark.gpu
def test_the_proof_verifies_and_the_publics_are_the_witnesss(zk, files, tmp_path):
    c, paths = files
    pj, qj = tmp_path / "proof.json", tmp_path / "public.json"
    r = run(paths["c.r1cs"], paths["p8.ptau"], paths["w.wtns"], str(pj), str(qj), env={"ZKHIP_SELFVERIFY": "1"})
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["proof.json", "public.json"]
    text = pj.read_text()
    raw = proof_bytes(text)
    assert zk.PlonkProof(raw).to_json() == text
    assert json.loads(qj.read_text()) == [str(v) for v in c.publics]
    assert qj.read_text() == zk.public_to_json(b"".join(v.to_bytes(32, "little") for v in c.witness), c.n_public)
    with zk.Kzg.from_ptau(paths["p8.ptau"], max_coeffs=64 + 6) as kzg, zk.PlonkProver.from_r1cs(kzg, paths["c.r1cs"]) as p:
        vk = p.vkey()
        assert zk.plonk_verify(vk, raw, c.publics) == 0
        assert zk.plonk_verify(vk, raw, [c.publics[1], c.publics[0]]) == 1


@pytest.mark.gpu
def test_a_bad_witness_exits_1_and_writes_no_file(files, tmp_path):
    c, paths = files
    out = (str(tmp_path / "proof.json"), str(tmp_path / "public.json"))
    r = run(paths["c.r1cs"], paths["p8.ptau"], paths["bad.wtns"], *out)
    assert r.returncode == 1 and r.stdout.startswith("INVALID: zk_plonk_prove_r1cs: the ") and not os.listdir(tmp_path)
    r = run(paths["c.r1cs"], paths["p8.ptau"], paths["other.wtns"], *out)      # another circuit's witness: refused before the device
    assert r.returncode == 255 and "witness does not match the r1cs" in r.stderr and not os.listdir(tmp_path)
    r = run(paths["c.r1cs"], paths["p8.ptau"], "/nonexistent.wtns", *out)
    assert r.returncode == 255 and r.stderr.startswith("open") and not os.listdir(tmp_path)
    r = run(paths["w.wtns"], paths["p8.ptau"], paths["w.wtns"], *out)
    assert r.returncode == 255 and "Invalid file type" in r.stderr and not os.listdir(tmp_path)
