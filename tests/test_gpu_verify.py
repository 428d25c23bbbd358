"""Groth16 verification on the GPU (zk_vkey_*, VerificationKey, `verifier`): every golden proof verifies through both key
forms, one thing changed gives the verdict the Python oracle gives, a batch across chunk and wave borders keeps every
verdict at its position, a fresh proof verifies, and the command's exit codes."""
import importlib.util
import json
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import CIRCUITS, ROOT, golden_bytes, golden_json, golden_path

from oracle import bn254 as bn, pairing as opair
from rapidsnark_old_amd import verify as V
from test_gpu_pairing import twist_point_outside_the_subgroup
from test_verify_host import vk_json_of

pytestmark = pytest.mark.gpu
RM, QM = bn.R_MOD, bn.Q_MOD
OK, INVALID, MALFORMED = 0, 1, 2
VERIFIER = os.path.join(ROOT, "rapidsnark-old_amd", "verifier")
_spec = importlib.util.spec_from_file_location("refcheck_verify", os.path.join(ROOT, "tools", "refcheck", "verify.py"))
refverify = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(refverify)


def inputs(name):
    return V.load_proof(golden_path(name, "proof.json")), V.load_public(golden_path(name, "public.json"))


def oracle_says(vk, proof, public):
    """oracle.pairing.groth16_verify on the library's byte layouts"""
    pts = (bn.g1_from_bytes(proof[:64]), bn.g2_from_bytes(proof[64:192]), bn.g1_from_bytes(proof[192:]))
    return opair.groth16_verify(vk, [int.from_bytes(public[i:i + 32], "little") for i in range(0, len(public), 32)], pts)


@pytest.mark.parametrize("name", CIRCUITS)
def test_goldens_verify_through_both_key_forms(zk, name, tmp_path):
    proof, public = inputs(name)
    with zk.VerificationKey.from_zkey(golden_path(name, "circuit.zkey")) as vk:
        assert vk.n_public == len(public) // 32
        assert vk.verify(proof, public).tolist() == [OK]
    p = tmp_path / "verification_key.json"
    p.write_text(json.dumps(vk_json_of(name)))
    with zk.VerificationKey.from_json(str(p)) as vk:
        assert vk.verify(proof, public).tolist() == [OK]
    assert zk.groth16_verify(str(p), golden_path(name, "public.json"), golden_path(name, "proof.json")) is True


def test_verdict_codes_with_one_thing_changed(zk):
    name = "r1cs_n64"
    proof, public = inputs(name)
    A, B, C = proof[:64], proof[64:192], proof[192:]
    ovk = refverify.vk_from_zkey(golden_path(name, "circuit.zkey"))
    a, b = bn.g1_from_bytes(A), bn.g2_from_bytes(B)

    def leaves(curve, make):
        """the first offset d >= 1 at which make(d) is not on the curve (asserted with the oracle)"""
        for d in range(1, 50):
            if not curve.is_on_curve(make(d)):
                return make(d)
        raise AssertionError("no offset leaves the curve")

    a_off = leaves(bn.G1, lambda d: ((a[0] + d) % QM, a[1]))
    b_off = leaves(bn.G2, lambda d: (((b[0][0] + d) % QM, b[0][1]), b[1]))
    c = bn.g1_from_bytes(C)
    pub_plus = ((int.from_bytes(public[:32], "little") + 1) % RM).to_bytes(32, "little") + public[32:]
    cases = [
        ("unchanged", proof, public, OK),
        ("A <- 2A", zk.g1_mul(A, 2) + B + C, public, INVALID),
        ("a public signal + 1", proof, pub_plus, INVALID),
        ("C <- -C", A + B + bn.g1_to_bytes((c[0], (-c[1]) % QM)), public, INVALID),
        ("A.x + d leaves the curve", bn.g1_to_bytes(a_off) + B + C, public, MALFORMED),
        ("B.x.re + d leaves the twist", A + bn.g2_to_bytes(b_off) + C, public, MALFORMED),
        ("B outside the subgroup", A + bn.g2_to_bytes(twist_point_outside_the_subgroup()) + C, public, MALFORMED),
        ("A = infinity", bytes(64) + B + C, public, MALFORMED),
        ("B = infinity", A + bytes(128) + C, public, MALFORMED),
        ("C = infinity", A + B + bytes(64), public, MALFORMED),
        ("a coordinate = q", QM.to_bytes(32, "little") + A[32:] + B + C, public, MALFORMED),
        ("a public signal = r", proof, public[:32] + RM.to_bytes(32, "little") + public[64:], MALFORMED),
    ]
    with zk.VerificationKey.from_zkey(golden_path(name, "circuit.zkey")) as vk:
        got = vk.verify(b"".join(c[1] for c in cases), b"".join(c[2] for c in cases)).tolist()
        single = [int(vk.verify(c[1], c[2])[0]) for c in cases[:4]]
    for (what, pr, pub, want), verdict in zip(cases, got):
        assert verdict == want, (what, verdict)
    assert single == [c[3] for c in cases[:4]]
    for what, pr, pub, want in cases[1:]:
        assert oracle_says(ovk, pr, pub) is False, what  # verdicts 1 and 2 are the oracle's False
    assert oracle_says(ovk, proof, public) is True


def rerandomised(zk, proof, t):
    """A' = t A, B' = t^-1 B, C' = C: another valid proof of the same statement, without proving"""
    return zk.g1_mul(proof[:64], t) + zk.g2_mul(proof[64:192], pow(t, -1, RM)) + proof[192:]


def test_batch_keeps_every_verdict_at_its_position(zk, monkeypatch):
    name, n = "multiplier2", 130                        # two full waves and two lanes
    proof, public = inputs(name)
    rng = random.Random(130)
    proofs = [rerandomised(zk, proof, rng.randrange(2, RM)) for _ in range(n)]
    assert len(set(proofs)) == n
    publics = [public] * n
    want = [OK] * n
    for i in sorted({0, 63, 64, 129} | set(rng.sample(range(n), 9))):
        kind = rng.randrange(4) if i not in (0, 129) else (0 if i == 0 else 2)
        if kind == 0:                                   # B not rescaled: well-formed, the equation fails
            proofs[i] = proofs[i][:64] + proof[64:192] + proofs[i][192:]
            want[i] = INVALID
        elif kind == 1:
            publics[i] = (5).to_bytes(32, "little")
            want[i] = INVALID
        elif kind == 2:
            proofs[i] = bytes(64) + proofs[i][64:]
            want[i] = MALFORMED
        else:
            publics[i] = RM.to_bytes(32, "little")
            want[i] = MALFORMED
    assert want[0] == INVALID and want[129] == MALFORMED and want[63] != OK and want[64] != OK
    monkeypatch.setenv("ZKHIP_VERIFY_CHUNK", "50")      # chunk borders at 50 and 100: inside both waves' ranges
    with zk.VerificationKey.from_zkey(golden_path(name, "circuit.zkey")) as vk:
        got = vk.verify(b"".join(proofs), b"".join(publics))
        back = vk.verify(b"".join(reversed(proofs)), b"".join(reversed(publics)))
        monkeypatch.delenv("ZKHIP_VERIFY_CHUNK")
        whole = vk.verify(b"".join(proofs), b"".join(publics))
        assert vk.verify(b"", b"").shape == (0,)
    assert got.dtype == np.uint8 and got.tolist() == want
    assert back.tolist() == want[::-1]
    assert whole.tolist() == want


def test_a_fresh_proof_verifies_and_another_key_refuses_it(zk):
    wt = golden_bytes("r1cs_n64", "witness.wtns")
    p = zk.Prover(golden_path("r1cs_n64", "circuit.zkey"), device=0)
    try:
        proof = p.prove(wt)                             # random (r, s)
    finally:
        p.close()
    assert proof.hex() != golden_json("r1cs_n64", "meta.json")["proof_bytes"]
    public = V.load_public(golden_path("r1cs_n64", "public.json"))
    with zk.VerificationKey.from_zkey(golden_path("r1cs_n64", "circuit.zkey")) as vk:
        assert vk.verify(proof, public).tolist() == [OK]
    with zk.VerificationKey.from_zkey(golden_path("r1cs_n256", "circuit.zkey")) as other:
        padded = (public + bytes(32 * other.n_public))[:32 * other.n_public]      # that key's count of signals
        assert other.verify(proof, padded).tolist() != [OK]


def run(*args):
    return subprocess.run([VERIFIER] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_verifier_command(tmp_path):
    name = "r1cs_n8"
    zkey, public, proof = (golden_path(name, f) for f in ("circuit.zkey", "public.json", "proof.json"))
    vkj = tmp_path / "verification_key.json"
    vkj.write_text(json.dumps(vk_json_of(name)))
    for key in (zkey, vkj):
        r = run(key, public, proof)
        assert (r.returncode, r.stdout, r.stderr) == (0, "OK: the proof verifies\n", "")
    changed = tmp_path / "public.json"
    pub = golden_json(name, "public.json")
    changed.write_text(json.dumps([str((int(pub[0]) + 1) % RM)] + pub[1:]))
    r = run(vkj, changed, proof)
    assert r.returncode == 1 and r.stdout.startswith("INVALID:") and "pairing equation" in r.stdout and "malformed" not in r.stdout
    pj = golden_json(name, "proof.json")
    b = refverify.g2(pj["pi_b"])
    d = next(d for d in range(1, 50) if not bn.G2.is_on_curve((((b[0][0] + d) % QM, b[0][1]), b[1])))
    pj["pi_b"][0][0] = str((b[0][0] + d) % QM)
    off = tmp_path / "proof.json"
    off.write_text(json.dumps(pj))
    r = run(zkey, public, off)
    assert r.returncode == 1 and r.stdout.startswith("INVALID:") and "malformed" in r.stdout
