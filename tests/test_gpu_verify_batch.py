"""Batch verification by random combination (zk_vkey_verify_batch, VerificationKey.verify_batch): the verdicts are those
of the per-proof path at every position, whatever the group and chunk sizes; the report's counts are the ones computed
here from the positions; errors that would cancel in unweighted sums are caught; the sums' edge cases; refusals."""
import random

import numpy as np
import pytest

from conftest import CIRCUITS, golden_bytes, golden_path

from oracle import bn254 as bn
from rapidsnark_old_amd import verify as V
from rapidsnark_old_amd.lib import ZkHipError

pytestmark = pytest.mark.gpu
RM, QM = bn.R_MOD, bn.Q_MOD
OK, INVALID, MALFORMED = 0, 1, 2
DEFAULT_CHUNK = 1 << 16
N = 130
_made = {}


def inputs(name):
    return V.load_proof(golden_path(name, "proof.json")), V.load_public(golden_path(name, "public.json"))


def rerandomised(zk, proof, t):
    """A' = t A, B' = t^-1 B, C' = C (test_gpu_verify.py's): another valid proof of the same statement"""
    return zk.g1_mul(proof[:64], t) + zk.g2_mul(proof[64:192], pow(t, -1, RM)) + proof[192:]


def valid_proofs(zk, name, n=N):
    """n distinct valid proofs of the circuit's golden statement and its public signals, made once"""
    if name not in _made:
        proof, public = inputs(name)
        rng = random.Random(len(name) * 1000 + N)
        _made[name] = ([rerandomised(zk, proof, rng.randrange(2, RM)) for _ in range(N)], public)
        assert len(set(_made[name][0])) == N
    proofs, public = _made[name]
    return list(proofs[:n]), public


def groups_of(n, group, chunk):
    """the index ranges the call forms: consecutive groups inside consecutive chunks, none across a chunk border"""
    out = []
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        out += [range(g0, min(c1, g0 + group)) for g0 in range(c0, c1, group)]
    return out


def expected_report(want, group, chunk):
    gs = [g for g in groups_of(len(want), group, chunk) if any(want[i] != MALFORMED for i in g)]
    failed = [g for g in gs if any(want[i] == INVALID for i in g)]
    return {"group": group, "groups": len(gs), "groups_failed": len(failed),
            "proofs_rechecked": sum(1 for g in failed for i in g if want[i] != MALFORMED), "malformed": want.count(MALFORMED)}


def counts(rep):
    return {k: rep[k] for k in ("group", "groups", "groups_failed", "proofs_rechecked", "malformed")}


def set_sizes(monkeypatch, group, chunk):
    monkeypatch.setenv("ZKHIP_VERIFY_GROUP", str(group))
    if chunk == DEFAULT_CHUNK:
        monkeypatch.delenv("ZKHIP_VERIFY_CHUNK", raising=False)
    else:
        monkeypatch.setenv("ZKHIP_VERIFY_CHUNK", str(chunk))


def scal(values):
    return b"".join(int(v).to_bytes(16, "little") for v in values)


@pytest.fixture(scope="module")
def keys(zk):
    made = {}

    def get(name):
        if name not in made:
            made[name] = zk.VerificationKey.from_zkey(golden_path(name, "circuit.zkey"))
        return made[name]

    yield get
    for vk in made.values():
        vk.close()


@pytest.mark.parametrize("chunk", [50, DEFAULT_CHUNK])
@pytest.mark.parametrize("group", [1, 5, 64, 200])
@pytest.mark.parametrize("name", CIRCUITS)
def test_all_valid(zk, keys, monkeypatch, name, group, chunk):
    proofs, public = valid_proofs(zk, name)
    set_sizes(monkeypatch, group, chunk)
    got, rep = keys(name).verify_batch(b"".join(proofs), public * N)
    assert got.dtype == np.uint8 and got.tolist() == [OK] * N
    assert counts(rep) == {"group": group, "groups": len(groups_of(N, group, chunk)), "groups_failed": 0, "proofs_rechecked": 0, "malformed": 0}
    assert rep["launches"] > 0
    info = keys(name).info()
    assert info["last_path"] == 2 and info["last_launches"] == rep["launches"]


def mixture(zk):
    """test_gpu_verify.py::test_batch_keeps_every_verdict_at_its_position's proofs and verdicts"""
    name = "multiplier2"
    proof, public = inputs(name)
    proofs, _ = valid_proofs(zk, name)
    rng = random.Random(130)
    publics = [public] * N
    want = [OK] * N
    for i in sorted({0, 63, 64, 129} | set(rng.sample(range(N), 9))):
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
    assert {INVALID, MALFORMED} <= set(want) and want.count(OK) >= N - 13
    return name, proofs, publics, want


@pytest.mark.parametrize("chunk", [50, DEFAULT_CHUNK])
@pytest.mark.parametrize("group", [64, 8])
def test_same_verdicts_as_the_per_proof_path(zk, keys, monkeypatch, group, chunk):
    name, proofs, publics, want = mixture(zk)
    vk = keys(name)
    set_sizes(monkeypatch, group, chunk)
    for pr, pu, w in ((proofs, publics, want), (proofs[::-1], publics[::-1], want[::-1])):
        before = vk.info()
        got, rep = vk.verify_batch(b"".join(pr), b"".join(pu))
        after = vk.info()
        single = vk.verify(b"".join(pr), b"".join(pu))
        assert got.tolist() == single.tolist() == w
        assert counts(rep) == expected_report(w, group, chunk)
        assert rep["groups_failed"] > 0 and rep["proofs_rechecked"] > 0
        # rechecked proofs ran on the per-proof paths and count there; the others count in neither
        assert (after["proofs_lanes"] + after["proofs_coop"]) - (before["proofs_lanes"] + before["proofs_coop"]) == rep["proofs_rechecked"]
        assert after["last_path"] == 2


def g1_plus(zk, point, k):
    """point + k G as 64 bytes (k may be negative)"""
    g = bn.G1.mul(bn.G1_GEN, k % RM)
    return bn.g1_to_bytes(bn.G1.add(bn.g1_from_bytes(point), g))


def test_errors_that_cancel_without_scalars(zk, keys, monkeypatch):
    name, n = "r1cs_n64", 12
    proofs, public = valid_proofs(zk, name, n)
    publics = [public] * n
    first = int.from_bytes(public[:32], "little")
    proofs[2] = proofs[2][:192] + g1_plus(zk, proofs[2][192:], 1)       # C + D and C - D: the plain sum of the Cs is honest
    proofs[5] = proofs[5][:192] + g1_plus(zk, proofs[5][192:], -1)
    publics[7] = ((first + 1) % RM).to_bytes(32, "little") + public[32:]   # +1 and -1: the plain sum of the signals is honest
    publics[9] = ((first - 1) % RM).to_bytes(32, "little") + public[32:]
    want = [INVALID if i in (2, 5, 7, 9) else OK for i in range(n)]
    set_sizes(monkeypatch, 64, DEFAULT_CHUNK)
    vk = keys(name)
    P, S = b"".join(proofs), b"".join(publics)
    assert vk.verify(P, S).tolist() == want
    got, rep = vk.verify_batch(P, S)                    # drawn scalars
    assert got.tolist() == want and counts(rep) == expected_report(want, 64, DEFAULT_CHUNK)
    rng = random.Random(12)
    distinct = [rng.getrandbits(128) | 1 for _ in range(n)]
    assert len(set(distinct)) == n
    got, rep = vk.verify_batch(P, S, scalars=scal(distinct))
    assert got.tolist() == want and rep["groups_failed"] == 1 and rep["proofs_rechecked"] == n
    # what the scalars are for: with equal weights the four errors cancel, the group passes and every proof is taken for valid
    got, rep = vk.verify_batch(P, S, scalars=scal([1] * n))
    assert got.tolist() == [OK] * n and rep["groups_failed"] == 0


@pytest.mark.parametrize("name", ["r1cs_n64", "r1cs_nopub"])
@pytest.mark.parametrize("value", [1, (1 << 128) - 1])
def test_equal_scalars_at_both_ends(zk, keys, monkeypatch, name, value):
    n = 70
    proofs, public = valid_proofs(zk, name, n)
    set_sizes(monkeypatch, 64, DEFAULT_CHUNK)
    got, rep = keys(name).verify_batch(b"".join(proofs), public * n, scalars=scal([value] * n))
    assert got.tolist() == [OK] * n
    assert counts(rep) == {"group": 64, "groups": 2, "groups_failed": 0, "proofs_rechecked": 0, "malformed": 0}


def test_a_sum_of_c_at_infinity(zk, keys, monkeypatch):
    name = "r1cs_n64"
    (p,), public = valid_proofs(zk, name, 1)
    c = bn.g1_from_bytes(p[192:])
    q = p[:192] + bn.g1_to_bytes((c[0], (-c[1]) % QM))
    set_sizes(monkeypatch, 2, DEFAULT_CHUNK)
    for r in (1, 0x1234567890abcdef1122334455667788):
        got, rep = keys(name).verify_batch(p + q, public * 2, scalars=scal([r, r]))
        assert got.tolist() == [OK, INVALID]
        assert counts(rep) == {"group": 2, "groups": 1, "groups_failed": 1, "proofs_rechecked": 2, "malformed": 0}


def test_groups_of_malformed_proofs_and_of_one_well_formed(zk, keys, monkeypatch):
    name, n = "multiplier2", 12
    proofs, public = valid_proofs(zk, name, n)
    publics = [public] * n
    for i in (0, 1, 2, 3):                              # group 0: nothing well-formed
        proofs[i] = bytes(64) + proofs[i][64:]
    for i in (4, 5, 7):                                 # group 1: proof 6 alone
        publics[i] = RM.to_bytes(32, "little")
    want = [MALFORMED] * 6 + [OK, MALFORMED] + [OK] * 4
    set_sizes(monkeypatch, 4, DEFAULT_CHUNK)
    vk = keys(name)
    got, rep = vk.verify_batch(b"".join(proofs), b"".join(publics))
    assert got.tolist() == want == vk.verify(b"".join(proofs), b"".join(publics)).tolist()
    assert counts(rep) == {"group": 4, "groups": 2, "groups_failed": 0, "proofs_rechecked": 0, "malformed": 7}
    # the lone well-formed proof of a group, invalid: the group fails and it alone is rechecked
    publics[6] = (5).to_bytes(32, "little")
    want[6] = INVALID
    got, rep = vk.verify_batch(b"".join(proofs), b"".join(publics))
    assert got.tolist() == want
    assert counts(rep) == {"group": 4, "groups": 2, "groups_failed": 1, "proofs_rechecked": 1, "malformed": 7}
    # a call of malformed proofs only evaluates no group
    got, rep = vk.verify_batch(b"".join(proofs[:4]), b"".join(publics[:4]))
    assert got.tolist() == [MALFORMED] * 4
    assert counts(rep) == {"group": 4, "groups": 0, "groups_failed": 0, "proofs_rechecked": 0, "malformed": 4}


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_sizes_around_one_group(zk, keys, monkeypatch, n):
    name = "r1cs_n8"
    proofs, public = valid_proofs(zk, name, n)
    set_sizes(monkeypatch, 64, DEFAULT_CHUNK)
    vk = keys(name)
    got, rep = vk.verify_batch(b"".join(proofs), public * n)
    assert got.shape == (n,) and got.tolist() == [OK] * n
    assert counts(rep) == {"group": 64, "groups": (n + 63) // 64, "groups_failed": 0, "proofs_rechecked": 0, "malformed": 0}
    if n:                                               # the last proof of the call, invalid
        bad = proofs[:-1] + [proofs[-1][:64] + inputs(name)[0][64:192] + proofs[-1][192:]]
        got, rep = vk.verify_batch(b"".join(bad), public * n)
        assert got.tolist() == [OK] * (n - 1) + [INVALID]
        assert rep["groups_failed"] == 1 and rep["proofs_rechecked"] == (n - 1) % 64 + 1


def test_key_handling(zk, monkeypatch):
    name, n = "r1cs_n64", 9
    wt = golden_bytes(name, "witness.wtns")
    p = zk.Prover(golden_path(name, "circuit.zkey"), device=0)
    try:
        fresh = p.prove(wt)                             # random (r, s)
    finally:
        p.close()
    proofs, public = valid_proofs(zk, name, n)
    proofs[4] = fresh
    set_sizes(monkeypatch, 4, DEFAULT_CHUNK)
    with zk.VerificationKey.from_zkey(golden_path(name, "circuit.zkey")) as vk:   # a key of this test's own: its first batch call
        first, rep1 = vk.verify_batch(b"".join(proofs), public * n)
        second, rep2 = vk.verify_batch(b"".join(proofs), public * n)
        assert first.tolist() == second.tolist() == [OK] * n
        assert counts(rep1) == counts(rep2) and rep1["launches"] == rep2["launches"] + 1   # the lines of beta, once
    with zk.VerificationKey.from_zkey(golden_path("r1cs_n256", "circuit.zkey")) as other:
        padded = (public + bytes(32 * other.n_public))[:32 * other.n_public]
        got, rep = other.verify_batch(b"".join(proofs), padded * n)
        assert got.tolist() == [INVALID] * n
        assert counts(rep) == {"group": 4, "groups": 3, "groups_failed": 3, "proofs_rechecked": n, "malformed": 0}


def test_refusals_leave_the_key_working(zk, monkeypatch):
    name, n = "multiplier2", 5
    proofs, public = valid_proofs(zk, name, n)
    P, S = b"".join(proofs), public * n
    set_sizes(monkeypatch, 4, DEFAULT_CHUNK)
    with zk.VerificationKey.from_zkey(golden_path(name, "circuit.zkey")) as vk:
        with pytest.raises(ZkHipError, match="scalar 3 is zero"):
            vk.verify_batch(P, S, scalars=scal([7, 8, 9, 0, 11]))
        with pytest.raises(ValueError, match="scalars"):
            vk.verify_batch(P, S, scalars=scal([7, 8, 9, 10]))
        with pytest.raises(ValueError, match="publics"):
            vk.verify_batch(P, S[:-32])
        for bad in ("0", "many", "-4", "16777217", "8x"):
            monkeypatch.setenv("ZKHIP_VERIFY_GROUP", bad)
            with pytest.raises(ZkHipError, match="ZKHIP_VERIFY_GROUP"):
                vk.verify_batch(P, S)
        monkeypatch.setenv("ZKHIP_VERIFY_GROUP", "4")
        got, rep = vk.verify_batch(P, S, scalars=scal([7, 8, 9, 10, 11]))
        assert got.tolist() == [OK] * n and rep["groups"] == 2
        monkeypatch.delenv("ZKHIP_VERIFY_GROUP")      # the default group
        got, rep = vk.verify_batch(P, S)
        assert got.tolist() == [OK] * n and rep["groups"] == 1 and rep["group"] >= 1
    with pytest.raises(ZkHipError, match="closed"):
        vk.verify_batch(P, S)
