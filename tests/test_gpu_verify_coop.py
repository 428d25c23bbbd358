"""zk_vkey_verify's two paths (a lane per proof, a workgroup per proof): which one a call takes, and equal verdicts from both
on the goldens, on every kind of defect alone and in one call, and on batches with more workgroups than the chip has
compute units.  ZKHIP_VERIFY_COOP_MAX = 0 forces the lane path, a value >= n the cooperative one."""
import json
import random

import pytest

from conftest import CIRCUITS, golden_json, golden_path

from oracle import bn254 as bn
from rapidsnark_old_amd import verify as V
from test_gpu_pairing import twist_point_outside_the_subgroup
from test_verify_host import vk_json_of

pytestmark = pytest.mark.gpu
RM, QM = bn.R_MOD, bn.Q_MOD
OK, INVALID, MALFORMED = 0, 1, 2
LANES, COOP = 0, 1


def inputs(name):
    return V.load_proof(golden_path(name, "proof.json")), V.load_public(golden_path(name, "public.json"))


def both_paths(vk, monkeypatch, proofs, publics):
    """the verdicts of the cooperative path, after asserting the lane path gives the same"""
    n = len(proofs) // 256
    monkeypatch.setenv("ZKHIP_VERIFY_COOP_MAX", "0")
    lanes = vk.verify(proofs, publics).tolist()
    assert vk.info()["last_path"] == LANES
    monkeypatch.setenv("ZKHIP_VERIFY_COOP_MAX", str(max(n, 1)))
    coop = vk.verify(proofs, publics).tolist()
    assert vk.info()["last_path"] == COOP and vk.info()["last_launches"] == 1
    assert coop == lanes
    return coop


def cofactor_point(i, kind="cofactor"):
    """a point of the twist from tests/golden/g2_cofactor_points.json: of small order dividing the cofactor, or outside the subgroup"""
    p = golden_json("g2_cofactor_points.json")[kind][i]
    pt = ((int(p["x"][0]), int(p["x"][1])), (int(p["y"][0]), int(p["y"][1])))
    assert bn.G2.is_on_curve(pt)
    return pt


def rerandomised(zk, proof, t):
    """A' = t A, B' = t^-1 B, C' = C: another valid proof of the same statement"""
    return zk.g1_mul(proof[:64], t) + zk.g2_mul(proof[64:192], pow(t, -1, RM)) + proof[192:]


def test_path_selection(zk, monkeypatch):
    name = "multiplier2"
    proof, public = inputs(name)
    monkeypatch.delenv("ZKHIP_VERIFY_COOP_MAX", raising=False)
    with zk.VerificationKey.from_zkey(golden_path(name, "circuit.zkey")) as vk:
        assert vk.verify(proof, public).tolist() == [OK]
        info = vk.info()
        assert info["last_path"] == COOP and info["last_launches"] == 1 and info["proofs_coop"] == 1 and info["proofs_lanes"] == 0
        monkeypatch.setenv("ZKHIP_VERIFY_COOP_MAX", "0")
        assert vk.verify(proof, public).tolist() == [OK]
        info = vk.info()
        assert info["last_path"] == LANES and info["coop_max"] == 0 and info["last_launches"] == 3
        assert info["proofs_coop"] == 1 and info["proofs_lanes"] == 1
        monkeypatch.setenv("ZKHIP_VERIFY_COOP_MAX", "4")
        assert vk.verify(proof * 4, public * 4).tolist() == [OK] * 4
        assert vk.info()["last_path"] == COOP and vk.info()["coop_max"] == 4
        assert vk.verify(proof * 5, public * 5).tolist() == [OK] * 5
        info = vk.info()
        assert info["last_path"] == LANES and info["proofs_coop"] == 5 and info["proofs_lanes"] == 6
        for bad in ("many", "-1", "16777217", "4 "):
            monkeypatch.setenv("ZKHIP_VERIFY_COOP_MAX", bad)
            with pytest.raises(zk.ZkHipError, match=r"ZKHIP_VERIFY_COOP_MAX: a number of proofs from 0 to 2\^24 expected"):
                vk.verify(proof, public)


@pytest.mark.parametrize("name", CIRCUITS)
def test_goldens_verify_on_both_paths_through_both_key_forms(zk, monkeypatch, name, tmp_path):
    proof, public = inputs(name)
    with zk.VerificationKey.from_zkey(golden_path(name, "circuit.zkey")) as vk:
        assert both_paths(vk, monkeypatch, proof, public) == [OK]
    p = tmp_path / "verification_key.json"
    p.write_text(json.dumps(vk_json_of(name)))
    with zk.VerificationKey.from_json(str(p)) as vk:
        assert both_paths(vk, monkeypatch, proof, public) == [OK]


def test_verdict_codes_with_one_thing_changed_alone_and_in_one_call(zk, monkeypatch):
    name = "r1cs_n64"
    proof, public = inputs(name)
    A, B, C = proof[:64], proof[64:192], proof[192:]
    a, b, c = bn.g1_from_bytes(A), bn.g2_from_bytes(B), bn.g1_from_bytes(C)

    def leaves(curve, make):
        for d in range(1, 50):
            if not curve.is_on_curve(make(d)):
                return make(d)
        raise AssertionError("no offset leaves the curve")

    a_off = leaves(bn.G1, lambda d: ((a[0] + d) % QM, a[1]))
    b_off = leaves(bn.G2, lambda d: (((b[0][0] + d) % QM, b[0][1]), b[1]))
    pub_plus = ((int.from_bytes(public[:32], "little") + 1) % RM).to_bytes(32, "little") + public[32:]
    pub_r = public[:32] + RM.to_bytes(32, "little") + public[64:]
    outside = bn.g2_to_bytes(twist_point_outside_the_subgroup())
    cases = [
        ("unchanged", proof, public, OK),
        ("A <- 2A", zk.g1_mul(A, 2) + B + C, public, INVALID),
        ("a public signal + 1", proof, pub_plus, INVALID),
        ("C <- -C", A + B + bn.g1_to_bytes((c[0], (-c[1]) % QM)), public, INVALID),
        ("A off the curve", bn.g1_to_bytes(a_off) + B + C, public, MALFORMED),
        ("B off the twist", A + bn.g2_to_bytes(b_off) + C, public, MALFORMED),
        ("B outside the subgroup", A + outside + C, public, MALFORMED),
        ("B of cofactor order", A + bn.g2_to_bytes(cofactor_point(0)) + C, public, MALFORMED),
        ("B outside the subgroup, the golden file's", A + bn.g2_to_bytes(cofactor_point(0, "outside")) + C, public, MALFORMED),
        ("A = infinity", bytes(64) + B + C, public, MALFORMED),
        ("B = infinity", A + bytes(128) + C, public, MALFORMED),
        ("C = infinity", A + B + bytes(64), public, MALFORMED),
        ("a coordinate = q", QM.to_bytes(32, "little") + A[32:] + B + C, public, MALFORMED),
        ("a public signal = r", proof, pub_r, MALFORMED),
        ("A off the curve and a signal = r", bn.g1_to_bytes(a_off) + B + C, pub_r, MALFORMED),
        ("A <- 2A and B outside the subgroup", zk.g1_mul(A, 2) + outside + C, public, MALFORMED),
    ]
    with zk.VerificationKey.from_zkey(golden_path(name, "circuit.zkey")) as vk:
        got = both_paths(vk, monkeypatch, b"".join(x[1] for x in cases), b"".join(x[2] for x in cases))
        monkeypatch.setenv("ZKHIP_VERIFY_COOP_MAX", "1")
        single = [int(vk.verify(x[1], x[2])[0]) for x in cases]
        assert vk.info()["last_path"] == COOP
    want = [x[3] for x in cases]
    assert got == want, [(x[0], g) for x, g in zip(cases, got) if g != x[3]]
    assert single == want, [(x[0], g) for x, g in zip(cases, single) if g != x[3]]


@pytest.mark.parametrize("n", [2, 65, 300])
def test_every_verdict_at_its_position(zk, monkeypatch, n):
    name = "multiplier2"
    proof, public = inputs(name)
    rng = random.Random(n)
    base = [rerandomised(zk, proof, rng.randrange(2, RM)) for _ in range(min(n, 16))]
    proofs = [base[i % len(base)] for i in range(n)]
    publics = [public] * n
    want = [OK] * n
    fixed = [i for i in (0, 255, 256, 299) if i < n]
    spots = sorted(set(fixed) | set(rng.sample(range(n), min(9, n - 1))))
    for at, i in enumerate(spots):
        kind = at % 4
        if kind == 0:                                   # B of another proof: well-formed, the equation fails
            proofs[i] = proofs[i][:64] + proof[64:192] + proofs[i][192:]
            want[i] = OK if proofs[i] == proof else INVALID
        elif kind == 1:
            publics[i] = (5).to_bytes(32, "little")
            want[i] = INVALID
        elif kind == 2:
            proofs[i] = bytes(64) + proofs[i][64:]
            want[i] = MALFORMED
        else:
            publics[i] = RM.to_bytes(32, "little")
            want[i] = MALFORMED
    assert len(set(want)) == 3 or n == 2
    with zk.VerificationKey.from_zkey(golden_path(name, "circuit.zkey")) as vk:
        assert both_paths(vk, monkeypatch, b"".join(proofs), b"".join(publics)) == want
        assert both_paths(vk, monkeypatch, b"".join(reversed(proofs)), b"".join(reversed(publics))) == want[::-1]


@pytest.fixture(scope="module")
def made_keys(zk, tmp_path_factory):
    """n_public -> (zkey path, proof, public bytes): valid keys of 2^7 rows made at run time, proved once, shared by the tests below"""
    import valid_key
    out = {}
    d = tmp_path_factory.mktemp("coop_keys")
    for n_public in (1, 63, 64, 65):
        wl, wit, trap, w = valid_key.build(zk, 7, 700 + n_public, n_public=n_public)
        zpath = d / ("valid_%d.zkey" % n_public)
        zpath.write_bytes(valid_key.zkey_bytes(wl))
        p = zk.Prover(str(zpath), device=0)
        try:
            proof = p.prove(valid_key.wtns_bytes(wl, wit), r=12345 + n_public, s=(1 << 200) + n_public)
        finally:
            p.close()
        out[n_public] = (str(zpath), proof, wit.tobytes()[32:32 * (1 + n_public)])
    return out


@pytest.mark.parametrize("n_public", [1, 63, 64, 65])
def test_signal_counts_at_the_edges_of_the_lane_per_signal_loop(zk, monkeypatch, made_keys, n_public):
    zpath, proof, public = made_keys[n_public]
    assert len(public) == 32 * n_public
    changed = sorted({0, min(63, n_public - 1), n_public - 1})          # the first, the 64th (where there is one) and the last
    proofs, publics, want = [proof], [public], [OK]
    for j in changed:
        v = (int.from_bytes(public[32 * j:32 * j + 32], "little") + 1) % RM
        publics.append(public[:32 * j] + v.to_bytes(32, "little") + public[32 * j + 32:])
        proofs.append(proof)
        want.append(INVALID)
    with zk.VerificationKey.from_zkey(zpath) as vk:
        assert vk.n_public == n_public
        assert both_paths(vk, monkeypatch, b"".join(proofs), b"".join(publics)) == want
        assert both_paths(vk, monkeypatch, proof, public) == [OK]


def test_a_key_whose_vk_x_is_the_point_at_infinity(zk, monkeypatch):
    """IC_1 = -IC_0 and the signal 1: vk_x = infinity, legal, e(vk_x, gamma) = 1.  No golden proof verifies under it."""
    name = "r1cs_n64"
    proof, _ = inputs(name)
    with zk.VerificationKey.from_zkey(golden_path(name, "circuit.zkey")) as vk:
        alpha1, beta2, gamma2, delta2, ic0 = vk.alpha1, vk.beta2, vk.gamma2, vk.delta2, vk.ic[:64]
    x, y = bn.g1_from_bytes(ic0)
    one = (1).to_bytes(32, "little")
    with zk.VerificationKey(alpha1, beta2, gamma2, delta2, ic0 + bn.g1_to_bytes((x, (-y) % QM))) as vk:
        assert vk.n_public == 1
        assert both_paths(vk, monkeypatch, proof, one) == [INVALID]
        two = (2).to_bytes(32, "little")                                # vk_x = -IC_0: not infinity, and no proof of it either
        assert both_paths(vk, monkeypatch, proof * 2, one + two) == [INVALID, INVALID]


def test_signals_whose_halves_are_extreme_for_the_endomorphism_split(zk, monkeypatch, made_keys):
    zpath, proof, public = made_keys[63]
    real = int.from_bytes(public[:32], "little")
    values = [0, 1, RM - 1, (1 << 128) - 1, 1 << 128, real]
    publics = b"".join(v.to_bytes(32, "little") + public[32:] for v in values)
    want = [OK if v == real else INVALID for v in values]
    with zk.VerificationKey.from_zkey(zpath) as vk:
        assert both_paths(vk, monkeypatch, proof * len(values), publics) == want
