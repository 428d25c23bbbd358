"""VerificationKeySet on the device: proofs under several keys in one call.  The yardstick of every verdict is
VerificationKey.verify on the same proof under the same key (checked against the oracle in test_gpu_verify.py); where
changes are planned, the plan is a yardstick too.  The five golden circuits give five different keys with 1, 1, 3, 0 and 2
public signals, so the ragged layout of `publics` is in every mixed call."""
import random

import numpy as np
import pytest

from conftest import CIRCUITS, golden_path

from oracle import bn254 as bn
from rapidsnark_old_amd import verify as V
from test_gpu_pairing import twist_point_outside_the_subgroup

pytestmark = pytest.mark.gpu
RM, QM = bn.R_MOD, bn.Q_MOD
OK, INVALID, MALFORMED = 0, 1, 2
LANES, COOP = 0, 1
N_PUBLIC = [1, 1, 3, 0, 2]
NOPUB = 3
KINDS = ["B not rescaled", "a signal + 1", "A off the curve", "B outside the subgroup", "C = infinity", "a signal = r"]
WANT = {"B not rescaled": INVALID, "a signal + 1": INVALID, "A off the curve": MALFORMED, "B outside the subgroup": MALFORMED,
        "C = infinity": MALFORMED, "a signal = r": MALFORMED}


def rerandomised(zk, proof, t):
    """A' = t A, B' = t^-1 B, C' = C: another valid proof of the same statement, without proving (test_gpu_verify.py's)"""
    return zk.g1_mul(proof[:64], t) + zk.g2_mul(proof[64:192], pow(t, -1, RM)) + proof[192:]


def changed(kind, proof, public, golden_proof):
    """(proof, public) with one thing changed; proof is a rerandomised copy of golden_proof"""
    A, B, C = proof[:64], proof[64:192], proof[192:]
    if kind == "B not rescaled":
        return A + golden_proof[64:192] + C, public
    if kind == "a signal + 1":
        return proof, ((int.from_bytes(public[:32], "little") + 1) % RM).to_bytes(32, "little") + public[32:]
    if kind == "A off the curve":
        a = bn.g1_from_bytes(A)
        off = next(p for p in (((a[0] + d) % QM, a[1]) for d in range(1, 50)) if not bn.G1.is_on_curve(p))
        return bn.g1_to_bytes(off) + B + C, public
    if kind == "B outside the subgroup":
        return A + bn.g2_to_bytes(twist_point_outside_the_subgroup()) + C, public
    if kind == "C = infinity":
        return A + B + bytes(64), public
    assert kind == "a signal = r"
    return proof, public[:-32] + RM.to_bytes(32, "little")


class World:
    """the keys, the golden inputs, a pool of rerandomised proofs per circuit, and a memo of the per-key yardstick"""

    def __init__(self, zk):
        self.zk = zk
        self.keys = [zk.VerificationKey.from_zkey(golden_path(c, "circuit.zkey")) for c in CIRCUITS]
        self.gold = [(V.load_proof(golden_path(c, "proof.json")), V.load_public(golden_path(c, "public.json"))) for c in CIRCUITS]
        assert [k.n_public for k in self.keys] == N_PUBLIC
        rng = random.Random(24)
        self.pool = [[rerandomised(zk, self.gold[c][0], rng.randrange(2, RM)) for _ in range(65)] for c in range(5)]
        assert len({p for pl in self.pool for p in pl}) == 5 * 65

    def yardstick(self, proofs, key_of, publics):
        """VerificationKey.verify of every key's subset, put back at the callers' positions"""
        out = np.full(len(proofs), 255, dtype=np.uint8)
        for k in sorted(set(key_of)):
            at = [i for i in range(len(proofs)) if key_of[i] == k]
            out[at] = self.keys[k].verify(b"".join(proofs[i] for i in at), b"".join(publics[i] for i in at))
        return out.tolist()

    def mixture(self):
        """200 proofs, keys round-robin, sixteen planned changes -> (proofs, key_of, publics, plan)"""
        n = 200
        rng = random.Random(200)
        key_of = [i % 5 for i in range(n)]
        proofs = [self.pool[i % 5][i // 5] for i in range(n)]
        publics = [self.gold[i % 5][1] for i in range(n)]
        plan = [OK] * n
        fixed = [0, 63, 64, 65, 127, 128, 199]
        spots = fixed + rng.sample(sorted(set(range(n)) - set(fixed)), 9)
        used, left = set(), []
        for i in sorted(spots):                         # the kinds in turn; the key without signals skips the two that need one
            fits = [k for k in left if key_of[i] != NOPUB or "signal" not in k]
            if not fits:
                left = list(KINDS)
                fits = left
            kind = fits[0]
            left.remove(kind)
            proofs[i], publics[i] = changed(kind, proofs[i], publics[i], self.gold[key_of[i]][0])
            plan[i] = WANT[kind]
            used.add(kind)
        assert len(spots) == 16 and used == set(KINDS)
        return proofs, key_of, publics, plan

    def close(self):
        for k in self.keys:
            k.close()


@pytest.fixture(scope="module")
def world(zk):
    w = World(zk)
    yield w
    w.close()


@pytest.fixture(scope="module")
def mixture(world):
    proofs, key_of, publics, plan = world.mixture()
    assert world.yardstick(proofs, key_of, publics) == plan   # computed once, by the single-key code
    return proofs, key_of, publics, plan


def call(ks, proofs, key_of, publics):
    return ks.verify(b"".join(proofs), key_of, b"".join(publics))


def test_the_five_goldens_in_one_call_in_any_order(zk, world):
    with zk.VerificationKeySet(world.keys) as ks:
        for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 4, 0, 3, 1]):
            got = call(ks, [world.gold[c][0] for c in order], order, [world.gold[c][1] for c in order])
            assert got.dtype == np.uint8 and got.tolist() == [OK] * 5, order
        info = ks.info()
        assert info["n_keys"] == 5 and info["last_path"] == COOP and info["last_launches"] == 1 and info["proofs_coop"] == 15


def test_a_one_key_set_is_verify(zk, world, monkeypatch):
    n = 130
    proofs = [world.pool[0][i % 65] for i in range(n)]
    publics = [world.gold[0][1]] * n
    for i, kind in ((0, "B not rescaled"), (64, "a signal = r"), (129, "C = infinity"), (77, "a signal + 1")):
        proofs[i], publics[i] = changed(kind, proofs[i], publics[i], world.gold[0][0])
    want = world.keys[0].verify(b"".join(proofs), b"".join(publics)).tolist()
    assert want[0] == INVALID and want[64] == MALFORMED and want[129] == MALFORMED and want[77] == INVALID and want.count(OK) == n - 4
    with zk.VerificationKeySet([world.keys[0]]) as ks:
        assert call(ks, proofs, [0] * n, publics).tolist() == want
        monkeypatch.setenv("ZKHIP_VERIFY_COOP_MAX", "0")
        assert call(ks, proofs, np.zeros(n, dtype=np.int32), publics).tolist() == want
        assert ks.info()["last_path"] == LANES and ks.info()["last_waves_padded"] == 1


@pytest.mark.parametrize("env", [{}, {"ZKHIP_VERIFY_COOP_MAX": "0"}, {"ZKHIP_VERIFY_COOP_MAX": "0", "ZKHIP_VERIFY_CHUNK": "50"}],
                         ids=["cooperative", "lanes", "lanes-chunk-50"])
def test_a_mixture_keeps_every_verdict_at_its_position(zk, world, mixture, monkeypatch, env):
    proofs, key_of, publics, plan = mixture
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with zk.VerificationKeySet(world.keys) as ks:
        got = call(ks, proofs, key_of, publics)
        info = ks.info()
    assert got.tolist() == plan
    if not env:
        assert info["last_path"] == COOP and info["last_launches"] == 1 and info["last_waves_padded"] == 0 and info["proofs_coop"] == 200
    else:
        chunks = 4 if "ZKHIP_VERIFY_CHUNK" in env else 1
        # 40 proofs a key in one chunk, 10 a key in each chunk of 50: every run ends inside a wave
        assert info["last_path"] == LANES and info["last_launches"] == 3 * chunks and info["last_waves_padded"] == 5 * chunks
        assert info["proofs_lanes"] == 200 and info["proofs_coop"] == 0


def test_runs_of_1_63_64_65_side_by_side_on_the_lane_path(zk, world, monkeypatch):
    runs = [(0, 1), (1, 63), (2, 64), (4, 65)]
    proofs, key_of, publics = [], [], []
    for k, length in runs:
        first = len(proofs)
        proofs += world.pool[k][:length]
        key_of += [k] * length
        publics += [world.gold[k][1]] * length
        for i, kind in ((first, "B not rescaled"), (len(proofs) - 1, "a signal = r")) if length > 1 else ():
            proofs[i], publics[i] = changed(kind, proofs[i], publics[i], world.gold[k][0])
    want = world.yardstick(proofs, key_of, publics)
    assert want.count(INVALID) == 3 and want.count(MALFORMED) == 3 and want[0] == OK
    monkeypatch.setenv("ZKHIP_VERIFY_COOP_MAX", "0")
    with zk.VerificationKeySet(world.keys) as ks:
        assert call(ks, proofs, key_of, publics).tolist() == want
        assert ks.info()["last_waves_padded"] == 3 and ks.info()["last_launches"] == 3      # 1, 63 and 65 leave idle lanes; 64 does not
        # the same proofs interleaved: the host groups them, the verdicts return to the callers' positions
        order = list(range(len(proofs)))
        random.Random(4).shuffle(order)
        got = call(ks, [proofs[i] for i in order], [key_of[i] for i in order], [publics[i] for i in order])
        assert got.tolist() == [want[i] for i in order]
        assert ks.info()["last_waves_padded"] == 3 and ks.info()["last_launches"] == 3


@pytest.mark.parametrize("coop_max", [None, "0"], ids=["cooperative", "lanes"])
def test_a_proof_under_another_key_is_invalid_not_an_error(zk, world, monkeypatch, coop_max):
    if coop_max is not None:
        monkeypatch.setenv("ZKHIP_VERIFY_COOP_MAX", coop_max)
    (p0, s0), (p1, s1) = world.gold[0], world.gold[1]   # multiplier2 and r1cs_n8: one public signal each
    want = world.yardstick([p0, p1, p0, p1], [1, 0, 0, 1], [s0, s1, s0, s1])
    assert want == [INVALID, INVALID, OK, OK]
    with zk.VerificationKeySet(world.keys) as ks:
        assert ks.verify(p0 + p1 + p0 + p1, [1, 0, 0, 1], s0 + s1 + s0 + s1).tolist() == want


@pytest.mark.parametrize("coop_max", [None, "0"], ids=["cooperative", "lanes"])
def test_the_key_without_public_signals(zk, world, monkeypatch, coop_max):
    if coop_max is not None:
        monkeypatch.setenv("ZKHIP_VERIFY_COOP_MAX", coop_max)
    key_of = [2, NOPUB, 4, NOPUB, NOPUB, 0, NOPUB]
    proofs = [world.pool[k][i] for i, k in enumerate(key_of)]
    publics = [world.gold[k][1] for k in key_of]
    proofs[3], publics[3] = changed("B not rescaled", proofs[3], publics[3], world.gold[NOPUB][0])
    proofs[2], publics[2] = changed("a signal + 1", proofs[2], publics[2], world.gold[4][0])
    want = [OK, OK, INVALID, INVALID, OK, OK, OK]
    assert world.yardstick(proofs, key_of, publics) == want
    with zk.VerificationKeySet(world.keys) as ks:
        assert call(ks, proofs, key_of, publics).tolist() == want
        only = [proofs[i] for i in (1, 3, 4, 6)]
        assert ks.verify(b"".join(only), [NOPUB] * 4, b"").tolist() == [OK, INVALID, OK, OK]
        assert ks.verify(b"".join(only), [NOPUB] * 4).tolist() == [OK, INVALID, OK, OK]


@pytest.mark.parametrize("coop_max", [None, "0"], ids=["cooperative", "lanes"])
def test_one_key_of_five_no_proofs_and_a_key_twice(zk, world, monkeypatch, coop_max):
    if coop_max is not None:
        monkeypatch.setenv("ZKHIP_VERIFY_COOP_MAX", coop_max)
    with zk.VerificationKeySet(world.keys) as ks:
        proofs = world.pool[4][:3]
        assert ks.verify(b"".join(proofs), [4, 4, 4], world.gold[4][1] * 3).tolist() == [OK] * 3
        before = ks.info()
        empty = ks.verify(b"", [], b"")
        assert empty.shape == (0,) and empty.dtype == np.uint8 and ks.info() == before
    with zk.VerificationKeySet([world.keys[2], world.keys[0], world.keys[2]]) as ks:
        assert ks.info()["n_keys"] == 3
        p2, s2 = world.gold[2]
        bad, _ = changed("B not rescaled", world.pool[2][0], s2, p2)
        assert ks.verify(p2 + bad + world.pool[2][1] + world.gold[0][0], [0, 2, 2, 1], s2 * 3 + world.gold[0][1]).tolist() == [OK, INVALID, OK, OK]


def test_the_launch_count_does_not_depend_on_the_keys(zk, world, mixture, monkeypatch):
    proofs, key_of, publics, plan = mixture
    one = [world.pool[0][i % 65] for i in range(200)]
    with zk.VerificationKeySet(world.keys) as five, zk.VerificationKeySet([world.keys[0]]) as single:
        assert call(five, proofs, key_of, publics).tolist() == plan and five.info()["last_launches"] == 1
        assert single.verify(b"".join(one), [0] * 200, world.gold[0][1] * 200).tolist() == [OK] * 200 and single.info()["last_launches"] == 1
        monkeypatch.setenv("ZKHIP_VERIFY_COOP_MAX", "0")
        for chunk in (None, "50"):
            if chunk:
                monkeypatch.setenv("ZKHIP_VERIFY_CHUNK", chunk)
            assert call(five, proofs, key_of, publics).tolist() == plan
            assert single.verify(b"".join(one), [0] * 200, world.gold[0][1] * 200).tolist() == [OK] * 200
            assert five.info()["last_path"] == single.info()["last_path"] == LANES
            assert five.info()["last_launches"] == single.info()["last_launches"] == (12 if chunk else 3)


def test_set_calls_leave_the_keys_as_they_were(zk, world, mixture, monkeypatch):
    proofs, key_of, publics, plan = mixture
    fresh = [zk.VerificationKey.from_zkey(golden_path(c, "circuit.zkey")) for c in CIRCUITS]
    try:
        for k, (p, s) in zip(fresh, world.gold):
            assert k.verify(p, s).tolist() == [OK]
        before = [k.info() for k in fresh]
        with zk.VerificationKeySet(fresh) as ks:
            assert call(ks, proofs, key_of, publics).tolist() == plan
            monkeypatch.setenv("ZKHIP_VERIFY_COOP_MAX", "0")
            assert call(ks, proofs, key_of, publics).tolist() == plan
            monkeypatch.delenv("ZKHIP_VERIFY_COOP_MAX")
            assert [k.info() for k in fresh] == before
            for k, (p, s) in zip(fresh, world.gold):      # the keys' own entries, the set still open
                assert k.verify(p, s).tolist() == [OK]
                verdicts, report = k.verify_batch(p + p, s + s)
                assert verdicts.tolist() == [OK, OK] and report["groups_failed"] == 0
        for k, (p, s) in zip(fresh, world.gold):          # and after it is closed
            assert k.verify(p, s).tolist() == [OK]
    finally:
        for k in fresh:
            k.close()


def test_refusals_carry_a_message(zk, world):
    import ctypes as C
    from rapidsnark_old_amd import lib as L
    lib = L.load_library()
    with pytest.raises(ValueError, match="at least one key"):
        zk.VerificationKeySet([])
    h = C.c_void_p()
    assert lib.zk_vkey_set_create(C.byref(h), (C.c_void_p * 1)(), 0) != 0 and not h
    assert "at least one key" in lib.zk_last_error().decode()
    p0, s0 = world.gold[0]
    p2, s2 = world.gold[2]
    with zk.VerificationKeySet(world.keys) as ks:
        with pytest.raises(ValueError, match=r"key_of\[1\] = 5"):
            ks.verify(p0 + p0, [0, 5], s0 + s0)
        with pytest.raises(ValueError, match="publics: 128 bytes expected .* got 96"):
            ks.verify(p0 + p2, [0, 2], s0 + s2[:64])
        # the library's own refusals, for callers of the C interface
        out = np.zeros(2, dtype=np.uint8)
        pr, pub = np.frombuffer(p0 + p2, dtype=np.uint8), np.frombuffer(s0 + s2, dtype=np.uint8)
        ko = np.array([0, 5], dtype=np.uint32)
        assert lib.zk_vkey_set_verify(ks._h, L._ptr(pr), L._ptr(ko), L._ptr(pub), pub.size, 2, L._ptr(out)) != 0
        msg = lib.zk_last_error().decode()
        assert "key_of[1] = 5" in msg and "5 keys" in msg
        ko = np.array([0, 2], dtype=np.uint32)
        assert lib.zk_vkey_set_verify(ks._h, L._ptr(pr), L._ptr(ko), L._ptr(pub), pub.size - 32, 2, L._ptr(out)) != 0
        msg = lib.zk_last_error().decode()
        assert "128 expected" in msg and "96 given" in msg
        assert lib.zk_vkey_set_verify(ks._h, L._ptr(pr), None, L._ptr(pub), pub.size, 2, L._ptr(out)) != 0
        assert "null argument" in lib.zk_last_error().decode()
        assert ks.info()["proofs_coop"] == 0 and ks.info()["proofs_lanes"] == 0      # refused before any launch
        assert lib.zk_vkey_set_verify(ks._h, L._ptr(pr), L._ptr(ko), L._ptr(pub), pub.size, 2, L._ptr(out)) == 0 and out.tolist() == [OK, OK]
