"""The PLONK verifier object on the GPU (zk_plonk_verifier_*): made from the key alone, m proofs a call, the transcript on the
device.  Two yardsticks, both exact.  The challenges of the device transcript are compared, row by row, with the Python
transcript of tests/plonk_prover_instance.py on inputs that are no valid proofs (random points of the curve, random values).
The verdicts are compared with zk_plonk_verify's, proof by proof, and for chosen proofs with that file's pairing-free
verifier at the known tau."""
import ctypes
import functools
import math
import random

import numpy as np
import pytest

import plonk_instance as pi
import plonk_prover_instance as pp
from conftest import golden_json
from oracle import bn254 as bn

pytestmark = pytest.mark.gpu

R, Q = bn.R_MOD, bn.Q_MOD
TAU, ALPHA, BETA = 0x1F3A9C5E77D1B2A49E0C6F5D3B8A17264C9E0F1D2B3A4958, 0x2B7E151628AED2A6ABF7158809CF4F3C, 0x3243F6A8885A308D313198A2E0370734
MAX_COEFFS = (1 << 11) + 6
OK, INVALID, MALFORMED = 0, 1, 2
DEFAULT_CHUNK = 65536
KNOB = "ZKHIP_PLONK_VERIFY_CHUNK"
TAU_G2 = bn.G2.mul(bn.G2_GEN, TAU)


def le(values):
    return np.frombuffer(pi.le(values), dtype=np.uint8)


@pytest.fixture(scope="module")
def ptau_path(zk, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("plonk_verifier") / "p12.ptau")
    zk.write_trapdoor_ptau(12, TAU, ALPHA, BETA, path, prepared=False)
    return path


@pytest.fixture(scope="module")
def kzg(zk, ptau_path):
    k = zk.Kzg.from_ptau(ptau_path, max_coeffs=MAX_COEFFS)
    yield k
    k.close()


def make_prover(zk, kzg, c):
    return zk.PlonkProver(kzg, *[le(x) for x in c.inst.circuit("monomial")], pi.K1, pi.K2, *c.maps, c.n_witness, c.n_public)


class Key:
    """one circuit: its case, its prover (module-scoped), its key, a few proofs with drawn blinds"""


@pytest.fixture(scope="module")
def keys(zk, kzg):
    out = {}
    for name, seed, log_n, n_public, count in (("small", 5003, 3, 2, 11), ("all_public", 5116, 4, 16, 3), ("large", 5011, 11, 2, 3), ("no_public", 5203, 3, 0, 3)):
        k = Key()
        k.case = pp.build(seed, log_n, n_public)
        k.log_n, k.n_public = log_n, n_public
        k.prover = make_prover(zk, kzg, k.case)
        k.vk = k.prover.vkey()
        k.proofs = [k.prover.prove(k.case.witness, k.case.publics if n_public else None).to_bytes() for _ in range(count)]
        out[name] = k
    small = out["small"]
    blind = random.Random(5003)
    small.ref = pp.prove(small.case, [blind.randrange(1, R) for _ in range(11)], TAU)        # the byte-exact reference proof
    small.proofs.insert(0, small.ref.to_bytes())
    small.vk_ref = pp.vkey_points(small.case.inst, TAU)
    yield out
    for k in out.values():
        k.prover.close()


# ---------------------------------------------------------------- the challenges are the transcript's
@functools.lru_cache(maxsize=None)
def point_pool():
    rng = random.Random(7100)
    return [bn.G1.mul(bn.G1_GEN, rng.randrange(1, R)) for _ in range(40)] + [None]


def random_key(zk, rng, log_n, n_public):
    pool = point_pool()
    pts = [pool[rng.randrange(40)] for _ in range(8)]
    return pts, zk.PlonkVKey.from_parts(log_n, n_public, pi.K1, pi.K2, pts, TAU_G2)


def subtractions(*items):
    """how often r goes into the digest of these items"""
    return int.from_bytes(pp.keccak256(b"".join(pp._enc(x) for x in items)), "big") // R


@pytest.mark.parametrize("n_public", [0, 1, 2, 12, 16])      # 12: the round-1 message is 1088 bytes = 8 x 136, the last block is padding only
def test_challenges_are_the_transcripts(zk, n_public):
    m = 70
    rng = random.Random(7200 + n_public)
    pool = point_pool()
    vk_pts, vk = random_key(zk, rng, 4, n_public)
    assert ((512 + 32 * n_public + 192) % 136 == 0) == (n_public == 12)
    rows = []
    for i in range(m):
        pts = [pool[rng.randrange(40)] for _ in range(9)]
        if i == 9:
            pts[rng.randrange(9)] = None                 # one at infinity
        rows.append((pts, [rng.randrange(R) for _ in range(6)], [rng.randrange(R) for _ in range(n_public)]))
    rows[11] = (rows[11][0], [0, R - 1, 1, 0, R - 1, 2], [R - 1] * n_public)
    raw = [bytearray(b"".join(bn.g1_to_bytes(P) for P in pts) + pi.le(ev)) for pts, ev, _ in rows]
    pub = [list(p) for _, _, p in rows]
    # malformed rows among them: a point off the curve, a coordinate = q, a value = r, a public = r
    bad = {5: "curve", 17: "q", 33: "r"}
    raw[5][2 * 64 + 32] ^= 1
    raw[17][6 * 64:6 * 64 + 32] = Q.to_bytes(32, "little")
    raw[33][576 + 4 * 32:576 + 5 * 32] = R.to_bytes(32, "little")
    if n_public:
        bad[50] = "public"
        pub[50][n_public - 1] = R
    assert all(pp.parse(bytes(raw[i])) is None for i in (5, 17, 33))
    with zk.PlonkVerifier(vk) as v:
        got, status = v.challenges([bytes(b) for b in raw], pub if n_public else None)
        again, status2 = v.challenges(np.frombuffer(b"".join(bytes(b) for b in raw), dtype=np.uint8).reshape(m, 768), pub if n_public else None)
    assert got == again and list(status) == list(status2)
    deep = 0
    for i, (pts, ev, publics) in enumerate(rows):
        if i in bad:
            assert status[i] == MALFORMED and got[i] == [0] * 6, (i, bad[i])
            continue
        c = pp.challenges(vk_pts, publics, pts, ev)
        assert status[i] == 0 and got[i] == [c.beta, c.gamma, c.alpha, c.zeta, c.v, c.u], i
        deep = max(deep, subtractions(c.beta), subtractions(pts[7], pts[8]), subtractions(c.zeta, *ev))
    assert deep >= 4                                     # a digest that needs four or five subtractions of r is among them


# ---------------------------------------------------------------- the verdicts are zk_plonk_verify's
def tamper(kind, good, publics, ref_points):
    """-> (proof bytes, publics) for one of the 31 kinds"""
    publics = list(publics)
    if kind < 15:                                        # one byte of each field
        at = kind * 64 + 5 if kind < 9 else 576 + (kind - 9) * 32 + 5
        bad = bytearray(good)
        bad[at] ^= 0x10
        return bytes(bad), publics
    if kind < 24:                                        # P + G in place of P
        f = kind - 15
        P = bn.g1_from_bytes(good[f * 64:(f + 1) * 64])
        return good[:f * 64] + bn.g1_to_bytes(bn.G1.add(P, bn.G1_GEN)) + good[(f + 1) * 64:], publics
    if kind == 24:
        return good, [publics[0], (publics[1] + 1) % R]
    if kind == 25:
        return good[:8 * 64] + bytes(64) + good[9 * 64:], publics               # W_zeta_omega = infinity: a point
    if kind == 26:
        return good[:64] + bn.g1_to_bytes((1, 3)) + good[128:], publics         # (1, 3): 9 != 1 + 3
    if kind == 27:
        return good[:96] + Q.to_bytes(32, "little") + good[128:], publics       # a coordinate that is not below q
    if kind == 28:
        return good[:576 + 64] + R.to_bytes(32, "little") + good[576 + 96:], publics
    if kind == 29:
        return good[:576 + 64] + ((1 << 256) - 1).to_bytes(32, "little") + good[576 + 96:], publics
    assert kind == 30
    return good, [publics[0], R]                         # a public input not below r


KINDS = 31


@pytest.fixture(scope="module")
def expected(zk, keys):
    """zk_plonk_verify's verdict for (proof, publics) under the small key, asked once a pair"""
    memo = {}

    def ask(proof, publics):
        key = (proof, tuple(publics))
        if key not in memo:
            memo[key] = zk.plonk_verify(keys["small"].vk, proof, publics)
        return memo[key]

    return ask


@pytest.mark.parametrize("m,first_kind", [(1, 0), (2, 0), (63, 8), (64, 16), (65, 24), (200, 0)])
def test_verdicts_are_zk_plonk_verifys(zk, keys, expected, m, first_kind):
    """index i = 3 (mod 7) is tampered, kind (first_kind + i // 7) mod 31: the batch of 200 holds kinds 0 .. 28, the one of 65
    kinds 24 .. 30 and 0 .. 2, so that every kind is met"""
    k = keys["small"]
    publics = k.case.publics
    proofs, pubs, clean = [], [], []
    for i in range(m):
        good = k.proofs[i % len(k.proofs)]
        if i % 7 == 3:
            p, q = tamper((first_kind + i // 7) % KINDS, good, publics, k.ref.points)
        else:
            p, q = good, list(publics)
            clean.append(i)
        proofs.append(p)
        pubs.append(q)
    with zk.PlonkVerifier(k.vk) as v:
        got = v.verify(proofs, pubs)
        info = v.info()
    want = [expected(p, q) for p, q in zip(proofs, pubs)]
    assert got.dtype == np.uint8 and list(got) == want
    assert all(got[i] == OK for i in clean)
    if m >= 4:
        assert any(got[i] != OK for i in range(m) if i % 7 == 3)
    assert info["last_chunks"] == 1 and info["last_launches"] == 4 and info["chunk"] == DEFAULT_CHUNK
    # the pairing-free verifier at the known tau, for eight indices
    verdict_of = {True: OK, False: INVALID, None: MALFORMED}
    for i in list(range(0, m, max(1, m // 8)))[:8] + [j for j in (3, 10, 17) if j < m]:
        pub_i = pubs[i]
        ref = None if any(x >= R for x in pub_i) else pp.verify(k.vk_ref, 3, pub_i, proofs[i], TAU)
        assert got[i] == verdict_of[ref], i


def test_every_tampered_kind_is_refused(zk, keys, expected):
    k = keys["small"]
    seen = set()
    for kind in range(KINDS):
        p, q = tamper(kind, k.proofs[0], k.case.publics, k.ref.points)
        seen.add(expected(p, q))
        assert expected(p, q) != OK, kind
    assert seen == {INVALID, MALFORMED}


@pytest.mark.parametrize("name", ["all_public", "large", "no_public"])
def test_verdicts_under_the_other_keys(zk, keys, name):
    k = keys[name]
    publics = k.case.publics
    proofs = list(k.proofs)
    pubs = [list(publics) for _ in proofs]
    bad = bytearray(proofs[0])
    bad[576 + 37] ^= 1                                   # a value changed
    proofs.append(bytes(bad))
    pubs.append(list(publics))
    if k.n_public:
        changed = list(publics)
        changed[-1] = (changed[-1] + 1) % R
        proofs.append(proofs[1])
        pubs.append(changed)
    with zk.PlonkVerifier(k.vk) as v:
        got = list(v.verify(proofs, pubs if k.n_public else None))
        if not k.n_public:
            assert list(v.verify(proofs)) == got and list(v.verify(proofs, [[] for _ in proofs])) == got
    want = [zk.plonk_verify(k.vk, p, q) for p, q in zip(proofs, pubs)]
    assert got == want
    assert got[:len(k.proofs)] == [OK] * len(k.proofs) and set(got[len(k.proofs):]) == {INVALID}
    assert pp.verify(pp.vkey_points(k.case.inst, TAU), k.log_n, publics, proofs[0], TAU) is True


# ---------------------------------------------------------------- the chunk does not matter
@pytest.mark.parametrize("m", [7, 130])
def test_the_chunk_changes_no_verdict(zk, keys, monkeypatch, m):
    k = keys["small"]
    proofs, pubs = [], []
    for i in range(m):
        good = k.proofs[i % len(k.proofs)]                   # every third is tampered: a changed value, a point off the curve, ..
        p, q = tamper((9 + 17 * (i // 3)) % KINDS, good, k.case.publics, k.ref.points) if i % 3 == 2 else (good, k.case.publics)
        proofs.append(p)
        pubs.append(list(q))
    with zk.PlonkVerifier(k.vk) as v:
        monkeypatch.delenv(KNOB, raising=False)
        want = list(v.verify(proofs, pubs))
        assert v.info()["last_chunks"] == 1 and set(want) == {OK, INVALID, MALFORMED}
        for chunk in (1, 3, 64):
            monkeypatch.setenv(KNOB, str(chunk))
            assert list(v.verify(proofs, pubs)) == want, chunk
            info = v.info()
            assert info["chunk"] == chunk and info["last_chunks"] == math.ceil(m / min(m, chunk))
            assert info["last_launches"] == 4 * info["last_chunks"]
            ch, st = v.challenges(proofs, pubs)
            assert [2 if x == MALFORMED else 0 for x in want] == list(st) and v.info()["last_launches"] == info["last_chunks"]
        for text in ("0", "1048577", "12x", "-3", " 5"):
            monkeypatch.setenv(KNOB, text)
            for call in (lambda: v.verify(proofs, pubs), lambda: v.challenges(proofs, pubs), v.info):
                with pytest.raises(zk.ZkHipError, match="^ZKHIP_PLONK_VERIFY_CHUNK: a number of proofs from 1 to 2\\^20 expected$"):
                    call()
        monkeypatch.delenv(KNOB)
        assert list(v.verify(proofs, pubs)) == want


# ---------------------------------------------------------------- the key alone is enough
def test_the_key_alone_is_enough(zk, ptau_path):
    c = pp.build(5003, 3, 2)
    own = zk.Kzg.from_ptau(ptau_path, max_coeffs=8 + 6)
    p = make_prover(zk, own, c)
    proof = p.prove(c.witness, c.publics)
    text = p.vkey().to_json()
    p.close()
    own.close()
    vk = zk.PlonkVKey.from_json(text)
    assert vk.kzg is None and vk.to_json() == text
    with pytest.raises(ValueError, match="the key names no Kzg .*PlonkVerifier"):
        zk.plonk_verify(vk, proof, c.publics)
    with zk.PlonkVerifier(vk) as v:
        assert list(v.verify([proof], [c.publics])) == [OK]
        assert list(v.verify([proof], [[c.publics[1], c.publics[0]]])) == [INVALID]
        info = v.info()
        assert info["log_n"] == 3 and info["n_public"] == 2 and info["device_bytes"] >= 2 * 66 * 192       # two line tables
    # one commitment moved by G: a good proof is INVALID under that key
    pts = [bn.g1_from_bytes(b) for b in vk.commitments.values()]
    pts[5] = bn.G1.add(pts[5], bn.G1_GEN)
    moved = zk.PlonkVKey.from_parts(3, 2, pi.K1, pi.K2, pts, vk.tau_g2)
    with zk.PlonkVerifier(moved) as v:
        assert list(v.verify([proof], [c.publics])) == [INVALID]


# ---------------------------------------------------------------- create
def test_tau_g2_is_checked(zk, keys):
    k = keys["small"]
    parts = list(k.vk.commitments.values())
    cof = golden_json("g2_cofactor_points.json")["outside"][1]
    outside = ((int(cof["x"][0]), int(cof["x"][1])), (int(cof["y"][0]), int(cof["y"][1])))
    off = bytearray(k.vk.tau_g2)
    off[64 + 7] ^= 4                                     # y changed: off the twist
    text = "zk_plonk_verifier_create: the key's \\[tau\\]G2 is not a point of the twist in the subgroup"
    for tau_g2 in (outside, bytes(off), None, Q.to_bytes(32, "little") + bytes(k.vk.tau_g2)[32:]):
        with pytest.raises(zk.ZkHipError, match=text):
            zk.PlonkVerifier(zk.PlonkVKey.from_parts(3, 2, pi.K1, pi.K2, parts, tau_g2))
    zk.PlonkVerifier(zk.PlonkVKey.from_parts(3, 2, pi.K1, pi.K2, parts, k.vk.tau_g2)).close()


def test_refusals(zk, keys):
    from rapidsnark_old_amd import lib as L
    lib = zk.load_library()
    k = keys["small"]
    parts = list(k.vk.commitments.values())

    def create(log_n=3, n_public=2, k1=pi.K1, commitments=parts, size=None):
        vk = zk.PlonkVKey.from_parts(log_n, n_public, k1, pi.K2, commitments, k.vk.tau_g2)
        if size is not None:
            vk._c.size = size
        h = ctypes.c_void_p()
        assert lib.zk_plonk_verifier_create(ctypes.byref(h), ctypes.byref(vk._c), -1) == 1 and not h
        return lib.zk_last_error().decode()

    assert create(size=8) == "zk_plonk_verifier_create: vk->size is not sizeof(zk_plonk_vkey)"
    assert create(log_n=2) == "zk_plonk_verifier_create: log_n 2 is outside 3 .. 25"
    assert create(log_n=26) == "zk_plonk_verifier_create: log_n 26 is outside 3 .. 25"
    assert create(n_public=9) == "zk_plonk_verifier_create: n_public 9 exceeds n = 8"
    assert create(k1=R) == "zk_plonk_verifier_create: k1 is not below r"
    assert create(commitments=parts[:3] + [(1, 3)] + parts[4:]) == "zk_plonk_verifier_create: a commitment of the key is not a point of the curve"
    assert lib.zk_plonk_verifier_create(None, ctypes.byref(k.vk._c), -1) == 1 and lib.zk_last_error().decode() == "null argument"
    h = ctypes.c_void_p()
    assert lib.zk_plonk_verifier_create(ctypes.byref(h), None, -1) == 1 and lib.zk_last_error().decode() == "null argument"
    P = lambda a: ctypes.c_void_p(a.ctypes.data)         # noqa: E731
    proof, pub = np.frombuffer(k.proofs[0], dtype=np.uint8).copy(), le(k.case.publics).copy()
    out, ch = np.full(1, 255, dtype=np.uint8), np.zeros(192, dtype=np.uint8)
    with zk.PlonkVerifier(k.vk) as v:
        hv = v._handle()
        for args in ((None, P(pub), 1, P(out)), (P(proof), None, 1, P(out)), (P(proof), P(pub), 1, None)):
            assert lib.zk_plonk_verifier_verify(hv, *args) == 1 and lib.zk_last_error().decode() == "null argument"
        assert lib.zk_plonk_verifier_challenges(hv, P(proof), P(pub), 1, None, P(out)) == 1 and lib.zk_last_error().decode() == "null argument"
        assert lib.zk_plonk_verifier_challenges(hv, P(proof), P(pub), 1, P(ch), None) == 1 and lib.zk_last_error().decode() == "null argument"
        assert lib.zk_plonk_verifier_verify(hv, P(proof), P(pub), 1 << 31, P(out)) == 1
        assert lib.zk_last_error().decode() == "zk_plonk_verifier_verify: m is not below 2^31"
        assert lib.zk_plonk_verifier_challenges(hv, P(proof), P(pub), 1 << 31, P(ch), P(out)) == 1
        assert lib.zk_last_error().decode() == "zk_plonk_verifier_challenges: m is not below 2^31"
        assert out[0] == 255 and lib.zk_plonk_verifier_verify(hv, P(proof), P(pub), 1, P(out)) == 0 and out[0] == OK
        plan = L.zk_plonk_verifier_plan()
        assert lib.zk_plonk_verifier_info(hv, ctypes.byref(plan)) == 1 and lib.zk_last_error().decode() == "zk_plonk_verifier_info: plan->size is not set"
        # Python's own: publics of the wrong count
        with pytest.raises(ValueError, match="publics\\[1\\]: 3 values, n_public = 2 expected"):
            v.verify(k.proofs[:2], [k.case.publics, k.case.publics + [1]])
        with pytest.raises(ValueError, match="publics: 1 rows for 2 proofs"):
            v.verify(k.proofs[:2], [k.case.publics])
        with pytest.raises(ValueError, match="publics: 2 rows of n_public = 2 values expected"):
            v.verify(k.proofs[:2])
        with pytest.raises(ValueError, match="a proof of 768 bytes expected, got 767"):
            v.verify([k.proofs[0][:-1]], [k.case.publics])
        with pytest.raises(ValueError, match="proofs: a uint8 array of m rows of 768 bytes expected"):
            v.verify(np.zeros((2, 767), dtype=np.uint8), [k.case.publics] * 2)
    with pytest.raises(zk.ZkHipError, match="the PlonkVerifier object is closed"):
        v.verify(k.proofs[:1], [k.case.publics])
    with pytest.raises(TypeError, match="a PlonkVKey expected"):
        zk.PlonkVerifier(None)
    with zk.PlonkVerifier(keys["no_public"].vk) as v:
        with pytest.raises(ValueError, match="publics: the key has no public inputs"):
            v.verify(keys["no_public"].proofs[:1], [[1]])


def test_no_proofs_and_a_second_call_leave_nothing_behind(zk, keys):
    k = keys["small"]
    bad, _ = tamper(26, k.proofs[1], k.case.publics, k.ref.points)
    with zk.PlonkVerifier(k.vk) as v:
        fresh = v.info()
        assert fresh["last_chunks"] == 0 and fresh["log_n"] == 3 and fresh["n_public"] == 2
        empty = v.verify([], [])
        assert empty.dtype == np.uint8 and empty.size == 0
        assert v.challenges([], []) [0] == [] and v.info()["device_bytes"] == fresh["device_bytes"]
        assert zk.load_library().zk_plonk_verifier_verify(v._handle(), None, None, 0, None) == 0
        first = list(v.verify([bad, k.proofs[0], k.proofs[1]], [k.case.publics] * 3))
        assert first == [MALFORMED, OK, OK]
        grown = v.info()["device_bytes"]
        assert grown > fresh["device_bytes"]
        assert list(v.verify([k.proofs[2], bad], [k.case.publics] * 2)) == [OK, MALFORMED]      # the malformed row of before is no one's now
        assert list(v.verify([k.proofs[0], k.proofs[1], bad], [k.case.publics] * 3)) == [OK, OK, MALFORMED]
        assert v.info()["device_bytes"] == grown
