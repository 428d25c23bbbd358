"""PLONK batch verification by random combination on the GPU (zk_plonk_verifier_verify_batch, zk_plonk_verifier_batch_sums).
The yardsticks: the groups' sums L and W are compared, byte for byte, with sum r_i L_i and sum r_i W_i made in Python integers
from the transcript of tests/plonk_prover_instance.py; the verdicts with zk_plonk_verifier_verify's, element by element;
the report with the counts the inputs were built to give; and a pair of wrong proofs built to cancel under given scalars
shows that the combined equation is what is evaluated.  The keys and proofs are made by the recipe of
tests/test_gpu_plonk_verifier.py: a trapdoor .ptau of power 12, four keys, a few proofs each, repeated to fill m."""
import ctypes
import random

import numpy as np
import pytest

import plonk_instance as pi
import plonk_prover_instance as pp
from oracle import bn254 as bn

pytestmark = pytest.mark.gpu

R, Q = bn.R_MOD, bn.Q_MOD
TAU, ALPHA, BETA = 0x1F3A9C5E77D1B2A49E0C6F5D3B8A17264C9E0F1D2B3A4958, 0x2B7E151628AED2A6ABF7158809CF4F3C, 0x3243F6A8885A308D313198A2E0370734
MAX_COEFFS = (1 << 11) + 6
OK, INVALID, MALFORMED = 0, 1, 2
GROUP, CHUNK = "ZKHIP_PLONK_VERIFY_GROUP", "ZKHIP_PLONK_VERIFY_CHUNK"
KINDS = 31
G = bn.G1


def le(values):
    return np.frombuffer(pi.le(values), dtype=np.uint8)


@pytest.fixture(scope="module")
def ptau_path(zk, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("plonk_verify_batch") / "p12.ptau")
    zk.write_trapdoor_ptau(12, TAU, ALPHA, BETA, path, prepared=False)
    return path


def make_prover(zk, kzg, c):
    return zk.PlonkProver(kzg, *[le(x) for x in c.inst.circuit("monomial")], pi.K1, pi.K2, *c.maps, c.n_witness, c.n_public)


class Key:
    """one circuit: its case, its key, a few proofs with drawn blinds, and a verifier (module-scoped)"""


@pytest.fixture(scope="module")
def keys(zk, ptau_path):
    out = {}
    kzg = zk.Kzg.from_ptau(ptau_path, max_coeffs=MAX_COEFFS)
    for name, seed, log_n, n_public, count in (("small", 5003, 3, 2, 11), ("all_public", 5116, 4, 16, 3), ("large", 5011, 11, 2, 3), ("no_public", 5203, 3, 0, 3)):
        k = Key()
        k.case = pp.build(seed, log_n, n_public)
        k.log_n, k.n_public = log_n, n_public
        prover = make_prover(zk, kzg, k.case)
        k.vk = zk.PlonkVKey.from_json(prover.vkey().to_json())           # the key alone: it names no Kzg
        k.proofs = [prover.prove(k.case.witness, k.case.publics if n_public else None).to_bytes() for _ in range(count)]
        prover.close()
        k.vk_pts = pp.vkey_points(k.case.inst, TAU)
        out[name] = k
    kzg.close()                                          # from here on the keys work alone
    for k in out.values():
        k.v = zk.PlonkVerifier(k.vk)
    yield out
    for k in out.values():
        k.v.close()


def tamper(kind, good, publics):
    """-> (proof bytes, publics) for one of the 31 kinds of tests/test_gpu_plonk_verifier.py; the two that change a public input
    change the last one, and a key without public inputs takes kinds 0 and 26 in their place"""
    publics = list(publics)
    if not publics and kind in (24, 30):
        kind = 0 if kind == 24 else 26
    if kind < 15:                                        # one byte of each field
        at = kind * 64 + 5 if kind < 9 else 576 + (kind - 9) * 32 + 5
        bad = bytearray(good)
        bad[at] ^= 0x10
        return bytes(bad), publics
    if kind < 24:                                        # P + G in place of P
        f = kind - 15
        P = bn.g1_from_bytes(good[f * 64:(f + 1) * 64])
        return good[:f * 64] + bn.g1_to_bytes(G.add(P, bn.G1_GEN)) + good[(f + 1) * 64:], publics
    if kind == 24:
        return good, publics[:-1] + [(publics[-1] + 1) % R]
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
    return good, publics[:-1] + [R]                      # a public input not below r


def filled(k, m, bad=None):
    """m proofs of key k, its few repeated; bad: {index: kind}"""
    proofs, pubs = [], []
    for i in range(m):
        p, q = k.proofs[i % len(k.proofs)], list(k.case.publics)
        if bad and i in bad:
            p, q = tamper(bad[i], p, q)
        proofs.append(p)
        pubs.append(q)
    return proofs, (pubs if k.n_public else None)


def launches_match(v, rep):
    info = v.info()
    assert info["last_launches"] == rep["launches"] and info["last_chunks"] == rep["chunks"]


# ---------------------------------------------------------------- the sums are exact
def l_and_w(k, publics, proof_bytes):
    """(L, W) of one well-formed proof from the Python transcript: e(L, G2) = e(W, [tau]G2) is its equation"""
    pts, ev = pp.parse(proof_bytes)
    n = 1 << k.log_n
    w = bn.fr_root(k.log_n)
    ch = pp.challenges(k.vk_pts, publics, pts, ev)
    al, be, ga, ze, v, u = ch.alpha, ch.beta, ch.gamma, ch.zeta, ch.v, ch.u
    a, b, c, s1, s2, zw = ev
    pi_v = [(R - p) % R for p in publics] + [0] * (n - len(publics))
    r0 = pp.po.r0_of(n, ev, ze, al, be, ga, pi.horner(bn.ntt(pi_v, inverse=True), ze))
    l1, zh = pp.po._l1_zh(n, ze)
    zn = pow(ze, n, R)
    qm, ql, qr, qo, qc, c1, c2, c3 = k.vk_pts
    A, B, C, Z, TLO, TMID, THI, WZ, WZW = pts
    f = (a + be * ze + ga) * (b + be * pp.K1 * ze + ga) % R * (c + be * pp.K2 * ze + ga) % R
    g = (a + be * s1 + ga) * (b + be * s2 + ga) % R
    e = (r0 + sum(pow(v, j + 1, R) * ev[j] for j in range(5)) + u * zw) % R
    terms = ((qm, a * b), (ql, a), (qr, b), (qo, c), (qc, 1), (Z, al * f + al * al * l1 + u), (c3, -(al * g % R * be % R * zw)), (TLO, -zh),
             (TMID, -zh * zn), (THI, -zh * zn % R * zn), (A, v), (B, pow(v, 2, R)), (C, pow(v, 3, R)), (c1, pow(v, 4, R)), (c2, pow(v, 5, R)),
             (bn.G1_GEN, -e), (WZ, ze), (WZW, u * ze % R * w))
    L = None
    for P, s in terms:
        L = G.add(L, G.mul(P, s % R))
    return L, G.add(WZ, G.mul(WZW, u))


def combined(k, rows, scalars):
    """(sum r L, sum r W) as bytes over rows of (publics, proof bytes)"""
    L = W = None
    for (publics, proof), r in zip(rows, scalars):
        Li, Wi = l_and_w(k, publics, proof)
        L, W = G.add(L, G.mul(Li, r)), G.add(W, G.mul(Wi, r))
    return bn.g1_to_bytes(L), bn.g1_to_bytes(W)


def test_sums_are_exact(keys, monkeypatch):
    k = keys["small"]
    monkeypatch.setenv(GROUP, "2")
    proofs, pubs = filled(k, 5, {1: 26, 3: 25})          # 1: a point off the curve; 3: W_zeta_omega at infinity, still a proof
    scalars = [3, (1 << 128) - 1, 0x0123456789ABCDEF0FEDCBA987654321, 1, (1 << 127) + 5]
    assert pp.parse(proofs[1]) is None and pp.parse(proofs[3])[0][8] is None
    got = k.v.batch_sums(proofs, pubs, scalars)
    rows = list(zip(pubs, proofs))
    want = [combined(k, [rows[0]], scalars[:1]),         # the malformed proof 1 is left out of its group
            combined(k, rows[2:4], scalars[2:4]), combined(k, rows[4:], scalars[4:])]
    assert got == want
    assert k.v.batch_sums(proofs, pubs, b"".join(s.to_bytes(16, "little") for s in scalars)) == want
    # a group of malformed proofs alone: 128 zero bytes, and the others as before
    proofs[0] = proofs[1]
    assert k.v.batch_sums(proofs, pubs, scalars) == [(bytes(64), bytes(64))] + want[1:]
    verdicts, rep = k.v.verify_batch(proofs, pubs, scalars)
    assert list(verdicts) == [MALFORMED, MALFORMED, OK, INVALID, OK] == list(k.v.verify(proofs, pubs))
    assert (rep["groups"], rep["groups_failed"], rep["proofs_rechecked"], rep["malformed"], rep["group"]) == (2, 1, 2, 2, 2)


# ---------------------------------------------------------------- the verdicts are verify's
CASES = [(name, m) for name in ("small", "no_public", "all_public", "large") for m in (1, 2, 63, 64, 65)] + [("small", 200), ("small", 257)]


@pytest.mark.parametrize("name,m", CASES)
def test_verdicts_are_verifys(keys, monkeypatch, name, m):
    """index i = 3 (mod 7) is tampered, kind (5 m + i // 7) mod 31; the scalars are drawn"""
    monkeypatch.delenv(GROUP, raising=False)
    monkeypatch.delenv(CHUNK, raising=False)
    k = keys[name]
    proofs, pubs = filled(k, m, {i: (5 * m + i // 7) % KINDS for i in range(3, m, 7)})
    want = list(k.v.verify(proofs, pubs))
    got, rep = k.v.verify_batch(proofs, pubs)
    assert got.dtype == np.uint8 and list(got) == want
    assert all(want[i] == OK for i in range(m) if i % 7 != 3) and all(want[i] != OK for i in range(3, m, 7))
    assert rep["malformed"] == want.count(MALFORMED) and rep["groups"] == 1 and rep["chunks"] == 1 and rep["group"] == m
    assert rep["groups_failed"] == (1 if INVALID in want else 0)
    assert rep["proofs_rechecked"] == (m - want.count(MALFORMED) if INVALID in want else 0)
    launches_match(k.v, rep)


# ---------------------------------------------------------------- the report
def test_the_report_counts(keys, monkeypatch):
    k = keys["small"]
    monkeypatch.setenv(GROUP, "64")
    monkeypatch.delenv(CHUNK, raising=False)

    def run(m, bad):
        proofs, pubs = filled(k, m, bad)
        verdicts, rep = k.v.verify_batch(proofs, pubs)
        launches_match(k.v, rep)
        assert list(verdicts) == [(MALFORMED if bad[i] == 26 else INVALID) if i in bad else OK for i in range(m)]
        return rep["group"], rep["groups"], rep["groups_failed"], rep["proofs_rechecked"], rep["malformed"], rep["chunks"]

    assert run(130, {}) == (64, 3, 0, 0, 0, 1)
    assert run(130, {70: 12}) == (64, 3, 1, 64, 0, 1)    # 12: a value changed
    assert run(130, {70: 12, 100: 26}) == (64, 3, 1, 63, 1, 1)
    assert run(130, {129: 17}) == (64, 3, 1, 2, 0, 1)    # the short last group
    monkeypatch.setenv(GROUP, "2")
    assert run(8, {4: 26, 5: 26}) == (2, 3, 0, 0, 2, 1)  # a group of malformed proofs alone is not counted
    assert run(8, {4: 26, 5: 26, 7: 20}) == (2, 3, 1, 2, 2, 1)


# ---------------------------------------------------------------- groups and chunks
def groups_of_call(m, chunk, group):
    """csrc/plonk_batch_dev.hpp's pb_groups_of_call, which tools/plonk_batch_host_test.cpp checks on these triples"""
    cap = min(m, chunk)
    g = min(group, cap)
    return sum(-(-min(cap, m - off) // g) for off in range(0, m, cap))


def test_groups_and_chunks_change_no_verdict(keys, monkeypatch):
    k = keys["small"]
    m = 130
    proofs, pubs = filled(k, m, {i: (9 + 17 * (i // 3)) % KINDS for i in range(2, m, 3)})
    monkeypatch.delenv(GROUP, raising=False)
    monkeypatch.delenv(CHUNK, raising=False)
    want = list(k.v.verify(proofs, pubs))
    assert set(want) == {OK, INVALID, MALFORMED}
    assert [groups_of_call(m, c, g) for c, g in ((65536, 1), (65536, 3), (100, 64), (64, 64), (7, 1000))] == [130, 44, 3, 3, 19]
    for chunk, group in ((65536, 1), (65536, 3), (100, 64), (64, 64), (7, 1000)):
        monkeypatch.setenv(CHUNK, str(chunk))
        monkeypatch.setenv(GROUP, str(group))
        got, rep = k.v.verify_batch(proofs, pubs)
        assert list(got) == want, (chunk, group)
        cap = min(m, chunk)
        g = min(group, cap)
        # the groups with a well-formed proof among those the call forms
        formed = [(off + lo, min(off + lo + g, off + cap, m)) for off in range(0, m, cap) for lo in range(0, min(cap, m - off), g)]
        assert len(formed) == groups_of_call(m, chunk, group)
        live = [any(want[i] != MALFORMED for i in range(lo, hi)) for lo, hi in formed]
        failed = [any(want[i] == INVALID for i in range(lo, hi)) for lo, hi in formed]
        assert (rep["groups"], rep["groups_failed"], rep["chunks"], rep["group"]) == (sum(live), sum(failed), -(-m // cap), g), (chunk, group)
        assert rep["proofs_rechecked"] == sum(sum(want[i] != MALFORMED for i in range(lo, hi)) for (lo, hi), f in zip(formed, failed) if f)
        launches_match(k.v, rep)
        if (chunk, group) == (100, 64):                  # a group ends at the chunk
            assert formed == [(0, 64), (64, 100), (100, 130)]


# ---------------------------------------------------------------- the combination is what is evaluated
def test_errors_that_cancel_pass_as_a_group(keys, monkeypatch):
    k = keys["small"]
    monkeypatch.delenv(GROUP, raising=False)
    monkeypatch.delenv(CHUNK, raising=False)
    publics = list(k.case.publics)
    pubs = [publics, publics]
    good = [k.proofs[1], k.proofs[2]]
    r1, r2 = 0x9E3779B97F4A7C15F39CC0605CEDC835, 0x0000000000000001000000000000002B

    def shifted(proof, d):                               # W_zeta + d G
        P = bn.g1_from_bytes(proof[7 * 64:8 * 64])
        return proof[:7 * 64] + bn.g1_to_bytes(G.add(P, G.mul(bn.G1_GEN, d % R))) + proof[8 * 64:]

    ch, status = k.v.challenges(good, pubs)
    z1, z2 = ch[0][3], ch[1][3]                          # zeta: the W's do not enter it
    d1 = 1
    d2 = (-r1 * (z1 - TAU) * d1) * pow(r2 * (z2 - TAU), -1, R) % R
    bad = [shifted(good[0], d1), shifted(good[1], d2)]
    ch_bad, _ = k.v.challenges(bad, pubs)
    assert [c[3] for c in ch_bad] == [z1, z2] and list(status) == [0, 0]
    # the construction cancels, by the Python transcript alone: each proof fails its own equation, the combination holds
    assert (r1 * (z1 - TAU) * d1 + r2 * (z2 - TAU) * d2) % R == 0
    lw = [l_and_w(k, publics, p) for p in bad]
    assert all(L != G.mul(W, TAU) for L, W in lw)
    Lc = G.add(G.mul(lw[0][0], r1), G.mul(lw[1][0], r2))
    Wc = G.add(G.mul(lw[0][1], r1), G.mul(lw[1][1], r2))
    assert Lc == G.mul(Wc, TAU)
    assert G.add(G.mul(lw[0][0], r1), G.mul(lw[1][0], r2 + 1)) != G.mul(G.add(G.mul(lw[0][1], r1), G.mul(lw[1][1], r2 + 1)), TAU)

    assert list(k.v.verify(bad, pubs)) == [INVALID, INVALID]
    verdicts, rep = k.v.verify_batch(bad, pubs, [r1, r2])
    assert list(verdicts) == [OK, OK] and (rep["groups"], rep["groups_failed"], rep["proofs_rechecked"]) == (1, 0, 0)
    (Lb, Wb), = k.v.batch_sums(bad, pubs, [r1, r2])
    assert (Lb, Wb) == (bn.g1_to_bytes(Lc), bn.g1_to_bytes(Wc)) and bn.g1_from_bytes(Lb) == G.mul(bn.g1_from_bytes(Wb), TAU)
    for scalars in (None, [r1, r2 + 1]):
        verdicts, rep = k.v.verify_batch(bad, pubs, scalars)
        assert list(verdicts) == [INVALID, INVALID] and (rep["groups"], rep["groups_failed"], rep["proofs_rechecked"]) == (1, 1, 2)
    # in groups of their own each is judged alone
    monkeypatch.setenv(GROUP, "1")
    verdicts, rep = k.v.verify_batch(bad, pubs, [r1, r2])
    assert list(verdicts) == [INVALID, INVALID] and rep["groups_failed"] == 2


# ---------------------------------------------------------------- refusals and edges
def test_refusals_and_edges(zk, keys, monkeypatch):
    from rapidsnark_old_amd import lib as L
    lib = zk.load_library()
    k = keys["small"]
    monkeypatch.delenv(GROUP, raising=False)
    monkeypatch.delenv(CHUNK, raising=False)
    proofs, pubs = filled(k, 5, {2: 12})
    before = list(k.v.verify(proofs, pubs))
    assert before == [OK, OK, INVALID, OK, OK]
    # a zero scalar is refused by name, through the C entry
    P = lambda a: ctypes.c_void_p(a.ctypes.data)         # noqa: E731
    a = np.frombuffer(b"".join(proofs), dtype=np.uint8).copy()
    pb = np.concatenate([le(q) for q in pubs]).copy()
    out = np.full(5, 255, dtype=np.uint8)
    sc = np.frombuffer(b"".join(s.to_bytes(16, "little") for s in (1, 2, 3, 0, 5)), dtype=np.uint8).copy()
    hv = k.v._handle()
    assert lib.zk_plonk_verifier_verify_batch(hv, P(a), P(pb), 5, P(sc), P(out), None) == 1
    assert lib.zk_last_error().decode() == "zk_plonk_verifier_verify_batch: scalar 3 is zero" and list(out) == [255] * 5
    n = ctypes.c_uint64(0)
    sums = np.zeros(5 * 128, dtype=np.uint8)
    assert lib.zk_plonk_verifier_batch_sums(hv, P(a), P(pb), 5, P(sc), P(sums), 5, ctypes.byref(n)) == 1
    assert lib.zk_last_error().decode() == "zk_plonk_verifier_batch_sums: scalar 3 is zero"
    sc[48] = 9
    assert lib.zk_plonk_verifier_verify_batch(hv, P(a), P(pb), 1 << 31, P(sc), P(out), None) == 1
    assert lib.zk_last_error().decode() == "zk_plonk_verifier_verify_batch: m is not below 2^31"
    monkeypatch.setenv(GROUP, "2")
    assert lib.zk_plonk_verifier_batch_sums(hv, P(a), P(pb), 5, P(sc), P(sums), 2, ctypes.byref(n)) == 1
    assert lib.zk_last_error().decode() == "zk_plonk_verifier_batch_sums: sums_cap 2 is below the call's 3 groups"
    monkeypatch.delenv(GROUP)
    for args in ((None, P(pb), 5, None, P(out), None), (P(a), None, 5, None, P(out), None), (P(a), P(pb), 5, None, None, None)):
        assert lib.zk_plonk_verifier_verify_batch(hv, *args) == 1 and lib.zk_last_error().decode() == "null argument"
    rep = L.zk_plonk_batch_report()
    rep.size = ctypes.sizeof(rep)
    assert lib.zk_plonk_verifier_verify_batch(hv, P(a), P(pb), 5, P(sc), P(out), ctypes.byref(rep)) == 0 and list(out) == before
    assert (rep.size, rep.group, rep.groups, rep.groups_failed, rep.proofs_rechecked, rep.malformed, rep.chunks) == (48, 5, 1, 1, 5, 0, 1)
    # m = 0: an empty result and a zeroed report
    verdicts, rep0 = k.v.verify_batch([], [])
    assert verdicts.dtype == np.uint8 and verdicts.size == 0
    assert rep0 == {"group": 65536, "groups": 0, "groups_failed": 0, "proofs_rechecked": 0, "malformed": 0, "launches": 0, "chunks": 0}
    assert lib.zk_plonk_verifier_verify_batch(hv, None, None, 0, None, None, None) == 0
    assert k.v.batch_sums([], [], []) == []
    # the group knob
    for text in ("0", "abc", str((1 << 20) + 1), " 5", "-3"):
        monkeypatch.setenv(GROUP, text)
        for call in (lambda: k.v.verify_batch(proofs, pubs), lambda: k.v.batch_sums(proofs, pubs, [1] * 5), lambda: k.v.verify_batch([], [])):
            with pytest.raises(zk.ZkHipError, match="^ZKHIP_PLONK_VERIFY_GROUP: a number of proofs from 1 to 2\\^20 expected$"):
                call()
        assert list(k.v.verify(proofs, pubs)) == before  # verify does not read it
    monkeypatch.setenv(GROUP, str(1 << 20))
    assert list(k.v.verify_batch(proofs, pubs)[0]) == before
    monkeypatch.delenv(GROUP)
    # the same scalars twice: the same verdicts and report
    scalars = [random.Random(77).randrange(1, 1 << 128) for _ in range(5)]
    first = k.v.verify_batch(proofs, pubs, scalars)
    second = k.v.verify_batch(proofs, pubs, scalars)
    assert list(first[0]) == list(second[0]) == before and first[1] == second[1]
    # verify after verify_batch: what it gave before, four launches a chunk
    assert list(k.v.verify(proofs, pubs)) == before
    info = k.v.info()
    assert info["last_launches"] == 4 and info["last_chunks"] == 1
    monkeypatch.setenv(CHUNK, "2")
    assert list(k.v.verify(proofs, pubs)) == before
    info = k.v.info()
    assert info["last_launches"] == 12 and info["last_chunks"] == 3
    # the batch buffers count in device_bytes
    with zk.PlonkVerifier(k.vk) as fresh:
        assert list(fresh.verify(proofs, pubs)) == before
        held = fresh.info()["device_bytes"]
        assert list(fresh.verify_batch(proofs, pubs)[0]) == before
        assert fresh.info()["device_bytes"] > held
    with pytest.raises(zk.ZkHipError, match="the PlonkVerifier object is closed"):
        fresh.verify_batch(proofs, pubs)


def test_the_key_works_alone(zk, keys):
    """every key here was read back from its file's text and the Kzg that made it is closed: the verifier needs neither"""
    for k in keys.values():
        assert k.vk.kzg is None
    k = keys["no_public"]
    verdicts, rep = k.v.verify_batch(k.proofs)
    assert list(verdicts) == [OK] * len(k.proofs) and (rep["groups"], rep["groups_failed"]) == (1, 0)
    assert list(k.v.verify_batch(k.proofs, [[] for _ in k.proofs])[0]) == [OK] * len(k.proofs)
