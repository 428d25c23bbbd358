"""The PLONK verifier over a key set on the GPU (zk_plonk_verifier_set_*, PlonkVerifierSet).  The yardsticks: every verdict of
set.verify is the one the single-key PlonkVerifier of the proof's key gives, proof by proof; the launches of a call depend
on its chunks alone; the groups' sums L and W of set.batch_sums are compared, byte for byte, with sum r_i L_i and sum r_i W_i
made in Python integers from the transcript of tests/plonk_prover_instance.py, over groups formed by a restatement of the
ordering rule (a chunk's proofs by key, keys rising, then consecutive groups); the batch verdicts and the report with the
counts the inputs were built to give.  Keys and proofs are those of tests/test_gpu_plonk_verify_batch.py, whose fixture and
helpers this file imports: a trapdoor .ptau of power 12, four keys over one Kzg, a few proofs each, repeated to fill m.
The set holds five entries: (log_n 3, 2 publics), (4, 16, all public), (3, 0), (11, 2), and the first key's struct again."""
import ctypes
import random

import numpy as np
import pytest

from oracle import bn254 as bn
from test_gpu_plonk_verify_batch import CHUNK, GROUP, INVALID, MALFORMED, OK, R, G, keys, l_and_w, le, ptau_path, tamper  # noqa: F401

pytestmark = pytest.mark.gpu

NAMES = ["small", "all_public", "no_public", "large", "small"]
N_PUBLIC = [2, 16, 0, 2, 2]
CORRUPT, PUBLIC_IS_R, FLIPPED, INFINITY = 26, 30, 12, 25     # kinds of tamper()


@pytest.fixture(scope="module")
def kset(zk, keys):
    with zk.PlonkVerifierSet([keys[n].vk for n in NAMES]) as s:
        assert s.n_public == N_PUBLIC
        yield s


def build(keys, entries, bad=None, proof_of=None):
    """(proofs, publics rows) for proofs labelled entries[i]; bad: {index: kind of tamper()}; proof_of: {index: the entry whose
    proof and publics stand there instead}"""
    proofs, pubs = [], []
    for i, e in enumerate(entries):
        k = keys[NAMES[proof_of[i] if proof_of and i in proof_of else e]]
        p, q = k.proofs[(i // 3) % len(k.proofs)], list(k.case.publics)
        if bad and i in bad:
            p, q = tamper(bad[i], p, q)
        proofs.append(p)
        pubs.append(q)
    return proofs, pubs


def single_key_verdicts(keys, proofs, entries, pubs):
    """what PlonkVerifier(key).verify gives every proof under the key it is labelled with, a call a key"""
    want = [None] * len(entries)
    for e in sorted(set(entries)):
        at = [i for i in range(len(entries)) if entries[i] == e]
        k = keys[NAMES[e]]
        got = k.v.verify([proofs[i] for i in at], [pubs[i] for i in at] if k.n_public else None)
        for i, v in zip(at, got):
            want[i] = int(v)
    return want


def groups_of(entries, chunk, group):
    """the rule restated: per chunk of min(m, chunk) proofs the positions by (key, position), cut into consecutive groups"""
    m = len(entries)
    cap = min(m, chunk)
    g = min(group, cap)
    out = []
    for off in range(0, m, cap):
        order = sorted(range(off, min(off + cap, m)), key=lambda i: (entries[i], i))
        out += [order[lo:lo + g] for lo in range(0, len(order), g)]
    return out


INTERLEAVED = [(0, 1, 3, 4)[(i * 7 + i // 5) % 4] for i in range(70)]          # entry 2 gets no proof


def tampered_70(keys):
    bad = {5: CORRUPT, 13: PUBLIC_IS_R, 22: FLIPPED, 44: INFINITY, 61: PUBLIC_IS_R}
    assert INTERLEAVED[13] == 1 and INTERLEAVED[61] == 4 and INTERLEAVED[32] == 3   # 13: the last of 16 publics, behind narrower rows
    proofs, pubs = build(keys, INTERLEAVED, bad, proof_of={32: 0})                 # 32: a valid proof of key 0 labelled key 3
    return proofs, pubs, bad


# ---------------------------------------------------------------- per-proof verdicts
@pytest.mark.parametrize("chunk", [None, 7])
def test_verdicts_are_the_single_key_verifiers(keys, kset, monkeypatch, chunk):
    monkeypatch.delenv(GROUP, raising=False)
    monkeypatch.delenv(CHUNK, raising=False)
    proofs, pubs, bad = tampered_70(keys)
    want = single_key_verdicts(keys, proofs, INTERLEAVED, pubs)
    assert [want[i] for i in (5, 13, 22, 32, 44, 61)] == [MALFORMED, MALFORMED, INVALID, INVALID, INVALID, MALFORMED]
    assert all(want[i] == OK for i in range(70) if i not in bad and i != 32)
    if chunk:
        monkeypatch.setenv(CHUNK, str(chunk))
    got = kset.verify(proofs, INTERLEAVED, pubs)
    assert got.dtype == np.uint8 and list(got) == want
    info = kset.info()
    assert (info["last_chunks"], info["last_launches"]) == ((10, 40) if chunk else (1, 4))
    assert info["n_keys"] == 5 and info["max_n_public"] == 16 and info["chunk"] == (chunk or 65536)
    # the flat ragged bytes are the rows back to back
    flat = b"".join(int(v).to_bytes(32, "little") for row in pubs for v in row)
    assert list(kset.verify(np.frombuffer(b"".join(proofs), dtype=np.uint8).reshape(70, 768), INTERLEAVED, flat)) == want
    # every entry, the key without publics among them
    entries = [4, 2, 1, 2, 0, 3, 2, 1, 4]
    proofs, pubs = build(keys, entries, {3: FLIPPED, 7: CORRUPT})
    want = single_key_verdicts(keys, proofs, entries, pubs)
    assert want == [OK, OK, OK, INVALID, OK, OK, OK, MALFORMED, OK]
    assert list(kset.verify(proofs, entries, pubs)) == want
    assert list(kset.verify(proofs[1:2], [2], None)) == [OK]                       # no publics at all: NULL


def test_launches_depend_on_the_chunks_alone(keys, kset, monkeypatch):
    monkeypatch.delenv(CHUNK, raising=False)
    one, spread = [0] * 20, [(0, 1, 2, 3)[i % 4] for i in range(20)]
    counts = {}
    for chunk in (None, 7):
        if chunk:
            monkeypatch.setenv(CHUNK, str(chunk))
        for name, entries in (("one", one), ("spread", spread)):
            proofs, pubs = build(keys, entries)
            assert list(kset.verify(proofs, entries, pubs)) == [OK] * 20
            info = kset.info()
            counts[name, chunk] = (info["last_launches"], info["last_chunks"])
    assert counts["one", None] == counts["spread", None] == (4, 1)
    assert counts["one", 7] == counts["spread", 7] == (12, 3)


# ---------------------------------------------------------------- errors of the call
def test_errors_of_the_call(zk, keys, kset, monkeypatch):
    from rapidsnark_old_amd import lib as L
    lib = zk.load_library()
    monkeypatch.delenv(GROUP, raising=False)
    monkeypatch.delenv(CHUNK, raising=False)
    entries = [0, 1, 2, 3, 4]
    proofs, pubs = build(keys, entries)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)         # noqa: E731
    err = lambda: lib.zk_last_error().decode()           # noqa: E731
    a = np.frombuffer(b"".join(proofs), dtype=np.uint8).copy()
    pb = np.concatenate([le(q) for q in pubs if q]).copy()
    ko = np.array(entries, dtype=np.uint32)
    out = np.full(5, 255, dtype=np.uint8)
    h = kset._handle()
    assert pb.size == 22 * 32
    assert lib.zk_plonk_verifier_set_verify(h, P(a), P(ko), P(pb), pb.size, 5, P(out)) == 0 and list(out) == [OK] * 5
    out[:] = 255
    far = np.array([0, 1, 7, 9, 4], dtype=np.uint32)
    rep = L.zk_plonk_set_batch_report()
    rep.size = ctypes.sizeof(rep)
    n = ctypes.c_uint64(0)
    sums = np.zeros(5 * 128, dtype=np.uint8)
    sc = np.frombuffer(b"".join(s.to_bytes(16, "little") for s in (1, 2, 3, 0, 5)), dtype=np.uint8).copy()
    calls = (("zk_plonk_verifier_set_verify", lambda k, q, qb, m, s: lib.zk_plonk_verifier_set_verify(h, P(a), k, q, qb, m, P(out))),
             ("zk_plonk_verifier_set_verify_batch", lambda k, q, qb, m, s: lib.zk_plonk_verifier_set_verify_batch(h, P(a), k, q, qb, m, s, P(out), ctypes.byref(rep))),
             ("zk_plonk_verifier_set_batch_sums", lambda k, q, qb, m, s: lib.zk_plonk_verifier_set_batch_sums(h, P(a), k, q, qb, m, s, P(sums), 5, ctypes.byref(n))))
    for who, call in calls:
        assert call(P(far), P(pb), pb.size, 5, None) == 1 and err() == who + ": key_of[2] = 7, the set holds 5 keys"
        assert call(P(ko), P(pb), pb.size - 32, 5, None) == 1 and err() == who + ": publics_bytes: 704 expected (22 values of 32 bytes), 672 given"
        assert call(P(ko), P(pb), pb.size, 1 << 31, None) == 1 and err() == who + ": m is not below 2^31"
        assert call(None, P(pb), pb.size, 5, None) == 1 and err() == "null argument"
        assert call(P(ko), None, pb.size, 5, None) == 1 and err() == "null argument"
        assert call(P(ko), None, 0, 0, None) == 0                                  # m = 0: nothing is read
        if who != "zk_plonk_verifier_set_verify":
            assert call(P(ko), P(pb), pb.size, 5, P(sc)) == 1 and err() == who + ": scalar 3 is zero"
    assert list(out) == [255] * 5
    assert lib.zk_plonk_verifier_set_verify(h, None, P(ko), P(pb), pb.size, 5, P(out)) == 1 and err() == "null argument"
    assert lib.zk_plonk_verifier_set_verify(h, P(a), P(ko), P(pb), pb.size, 5, None) == 1 and err() == "null argument"
    sc[48] = 9
    monkeypatch.setenv(GROUP, "2")
    assert lib.zk_plonk_verifier_set_batch_sums(h, P(a), P(ko), P(pb), pb.size, 5, P(sc), P(sums), 2, ctypes.byref(n)) == 1
    assert err() == "zk_plonk_verifier_set_batch_sums: sums_cap 2 is below the call's 3 groups"
    monkeypatch.delenv(GROUP)
    # m = 0 through the class: empty results, a zeroed report
    assert kset.verify([], []).size == 0
    verdicts, rep0 = kset.verify_batch([], [])
    assert verdicts.size == 0 and rep0 == {"group": 65536, "launches": 0, "chunks": 0, "groups": 0, "groups_failed": 0, "segments": 0, "proofs_rechecked": 0,
                                           "malformed": 0}
    assert kset.batch_sums([], [], [], []) == []
    # the knobs keep their errors
    for name, text in ((CHUNK, "0"), (CHUNK, "abc"), (GROUP, " 5"), (GROUP, str((1 << 20) + 1))):
        monkeypatch.setenv(name, text)
        with pytest.raises(zk.ZkHipError, match="^%s: a number of proofs from 1 to 2\\^20 expected$" % name):
            kset.verify_batch(proofs, entries, pubs)
        if name == CHUNK:
            with pytest.raises(zk.ZkHipError, match="^%s: a number of proofs from 1 to 2\\^20 expected$" % name):
                kset.verify(proofs, entries, pubs)
        monkeypatch.delenv(name)
    # creation: keys over two [tau]G2
    other = L.zk_plonk_vkey.from_buffer_copy(bytes(keys["large"].vk._c))
    other.tau_g2[0] ^= 1                                 # the bytes are compared before a device is touched
    vks = [keys["small"].vk, keys["all_public"].vk, keys["no_public"].vk, zk.PlonkVKey(None, other)]
    with pytest.raises(zk.ZkHipError, match="^zk_plonk_verifier_set_create: key 3's \\[tau\\]G2 is not key 0's$"):
        zk.PlonkVerifierSet(vks)
    # a closed set
    with zk.PlonkVerifierSet(vks[:3]) as fresh:
        assert list(fresh.verify(proofs[:3], [0, 1, 2], pubs[:3])) == [OK] * 3
        held = fresh.info()["device_bytes"]
        assert list(fresh.verify_batch(proofs[:3], [0, 1, 2], pubs[:3])[0]) == [OK] * 3
        assert fresh.info()["device_bytes"] > held       # the batch buffers count
    with pytest.raises(zk.ZkHipError, match="the PlonkVerifierSet object is closed"):
        fresh.verify(proofs[:3], [0, 1, 2], pubs[:3])


# ---------------------------------------------------------------- batch: the sums are exact
_LW = {}


def lw_of(keys, entry, publics, proof):
    """l_and_w of tests/test_gpu_plonk_verify_batch.py, once a distinct (key, publics, proof)"""
    at = (NAMES[entry], tuple(publics), proof)
    if at not in _LW:
        _LW[at] = l_and_w(keys[NAMES[entry]], publics, proof)
    return _LW[at]


def expected_sums(keys, proofs, entries, pubs, scalars, want, chunk, group):
    """(L, W) bytes a group: sum r_i L_i and sum r_i W_i over the group's well-formed proofs, each under its own key; the
    scalars of equal proofs are added first, which changes no sum"""
    out = []
    for members in groups_of(entries, chunk, group):
        by_proof = {}
        for i in members:
            if want[i] != MALFORMED:
                at = (entries[i], tuple(pubs[i]), proofs[i])
                by_proof[at] = (by_proof.get(at, 0) + scalars[i]) % R
        if not by_proof:
            out.append((bytes(64), bytes(64)))
            continue
        L = W = None
        for (e, q, p), r in by_proof.items():
            Li, Wi = lw_of(keys, e, list(q), p)
            L, W = G.add(L, G.mul(Li, r)), G.add(W, G.mul(Wi, r))
        out.append((bn.g1_to_bytes(L), bn.g1_to_bytes(W)))
    return out


def test_sums_are_exact(keys, kset, monkeypatch):
    rng = random.Random(4242)
    # 23 proofs over all five entries; 8 and 9 are the only proofs of entry 2 that land in one group of 5 under chunk 7 and both
    # are malformed there, so that segment's eight sums are 0; 14 holds a point at infinity, 17 is INVALID and takes part
    entries = [3, 0, 4, 1, 0, 3, 1, 4, 2, 2, 0, 1, 3, 4, 0, 2, 1, 3, 0, 4, 1, 2, 3]
    proofs, pubs = build(keys, entries, {8: CORRUPT, 9: 27, 14: INFINITY, 17: FLIPPED, 20: PUBLIC_IS_R})
    scalars = [1, (1 << 128) - 1, 2, 1 << 127] + [rng.randrange(1, 1 << 128) for _ in range(19)]
    want = single_key_verdicts(keys, proofs, entries, pubs)
    assert [want[i] for i in (8, 9, 14, 17, 20)] == [MALFORMED, MALFORMED, INVALID, INVALID, MALFORMED]
    for chunk, group in ((7, 5), (65536, 65536), (65536, 1)):
        monkeypatch.setenv(CHUNK, str(chunk))
        monkeypatch.setenv(GROUP, str(group))
        formed = groups_of(entries, chunk, group)
        if (chunk, group) == (7, 5):
            assert len(formed) == 7 and [8, 9] == [i for i in formed[2] if entries[i] == 2]       # chunk 7 .. 13: a segment of malformed proofs alone
            assert any(len({entries[i] for i in g}) >= 3 for g in formed)
        got = kset.batch_sums(proofs, entries, pubs, scalars)
        assert got == expected_sums(keys, proofs, entries, pubs, scalars, want, chunk, group), (chunk, group)
        if group == 1:
            assert got[[g[0] for g in formed].index(8)] == (bytes(64), bytes(64))                 # a group of a malformed proof alone
        verdicts, rep = kset.verify_batch(proofs, entries, pubs, scalars)
        assert list(verdicts) == want, (chunk, group)
        live = [[i for i in g if want[i] != MALFORMED] for g in formed]
        failed = [g for g in live if any(want[i] == INVALID for i in g)]
        assert rep == {"group": min(group, chunk, 23), "launches": kset.info()["last_launches"], "chunks": -(-23 // min(chunk, 23)),
                       "groups": sum(1 for g in live if g), "groups_failed": len(failed), "segments": sum(len({entries[i] for i in g}) for g in live),
                       "proofs_rechecked": sum(len(g) for g in failed), "malformed": 3}, (chunk, group)


def test_sums_across_the_fold_s_borders(keys, kset, monkeypatch):
    """a segment of 300 proofs (two workgroups of the first pass) and two of 150 in ONE group of 600 (three workgroups for the
    generator's term): the second pass adds workgroup sums; valid proofs repeated"""
    monkeypatch.delenv(CHUNK, raising=False)
    monkeypatch.setenv(GROUP, "600")
    rng = random.Random(600)
    entries = [(0, 3, 4, 0)[i % 4] for i in range(600)]                            # 300 of entry 0, 150 of 3, 150 of 4, interleaved
    proofs, pubs = build(keys, entries)
    scalars = [rng.randrange(1, 1 << 128) for _ in range(600)]
    want = [OK] * 600
    got = kset.batch_sums(proofs, entries, pubs, scalars)
    assert len(got) == 1 and got == expected_sums(keys, proofs, entries, pubs, scalars, want, 65536, 600)
    verdicts, rep = kset.verify_batch(proofs, entries, pubs)
    assert list(verdicts) == want
    assert (rep["group"], rep["groups"], rep["groups_failed"], rep["segments"], rep["proofs_rechecked"], rep["malformed"]) == (600, 1, 0, 3, 0, 0)


# ---------------------------------------------------------------- batch: the verdicts
SPREAD = [(0, 1, 2, 3, 4, 3, 0)[(i * 3 + i // 9) % 7] for i in range(70)]


def test_all_valid_no_group_fails(keys, kset, monkeypatch):
    """the recheck would hide a wrong fold: with every proof valid no group may fail"""
    monkeypatch.delenv(CHUNK, raising=False)
    proofs, pubs = build(keys, SPREAD)
    assert set(SPREAD) == {0, 1, 2, 3, 4}
    for group in (16, 65536, 1):
        monkeypatch.setenv(GROUP, str(group))
        formed = groups_of(SPREAD, 65536, group)
        verdicts, rep = kset.verify_batch(proofs, SPREAD, pubs)
        assert list(verdicts) == [OK] * 70
        assert rep["groups_failed"] == 0 and rep["proofs_rechecked"] == 0 and rep["malformed"] == 0
        assert rep["groups"] == len(formed) and rep["segments"] == sum(len({SPREAD[i] for i in g}) for g in formed)
        assert rep["launches"] == kset.info()["last_launches"] and rep["chunks"] == 1
    monkeypatch.setenv(GROUP, "5")
    monkeypatch.setenv(CHUNK, "7")
    verdicts, rep = kset.verify_batch(proofs, SPREAD, pubs)
    assert list(verdicts) == [OK] * 70 and (rep["groups"], rep["groups_failed"], rep["proofs_rechecked"], rep["chunks"]) == (20, 0, 0, 10)


def test_one_invalid_proof_fails_one_group(keys, kset, monkeypatch):
    monkeypatch.delenv(CHUNK, raising=False)
    monkeypatch.setenv(GROUP, "16")
    bad = {12: CORRUPT, 40: FLIPPED, 41: PUBLIC_IS_R, 55: 27}
    assert SPREAD[41] != 2
    proofs, pubs = build(keys, SPREAD, bad)
    want = [MALFORMED if i in (12, 41, 55) else INVALID if i == 40 else OK for i in range(70)]
    formed = groups_of(SPREAD, 65536, 16)
    hit, = [g for g in formed if 40 in g]
    for scalars in (None, [random.Random(16).randrange(1, 1 << 128) for _ in range(70)]):
        verdicts, rep = kset.verify_batch(proofs, SPREAD, pubs, scalars)
        assert list(verdicts) == want
        assert (rep["group"], rep["groups"], rep["groups_failed"], rep["malformed"], rep["chunks"]) == (16, 5, 1, 3, 1)
        assert rep["proofs_rechecked"] == sum(want[i] != MALFORMED for i in hit)
    assert list(kset.verify(proofs, SPREAD, pubs)) == want


def test_a_group_of_malformed_proofs_evaluates_nothing(keys, kset, monkeypatch):
    monkeypatch.delenv(CHUNK, raising=False)
    monkeypatch.setenv(GROUP, "2")
    entries = [3, 0, 1, 0, 4, 2]                         # by key: positions 1 3 | 2 5 | 0 4
    proofs, pubs = build(keys, entries, {1: CORRUPT, 3: 27})
    verdicts, rep = kset.verify_batch(proofs, entries, pubs)
    assert list(verdicts) == [OK, MALFORMED, OK, MALFORMED, OK, OK]
    assert (rep["groups"], rep["groups_failed"], rep["segments"], rep["proofs_rechecked"], rep["malformed"]) == (2, 0, 4, 0, 2)
    assert kset.batch_sums(proofs, entries, pubs, [5] * 6)[0] == (bytes(64), bytes(64))
