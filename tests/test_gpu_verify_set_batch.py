"""VerificationKeySet.verify_batch on the device: one random combination for proofs under many keys.  The yardstick of
every verdict is VerificationKeySet.verify on the same input; where changes are planned, the plan is the yardstick.  The
report's counts come from `layout` below, a restatement of the grouping rule applied to the positions: inside a chunk the
proofs in key order (stable), a group closed when it holds ZKHIP_VERIFY_GROUP proofs or when the next proof would bring a
key beyond the ZKHIP_VERIFY_GROUP_KEYS-th into it."""
import random

import numpy as np
import pytest

from conftest import CIRCUITS, golden_json, golden_path

from oracle import bn254 as bn
from rapidsnark_old_amd import verify as V
from rapidsnark_old_amd.lib import ZkHipError
from test_gpu_verify_batch import g1_plus, scal
from test_gpu_verify_set import NOPUB, World, changed

pytestmark = pytest.mark.gpu
RM, QM = bn.R_MOD, bn.Q_MOD
OK, INVALID, MALFORMED = 0, 1, 2
BATCH = 2
DEFAULT_CHUNK = 1 << 16
COUNTS = ("group", "group_keys", "groups", "segments", "groups_failed", "proofs_rechecked", "malformed")


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


def set_sizes(monkeypatch, group, keys, chunk=DEFAULT_CHUNK):
    monkeypatch.setenv("ZKHIP_VERIFY_GROUP", str(group))
    monkeypatch.setenv("ZKHIP_VERIFY_GROUP_KEYS", str(keys))
    if chunk == DEFAULT_CHUNK:
        monkeypatch.delenv("ZKHIP_VERIFY_CHUNK", raising=False)
    else:
        monkeypatch.setenv("ZKHIP_VERIFY_CHUNK", str(chunk))


def layout(key_of, group, keys, chunk=DEFAULT_CHUNK):
    """the groups the call forms, each a list of caller positions"""
    out = []
    for c0 in range(0, len(key_of), chunk):
        cur = []
        for i in sorted(range(c0, min(len(key_of), c0 + chunk)), key=lambda p: key_of[p]):   # stable: a key's proofs in the caller's order
            inside = {key_of[p] for p in cur}
            if cur and (len(cur) == group or (key_of[i] not in inside and len(inside) == keys)):
                out.append(cur)
                cur = []
            cur.append(i)
        if cur:
            out.append(cur)
    return out


def expected(want, key_of, group, keys, chunk=DEFAULT_CHUNK):
    """the report of a call whose scalars let no error cancel"""
    live = [g for g in layout(key_of, group, keys, chunk) if any(want[i] != MALFORMED for i in g)]
    failed = [g for g in live if any(want[i] == INVALID for i in g)]
    return {"group": group, "group_keys": keys, "groups": len(live), "groups_failed": len(failed),
            "segments": sum(len({key_of[i] for i in g if want[i] != MALFORMED}) for g in live),
            "proofs_rechecked": sum(1 for g in failed for i in g if want[i] != MALFORMED), "malformed": list(want).count(MALFORMED)}


def counts(rep):
    return {k: rep[k] for k in COUNTS}


def batch(ks, proofs, key_of, publics, scalars=None):
    got, rep = ks.verify_batch(b"".join(proofs), key_of, b"".join(publics), scalars=None if scalars is None else scal(scalars))
    assert got.dtype == np.uint8 and got.shape == (len(proofs),)
    info = ks.info()
    if proofs:
        assert info["last_path"] == BATCH and info["last_launches"] == rep["launches"]
    return got.tolist(), rep


def single(ks, proofs, key_of, publics):
    return ks.verify(b"".join(proofs), key_of, b"".join(publics)).tolist()


def odd_scalars(n, seed):
    rng = random.Random(seed)
    out = [rng.getrandbits(128) | 1 for _ in range(n)]
    assert len(set(out)) == n
    return out


def test_the_five_goldens_all_valid(zk, world, monkeypatch):
    with zk.VerificationKeySet(world.keys) as ks:
        for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 4, 0, 3, 1]):
            proofs, publics = [world.gold[c][0] for c in order], [world.gold[c][1] for c in order]
            set_sizes(monkeypatch, 64, 8)
            got, rep = batch(ks, proofs, order, publics)
            assert got == [OK] * 5 == single(ks, proofs, order, publics), order
            assert counts(rep) == {"group": 64, "group_keys": 8, "groups": 1, "segments": 5, "groups_failed": 0, "proofs_rechecked": 0, "malformed": 0}
            set_sizes(monkeypatch, 64, 1)
            got, rep = batch(ks, proofs, order, publics)
            assert got == [OK] * 5, order
            assert counts(rep) == {"group": 64, "group_keys": 1, "groups": 5, "segments": 5, "groups_failed": 0, "proofs_rechecked": 0, "malformed": 0}


@pytest.mark.parametrize("group,keys,chunk", [(64, 8, DEFAULT_CHUNK), (8, 2, DEFAULT_CHUNK), (200, 5, 50), (1, 1, DEFAULT_CHUNK)])
def test_the_mixture_forward_and_reversed(zk, world, mixture, monkeypatch, group, keys, chunk):
    proofs, key_of, publics, plan = mixture
    set_sizes(monkeypatch, group, keys, chunk)
    with zk.VerificationKeySet(world.keys) as ks:
        for pr, ko, pu, want in ((proofs, key_of, publics, plan), (proofs[::-1], key_of[::-1], publics[::-1], plan[::-1])):
            exp = expected(want, ko, group, keys, chunk)
            assert exp["groups_failed"] > 0 and exp["malformed"] > 0 and exp["segments"] >= exp["groups"]
            for scalars in (None, odd_scalars(len(pr), group)):
                before = ks.info()
                got, rep = batch(ks, pr, ko, pu, scalars)
                after = ks.info()
                assert got == want
                assert counts(rep) == exp
                assert (after["proofs_coop"] + after["proofs_lanes"]) - (before["proofs_coop"] + before["proofs_lanes"]) == rep["proofs_rechecked"]
            assert single(ks, pr, ko, pu) == want


@pytest.mark.parametrize("group", [64, 200])
def test_a_one_key_set_is_the_keys_verify_batch(zk, world, monkeypatch, group):
    n, c = 130, 2                                       # r1cs_n64
    proofs = [world.pool[c][i % 65] for i in range(n)]
    publics = [world.gold[c][1]] * n
    for i, kind in ((0, "B not rescaled"), (64, "a signal = r"), (129, "C = infinity"), (77, "a signal + 1")):
        proofs[i], publics[i] = changed(kind, proofs[i], publics[i], world.gold[c][0])
    scalars = odd_scalars(n, 130)
    set_sizes(monkeypatch, group, 4)
    want, wrep = world.keys[c].verify_batch(b"".join(proofs), b"".join(publics), scalars=scal(scalars))
    assert want.tolist().count(INVALID) == 2 and want.tolist().count(MALFORMED) == 2
    with zk.VerificationKeySet([world.keys[c]]) as ks:
        got, rep = batch(ks, proofs, [0] * n, publics, scalars)
        assert got == want.tolist() == single(ks, proofs, [0] * n, publics)
        for name in ("group", "groups", "groups_failed", "proofs_rechecked", "malformed"):
            assert rep[name] == wrep[name], name
        assert rep["segments"] == rep["groups"]


def delta_of(name):
    """the key's delta among the golden's toxic values: the one whose multiple of the G2 generator is vk_delta2"""
    delta2 = V.VerificationKey.read_zkey(golden_path(name, "circuit.zkey"))[3]
    found = [int(t) for t in golden_json(name, "meta.json")["toxic"] if bn.g2_to_bytes(bn.G2.mul(bn.G2_GEN, int(t) % RM)) == delta2]
    assert len(golden_json(name, "meta.json")["toxic"]) == 5 and len(found) == 1, name
    return found[0]


def test_one_equation_across_keys(zk, world, monkeypatch):
    """C + delta_b G under key a and C - delta_a G under key b: d_a = e(G, G2)^(-delta_a delta_b) and d_b is its inverse,
    so the errors cancel only in an equation that holds both keys.  Per-key groups cannot pass this."""
    a, b = 0, 2
    da, db = delta_of(CIRCUITS[a]), delta_of(CIRCUITS[b])
    pa, pb = world.pool[a][3], world.pool[b][3]
    proofs = [pa[:192] + g1_plus(zk, pa[192:], db), pb[:192] + g1_plus(zk, pb[192:], -da)]
    key_of, publics = [a, b], [world.gold[a][1], world.gold[b][1]]
    with zk.VerificationKeySet(world.keys) as ks:
        assert single(ks, proofs, key_of, publics) == [INVALID, INVALID]
        set_sizes(monkeypatch, 64, 8)
        got, rep = batch(ks, proofs, key_of, publics, [1, 1])
        assert got == [OK, OK] and rep["groups"] == 1 and rep["segments"] == 2 and rep["groups_failed"] == 0
        got, rep = batch(ks, proofs, key_of, publics, [3, 5])
        assert got == [INVALID, INVALID] and rep["groups"] == 1 and rep["groups_failed"] == 1 and rep["proofs_rechecked"] == 2
        got, rep = batch(ks, proofs, key_of, publics)
        assert got == [INVALID, INVALID] and rep["groups_failed"] == 1
        set_sizes(monkeypatch, 64, 1)                   # separate groups: nothing to cancel against
        got, rep = batch(ks, proofs, key_of, publics, [1, 1])
        assert got == [INVALID, INVALID] and rep["groups"] == 2 and rep["groups_failed"] == 2


def test_errors_that_cancel_inside_one_segment(zk, world, monkeypatch):
    c, n = 2, 12                                        # r1cs_n64, between three proofs of key 0 and three of key 4
    mid = list(world.pool[c][:n])
    public = world.gold[c][1]
    pubs = [public] * n
    first = int.from_bytes(public[:32], "little")
    mid[2] = mid[2][:192] + g1_plus(zk, mid[2][192:], 1)
    mid[5] = mid[5][:192] + g1_plus(zk, mid[5][192:], -1)
    pubs[7] = ((first + 1) % RM).to_bytes(32, "little") + public[32:]
    pubs[9] = ((first - 1) % RM).to_bytes(32, "little") + public[32:]
    proofs = world.pool[0][:3] + mid + world.pool[4][:3]
    key_of = [0] * 3 + [c] * n + [4] * 3
    publics = [world.gold[0][1]] * 3 + pubs + [world.gold[4][1]] * 3
    want = [INVALID if i in (5, 8, 10, 12) else OK for i in range(n + 6)]
    set_sizes(monkeypatch, 64, 8)
    with zk.VerificationKeySet(world.keys) as ks:
        assert single(ks, proofs, key_of, publics) == want
        got, rep = batch(ks, proofs, key_of, publics)
        assert got == want and counts(rep) == expected(want, key_of, 64, 8) and rep["segments"] == 3
        got, rep = batch(ks, proofs, key_of, publics, odd_scalars(n + 6, 12))
        assert got == want and rep["groups_failed"] == 1 and rep["proofs_rechecked"] == n + 6
        # what the scalars are for: with equal weights the four errors cancel and every proof is taken for valid
        got, rep = batch(ks, proofs, key_of, publics, [1] * (n + 6))
        assert got == [OK] * (n + 6) and rep["groups_failed"] == 0


@pytest.mark.parametrize("value", [1, (1 << 128) - 1])
def test_equal_scalars_at_both_ends(zk, world, monkeypatch, value):
    key_of = [i % 5 for i in range(20)]
    proofs = [world.pool[i % 5][i // 5] for i in range(20)]
    publics = [world.gold[i % 5][1] for i in range(20)]
    set_sizes(monkeypatch, 64, 8)
    with zk.VerificationKeySet(world.keys) as ks:
        got, rep = batch(ks, proofs, key_of, publics, [value] * 20)
        assert got == [OK] * 20
        assert counts(rep) == {"group": 64, "group_keys": 8, "groups": 1, "segments": 5, "groups_failed": 0, "proofs_rechecked": 0, "malformed": 0}


def test_a_segment_whose_sum_of_c_is_infinity(zk, world, monkeypatch):
    p = world.pool[2][0]
    c = bn.g1_from_bytes(p[192:])
    q = p[:192] + bn.g1_to_bytes((c[0], (-c[1]) % QM))
    proofs = [world.pool[0][0], p, q, world.pool[4][0]]
    key_of = [0, 2, 2, 4]
    publics = [world.gold[k][1] for k in key_of]
    set_sizes(monkeypatch, 64, 8)
    with zk.VerificationKeySet(world.keys) as ks:
        assert single(ks, proofs, key_of, publics) == [OK, OK, INVALID, OK]
        for r in (1, 0x1234567890abcdef1122334455667788):
            got, rep = batch(ks, proofs, key_of, publics, [7, r, r, 9])
            assert got == [OK, OK, INVALID, OK]
            assert counts(rep) == {"group": 64, "group_keys": 8, "groups": 1, "segments": 3, "groups_failed": 1, "proofs_rechecked": 4, "malformed": 0}


def test_runs_of_1_63_64_65_side_by_side_and_shuffled(zk, world, monkeypatch):
    proofs, key_of, publics = [], [], []
    for k, length in [(0, 1), (1, 63), (2, 64), (4, 65)]:
        first = len(proofs)
        proofs += world.pool[k][:length]
        key_of += [k] * length
        publics += [world.gold[k][1]] * length
        for i, kind in ((first, "B not rescaled"), (len(proofs) - 1, "a signal = r")) if length > 1 else ():
            proofs[i], publics[i] = changed(kind, proofs[i], publics[i], world.gold[k][0])
    order = list(range(len(proofs)))
    random.Random(4).shuffle(order)
    with zk.VerificationKeySet(world.keys) as ks:
        want = single(ks, proofs, key_of, publics)
        assert want.count(INVALID) == 3 and want.count(MALFORMED) == 3 and want[0] == OK
        for group, keys in ((64, 8), (64, 1), (1024, 2)):
            set_sizes(monkeypatch, group, keys)
            got, rep = batch(ks, proofs, key_of, publics)
            assert got == want and counts(rep) == expected(want, key_of, group, keys), (group, keys)
            got, rep = batch(ks, [proofs[i] for i in order], [key_of[i] for i in order], [publics[i] for i in order])
            assert got == [want[i] for i in order]
            assert counts(rep) == expected([want[i] for i in order], [key_of[i] for i in order], group, keys), (group, keys)


def test_no_proof_and_one_proof(zk, world, monkeypatch):
    set_sizes(monkeypatch, 64, 8)
    with zk.VerificationKeySet(world.keys) as ks:
        before = ks.info()
        got, rep = ks.verify_batch(b"", [], b"")
        assert got.shape == (0,) and got.dtype == np.uint8 and ks.info() == before
        assert rep == {"group": 64, "group_keys": 8, "launches": 0, "groups": 0, "groups_failed": 0, "segments": 0, "proofs_rechecked": 0, "malformed": 0}
        for k in range(5):
            got, rep = batch(ks, [world.gold[k][0]], [k], [world.gold[k][1]])
            assert got == [OK] and rep["groups"] == 1 and rep["segments"] == 1 and rep["groups_failed"] == 0
        bad, pub = changed("B not rescaled", world.pool[2][0], world.gold[2][1], world.gold[2][0])
        got, rep = batch(ks, [bad], [2], [pub])
        assert got == [INVALID] and rep["groups_failed"] == 1 and rep["proofs_rechecked"] == 1


def test_a_group_closed_by_the_key_limit_and_a_chunk_that_cuts_a_run(zk, world, monkeypatch):
    key_of = [k for k in range(5) for _ in range(3)]
    proofs = [world.pool[k][j] for k in range(5) for j in range(3)]
    publics = [world.gold[k][1] for k in key_of]
    with zk.VerificationKeySet(world.keys) as ks:
        set_sizes(monkeypatch, 64, 2)                   # keys {0, 1}, {2, 3}, {4}: no group is full
        got, rep = batch(ks, proofs, key_of, publics)
        assert got == [OK] * 15 and rep["groups"] == 3 and rep["segments"] == 5 and counts(rep) == expected(got, key_of, 64, 2)
        set_sizes(monkeypatch, 4, 2)                    # full groups cut the runs: 0001 1122 2333 444
        got, rep = batch(ks, proofs, key_of, publics)
        assert got == [OK] * 15 and rep["groups"] == 4 and rep["segments"] == 7 and counts(rep) == expected(got, key_of, 4, 2)
        # 120 proofs, 60 a key in the caller's order 0 1 0 1 ...: chunks of 50 hold 25 of each, so both runs are cut twice
        key_of = [i % 2 for i in range(120)]
        proofs = [world.pool[i % 2][i // 2] for i in range(120)]
        publics = [world.gold[i % 2][1] for i in range(120)]
        proofs[77], publics[77] = changed("a signal + 1", proofs[77], publics[77], world.gold[1][0])
        want = [INVALID if i == 77 else OK for i in range(120)]
        set_sizes(monkeypatch, 64, 8, 50)
        got, rep = batch(ks, proofs, key_of, publics)
        assert got == want == single(ks, proofs, key_of, publics)
        assert counts(rep) == expected(want, key_of, 64, 8, 50) and rep["groups"] == 3 and rep["segments"] == 6 and rep["proofs_rechecked"] == 50


def test_the_key_without_public_signals(zk, world, monkeypatch):
    key_of = [2, NOPUB, 4, NOPUB, NOPUB, 0, NOPUB]
    proofs = [world.pool[k][i] for i, k in enumerate(key_of)]
    publics = [world.gold[k][1] for k in key_of]
    proofs[3], publics[3] = changed("B not rescaled", proofs[3], publics[3], world.gold[NOPUB][0])
    proofs[2], publics[2] = changed("a signal + 1", proofs[2], publics[2], world.gold[4][0])
    want = [OK, OK, INVALID, INVALID, OK, OK, OK]
    with zk.VerificationKeySet(world.keys) as ks:
        assert single(ks, proofs, key_of, publics) == want
        for group, keys in ((64, 8), (64, 1), (2, 2)):
            set_sizes(monkeypatch, group, keys)
            got, rep = batch(ks, proofs, key_of, publics)
            assert got == want and counts(rep) == expected(want, key_of, group, keys)
        only = [proofs[i] for i in (1, 3, 4, 6)]
        set_sizes(monkeypatch, 64, 8)                   # alone: one group of one segment
        got, rep = ks.verify_batch(b"".join(only), [NOPUB] * 4, b"")
        assert got.tolist() == [OK, INVALID, OK, OK] and rep["segments"] == 1
        got, rep = ks.verify_batch(b"".join(only), [NOPUB] * 4)
        assert got.tolist() == [OK, INVALID, OK, OK]


def test_a_key_at_two_indices_and_a_proof_under_another_key(zk, world, monkeypatch):
    set_sizes(monkeypatch, 64, 8)
    with zk.VerificationKeySet([world.keys[2], world.keys[0], world.keys[2]]) as ks:
        p2, s2 = world.gold[2]
        bad, _ = changed("B not rescaled", world.pool[2][0], s2, p2)
        proofs, key_of, publics = [p2, bad, world.pool[2][1], world.gold[0][0]], [0, 2, 2, 1], [s2, s2, s2, world.gold[0][1]]
        got, rep = batch(ks, proofs, key_of, publics)
        assert got == [OK, INVALID, OK, OK] == single(ks, proofs, key_of, publics)
        assert rep["segments"] == 3 and rep["groups"] == 1            # the two indices are two keys to the grouping
        got, rep = batch(ks, [p2, world.pool[2][1]], [0, 2], [s2, s2])
        assert got == [OK, OK] and rep["segments"] == 2
    (p0, s0), (p1, s1) = world.gold[0], world.gold[1]   # multiplier2 and r1cs_n8: one public signal each
    with zk.VerificationKeySet(world.keys) as ks:
        proofs, key_of, publics = [p0, p1, p0, p1], [1, 0, 0, 1], [s0, s1, s0, s1]
        assert single(ks, proofs, key_of, publics) == [INVALID, INVALID, OK, OK]
        got, rep = batch(ks, proofs, key_of, publics)
        assert got == [INVALID, INVALID, OK, OK] and counts(rep) == expected(got, key_of, 64, 8)


def test_groups_and_segments_of_malformed_proofs(zk, world, monkeypatch):
    key_of = [0] * 4 + [1] * 2 + [2] * 2
    proofs = world.pool[0][:4] + world.pool[1][:2] + world.pool[2][:2]
    publics = [world.gold[k][1] for k in key_of]
    for i in (0, 1, 2, 3):                              # key 0: nothing well-formed
        proofs[i] = bytes(64) + proofs[i][64:]
    want = [MALFORMED] * 4 + [OK] * 4
    with zk.VerificationKeySet(world.keys) as ks:
        assert single(ks, proofs, key_of, publics) == want
        set_sizes(monkeypatch, 4, 8)                    # groups 0000 1122: the first is not evaluated
        got, rep = batch(ks, proofs, key_of, publics)
        assert got == want
        assert counts(rep) == {"group": 4, "group_keys": 8, "groups": 1, "segments": 2, "groups_failed": 0, "proofs_rechecked": 0, "malformed": 4}
        set_sizes(monkeypatch, 64, 8)                   # one group: key 0's segment takes no part
        got, rep = batch(ks, proofs, key_of, publics)
        assert got == want
        assert counts(rep) == {"group": 64, "group_keys": 8, "groups": 1, "segments": 2, "groups_failed": 0, "proofs_rechecked": 0, "malformed": 4}
        # the same with an invalid proof in the live part: only the well-formed proofs are rechecked
        proofs[5], publics[5] = changed("a signal + 1", proofs[5], publics[5], world.gold[1][0])
        want[5] = INVALID
        got, rep = batch(ks, proofs, key_of, publics)
        assert got == want and rep["groups_failed"] == 1 and rep["proofs_rechecked"] == 4
        # a chunk without a well-formed proof launches the check only
        got, rep = batch(ks, proofs[:4], key_of[:4], publics[:4])
        assert got == [MALFORMED] * 4 and rep["launches"] == 1
        assert counts(rep) == {"group": 64, "group_keys": 8, "groups": 0, "segments": 0, "groups_failed": 0, "proofs_rechecked": 0, "malformed": 4}


def test_the_launch_count_does_not_depend_on_the_keys(zk, world, monkeypatch):
    n = 200
    key_of = [i % 5 for i in range(n)]
    proofs = [world.pool[i % 5][i // 5] for i in range(n)]
    publics = [world.gold[i % 5][1] for i in range(n)]
    one = [world.pool[0][i % 65] for i in range(n)]
    with zk.VerificationKeySet(world.keys) as five, zk.VerificationKeySet([world.keys[0]]) as lone:
        for group, keys in ((64, 5), (200, 8), (1, 5)):
            set_sizes(monkeypatch, group, keys)
            got5, rep5 = batch(five, proofs, key_of, publics)
            got1, rep1 = batch(lone, one, [0] * n, [world.gold[0][1]] * n)
            assert got5 == got1 == [OK] * n
            if group == 64:                             # the first batch call of either set made its lines of beta: one launch more
                again5 = batch(five, proofs, key_of, publics)[1]
                again1 = batch(lone, one, [0] * n, [world.gold[0][1]] * n)[1]
                assert rep5["launches"] == again5["launches"] + 1 and rep1["launches"] == again1["launches"] + 1
                rep5, rep1 = again5, again1
            assert rep5["launches"] == rep1["launches"] > 0, (group, keys)
            assert rep5["groups"] == rep1["groups"] == -(-n // group)


def test_set_batch_calls_leave_the_keys_as_they_were(zk, world, mixture, monkeypatch):
    proofs, key_of, publics, plan = mixture
    fresh = [zk.VerificationKey.from_zkey(golden_path(c, "circuit.zkey")) for c in CIRCUITS]
    try:
        before = [k.info() for k in fresh]
        set_sizes(monkeypatch, 64, 8)
        with zk.VerificationKeySet(fresh) as ks:
            start = ks.info()
            got, rep = batch(ks, proofs, key_of, publics)
            assert got == plan and rep["proofs_rechecked"] > 0
            info = ks.info()
            assert info["last_path"] == BATCH and info["last_launches"] == rep["launches"] and info["n_keys"] == 5
            assert (info["proofs_coop"] + info["proofs_lanes"]) - (start["proofs_coop"] + start["proofs_lanes"]) == rep["proofs_rechecked"]
            assert [k.info() for k in fresh] == before
            for k, (p, s) in zip(fresh, world.gold):      # the keys' own entries, the set still open
                assert k.verify(p, s).tolist() == [OK]
                verdicts, krep = k.verify_batch(p + p, s + s)
                assert verdicts.tolist() == [OK, OK] and krep["groups_failed"] == 0
            assert batch(ks, proofs, key_of, publics)[0] == plan
    finally:
        for k in fresh:
            k.close()


def test_refusals_leave_the_set_working(zk, world, monkeypatch):
    key_of = [0, 2, 4, 1, 3]
    proofs = [world.pool[k][0] for k in key_of]
    publics = [world.gold[k][1] for k in key_of]
    P, S = b"".join(proofs), b"".join(publics)
    set_sizes(monkeypatch, 4, 2)
    with zk.VerificationKeySet(world.keys) as ks:
        start = ks.info()
        with pytest.raises(ZkHipError, match="scalar 3 is zero"):
            ks.verify_batch(P, key_of, S, scalars=scal([7, 8, 9, 0, 11]))
        with pytest.raises(ValueError, match="scalars"):
            ks.verify_batch(P, key_of, S, scalars=scal([7, 8, 9, 10]))
        with pytest.raises(ValueError, match=r"key_of\[1\] = 5"):
            ks.verify_batch(P, [0, 5, 4, 1, 3], S)
        with pytest.raises(ValueError, match="publics: .* bytes expected"):
            ks.verify_batch(P, key_of, S[:-32])
        for name in ("ZKHIP_VERIFY_GROUP", "ZKHIP_VERIFY_GROUP_KEYS"):
            for bad in ("0", "many", "-4", "16777217" if name.endswith("GROUP") else "65537", "8x"):
                monkeypatch.setenv(name, bad)
                with pytest.raises(ZkHipError, match=name + ":"):
                    ks.verify_batch(P, key_of, S)
            monkeypatch.setenv(name, "4" if name.endswith("GROUP") else "2")
        # the library's own refusals, for callers of the C interface
        import ctypes as C
        from rapidsnark_old_amd import lib as L
        lib = L.load_library()
        out = np.zeros(5, dtype=np.uint8)
        pr, pub = np.frombuffer(P, dtype=np.uint8), np.frombuffer(S, dtype=np.uint8)
        ko = np.array([0, 5, 4, 1, 3], dtype=np.uint32)
        assert lib.zk_vkey_set_verify_batch(ks._h, L._ptr(pr), L._ptr(ko), L._ptr(pub), pub.size, 5, None, L._ptr(out), None) != 0
        msg = lib.zk_last_error().decode()
        assert "key_of[1] = 5" in msg and "5 keys" in msg
        ko = np.array(key_of, dtype=np.uint32)
        assert lib.zk_vkey_set_verify_batch(ks._h, L._ptr(pr), L._ptr(ko), L._ptr(pub), pub.size - 32, 5, None, L._ptr(out), None) != 0
        msg = lib.zk_last_error().decode()
        assert "%d expected" % pub.size in msg and "%d given" % (pub.size - 32) in msg
        assert ks.info() == start                       # refused before any launch
        assert lib.zk_vkey_set_verify_batch(ks._h, L._ptr(pr), L._ptr(ko), L._ptr(pub), pub.size, 5, None, L._ptr(out), None) == 0 and out.tolist() == [OK] * 5
        got, rep = batch(ks, proofs, key_of, publics, [7, 8, 9, 10, 11])
        assert got == [OK] * 5 and counts(rep) == expected(got, key_of, 4, 2) and rep["groups"] == 3
        monkeypatch.delenv("ZKHIP_VERIFY_GROUP")      # the default limits
        monkeypatch.delenv("ZKHIP_VERIFY_GROUP_KEYS")
        got, rep = batch(ks, proofs, key_of, publics)
        assert got == [OK] * 5 and rep["group"] == 1024 and 1 <= rep["group_keys"] <= 65536
        assert counts(rep) == expected(got, key_of, rep["group"], rep["group_keys"])
    with pytest.raises(ZkHipError, match="closed"):
        ks.verify_batch(P, key_of, S)
