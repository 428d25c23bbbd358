"""Is a .zkey the key of its circuit over a .ptau (zk_zkey_verify, rapidsnark_old_amd.zkey_verify, `zkeyverify`): keys that
pass (setup keys, contributed keys, an oracle key with gamma = 1), the committed golden keys (random gamma: exactly
gamma2 and IC fail), circuits whose shapes the golden ones miss, one tamper per item with the exact set of findings, and
malformed points.  Every comparison is exact; the only chance involved is that of the check itself, below 2^29 / r."""
import copy
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from conftest import CIRCUITS, ROOT, golden_bytes, golden_json

from oracle import bn254 as bn, groth16_ref as g
from rapidsnark_old_amd import r1cs as R, zkgen

pytestmark = pytest.mark.gpu
RM, QM = bn.R_MOD, bn.Q_MOD
BIN = os.path.join(ROOT, "rapidsnark-old_amd", "zkeyverify")
TOXIC3 = (0x1234567 * 0x89ABCDEF + 17, 0xA1FA << 200 | 99, 0xBE7A << 180 | 7)        # tau, alpha, beta of the small ptaus
S1, S2 = 0xC0FFEE << 100 | 5, RM - 12345
D1, D2 = 0xD17A << 150 | 3, 987654321987654321
ALL6 = {"A", "B1", "B2", "IC", "C", "H"}


def golden_circuits():
    """multiplier2 and the random circuits of oracle/gen_golden.py (the same seeded calls)"""
    out = {"multiplier2": g.multiplier2_r1cs()}
    rng = random.Random(7)
    for name, args in (("r1cs_n8", (5, 1)), ("r1cs_n64", (50, 3)), ("r1cs_nopub", (10, 0)), ("r1cs_n256", (200, 2))):
        out[name] = g.random_r1cs(rng, *args)[0]
    return out


GOLD = golden_circuits()


def write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


@pytest.fixture(scope="module")
def box(zk, tmp_path_factory):
    """the files the tests share, made once: trapdoor ptaus by (power, toxic), the circuits' .r1cs, their setup keys (as
    dicts and files) and those keys after two contributions"""
    d = tmp_path_factory.mktemp("zkv")

    class Box:
        dir = d
        _ptau, _r1cs, _key = {}, {}, {}

        def ptau(self, power, toxic=TOXIC3):
            k = (power, tuple(toxic))
            if k not in self._ptau:
                self._ptau[k] = str(d / ("p%d_%d.ptau" % (power, len(self._ptau))))
                zk.write_trapdoor_ptau(power, *toxic, self._ptau[k])
            return self._ptau[k]

        def r1cs(self, name):
            if name not in self._r1cs:
                c = GOLD[name]
                self._r1cs[name] = write(str(d / (name + ".r1cs")), R.write_r1cs_rows(c.A, c.B, c.C, c.nVars, c.nPublic))
            return self._r1cs[name]

        def key(self, name, power):
            """-> (key dict, path of the setup key, path of the key after the contributions D1 and D2)"""
            if (name, power) not in self._key:
                key = zk.groth16_setup(self.r1cs(name), self.ptau(power), device=0)
                p0, p1, p2 = (str(d / ("%s_%d_%d.zkey" % (name, power, i))) for i in range(3))
                zkgen.write_zkey(key, p0)
                zk.zkey_contribute(p0, p1, d=D1, device=0)
                zk.zkey_contribute(p1, p2, d=D2, device=0)
                self._key[(name, power)] = (key, p0, p2)
            return self._key[(name, power)]
    return Box()


def cli(*args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    e.setdefault("ZKHIP_DEVICE", "0")
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300, env=e)


def assert_ok(rep, starting):
    assert rep.ok and rep.verdict == 0 and not rep.failed and not rep.not_checked and not rep.shape_failed, rep
    assert rep.delta_is_generator == starting and rep.coef_rows_differing == 0 and rep.coef_first_row is None, rep


# ---------------------------------------------------------------- 1. keys that pass
CASES = [(name, power) for name in CIRCUITS for power in (9, 8)]


@pytest.mark.parametrize("name,power", CASES)
def test_setup_keys_and_contributed_keys_pass(zk, box, name, power):
    _key, p0, p2 = box.key(name, power)
    for s in (S1, S2, None):
        assert_ok(zk.zkey_verify(box.r1cs(name), box.ptau(power), p0, s=s, device=0), True)
        assert_ok(zk.zkey_verify(box.r1cs(name), box.ptau(power), p2, s=s, device=0), False)


@pytest.mark.parametrize("name,power", [("r1cs_n256", 8), ("r1cs_nopub", 9)])
def test_passing_keys_through_the_cli(box, name, power):
    _key, p0, p2 = box.key(name, power)
    for path, starting in ((p0, True), (p2, False)):
        res = cli(box.r1cs(name), box.ptau(power), path)
        assert res.returncode == 0 and res.stderr == "", (res.stdout, res.stderr)
        assert res.stdout.startswith("OK: ") and len(res.stdout.splitlines()) == 1
        assert ("starting key" in res.stdout) == starting and ("not safe to prove with" in res.stdout) == starting
        assert "transcript (section 10) is not checked" in res.stdout


# ---------------------------------------------------------------- 2. the committed golden keys: gamma and delta random
@pytest.mark.parametrize("name", CIRCUITS)
def test_golden_keys_fail_gamma2_and_ic_only(zk, box, name):
    toxic = [int(x) for x in golden_json(name, "meta.json")["toxic"]]
    assert toxic[3] != 1 and toxic[4] != 1
    key = write(str(box.dir / "golden.zkey"), golden_bytes(name, "circuit.zkey"))
    rep = zk.zkey_verify(box.r1cs(name), box.ptau(9, toxic[:3]), key, device=0)      # power 9 > k: H has its top power
    assert rep.verdict == 1 and rep.failed == {"gamma2", "IC"} and not rep.not_checked and not rep.delta_is_generator, rep


# ---------------------------------------------------------------- 3. an oracle key with gamma = 1 and delta random
@pytest.mark.parametrize("name", ["multiplier2", "r1cs_n8"])
def test_oracle_key_with_gamma_one_passes(zk, box, name):
    ozk, _trap = g.setup(GOLD[name], (*TOXIC3, 1, 0xDE17A << 120 | 11))
    key = write(str(box.dir / "oracle.zkey"), g.write_zkey(ozk))
    assert_ok(zk.zkey_verify(box.r1cs(name), box.ptau(9), key, device=0), False)


# ---------------------------------------------------------------- 4. structure the golden circuits miss
def structured(kind):
    """-> (A, B, C rows as lists of (wire, value) with repeats, nWires, nPublic).  One row of 300 terms in each matrix (the
    segmented sum cuts at 16: 300 -> 19 -> 2 -> 1, three passes), the constant wire in every row, the same (row, wire) pair
    twice, a wire that no matrix mentions (the last one)."""
    rng = random.Random(kind)
    val = lambda: rng.randrange(1, RM)
    if kind == "wide":                                            # nVars 331 > domain 32
        m, nw, npub = 20, 331, 3
        long_row = lambda: [(1 + t, val()) for t in range(300)]
    else:                                                         # "narrow": nVars 21 < domain 64, the 300 terms over 19 wires
        m, nw, npub = 40, 21, 2
        long_row = lambda: [(1 + t % 19, val()) for t in range(300)]
    A = [[(0, val()), (1 + i % (nw - 2), val())] for i in range(m)]
    B = [[(0, val()), (1 + (i * 7) % (nw - 2), RM - 1)] for i in range(m)]
    C = [[(0, 1), (1 + (i * 3) % (nw - 2), val())] for i in range(m)]
    A[2] += long_row()
    B[5] += long_row()
    C[7] += long_row()
    A[4] += [(6, 5), (6, 5)]
    B[4] += [(9, 3), (9, 3), (9, RM - 1)]
    C[4] += [(12, 2), (12, 2)]
    assert all(w < nw - 1 for M in (A, B, C) for row in M for w, _ in row)
    return A, B, C, nw, npub


@pytest.mark.parametrize("kind", ["wide", "narrow"])
def test_structured_circuits_pass_in_one_chunk_and_in_many(zk, box, kind):
    A, B, C, nw, npub = structured(kind)
    rp = write(str(box.dir / (kind + ".r1cs")), R.write_r1cs_rows(A, B, C, nw, npub))
    key = zk.groth16_setup(rp, box.ptau(9), device=0)
    assert (key["nVars"], key["domainSize"]) == ((331, 32) if kind == "wide" else (21, 64))
    last = lambda name, nb: np.asarray(key[name]).reshape(-1, nb)[-1]
    for name, nb in (("pointsA", 64), ("pointsB1", 64), ("pointsB2", 128), ("pointsC", 64)):
        assert not last(name, nb).any()                           # the unmentioned wire: infinity in sections 5 to 8, legal
    zp = str(box.dir / (kind + ".zkey"))
    zkgen.write_zkey(key, zp)
    assert_ok(zk.zkey_verify(rp, box.ptau(9), zp, s=S1, device=0), True)
    res = cli(rp, box.ptau(9), zp, env={"ZKHIP_ZKEY_VERIFY_CHUNK": "64", "ZKHIP_ZKEY_VERIFY_SCALAR": str(S1)})
    assert res.returncode == 0 and res.stdout.startswith("OK: "), (res.stdout, res.stderr)
    bad = copy.copy(key)                                          # and a wrong point is still found across the chunks
    bad["pointsA"] = np.asarray(key["pointsA"]).copy()
    bad["pointsA"][:64], bad["pointsA"][64:128] = key["pointsA"][64:128], key["pointsA"][:64]
    assert not np.array_equal(bad["pointsA"], key["pointsA"])
    zkgen.write_zkey(bad, zp)
    res = cli(rp, box.ptau(9), zp, env={"ZKHIP_ZKEY_VERIFY_CHUNK": "64"})
    assert res.returncode == 1 and [ln.split(":")[1].strip() for ln in res.stdout.splitlines()] == ["A"], (res.stdout, res.stderr)


# ---------------------------------------------------------------- 5. one tamper per item
NAME, POWER = "r1cs_n64", 9


def load_key(path):
    """a key file -> dict of zkgen.write_zkey's fields (numpy copies)"""
    zkb = open(path, "rb").read()
    (nsec,) = struct.unpack_from("<I", zkb, 8)
    at, secs = 12, {}
    for _ in range(nsec):
        sid, size = struct.unpack_from("<IQ", zkb, at)
        secs[sid] = np.frombuffer(zkb[at + 12:at + 12 + size], dtype=np.uint8).copy()
        at += 12 + size
    s2 = secs[2]
    key = dict(zip(("nVars", "nPublic", "domainSize"), (int(x) for x in struct.unpack_from("<III", s2.tobytes(), 72))))
    at = 84
    for name, nb in (("vk_alpha1", 64), ("vk_beta1", 64), ("vk_beta2", 128), ("vk_gamma2", 128), ("vk_delta1", 64), ("vk_delta2", 128)):
        key[name] = s2[at:at + nb].copy()
        at += nb
    for sid, name in ((3, "pointsIC"), (4, "coefs"), (5, "pointsA"), (6, "pointsB1"), (7, "pointsB2"), (8, "pointsC"), (9, "pointsH")):
        key[name] = secs[sid]
    return key


def first_point(arr, nb, start=0):
    """the lowest index >= start of a point that is not infinity"""
    pts = np.asarray(arr).reshape(-1, nb)
    return next(i for i in range(start, len(pts)) if pts[i].any())


def g1_times(zk, key, name, i, k):
    key[name][64 * i:64 * i + 64] = np.frombuffer(zk.g1_mul(key[name][64 * i:64 * i + 64].tobytes(), k), np.uint8)


def t_swap_a(zk, key):
    i = first_point(key["pointsA"], 64)
    j = next(j for j in range(i + 1, key["nVars"]) if not np.array_equal(key["pointsA"][64 * j:64 * j + 64], key["pointsA"][64 * i:64 * i + 64]))
    a, b = key["pointsA"][64 * i:64 * i + 64].copy(), key["pointsA"][64 * j:64 * j + 64].copy()
    key["pointsA"][64 * i:64 * i + 64], key["pointsA"][64 * j:64 * j + 64] = b, a


def t_double_c3(zk, key):
    assert key["pointsC"][64 * 3:64 * 4].any()
    g1_times(zk, key, "pointsC", 3, 2)


def t_h_last(zk, key):
    assert not np.array_equal(key["pointsH"][-64:], key["pointsH"][:64])
    key["pointsH"][-64:] = key["pointsH"][:64]


def t_b2(zk, key):
    i = first_point(key["pointsB2"], 128)
    key["pointsB2"][128 * i:128 * i + 128] = np.frombuffer(zk.g2_mul(key["pointsB2"][128 * i:128 * i + 128].tobytes(), 3), np.uint8)


def t_b1(zk, key):
    g1_times(zk, key, "pointsB1", first_point(key["pointsB1"], 64), 2)


def t_ic(zk, key):
    g1_times(zk, key, "pointsIC", key["nPublic"], 5)


def t_alpha(zk, key):
    g1_times(zk, key, "vk_alpha1", 0, 2)


def t_delta1(zk, key):
    g1_times(zk, key, "vk_delta1", 0, 7)


TAMPERS = {"swap_A": (t_swap_a, {"A"}), "double_C3": (t_double_c3, {"C"}), "H_last": (t_h_last, {"H"}), "B2": (t_b2, {"B2"}), "B1": (t_b1, {"B1"}),
           "IC": (t_ic, {"IC"}), "alpha1": (t_alpha, {"alpha1"}), "two_at_once": (lambda zk, key: (t_b1(zk, key), t_h_last(zk, key)), {"B1", "H"})}


@pytest.mark.parametrize("case", sorted(TAMPERS))
def test_one_tamper_one_item(zk, box, case):
    fn, want = TAMPERS[case]
    key = load_key(box.key(NAME, POWER)[2])                       # after two contributions: delta is not 1
    fn(zk, key)
    zp = str(box.dir / "tampered.zkey")
    zkgen.write_zkey(key, zp)
    rep = zk.zkey_verify(box.r1cs(NAME), box.ptau(POWER), zp, device=0)
    assert rep.verdict == 1 and rep.failed == want and not rep.not_checked, (case, rep)
    res = cli(box.r1cs(NAME), box.ptau(POWER), zp)
    assert res.returncode == 1 and res.stderr == "", (res.stdout, res.stderr)
    assert {ln.split(":")[1].strip() for ln in res.stdout.splitlines()} == want and all(ln.startswith("INVALID: ") for ln in res.stdout.splitlines())


def test_delta1_of_another_d_leaves_c_and_h_unchecked(zk, box):
    key = load_key(box.key(NAME, POWER)[2])
    t_delta1(zk, key)
    zp = str(box.dir / "delta.zkey")
    zkgen.write_zkey(key, zp)
    rep = zk.zkey_verify(box.r1cs(NAME), box.ptau(POWER), zp, device=0)
    assert rep.verdict == 1 and rep.failed == {"delta"} and rep.not_checked == {"C", "H"}, rep
    res = cli(box.r1cs(NAME), box.ptau(POWER), zp)
    assert res.returncode == 1 and [ln.split(":")[0] + ":" + ln.split(":")[1] for ln in res.stdout.splitlines()] == \
        ["INVALID: delta", "NOT CHECKED: C", "NOT CHECKED: H"], res.stdout


def test_a_coefficient_changed_in_the_r1cs_only(zk, box):
    c = GOLD[NAME]
    row, wire = next((i, w) for i, r in enumerate(c.A) for w in sorted(r) if w > c.nPublic)
    A = [dict(r) for r in c.A]
    A[row][wire] = (A[row][wire] + 1) % RM or 2
    rp = write(str(box.dir / "changed.r1cs"), R.write_r1cs_rows(A, c.B, c.C, c.nVars, c.nPublic))
    rep = zk.zkey_verify(rp, box.ptau(POWER), box.key(NAME, POWER)[2], device=0)
    assert rep.verdict == 1 and rep.failed == {"coefs", "A", "C"} and not rep.not_checked, rep
    assert (rep.coef_rows_differing, rep.coef_first_row) == (1, row)
    res = cli(rp, box.ptau(POWER), box.key(NAME, POWER)[2])
    assert res.returncode == 1 and "INVALID: coefs: section 4 differs from the circuit in 1 rows, the first is row %d" % row in res.stdout


def test_a_ptau_of_another_tau_fails_every_populated_section(zk, box):
    key, _p0, p2 = box.key(NAME, POWER)
    populated = {n for n, f in (("A", "pointsA"), ("B1", "pointsB1"), ("B2", "pointsB2"), ("IC", "pointsIC"), ("C", "pointsC"), ("H", "pointsH"))
                 if np.asarray(key[f]).any()}
    assert populated == ALL6
    other = box.ptau(POWER, (TOXIC3[0] + 1, TOXIC3[1], TOXIC3[2]))
    rep = zk.zkey_verify(box.r1cs(NAME), other, p2, device=0)
    assert rep.verdict == 1 and rep.failed == populated and not rep.not_checked, rep


# ---------------------------------------------------------------- 6. malformed points
def verify_key(zk, box, key, name="malformed.zkey"):
    zp = str(box.dir / name)
    zkgen.write_zkey(key, zp)
    return zk.zkey_verify(box.r1cs(NAME), box.ptau(POWER), zp, device=0), zp


def off_curve(key, name, nb, i):
    key[name][nb * i + nb // 2] ^= 1                              # the low byte of y


def test_a_cofactor_point_in_b2_is_named(zk, box, monkeypatch):
    pts = golden_json("g2_cofactor_points.json")["cofactor"]
    dec = lambda p: ((int(p["x"][0]), int(p["x"][1])), (int(p["y"][0]), int(p["y"][1])))
    for route in ("", "1"):
        monkeypatch.setenv("ZKHIP_SUBGROUP_PLAIN", route)
        for at, p in ((5, pts[0]), (0, pts[3])):
            key = load_key(box.key(NAME, POWER)[2])
            key["pointsB2"][128 * at:128 * at + 128] = np.frombuffer(bn.g2_to_bytes(dec(p)), np.uint8)
            rep, zp = verify_key(zk, box, key)
            assert (rep.verdict, rep.bad_section, rep.bad_index, rep.bad_kind) == (2, 7, at, 3) and not rep.failed, rep
    res = cli(box.r1cs(NAME), box.ptau(POWER), zp)
    assert res.returncode == 1 and res.stdout == "INVALID: section 7: point 0 is not in the subgroup\n", (res.stdout, res.stderr)


def test_malformed_kinds_and_the_first_section_wins(zk, box):
    base = load_key(box.key(NAME, POWER)[2])
    nC = base["nVars"] - base["nPublic"] - 1
    key = copy.deepcopy(base)
    off_curve(key, "pointsC", 64, nC - 1)
    rep, _ = verify_key(zk, box, key)
    assert (rep.verdict, rep.bad_section, rep.bad_index, rep.bad_kind) == (2, 8, nC - 1, 2), rep
    key = copy.deepcopy(base)
    key["pointsH"][64 * 17:64 * 17 + 32] = np.frombuffer(QM.to_bytes(32, "little"), np.uint8)         # x = q
    rep, _ = verify_key(zk, box, key)
    assert (rep.verdict, rep.bad_section, rep.bad_index, rep.bad_kind) == (2, 9, 17, 1), rep
    key = copy.deepcopy(base)                                     # two in section 6, one in 5 after them, one in 8: section 5 wins
    off_curve(key, "pointsB1", 64, 9)
    off_curve(key, "pointsB1", 64, 4)
    off_curve(key, "pointsC", 64, 0)
    rep, _ = verify_key(zk, box, key)
    assert (rep.verdict, rep.bad_section, rep.bad_index, rep.bad_kind) == (2, 6, 4, 2), rep
    off_curve(key, "pointsA", 64, 30)
    rep, _ = verify_key(zk, box, key)
    assert (rep.verdict, rep.bad_section, rep.bad_index, rep.bad_kind) == (2, 5, 30, 2), rep
    key = copy.deepcopy(base)                                     # infinity is not legal in section 2: gamma2 is its point 3
    key["vk_gamma2"][:] = 0
    rep, _ = verify_key(zk, box, key)
    assert (rep.verdict, rep.bad_section, rep.bad_index, rep.bad_kind) == (2, 2, 3, 4), rep
