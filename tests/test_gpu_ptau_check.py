"""The .ptau check on the GPU (zk_g2_in_subgroup, zk_g1_power_msm / zk_g2_power_msm, zk_fr_power_dft, zk_ptau_check,
ptau.ptau_check, `ptaucheck`): the operators against the big-integer oracle, whole files made on the CPU, and files
tampered with one thing at a time, where the expected value is the exact set of failed equations.

The subgroup tests are also the finite check behind the exactness of the endomorphism test: the
twist's group is cyclic of order r h2, h2 a product of four distinct primes, an endomorphism acts on each prime-order part
as a scalar, so a criterion that holds on G2 and fails on one non-zero point of each of the four parts holds exactly on
the order-r subgroup.  tests/golden/g2_cofactor_points.json holds those four points."""
import functools
import os
import random
import struct
import subprocess
import sys

import pytest

from conftest import ROOT, golden_json

from oracle import bn254 as bn
from rapidsnark_old_amd import ptau as P

pytestmark = pytest.mark.gpu
RM, QM = bn.R_MOD, bn.Q_MOD
BIN = os.path.join(ROOT, "rapidsnark-old_amd")
TAU, ALPHA, BETA = 1234567, 89101112, 13141516
TAU2, BETA2 = 7654321, 16151413
TOXIC3 = (0x1234567 * 0x89ABCDEF + 17, 0xA1FA << 200 | 99, 0xBE7A << 180 | 7)
S1, S2 = 0x1D0F5EED << 190 | 0xC0FFEE, 3
LAG = (12, 13, 14, 15)
NB = {2: 64, 3: 128, 4: 64, 5: 64, 6: 128, 12: 64, 13: 128, 14: 64, 15: 64}
GROUPS = {"g1": (bn.G1, bn.g1_to_bytes, bn.g1_from_bytes, 64), "g2": (bn.G2, bn.g2_to_bytes, bn.g2_from_bytes, 128)}


def g1(x):
    return bn.g1_to_bytes(bn.G1.mul(bn.G1.gen, x % RM))


def g2(x):
    return bn.g2_to_bytes(bn.G2.mul(bn.G2.gen, x % RM))


def fixture_points():
    d = golden_json("g2_cofactor_points.json")
    dec = lambda p: ((int(p["x"][0]), int(p["x"][1])), (int(p["y"][0]), int(p["y"][1])))
    return [dec(p) for p in d["cofactor"]], [dec(p) for p in d["outside"]]


# ---------------------------------------------------------------- the subgroup operator
SUBGROUP_SIZES = (1, 63, 64, 65, 257)
# the first and last lane of a wave and of a block (both 64 lanes), then their neighbours: 21 places, all below 257
PLACES = (0, 63, 64, 127, 128, 191, 192, 255, 256, 1, 2, 3, 62, 65, 66, 126, 129, 130, 190, 193, 254)
ROTATE = {1: 5, 63: 4, 64: 3, 65: 7, 257: 0}            # which special point comes first: n = 1 is a cofactor point


@functools.lru_cache(maxsize=None)
def subgroup_cases():
    """{n: (bytes of n points, expected flags)}: every special point of the issue's list, placed at wave and block edges"""
    E = bn.G2
    cof, outside = fixture_points()
    rng = random.Random(0x5B6)
    inside = [E.mul(E.gen, k) for k in (1, 2, RM - 1, rng.randrange(3, RM))]
    special = [(p, 1) for p in inside] + [(None, 1)] + [(p, 0) for p in cof]
    special += [(E.add(E.mul(E.gen, rng.randrange(1, RM)), p), 0) for p in cof] + [(p, 0) for p in outside]
    assert len(special) == len(PLACES) == 21
    filler = [E.mul(E.gen, rng.randrange(1, RM)) for _ in range(5)]
    out = {}
    for n in SUBGROUP_SIZES:
        pts, want = [filler[i % 5] for i in range(n)], [1] * n
        rot = special[ROTATE[n]:] + special[:ROTATE[n]]
        for place, (p, flag) in zip((q for q in PLACES if q < n), rot):
            pts[place], want[place] = p, flag
        out[n] = (b"".join(bn.g2_to_bytes(p) for p in pts), want)
    assert sum(1 for w in out[257][1] if w == 0) == 16
    return out


@pytest.mark.parametrize("n", SUBGROUP_SIZES)
def test_subgroup_verdicts(zk, n):
    data, want = subgroup_cases()[n]
    assert zk.g2_in_subgroup(data).tolist() == want


def test_subgroup_of_nothing_and_of_infinity(zk):
    assert zk.g2_in_subgroup(b"").size == 0
    assert zk.g2_in_subgroup(bytes(3 * 128)).tolist() == [1, 1, 1]


def test_subgroup_chunks(zk, monkeypatch):
    monkeypatch.setenv("ZKHIP_PTAU_CHUNK", "100")                            # 257 points: three chunks, the last short
    data, want = subgroup_cases()[257]
    assert zk.g2_in_subgroup(data).tolist() == want


def test_subgroup_plain_route_gives_the_same_bytes(zk, tmp_path):
    """[r] Q in a child process (the variable is read per call, but a child shows the program a user would run)"""
    cases = subgroup_cases()
    inp = str(tmp_path / "points.bin")
    with open(inp, "wb") as f:
        f.write(b"".join(cases[n][0] for n in SUBGROUP_SIZES))
    code = ("import sys; sys.path.insert(0, %r); import rapidsnark_old_amd as zk; d = open(%r, 'rb').read(); at = 0\n"
            "for n in %r:\n    print(zk.g2_in_subgroup(d[at:at + 128 * n]).tobytes().hex()); at += 128 * n\n" % (ROOT, inp, SUBGROUP_SIZES))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, ZKHIP_SUBGROUP_PLAIN="1"))
    assert res.returncode == 0, res.stderr
    got = res.stdout.split()
    assert got == [bytes(cases[n][1]).hex() for n in SUBGROUP_SIZES]
    assert got == [zk.g2_in_subgroup(cases[n][0]).tobytes().hex() for n in SUBGROUP_SIZES]


def test_subgroup_names_a_point_off_the_twist(zk):
    data = bytearray(subgroup_cases()[65][0])
    data[64 * 128 + 3] ^= 1
    data[40 * 128 + 70] ^= 1
    with pytest.raises(zk.ZkHipError, match="zk_g2_in_subgroup: point 40 is not on the curve"):
        zk.g2_in_subgroup(bytes(data))
    bad = bytearray(subgroup_cases()[1][0] * 2)
    bad[128:160] = QM.to_bytes(32, "little")                                # a coordinate that is not below q
    with pytest.raises(zk.ZkHipError, match="point 1 is not on the curve"):
        zk.g2_in_subgroup(bytes(bad))


# ---------------------------------------------------------------- the power MSM
@functools.lru_cache(maxsize=None)
def msm_points(group):
    E = GROUPS[group][0]
    rng = random.Random("msm" + group)
    pts = [E.mul(E.gen, rng.randrange(1, RM)) for _ in range(17)]
    pts[3] = None                                                           # infinity
    pts[5] = pts[4]                                                         # P_i = P_j
    pts[9] = E.neg(pts[4])
    pts[12] = None
    return pts


@pytest.mark.parametrize("group", ["g1", "g2"])
@pytest.mark.parametrize("n", [1, 2, 3, 17])
def test_power_msm_against_the_oracle(zk, group, n):
    E, to_bytes, _, nb = GROUPS[group]
    fn = zk.g1_power_msm if group == "g1" else zk.g2_power_msm
    pts = msm_points(group)[:n]
    data = b"".join(to_bytes(p) for p in pts)
    rng = random.Random(n)
    for s in (rng.randrange(2, RM), 1):
        for first in (0, 5):
            want = E.msm(pts, [pow(s, first + i, RM) for i in range(n)])
            assert fn(data, s, first) == to_bytes(want), (s, first)


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_power_msm_edge_scalars_and_inputs(zk, group):
    E, to_bytes, _, nb = GROUPS[group]
    fn = zk.g1_power_msm if group == "g1" else zk.g2_power_msm
    pts = msm_points(group)
    data = b"".join(to_bytes(p) for p in pts)
    assert fn(b"", 7) == bytes(nb)                                          # nothing
    assert fn(bytes(4 * nb), 7) == bytes(nb)                                # nothing but infinity
    assert fn(data, 0) == to_bytes(pts[0])                                  # 0^0 = 1
    assert fn(data, 0, 3) == bytes(nb)
    assert fn(to_bytes(pts[4]) * 6, RM - 1) == bytes(nb)                    # P - P + P - P + P - P
    with pytest.raises(zk.ZkHipError, match="not below r"):
        fn(data, RM)
    bad = bytearray(data)
    bad[7 * nb + 1] ^= 2
    with pytest.raises(zk.ZkHipError, match="point 7 is not on the curve"):
        fn(bytes(bad), 5)


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_power_msm_in_chunks_against_the_plain_msm(zk, group, monkeypatch):
    """3000 points, chunks of 1024 (three, the last short), against zk_msm_* with scalars made on the host"""
    E, to_bytes, _, nb = GROUPS[group]
    chain, msm, fn = (zk.synth_chain_g1, zk.msm_g1, zk.g1_power_msm) if group == "g1" else (zk.synth_chain_g2, zk.msm_g2, zk.g2_power_msm)
    n, s, first = 3000, 0xABCDEF << 200 | 12345, 9
    pts = chain(n, to_bytes(E.mul(E.gen, 11)), to_bytes(E.mul(E.gen, 5))).tobytes()
    scalars = b"".join(pow(s, first + i, RM).to_bytes(32, "little") for i in range(n))
    want = msm(pts, scalars)
    monkeypatch.setenv("ZKHIP_PTAU_CHUNK", "1024")
    assert fn(pts, s, first) == want
    monkeypatch.delenv("ZKHIP_PTAU_CHUNK")
    assert fn(pts, s, first) == want                                        # and in one piece


# ---------------------------------------------------------------- the DFT of the powers
@pytest.mark.parametrize("log_n", range(7))
def test_power_dft_against_the_oracle(zk, log_n):
    n = 1 << log_n
    rng = random.Random(log_n)
    for s in (0, 1, pow(bn.fr_root(3), -3, RM), rng.randrange(2, RM)):      # the third: s w^j = 1 for one j from n = 8 on
        want = bn.ntt([pow(s, i, RM) for i in range(n)])
        assert zk.fr_power_dft(s, log_n) == want, s
    if log_n >= 3:
        s = pow(bn.fr_root(3), -3, RM)
        assert sum(1 for j in range(n) if s * pow(bn.fr_root(log_n), j, RM) % RM == 1) == 1


def test_power_dft_of_2_to_the_12_against_the_ntt(zk, monkeypatch):
    s, n = 0x5EED << 230 | 77, 1 << 12
    powers = b"".join(bn.to_mont(pow(s, i, RM), RM).to_bytes(32, "little") for i in range(n))
    raw = zk.fr_ntt(powers)
    want = [bn.from_mont(int.from_bytes(raw[32 * j:32 * j + 32], "little"), RM) for j in range(n)]
    assert zk.fr_power_dft(s, 12) == want
    monkeypatch.setenv("ZKHIP_PTAU_CHUNK", "1001")                           # chunks that are no multiple of a lane's four values
    assert zk.fr_power_dft(s, 12) == want


# ---------------------------------------------------------------- whole files made on the CPU
def lagrange(tau, n, zero_top=False, inverse_root=True):
    """L_j^(n)(tau) = 1/n sum_k tau^k w^-jk, the top power left out on request; inverse_root=False: with w in place of 1/w,
    the mistake of taking the wrong transform direction"""
    w = bn.fr_root(n.bit_length() - 1)
    wj, ninv = (pow(w, -1, RM) if inverse_root else w), pow(n, -1, RM)
    kmax = n - 1 if zero_top else n
    return [sum(pow(tau, k, RM) * pow(wj, j * k, RM) for k in range(kmax)) * ninv % RM for j in range(n)]


@functools.lru_cache(maxsize=None)
def make_sections(power, tau=TAU, alpha=ALPHA, beta=BETA, prepared=True, inverse_root=True):
    n = 1 << power
    secs = {
        1: struct.pack("<I", 32) + QM.to_bytes(32, "little") + struct.pack("<II", power, power),
        2: b"".join(g1(pow(tau, i, RM)) for i in range(2 * n - 1)),
        3: b"".join(g2(pow(tau, i, RM)) for i in range(n)),
        4: b"".join(g1(alpha * pow(tau, i, RM)) for i in range(n)),
        5: b"".join(g1(beta * pow(tau, i, RM)) for i in range(n)),
        6: g2(beta),
        7: struct.pack("<I", 0),
    }
    if prepared:
        levels = lambda top, zt: [lagrange(tau, 1 << p, zero_top=(zt and p == top), inverse_root=inverse_root) for p in range(top + 1)]
        l12 = [x for lvl in levels(power + 1, True) for x in lvl]
        l13 = [x for lvl in levels(power, False) for x in lvl]
        secs.update({12: b"".join(g1(x) for x in l12), 13: b"".join(g2(x) for x in l13),
                     14: b"".join(g1(alpha * x) for x in l13), 15: b"".join(g1(beta * x) for x in l13)})
    return secs


def build(secs):
    out = [b"ptau", struct.pack("<II", 1, len(secs))]
    for sid, payload in secs.items():
        out += [struct.pack("<IQ", sid, len(payload)), payload]
    return b"".join(out)


def cli(tmp_path, data, s=S1, name="f.ptau"):
    path = str(tmp_path / name)
    if data is not None:
        with open(path, "wb") as f:
            f.write(data)
    env = dict(os.environ)
    if s is not None:
        env["ZKHIP_PTAU_CHECK_SCALAR"] = str(s)
    return subprocess.run([os.path.join(BIN, "ptaucheck"), path], capture_output=True, text=True, timeout=300, env=env)


def no_lagrange():
    return {sid: set() for sid in LAG}


@pytest.mark.parametrize("prepared", [False, True])
@pytest.mark.parametrize("power", [1, 2, 3])
def test_good_files_are_ok(zk, tmp_path, power, prepared):
    data = build(make_sections(power, prepared=prepared))
    for s in (S1, S2, None):                                                # None: the library draws s
        rep = zk.ptau_check(data, s=s)
        assert rep.ok and rep.verdict == 0 and rep.failed == set() and rep.lagrange_failed == no_lagrange(), (s, rep)
        assert rep.prepared == prepared
    res = cli(tmp_path, data, s=None)
    assert res.returncode == 0 and res.stdout.startswith("OK: power %d" % power) and res.stderr == "", (res.stdout, res.stderr)
    assert ("present and were checked" in res.stdout) == prepared and ("no Lagrange sections" in res.stdout) == (not prepared)


def replaced(secs, sid, payload):
    s = dict(secs)
    s[sid] = payload
    return s


def patched(secs, sid, index, new):
    nb = NB[sid]
    s = dict(secs)
    s[sid] = s[sid][:index * nb] + new + s[sid][(index + 1) * nb:]
    return s


def doubled(secs, sid, index):
    E, to_bytes, from_bytes, nb = GROUPS["g2" if NB[sid] == 128 else "g1"]
    p = from_bytes(secs[sid][index * nb:(index + 1) * nb])
    assert p is not None
    return patched(secs, sid, index, to_bytes(E.dbl(p)))


def level_point(p, j):
    return (1 << p) - 1 + j


@functools.lru_cache(maxsize=None)
def tamper_cases():
    """name -> (sections, failed, lagrange_failed) at power 3 (N = 8)"""
    N = 8
    base = make_sections(3)
    other = make_sections(3, tau=TAU2)
    c = {}
    # A prepared file's Lagrange sections are checked against the powers IN THE FILE, so a changed power P_k also fails every
    # level of its Lagrange section that contains it: the levels p with 2^p > k.  (Changing it in an unprepared file gives
    # the same `failed` and nothing else: test_tampering_an_unprepared_file.)
    above = lambda k, top: {p for p in range(top + 1) if (1 << p) > k}
    # T_1 is the tau-point section 3 is measured against, so doubling it fails section 3's equation too; the other
    # indices of section 2 leave that equation alone
    c["T_1"] = (doubled(base, 2, 1), {2, 3}, {12: above(1, 4)})
    for k in (2, N, 2 * N - 2):
        c["T_%d" % k] = (doubled(base, 2, k), {2}, {12: above(k, 4)})
    for k in (2, N - 1):
        c["U_%d" % k] = (doubled(base, 3, k), {3}, {13: above(k, 3)})
    c["U_1"] = (doubled(base, 3, 1), {2, 3, 4, 5}, {13: above(1, 3)})       # the G1 rows are measured against U_1
    c["section_3_of_another_tau"] = (replaced(base, 3, other[3]), {2, 3, 4, 5}, {13: above(1, 3)})     # U_0 = G2 whatever tau is
    c["section_4_of_another_tau"] = (replaced(base, 4, other[4]), {4}, {14: above(1, 3)})
    c["B_2"] = (doubled(base, 5, 2), {5}, {15: above(2, 3)})
    c["beta2_of_another_beta"] = (replaced(base, 6, g2(BETA2)), {6}, {})
    c["T_0"] = (patched(base, 2, 0, g1(2)), {0, 2}, {12: above(0, 4)})
    for p in (0, 2, 4):
        c["section_12_level_%d" % p] = (doubled(base, 12, level_point(p, (1 << p) - 1)), set(), {12: {p}})
    c["section_13_level_3"] = (doubled(base, 13, level_point(3, 0)), set(), {13: {3}})
    c["section_14_level_1"] = (doubled(base, 14, level_point(1, 1)), set(), {14: {1}})
    c["section_15_level_2"] = (doubled(base, 15, level_point(2, 2)), set(), {15: {2}})
    a, b = level_point(3, 1), level_point(3, 6)
    pa, pb = base[12][a * 64:(a + 1) * 64], base[12][b * 64:(b + 1) * 64]
    c["section_12_two_points_swapped"] = (patched(patched(base, 12, a, pb), 12, b, pa), set(), {12: {3}})
    # the transform taken with w instead of 1/w: every level of 4 points or more comes out reversed, levels 0 and 1 do not change
    wrong = make_sections(3, inverse_root=False)
    assert all(wrong[sid][:3 * NB[sid]] == base[sid][:3 * NB[sid]] and wrong[sid] != base[sid] for sid in LAG)
    c["lagrange_of_the_wrong_root"] = (wrong, set(), {12: {2, 3, 4}, 13: {2, 3}, 14: {2, 3}, 15: {2, 3}})
    return c


@pytest.mark.parametrize("name", ["T_1", "T_2", "T_8", "T_14", "U_2", "U_7", "U_1", "section_3_of_another_tau", "section_4_of_another_tau", "B_2",
                                  "beta2_of_another_beta", "T_0", "section_12_level_0", "section_12_level_2", "section_12_level_4",
                                  "section_13_level_3", "section_14_level_1", "section_15_level_2", "section_12_two_points_swapped",
                                  "lagrange_of_the_wrong_root"])
def test_tampering_is_reported_as_the_exact_set(zk, tmp_path, name):
    secs, failed, lag = tamper_cases()[name]
    want_lag = no_lagrange()
    want_lag.update(lag)
    data = build(secs)
    for s in (S1, S2):
        rep = zk.ptau_check(data, s=s)
        assert rep.verdict == 1 and not rep.ok, rep
        assert rep.failed == failed and rep.lagrange_failed == want_lag, rep
    res = cli(tmp_path, data)
    assert res.returncode == 1 and res.stderr == "", (res.stdout, res.stderr)
    lines = res.stdout.splitlines()
    assert all(l.startswith("INVALID: ") for l in lines)
    assert len(lines) == len(failed) + sum(len(v) for v in lag.values())
    for sid in failed - {0, 6}:
        assert any("section %d (" % sid in l and "is not a sequence of powers of the file's tau" in l for l in lines)
    for sid, levels in lag.items():
        for p in levels:
            assert "INVALID: section %d, level %d is not the Lagrange form of section %d" % (sid, p, sid - 10) in lines


def test_tamper_cases_cover_the_list():
    assert len(tamper_cases()) == 20


@pytest.mark.parametrize("name,failed", [("T_1", {2, 3}), ("T_14", {2}), ("U_7", {3}), ("U_1", {2, 3, 4, 5}), ("B_2", {5}), ("T_0", {0, 2})])
def test_tampering_an_unprepared_file(zk, name, failed):
    secs = {sid: v for sid, v in tamper_cases()[name][0].items() if sid not in LAG}
    rep = zk.ptau_check(build(secs), s=S1)
    assert rep.verdict == 1 and rep.failed == failed and rep.lagrange_failed == no_lagrange() and not rep.prepared, rep


# ---------------------------------------------------------------- malformed points
def test_a_point_outside_the_subgroup_is_named(zk, tmp_path):
    base = make_sections(3)
    cof, _ = fixture_points()
    p = bn.G2.add(bn.g2_from_bytes(base[3][5 * 128:6 * 128]), cof[0])       # + the point of order 10069
    bad = patched(base, 3, 5, bn.g2_to_bytes(p))
    bad = doubled(bad, 4, 1)                                                # an equation that would fail is not reported
    rep = zk.ptau_check(build(bad), s=S1)
    assert (rep.verdict, rep.bad_section, rep.bad_index, rep.bad_kind) == (2, 3, 5, 3) and rep.failed == set() and not rep.ok
    res = cli(tmp_path, build(bad))
    assert res.returncode == 1 and res.stdout == "INVALID: section 3: point 5 is not in the subgroup\n" and res.stderr == ""
    in13 = patched(base, 13, 6, bn.g2_to_bytes(bn.G2.add(bn.g2_from_bytes(base[13][6 * 128:7 * 128]), cof[3])))
    rep = zk.ptau_check(build(in13), s=S1)
    assert (rep.verdict, rep.bad_section, rep.bad_index, rep.bad_kind) == (2, 13, 6, 3)
    in6 = replaced(base, 6, bn.g2_to_bytes(bn.G2.add(bn.g2_from_bytes(base[6]), cof[1])))
    rep = zk.ptau_check(build(in6), s=S1)
    assert (rep.verdict, rep.bad_section, rep.bad_index, rep.bad_kind) == (2, 6, 0, 3)


def test_malformed_kinds_and_the_first_section_wins(zk, tmp_path):
    base = make_sections(3)
    x, y = bn.g1_from_bytes(base[4][3 * 64:4 * 64])
    off = patched(base, 4, 3, bn.g1_to_bytes((x, (y + 1) % QM)))
    rep = zk.ptau_check(build(off), s=S1)
    assert (rep.verdict, rep.bad_section, rep.bad_index, rep.bad_kind) == (2, 4, 3, 2)
    res = cli(tmp_path, build(off))
    assert res.returncode == 1 and res.stdout == "INVALID: section 4: point 3 is not on the curve\n"
    big = patched(base, 5, 2, QM.to_bytes(32, "little") + base[5][2 * 64 + 32:3 * 64])
    rep = zk.ptau_check(build(big), s=S1)
    assert (rep.verdict, rep.bad_section, rep.bad_index, rep.bad_kind) == (2, 5, 2, 1)
    inf = patched(patched(base, 2, 9, bytes(64)), 2, 11, bytes(64))
    rep = zk.ptau_check(build(inf), s=S1)
    assert (rep.verdict, rep.bad_section, rep.bad_index, rep.bad_kind) == (2, 2, 9, 4)
    res = cli(tmp_path, build(inf))
    assert res.returncode == 1 and res.stdout == "INVALID: section 2: point 9 is the point at infinity\n"
    both = patched(patched(off, 14, 0, off[14][:32] + bytes(32)), 3, 7, bytes(128))      # sections 3, 4 and 14: section 3 is named
    rep = zk.ptau_check(build(both), s=S1)
    assert (rep.verdict, rep.bad_section, rep.bad_index, rep.bad_kind) == (2, 3, 7, 4)
    g2off = bytearray(base[13])
    g2off[4 * 128 + 100] ^= 8
    rep = zk.ptau_check(build(replaced(base, 13, bytes(g2off))), s=S1)
    assert (rep.verdict, rep.bad_section, rep.bad_index, rep.bad_kind) == (2, 13, 4, 2)


def test_infinity_is_legal_in_the_lagrange_sections(zk, tmp_path):
    """tau = 1: every power is the generator and L_j(1) = 0 for j > 0, so most Lagrange points are at infinity"""
    secs = make_sections(2, tau=1)
    assert secs[12][128:192] == bytes(64) and secs[13][256:384] == bytes(128)      # L_1^(2)(1) = (1 - 1) / 2
    rep = zk.ptau_check(build(secs), s=S1)
    assert rep.ok and rep.failed == set() and rep.lagrange_failed == no_lagrange(), rep
    assert cli(tmp_path, build(secs)).returncode == 0
    rep = zk.ptau_check(build(patched(secs, 12, 2, g1(1))), s=S1)            # a point where infinity belongs
    assert rep.verdict == 1 and rep.failed == set() and rep.lagrange_failed == replaced(no_lagrange(), 12, {1})


# ---------------------------------------------------------------- chunk boundaries
@pytest.fixture(scope="module")
def power12(zk, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ptau12") / "p12.ptau")
    zk.write_trapdoor_ptau(12, *TOXIC3, path)
    with open(path, "rb") as f:
        data = f.read()
    pf = P.PtauFile(data)
    at = {sid: pf.sections[sid][0] for sid in (2, 13)}
    pf.close()
    return data, at


def double_in_file(zk, data, pos, nb):
    mul = zk.g1_mul if nb == 64 else zk.g2_mul
    return data[:pos] + mul(data[pos:pos + nb], 2) + data[pos + nb:]


@pytest.mark.parametrize("case", ["untouched", "first_of_the_second_chunk", "last_of_section_2", "last_of_the_top_level_of_13"])
def test_chunk_boundaries(zk, power12, monkeypatch, case):
    data, at = power12
    monkeypatch.setenv("ZKHIP_PTAU_CHUNK", "1024")
    assert P.ptau_check_sizes(data) == dict(P.ptau_check_sizes(data), prepared=1, chunk_points=1024)
    want_failed, want_lag = set(), no_lagrange()
    if case == "first_of_the_second_chunk":
        data, want_failed = double_in_file(zk, data, at[2] + 1024 * 64, 64), {2}
        want_lag[12] = {11, 12, 13}                                         # the levels that hold power 1024
    elif case == "last_of_section_2":
        data, want_failed = double_in_file(zk, data, at[2] + ((2 << 12) - 2) * 64, 64), {2}
        want_lag[12] = {13}
    elif case == "last_of_the_top_level_of_13":
        data = double_in_file(zk, data, at[13] + ((2 << 12) - 2) * 128, 128)
        want_lag[13] = {12}
    rep = zk.ptau_check(data, s=S1)
    assert rep.verdict == (0 if case == "untouched" else 1), rep
    assert rep.failed == want_failed and rep.lagrange_failed == want_lag, rep


# ---------------------------------------------------------------- the chain
def test_ptaucheck_accepts_what_ptauprepare_writes(zk, tmp_path):
    bare, out = str(tmp_path / "bare.ptau"), str(tmp_path / "out.ptau")
    with open(bare, "wb") as f:
        f.write(build(make_sections(3, prepared=False)))
    res = subprocess.run([os.path.join(BIN, "ptauprepare"), bare, out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    for path, prepared in ((bare, False), (out, True)):
        res = subprocess.run([os.path.join(BIN, "ptaucheck"), path], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0 and res.stdout.startswith("OK: power 3"), (res.stdout, res.stderr)
        assert ("present and were checked" in res.stdout) == prepared
