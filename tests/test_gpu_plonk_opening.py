"""PLONK rounds 4 and 5 on the GPU: evaluations, the linearisation polynomial F and the two opening proofs.  Exact
arithmetic: every expected value comes from Python integers (tests/plonk_opening_instance.py: the prover's side, reference
A, and the verifier's, reference B), F is compared byte for byte, and the proofs with [q(tau)] G at the known tau of a
trapdoor file."""
import ctypes
import functools
import random

import numpy as np
import pytest

import plonk_instance as pi
import plonk_opening_instance as po
from oracle import bn254 as bn

pytestmark = pytest.mark.gpu

R = bn.R_MOD
TAU, ALPHA, BETA = 0x1F3A9C5E77D1B2A49E0C6F5D3B8A17264C9E0F1D2B3A4958, 0x2B7E151628AED2A6ABF7158809CF4F3C, 0x3243F6A8885A308D313198A2E0370734
BIG = 0x1A3C09F0A58A7E8500E0A7EB8EF62ABC402D111E41112ED49BD61B6E725B19EF       # 253 bits, below r
MAX_COEFFS = (1 << 12) + 6
DEFAULT_SEG = 16
ints = pi.ints


def le(values):
    return np.frombuffer(pi.le(values), dtype=np.uint8)


def at_tau(coeffs):
    return bn.g1_to_bytes(bn.G1.mul(bn.G1_GEN, pi.horner(coeffs, TAU))) if coeffs else bytes(64)


def set_seg(monkeypatch, seg):
    if seg is None:
        monkeypatch.delenv("ZKHIP_OPEN_SEG", raising=False)
    else:
        monkeypatch.setenv("ZKHIP_OPEN_SEG", seg)


@pytest.fixture(scope="module")
def kzg(zk, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("plonk_opening") / "p12.ptau")
    zk.write_trapdoor_ptau(12, TAU, ALPHA, BETA, path, prepared=False)
    k = zk.Kzg.from_ptau(path, max_coeffs=MAX_COEFFS)
    yield k
    k.close()


@functools.lru_cache(maxsize=None)
def case(seed, log_n, blind=pi.BLIND, from_b=False, blind_parts=True, zeta=None, v=None, **kw):
    """(instance, parts, zeta, v, reference A), made once"""
    t = pi.oracle_b(pi.make(seed, log_n, blind, **dict(kw))) if from_b else None
    I, parts, ze, vv = po.make(seed, log_n, blind, t=t, blind_parts=blind_parts, zeta=zeta, v=v, **dict(kw))
    return I, parts, ze, vv, po.reference_a(I, parts, ze, vv)


def opening(zk, kzg, I, basis="monomial"):
    return zk.PlonkOpening(kzg, *[le(x) for x in I.circuit(basis)], pi.K1, pi.K2, basis=basis)


def rounds(o, I, parts, zeta, v, pi_zeta="instance", want_f=True):
    ev = o.evaluate(le(I.a), le(I.b), le(I.c), le(I.z), zeta)
    kw = {} if pi_zeta is None else {"pi_zeta": pi.horner(I.pi, zeta) if pi_zeta == "instance" else pi_zeta}
    return ev, o.open(le(parts[0]), le(parts[1]), le(parts[2]), I.alpha, I.beta, I.gamma, v, want_f=want_f, **kw)


def check(got, ref):
    """evaluate's and open's results against reference A: the values, F byte for byte, r(zeta), and both proofs"""
    ev, (wz, wzw, rz, f) = got
    assert ev == ref.evals
    assert f.size == len(ref.F) * 32 and ints(f) == ref.F
    assert rz == ref.r_zeta
    assert bytes(wz) == at_tau(ref.q_zeta) and bytes(wzw) == at_tau(ref.q_zw)


# ---------------------------------------------------------------- fr_poly_eval
@pytest.mark.parametrize("m", [1, 6])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1024 + 3, 4096])      # a ragged workgroup, exactly one, the first lane's second point, several partials
def test_poly_eval_matches_horner_at_every_segment(zk, monkeypatch, n, m):
    rng = random.Random(3100 + n)
    points = [0, 1, R - 1, bn.fr_root(max(n - 1, 1).bit_length()), rng.getrandbits(254) % R, BIG]
    polys = []
    for j in range(6):
        c = [rng.randrange(R) for _ in range(n)]
        c[0], c[-1] = ((0, R - 1), (R - 1, 0), (R - 1, R - 1))[j % 3] if n > 1 else (c[0], (0, R - 1, 1)[j % 3])
        polys.append(c)
    want = [pi.horner(c, z) for c, z in zip(polys, points)]
    seen = set()
    for seg in ("1", "3", None):
        set_seg(monkeypatch, seg)
        if m == 6:
            got = zk.fr_poly_eval(np.stack([le(c) for c in polys]), points)
        else:
            got = [zk.fr_poly_eval(c, z)[0] for c, z in zip(polys, points)]
        assert got == want, seg
        seen.add(tuple(got))
    assert len(seen) == 1


# ---------------------------------------------------------------- evaluate
@pytest.mark.parametrize("log_n", [3, 6, 11])
def test_evaluate_matches_horner(zk, kzg, log_n):
    I = pi.make(3200 + log_n, log_n, pi.BLIND)
    n = I.n
    assert [len(p) for p in (I.a, I.b, I.c, I.z)] == [n + 2, n + 2, n + 2, n + 3]
    zeta = po.challenges(3200 + log_n)[0]
    with opening(zk, kzg, I) as o:
        assert o.evaluate(le(I.a), le(I.b), le(I.c), le(I.z), zeta) == po.evaluations(I, zeta)
        assert o.info()["pending"] == 1 and o.info()["last_launches"] == 2


def test_evaluate_with_unequal_lengths_and_length_one(zk, kzg):
    I = pi.make(3231, 3, (0, 2, 5, 3))
    assert [len(p) for p in (I.a, I.b, I.c, I.z)] == [8, 10, 13, 11]
    with opening(zk, kzg, I) as o:
        for zeta in (BIG, 0, 1, R - 1, bn.fr_root(3)):
            assert o.evaluate(le(I.a), le(I.b), le(I.c), le(I.z), zeta) == po.evaluations(I, zeta)
        w = bn.fr_root(3)
        got = o.evaluate([5], [R - 1], [0], I.z[:1], BIG)
        assert got == [5, R - 1, 0, pi.horner(I.s1, BIG), pi.horner(I.s2, BIG), I.z[0]]
        full = [R - 1] * MAX_COEFFS
        assert o.evaluate(full, [1], [1], full, w)[::5] == [pi.horner(full, w), pi.horner(full, w * w % R)]


# ---------------------------------------------------------------- open against reference A
@pytest.mark.parametrize("log_n", [3, 4, 6, 8])
def test_open_matches_the_reference_blinded(zk, kzg, log_n):
    I, parts, zeta, v, ref = case(3300 + log_n, log_n)
    assert [len(p) for p in parts] == [I.n + 1, I.n + 1, I.n + 6] and len(ref.F) == I.n + 6 and ref.r_zeta == 0
    with opening(zk, kzg, I) as o:
        check(rounds(o, I, parts, zeta, v), ref)
        assert o.info()["pending"] == 0


def test_open_matches_the_reference_unblinded(zk, kzg):
    I, parts, zeta, v, ref = case(3313, 3, None, blind_parts=False)
    assert [len(p) for p in parts] == [I.n, I.n, I.n - 3] and len(ref.F) == I.n and ref.r_zeta == 0
    with opening(zk, kzg, I) as o:
        check(rounds(o, I, parts, zeta, v), ref)


def test_open_at_2_to_11_with_the_coset_route_quotient(zk, kzg):
    I, parts, zeta, v, ref = case(3311, 11, from_b=True)
    assert len(ref.F) == I.n + 6 and ref.r_zeta == 0
    b = po.reference_b(I, parts, zeta, v)
    assert b.F == ref.F and po.check_b(b, ref.q_zeta, ref.q_zw, 0)
    with opening(zk, kzg, I, "lagrange") as o:
        check(rounds(o, I, parts, zeta, v), ref)


def test_a_broken_gate_gives_the_references_non_zero_r_zeta(zk, kzg):
    I, parts, zeta, v, ref = case(3334, 4, break_gate=3)
    assert ref.r_zeta != 0 and ref.r_zeta == po.reference_b(I, parts, zeta, v).r_zeta
    with opening(zk, kzg, I) as o:
        check(rounds(o, I, parts, zeta, v), ref)


@pytest.mark.parametrize("edge", ["alpha0", "beta0", "gamma0", "v0", "v1", "zeta0", "zeta1", "zeta_omega"])
def test_open_at_the_edges_of_the_challenges(zk, kzg, edge):
    kw = {"alpha0": {"alpha": 0}, "beta0": {"beta": 0}, "gamma0": {"gamma": 0}, "v0": {"v": 0}, "v1": {"v": 1}, "zeta0": {"zeta": 0}, "zeta1": {"zeta": 1},
          "zeta_omega": {"zeta": bn.fr_root(4)}}[edge]
    I, parts, zeta, v, ref = case(3340, 4, **kw)
    assert ref.r_zeta == 0
    with opening(zk, kzg, I) as o:
        check(rounds(o, I, parts, zeta, v), ref)


def test_pi_zeta_given_and_omitted(zk, kzg):
    I, parts, zeta, v, ref = case(3351, 4, public=False)
    assert not any(I.pi) and ref.r_zeta == 0
    with opening(zk, kzg, I) as o:
        check(rounds(o, I, parts, zeta, v, pi_zeta=None), ref)
        check(rounds(o, I, parts, zeta, v, pi_zeta=0), ref)
    I, parts, zeta, v, ref = case(3352, 4)                # public inputs, and a caller that leaves them out: r(zeta) = -PI(zeta)
    without = po.reference_a(I, parts, zeta, v, pi_zeta=0)
    assert without.r_zeta == (R - pi.horner(I.pi, zeta)) % R != 0
    with opening(zk, kzg, I) as o:
        check(rounds(o, I, parts, zeta, v, pi_zeta=None), without)
        check(rounds(o, I, parts, zeta, v), ref)


def test_a_part_of_t_of_length_one(zk, kzg):
    """the parts are not checked to be the split of the quotient: F follows the parts it is given"""
    I, parts, zeta, v, _ = case(3300 + 4, 4)
    for odd in ((parts[0], parts[1], [7]), ([R - 1], parts[1], parts[2]), ([1], [0], [R - 1])):
        ref = po.reference_a(I, odd, zeta, v)
        assert ref.r_zeta != 0
        with opening(zk, kzg, I) as o:
            check(rounds(o, I, odd, zeta, v), ref)


@pytest.mark.parametrize("seg", ["1", "3", None])
def test_bytes_do_not_depend_on_the_segment(zk, kzg, monkeypatch, seg):
    """n + 6 = 518 coefficients: three workgroups of one a lane, one of three (the last lanes take two), one of sixteen"""
    set_seg(monkeypatch, seg)
    I, parts, zeta, v, ref = case(3369, 9)
    with opening(zk, kzg, I) as o:
        check(rounds(o, I, parts, zeta, v), ref)
        assert o.info()["seg"] == (int(seg) if seg else DEFAULT_SEG)


@pytest.mark.parametrize("basis", ["monomial", "lagrange"])
@pytest.mark.parametrize("log_n", [1, 6])
def test_both_bases_of_the_circuit_view(zk, kzg, basis, log_n):
    I, parts, zeta, v, ref = case(3370 + log_n, log_n, None, blind_parts=False)
    with opening(zk, kzg, I, basis) as o:
        check(rounds(o, I, parts, zeta, v), ref)


# ---------------------------------------------------------------- the verifier's equation, through existing entries only
def test_the_proofs_verify_and_a_changed_evaluation_does_not(zk, kzg):
    I, parts, zeta, v, ref = case(3306, 6)
    w = bn.fr_root(I.log_n)
    with opening(zk, kzg, I) as o:
        ev, (wz, wzw, rz, f) = rounds(o, I, parts, zeta, v)
    E = sum(pow(v, j + 1, R) * ev[j] for j in range(5)) % R
    cf, cz = kzg.commit(f), kzg.commit(le(I.z))
    zw = zeta * w % R
    assert list(kzg.verify(np.concatenate([cf, cz]), [zeta, zw], [(E + rz) % R, ev[5]], np.concatenate([wz, wzw]))) == [zk.kzg.VERIFY_OK] * 2
    bad = list(ev)
    bad[1] ^= 1 << 8                                       # one byte of b(zeta)
    bad[5] ^= 1 << 16                                      # one byte of z(zeta w)
    E_bad = sum(pow(v, j + 1, R) * bad[j] for j in range(5)) % R
    assert list(kzg.verify(np.concatenate([cf, cz]), [zeta, zw], [(E_bad + rz) % R, bad[5]], np.concatenate([wz, wzw]))) == [zk.kzg.VERIFY_INVALID] * 2


def test_agreement_with_the_route_through_kzg_open(zk, kzg):
    """six Kzg.open calls give evaluate's values, and Kzg.open of the reference's F gives W_zeta byte for byte"""
    I, parts, zeta, v, ref = case(3306, 6)
    w = bn.fr_root(I.log_n)
    with opening(zk, kzg, I) as o:
        ev, (wz, wzw, rz, f) = rounds(o, I, parts, zeta, v)
    old = [kzg.open(le(p), zeta)[0][0] for p in (I.a, I.b, I.c, I.s1, I.s2)]
    yz, pz = kzg.open(le(I.z), zeta * w % R)
    assert old + yz == ev
    yf, pf = kzg.open(le(ref.F), zeta)
    assert bytes(pf) == bytes(wz) and bytes(pz) == bytes(wzw) and yf[0] == ref.f_zeta == (ref.E + rz) % R


# ---------------------------------------------------------------- info
def test_info_reports_the_launches(zk, kzg):
    """evaluate: two launches.  open: the linearisation and, twice, Kzg.open's own launches (three of the division and the
    multiplication's)"""
    I, parts, zeta, v, ref = case(3306, 6)
    w = bn.fr_root(I.log_n)
    with opening(zk, kzg, I) as o:
        info = o.info()
        assert info["log_n"] == 6 and info["pending"] == 0 and info["seg"] == DEFAULT_SEG
        assert info["device_bytes"] >= (8 * I.n + 9 * MAX_COEFFS) * 32
        o.evaluate(le(I.a), le(I.b), le(I.c), le(I.z), zeta)
        assert o.info()["last_launches"] == 2 and o.info()["pending"] == 1
        o.open(le(parts[0]), le(parts[1]), le(parts[2]), I.alpha, I.beta, I.gamma, v)
        launches = o.info()["last_launches"]
    kzg.open(le(ref.F), zeta)
    of = kzg.info()["last_launches"]
    kzg.open(le(I.z), zeta * w % R)
    assert launches == 1 + of + kzg.info()["last_launches"]


# ---------------------------------------------------------------- refusals
def test_refusals_of_the_c_entries(zk, kzg, monkeypatch):
    from rapidsnark_old_amd import lib as L
    lib = zk.load_library()
    P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None       # noqa: E731

    def err(rc):
        assert rc == 1
        return lib.zk_last_error().decode()

    n = 4
    good, bad = le([1, 2, 3, 4]).copy(), le([1, 2, R, R + 1]).copy()
    names = ("ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3")

    def create(log_n=2, k1=2, swap=None, basis=0, device=-1, rows=good):
        v = L.zk_plonk_circuit_view()
        v.log_n, v.basis = log_n, basis
        for name in names:
            setattr(v, name, (bad if name == swap else rows).ctypes.data)
        ctypes.memmove(v.k1, pi.le([k1]), 32)
        ctypes.memmove(v.k2, pi.le([3]), 32)
        h = ctypes.c_void_p()
        return lib.zk_plonk_opening_create(ctypes.byref(h), kzg._handle(), ctypes.byref(v), device), h

    assert err(create(log_n=0)[0]) == "zk_plonk_opening_create: log_n 0 is outside 1 .. 25"
    assert err(create(log_n=26)[0]) == "zk_plonk_opening_create: log_n 26 is outside 1 .. 25"
    assert err(create(basis=7)[0]) == "zk_plonk_opening_create: basis 7 is unknown"
    assert err(create(log_n=13)[0]) == "zk_plonk_opening_create: n + 6 = 8198 exceeds the kzg's max_coeffs = 4102"
    assert err(create(device=77)[0]).startswith("zk_plonk_opening_create: device 77 is not the kzg's device ")
    assert err(create(k1=R)[0]) == "zk_plonk_opening_create: k1 is not below r"
    for name in names:
        assert err(create(swap=name)[0]) == "zk_plonk_opening_create: %s 2 is not below r" % name
    rc, h = create()
    assert rc == 0 and h
    ev, one, big = np.zeros(6 * 32, dtype=np.uint8), le([1]).copy(), le([R]).copy()
    wz, wzw, rz = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8), np.zeros(32, dtype=np.uint8)
    long = le([1] * (MAX_COEFFS + 1)).copy()

    def evaluate(a=good, al=n, b=good, bl=n, c=good, cl=n, z=good, zl=n, zeta=one):
        return lib.zk_plonk_evaluate(h, P(ev), P(a), al, P(b), bl, P(c), cl, P(z), zl, P(zeta))

    def open_(lo=good, ll=n, mid=good, ml=n, hi=good, hl=n, p=None, alpha=one, beta=one, gamma=one, v=one):
        return lib.zk_plonk_open(h, P(wz), P(wzw), P(rz), None, None, P(lo), ll, P(mid), ml, P(hi), hl, P(p), P(alpha), P(beta), P(gamma), P(v))

    assert err(open_()) == "zk_plonk_open: no evaluation is pending: call zk_plonk_evaluate first"
    assert err(evaluate(al=0)) == "zk_plonk_evaluate: a_len 0 is outside 1 .. max_coeffs = 4102"
    assert err(evaluate(z=long, zl=MAX_COEFFS + 1)) == "zk_plonk_evaluate: z_len 4103 is outside 1 .. max_coeffs = 4102"
    for j, name in enumerate("abcz"):
        assert err(evaluate(**{"abcz"[j]: bad})) == "zk_plonk_evaluate: %s 2 is not below r" % name
    assert err(evaluate(zeta=big)) == "zk_plonk_evaluate: zeta is not below r"
    assert err(open_()) == "zk_plonk_open: no evaluation is pending: call zk_plonk_evaluate first"       # a refused evaluate leaves none
    assert evaluate() == 0
    assert err(open_(ml=0)) == "zk_plonk_open: mid_len 0 is outside 1 .. max_coeffs = 4102"
    assert err(open_(hi=long, hl=MAX_COEFFS + 1)) == "zk_plonk_open: hi_len 4103 is outside 1 .. max_coeffs = 4102"
    assert err(open_(lo=bad)) == "zk_plonk_open: t_lo 2 is not below r"
    assert err(open_(mid=bad)) == "zk_plonk_open: t_mid 2 is not below r"
    assert err(open_(hi=bad)) == "zk_plonk_open: t_hi 2 is not below r"
    for name in ("alpha", "beta", "gamma", "v"):
        assert err(open_(**{name: big})) == "zk_plonk_open: %s is not below r" % name
    assert err(open_(p=big)) == "zk_plonk_open: pi_zeta is not below r"
    for value in ("0", "4097", "x"):
        monkeypatch.setenv("ZKHIP_OPEN_SEG", value)
        assert err(open_()) == "ZKHIP_OPEN_SEG: a number of coefficients per lane from 1 to 4096 expected"
        assert err(evaluate()) == "ZKHIP_OPEN_SEG: a number of coefficients per lane from 1 to 4096 expected"
        assert err(lib.zk_fr_poly_eval(P(rz), P(good), 4, 1, P(one), -1)) == "ZKHIP_OPEN_SEG: a number of coefficients per lane from 1 to 4096 expected"
    monkeypatch.setenv("ZKHIP_OPEN_SEG", "4096")
    assert open_() == 0                                    # the refused calls consumed nothing
    monkeypatch.delenv("ZKHIP_OPEN_SEG")
    assert err(open_()) == "zk_plonk_open: no evaluation is pending: call zk_plonk_evaluate first"       # open twice after one evaluate
    lib.zk_plonk_opening_destroy(h)


def test_python_refusals_and_use_after_close(zk, kzg):
    I, parts, zeta, v, ref = case(3300 + 3, 3)
    big = pi.make(3390, 13)
    with pytest.raises(ValueError, match="n \\+ 6 = 8198 exceeds the kzg's max_coeffs = 4102"):
        opening(zk, kzg, big)
    with pytest.raises(TypeError, match="a Kzg expected"):
        zk.PlonkOpening("p12.ptau", *[le(x) for x in I.circuit()], pi.K1, pi.K2)
    o = opening(zk, kzg, I)
    with pytest.raises(zk.ZkHipError, match="zk_plonk_open: no evaluation is pending: call zk_plonk_evaluate first"):
        o.open(le(parts[0]), le(parts[1]), le(parts[2]), I.alpha, I.beta, I.gamma, v)
    with pytest.raises(zk.ZkHipError, match="zk_plonk_evaluate: c 1 is not below r"):
        o.evaluate(le([1] * 4), le([1] * 4), le([1, R, 3, 4]), le([1] * 4), zeta)
    check(rounds(o, I, parts, zeta, v), ref)
    with pytest.raises(zk.ZkHipError, match="zk_plonk_open: no evaluation is pending"):
        o.open(le(parts[0]), le(parts[1]), le(parts[2]), I.alpha, I.beta, I.gamma, v)
    o.close()
    o.close()
    with pytest.raises(zk.ZkHipError, match="the PlonkOpening object is closed"):
        o.evaluate(le(I.a), le(I.b), le(I.c), le(I.z), zeta)
    with pytest.raises(zk.ZkHipError, match="the PlonkOpening object is closed"):
        o.info()
