"""KZG over a .ptau on the GPU: division by X - z, commit, open, verify, verify_batch, create.  Exact arithmetic: every
expected value comes from Python integers and oracle.bn254 on trapdoor files whose tau is known (p(tau) G, q(tau) G, p(z)),
and is compared byte for byte.  The files: power 6 prepared and power 10 not prepared, made once per session."""
import ctypes
import random

import numpy as np
import pytest

from oracle import bn254 as bn
from conftest import golden_json

pytestmark = pytest.mark.gpu

R, Q = bn.R_MOD, bn.Q_MOD
TAU, ALPHA, BETA = 0x1F3A9C5E77D1B2A49E0C6F5D3B8A17264C9E0F1D2B3A4958, 0x2B7E151628AED2A6ABF7158809CF4F3C, 0x3243F6A8885A308D313198A2E0370734
TAU2 = TAU + 12345
OK, INVALID, MALFORMED = 0, 1, 2
DEFAULT_SEG = 16                                       # ZKHIP_KZG_SEG when the variable is not set: zk_kzg_info reports it
SEGS = {"seg1": "1", "seg3": "3", "default": None}


# ---------------------------------------------------------------- the oracle
def le(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8)


def ints(rows):
    b = bytes(rows)
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def divide(c, z):
    """Horner: (q, y) with q (X - z) + y = p"""
    q, t = [0] * (len(c) - 1), 0
    for i in range(len(c) - 1, 0, -1):
        t = (c[i] + z * t) % R
        q[i - 1] = t
    return q, (c[0] + z * t) % R


def evaluate(c, x):
    t = 0
    for v in reversed(c):
        t = (v + x * t) % R
    return t


def commitment(c, tau=TAU):
    return bn.g1_to_bytes(bn.G1.mul(bn.G1_GEN, evaluate(c, tau)))


def poly(rng, n, special=True):
    c = [rng.getrandbits(253) for _ in range(n)] if n > 5000 else [rng.randrange(R) for _ in range(n)]      # 2^253 < r
    if special and n >= 4:
        c[rng.randrange(n)] = 0
        c[rng.randrange(n)] = R - 1
    return c


def with_root(rng, n, z):
    """n coefficients of (X - z) g(X), g random of n - 1 coefficients"""
    g = poly(rng, n - 1, special=False)
    return [(-z * g[0]) % R] + [(g[i - 1] - z * g[i]) % R for i in range(1, n - 1)] + [g[n - 2]]


# ---------------------------------------------------------------- the files and the objects
@pytest.fixture(scope="session")
def files(zk, tmp_path_factory):
    d = tmp_path_factory.mktemp("kzg")
    paths = {"p6": str(d / "p6.ptau"), "p10": str(d / "p10.ptau"), "other": str(d / "other.ptau")}
    zk.write_trapdoor_ptau(6, TAU, ALPHA, BETA, paths["p6"])
    zk.write_trapdoor_ptau(10, TAU, ALPHA, BETA, paths["p10"], prepared=False)
    zk.write_trapdoor_ptau(6, TAU2, ALPHA, BETA, paths["other"], prepared=False)
    return paths


@pytest.fixture(scope="module")
def k6(zk, files):
    k = zk.Kzg.from_ptau(files["p6"], lagrange_log_n=6)
    yield k
    k.close()


@pytest.fixture(scope="module")
def k10(zk, files):
    k = zk.Kzg.from_ptau(files["p10"])
    yield k
    k.close()


@pytest.fixture(scope="module")
def openings(k10):
    """valid openings of two polynomials of 17 coefficients at three points: (C, z, y, pi) as bytes / ints, checked against
    the oracle once"""
    rng = random.Random(99)
    p = [poly(rng, 17), poly(rng, 17)]
    z = [rng.randrange(R) for _ in range(3)]
    C = bytes(k10.commit(p))
    out = []
    for j in range(2):
        for zz in z:
            ys, pi = k10.open(p[j], zz)
            q, y = divide(p[j], zz)
            assert ys == [y] and bytes(pi) == commitment(q) and C[64 * j:64 * j + 64] == commitment(p[j])
            out.append((C[64 * j:64 * j + 64], zz, y, bytes(pi)))
    return out


def pack(ops):
    return b"".join(o[0] for o in ops), [o[1] for o in ops], [o[2] for o in ops], b"".join(o[3] for o in ops)


# ---------------------------------------------------------------- division
def tier_sizes(seg):
    """n = 1, 2, 3 and b - 1, b, b + 1, 2 b + 1 around every boundary b of the scan at `seg` coefficients a lane: a lane's
    segment, a wave (64 lanes), a workgroup (4 waves), and the carry pass, whose lanes take one workgroup sum each up to 256
    workgroups and more beyond"""
    out = [("small", n) for n in (1, 2, 3)]
    for tier, b in (("lane", seg), ("wave", 64 * seg), ("workgroup", 256 * seg), ("carry", 65536 * seg)):
        out += [(tier, n) for n in (b - 1, b, b + 1, 2 * b + 1) if n >= 1]
    seen, uniq = set(), []
    for tier, n in out:
        if n not in seen:
            seen.add(n)
            uniq.append((tier, n))
    return uniq


DIV_CASES = [pytest.param(name, tier, n, id="%s-%s-%d" % (name, tier, n))
             for name, env in SEGS.items() for tier, n in tier_sizes(int(env) if env else DEFAULT_SEG)]


def set_seg(monkeypatch, name):
    if SEGS[name] is None:
        monkeypatch.delenv("ZKHIP_KZG_SEG", raising=False)
    else:
        monkeypatch.setenv("ZKHIP_KZG_SEG", SEGS[name])


@pytest.mark.parametrize("name,tier,n", DIV_CASES)
def test_division_equals_horner_at_every_tier_boundary(zk, monkeypatch, name, tier, n):
    set_seg(monkeypatch, name)
    rng = random.Random(n * 7 + len(name))
    if n > 5000:                                       # Fr only, one pass of Python over the coefficients
        c, z = poly(rng, n), rng.randrange(R)
        q, y = zk.fr_poly_divide(le(c), z)
        wq, wy = divide(c, z)
        assert y == wy and bytes(q) == bytes(le(wq))
        return
    c = poly(rng, n)
    for z in (0, 1, R - 1, rng.randrange(R)):
        q, y = zk.fr_poly_divide(c, z)
        wq, wy = divide(c, z)
        assert y == wy and bytes(q) == bytes(le(wq)), (n, z)
        t = rng.randrange(R)                           # q (X - z) + y = p at a random point
        assert (evaluate(ints(q), t) * (t - z) + y) % R == evaluate(c, t)
    if n >= 2:                                         # z a root of p: y = 0
        z = rng.randrange(R)
        c = with_root(rng, n, z)
        q, y = zk.fr_poly_divide(c, z)
        assert y == 0 and bytes(q) == bytes(le(divide(c, z)[0]))


@pytest.mark.parametrize("name", list(SEGS))
def test_division_special_coefficients(zk, monkeypatch, name):
    set_seg(monkeypatch, name)
    rng = random.Random(5)
    seg = int(SEGS[name] or DEFAULT_SEG)
    for n in (1, 2, 64 * seg + 3, 256 * seg + 5):
        lead0 = poly(rng, n)
        lead0[-1] = 0                                  # a zero leading coefficient
        for c in (lead0, [0] * n, [R - 1] * n, [0] * (n - 1) + [1]):
            for z in (0, 1, R - 1, rng.randrange(R)):
                q, y = zk.fr_poly_divide(c, z)
                wq, wy = divide(c, z)
                assert y == wy and bytes(q) == bytes(le(wq)), (n, z)


def test_division_refuses_values_not_below_r_and_a_bad_knob(zk, monkeypatch):
    c = le([1, 2, 3, 4, 5, 6, 7]).copy()
    c[5 * 32:6 * 32] = le([R])
    with pytest.raises(zk.ZkHipError, match="zk_fr_poly_divide: coefficient 5 is not below r"):
        zk.fr_poly_divide(c, 3)
    with pytest.raises(zk.ZkHipError, match="zk_fr_poly_divide: z is not below r"):
        zk.fr_poly_divide(le([1, 2, 3]), le([R]))
    lib = zk.load_library()
    y = np.zeros(32, dtype=np.uint8)
    assert lib.zk_fr_poly_divide(None, y.ctypes.data, y.ctypes.data, 0, y.ctypes.data, -1) == 1
    assert b"zk_fr_poly_divide: n is 0" in lib.zk_last_error()
    for bad in ("0", "4097", "x", "-1"):
        monkeypatch.setenv("ZKHIP_KZG_SEG", bad)
        with pytest.raises(zk.ZkHipError, match="ZKHIP_KZG_SEG: a number of coefficients per lane from 1 to 4096 expected"):
            zk.fr_poly_divide([1, 2, 3], 3)
    monkeypatch.setenv("ZKHIP_KZG_SEG", "4096")                          # the largest the knob takes: one lane holds it all
    c = poly(random.Random(4096), 4097)
    q, y = zk.fr_poly_divide(c, 7)
    assert (bytes(q), y) == (bytes(le(divide(c, 7)[0])), divide(c, 7)[1])


# ---------------------------------------------------------------- commit
@pytest.mark.parametrize("n", [1, 2, 17, 2047])
@pytest.mark.parametrize("m", [1, 3])
def test_commit_monomial(k10, n, m):
    rng = random.Random(n + m)
    p = [poly(rng, n) for _ in range(m)]
    got = bytes(k10.commit(p if m > 1 else p[0]))
    assert got == b"".join(commitment(c) for c in p)
    assert bytes(k10.commit(np.stack([le(c) for c in p]))) == got      # rows of bytes, a second call: the same bytes


def test_commit_lagrange_and_the_basis_convention(zk, k6):
    rng = random.Random(64)
    ev = [poly(rng, 64) for _ in range(3)]
    got = bytes(k6.commit(ev, basis="lagrange"))
    coeffs = [bn.ntt(e, inverse=True) for e in ev]      # evaluations at w^j -> coefficients
    assert got == b"".join(commitment(c) for c in coeffs)
    assert bytes(k6.commit(ev[0], basis="lagrange")) == got[:64]
    # the product's own inverse transform gives the polynomial whose monomial commitment this is
    own = [zk.fr_ntt(le(e), inverse=True) for e in ev]
    assert bytes(k6.commit(np.stack([np.frombuffer(o, dtype=np.uint8) for o in own]))) == got


def test_commit_edges_and_refusals(zk, files, k6, k10, monkeypatch):
    assert bytes(k10.commit([0] * 33)) == bytes(64)                     # the zero polynomial: infinity
    assert bytes(k6.commit([0] * 64, basis="lagrange")) == bytes(64)
    top = [R - 1] * 100
    first = bytes(k10.commit(top))
    assert first == commitment(top)
    monkeypatch.setenv("ZKHIP_KZG_SEG", "3")                            # the knob is the division's: a commitment does not move
    assert bytes(k10.commit(top)) == first and k10.info()["seg"] == 3
    monkeypatch.delenv("ZKHIP_KZG_SEG")
    info = k10.info()
    assert info["seg"] == DEFAULT_SEG and info["max_coeffs"] == 2047 and info["lagrange_log_n"] is None
    assert info["device_bytes"] >= 2047 * 64 and info["last_launches"] > 0
    assert k6.info()["lagrange_log_n"] == 6 and k6.info()["max_coeffs"] == 127
    lib = zk.load_library()
    out, c = np.zeros(64, dtype=np.uint8), le([1] * 2048)
    assert lib.zk_kzg_commit(k10._h, out.ctypes.data, c.ctypes.data, 2048, 1, 0) == 1
    assert b"zk_kzg_commit: n = 2048 exceeds max_coeffs = 2047" in lib.zk_last_error()
    bad = le([1, 2, 3, R, 5] * 2).copy()
    assert lib.zk_kzg_commit(k10._h, out.ctypes.data, bad.ctypes.data, 5, 2, 0) == 1
    assert b"zk_kzg_commit: polynomial 0, coefficient 3 is not below r" in lib.zk_last_error()
    assert lib.zk_kzg_commit(k10._h, out.ctypes.data, c.ctypes.data, 1024, 1, 1) == 1
    assert b"zk_kzg_commit: the object holds no Lagrange level" in lib.zk_last_error()
    assert lib.zk_kzg_commit(k6._h, out.ctypes.data, c.ctypes.data, 32, 1, 1) == 1
    assert b"zk_kzg_commit: n = 32, the Lagrange level holds 64 points" in lib.zk_last_error()
    with pytest.raises(ValueError, match="needs a prepared file"):
        zk.Kzg.from_ptau(files["p10"], lagrange_log_n=4)                # Lagrange on the file that is not prepared
    f = zk.PtauFile(files["p10"])
    h = ctypes.c_void_p()
    assert lib.zk_kzg_create(ctypes.byref(h), ctypes.byref(f.kzg_view()), 100, 4, -1) == 1 and not h
    assert b"a Lagrange level needs a prepared file" in lib.zk_last_error()
    f.close()


# ---------------------------------------------------------------- open
def open_sizes(seg):
    return sorted({n for _, n in tier_sizes(seg) if n <= 2047} | {2047})


@pytest.mark.parametrize("name", list(SEGS))
def test_open_equals_the_oracle_and_verifies(k10, monkeypatch, name):
    set_seg(monkeypatch, name)
    rng = random.Random(11)
    ops = []
    for n in open_sizes(int(SEGS[name] or DEFAULT_SEG)):
        p, z = [poly(rng, n), poly(rng, n)], [rng.randrange(R), rng.randrange(R)]
        ys, pis = k10.open(p, z)
        C = bytes(k10.commit(p))
        for j in range(2):
            q, y = divide(p[j], z[j])
            assert ys[j] == y and bytes(pis[64 * j:64 * j + 64]) == commitment(q), (n, j)
            if n == 1:
                assert bytes(pis[64 * j:64 * j + 64]) == bytes(64)      # a constant: the proof is infinity
            ops.append((C[64 * j:64 * j + 64], z[j], y, bytes(pis[64 * j:64 * j + 64])))
    assert list(k10.verify(*pack(ops))) == [OK] * len(ops)


def test_open_refusals(zk, k10):
    lib = zk.load_library()
    ys, pr, c = np.zeros(64, dtype=np.uint8), np.zeros(128, dtype=np.uint8), le([1, 2, 3, 4])
    zs = le([5, R])
    assert lib.zk_kzg_open(k10._h, ys.ctypes.data, pr.ctypes.data, c.ctypes.data, 2, 2, zs.ctypes.data) == 1
    assert b"zk_kzg_open: z 1 is not below r" in lib.zk_last_error()
    big = le([1] * 2048)
    assert lib.zk_kzg_open(k10._h, ys.ctypes.data, pr.ctypes.data, big.ctypes.data, 2048, 1, zs.ctypes.data) == 1
    assert b"zk_kzg_open: n = 2048 exceeds max_coeffs = 2047" in lib.zk_last_error()


# ---------------------------------------------------------------- verify
def mixture(openings):
    """(openings, verdicts): every way an opening can be wrong, once"""
    (C1, z1, y1, pi1), (_, z2, y2, pi2), _, (C2, z4, y4, pi4) = openings[:4]
    two_pi = bn.g1_to_bytes(bn.G1.dbl(bn.g1_from_bytes(pi1)))
    off = bytearray(C1)
    off[33] ^= 4                                       # y changed: off the curve
    coord_q = Q.to_bytes(32, "little") + C1[32:]
    ops = [((C1, z1, y1, pi1), OK),
           ((C1, z1, (y1 + 1) % R, pi1), INVALID),
           ((C1, z1, y1, two_pi), INVALID),
           ((C2, z1, y1, pi1), INVALID),               # the commitment of another polynomial
           ((C1, z2, y1, pi1), INVALID),               # the point of another opening
           ((bytes(off), z1, y1, pi1), MALFORMED),
           ((coord_q, z1, y1, pi1), MALFORMED),
           ((C1, z1, R, pi1), MALFORMED),
           ((C2, z4, y4, pi4), OK),
           ((bytes(64), z2, 0, bytes(64)), OK),        # the zero polynomial's opening
           ((C1, z2, y2, pi2), OK)]
    return [o for o, _ in ops], [v for _, v in ops]


def test_verify_gives_every_opening_its_own_verdict(zk, files, k10, openings):
    ops, want = mixture(openings)
    assert list(k10.verify(*pack(ops))) == want
    assert list(k10.verify(*pack(ops[::-1]))) == want[::-1]
    other = zk.Kzg.from_ptau(files["other"], max_coeffs=1)             # another tau: nothing of this file's verifies
    try:
        assert list(other.verify(*pack(openings))) == [INVALID] * len(openings)
    finally:
        other.close()


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65])
def test_verify_sizes_and_chunks(k10, openings, monkeypatch, m):
    ops, want = mixture(openings)
    many = [ops[i % len(ops)] for i in range(m)]
    wanted = [want[i % len(want)] for i in range(m)]
    assert list(k10.verify(*pack(many))) == wanted
    if m == 65:
        monkeypatch.setenv("ZKHIP_VERIFY_CHUNK", "50")                  # two chunks, the second of 15
        assert list(k10.verify(*pack(many))) == wanted


# ---------------------------------------------------------------- verify_batch
@pytest.mark.parametrize("m", [1, 64, 130])
def test_batch_all_valid_and_one_invalid_anywhere(k10, openings, m):
    rng = random.Random(m)
    valid = [openings[i % len(openings)] for i in range(m)]
    assert k10.verify_batch(*pack(valid)) == OK
    assert k10.verify_batch(*pack(valid), scalars=[(1 << 128) - 1] * m) == OK
    for at in sorted({0, m // 2, m - 1}):
        C, z, y, pi = valid[at]
        bad = valid[:at] + [(C, z, (y + 1) % R, pi)] + valid[at + 1:]
        assert k10.verify_batch(*pack(bad)) == INVALID                          # drawn scalars
        assert k10.verify_batch(*pack(bad), scalars=[(1 << 128) - 1] * m) == INVALID
        assert k10.verify_batch(*pack(bad), scalars=[rng.randrange(1, 1 << 128) for _ in range(m)]) == INVALID


def test_batch_malformed_cancelling_errors_and_a_zero_scalar(zk, k10, openings):
    ops, want = mixture(openings)
    valid = [o for o, v in zip(ops, want) if v == OK]
    assert k10.verify_batch(*pack(valid)) == OK and k10.verify_batch(*pack([])) == OK
    for o, v in zip(ops, want):
        if v == MALFORMED:
            assert k10.verify_batch(*pack(valid + [o])) == MALFORMED
            assert k10.verify_batch(*pack([o] + valid + [ops[1]])) == MALFORMED   # malformed wins over invalid
    # Two wrong openings at ONE point z whose errors are +1 and -1: with r_1 = r_2 = 1 the sum sum r_i y_i is the right one and
    # the batch passes.  This is what scalars known to the prover cost; drawn scalars do not let the errors cancel.
    (C1, z1, y1, pi1), (C2, z4, y4, pi4) = openings[0], openings[3]
    assert z1 == z4
    pair = [(C1, z1, (y1 + 1) % R, pi1), (C2, z4, (y4 - 1) % R, pi4)]
    assert list(k10.verify(*pack(pair))) == [INVALID, INVALID]
    assert k10.verify_batch(*pack(pair), scalars=[1, 1]) == OK
    assert k10.verify_batch(*pack(pair)) == INVALID
    assert k10.verify_batch(*pack(pair), scalars=[1, 2]) == INVALID
    with pytest.raises(zk.ZkHipError, match="zk_kzg_verify_batch: scalar 1 is zero"):
        k10.verify_batch(*pack(valid[:3]), scalars=bytes([1] + [0] * 15) + bytes(16) + bytes([2] + [0] * 15))


# ---------------------------------------------------------------- create
def test_create_refuses_what_the_header_says(zk, files):
    f = zk.PtauFile(files["p6"])
    raw = bytes(f.raw)
    pos = {sid: f.sections[sid][0] for sid in (2, 3, 12)}
    f.close()
    cof = golden_json("g2_cofactor_points.json")["outside"][1]
    outside = bn.g2_to_bytes(((int(cof["x"][0]), int(cof["x"][1])), (int(cof["y"][0]), int(cof["y"][1]))))

    def patched(sid, at, nb, new=None):
        b = bytearray(raw)
        o = pos[sid] + at * nb
        if new is None:
            b[o + nb // 2 + 1] ^= 4                    # y changed: off the curve
        else:
            b[o:o + nb] = new
        return zk.PtauFile(bytes(b))

    two_g = bn.g1_to_bytes(bn.G1.dbl(bn.G1_GEN))
    cases = [(patched(2, 5, 64), {}, "zk_kzg_create: ptau section 2: point 5 is not on the curve"),
             (patched(2, 126, 64), {"max_coeffs": 126}, None),                                    # a bad point that is not kept
             (patched(2, 9, 64, Q.to_bytes(32, "little") + bytes(31) + b"\x01"), {}, "zk_kzg_create: ptau section 2: point 9 has a coordinate that is not below q"),
             (patched(2, 0, 64, two_g), {}, "zk_kzg_create: ptau section 2: point 0 is not the generator of G1"),
             (patched(3, 0, 128, outside), {}, "zk_kzg_create: ptau section 3: point 0 is not the generator of G2"),
             (patched(3, 1, 128, outside), {}, "zk_kzg_create: ptau section 3: point 1 is not in the subgroup"),
             (patched(3, 1, 128, bytes(128)), {}, "zk_kzg_create: ptau section 3: point 1 is the point at infinity"),
             (patched(3, 1, 128), {}, "zk_kzg_create: ptau section 3: point 1 is not on the curve"),
             (patched(12, 63 + 7, 64), {"lagrange_log_n": 6}, "zk_kzg_create: ptau section 12: point 70 is not on the curve"),
             (patched(12, 63 + 7, 64), {"lagrange_log_n": 5}, None)]
    for pf, kw, msg in cases:
        if msg is None:
            zk.Kzg(pf, **kw).close()
        else:
            with pytest.raises(zk.ZkHipError) as e:
                zk.Kzg(pf, **kw)
            assert str(e.value) == msg
        pf.close()
    # a short section: the view says so
    f = zk.PtauFile(files["p6"])
    lib = zk.load_library()
    for field, sec, have, level, need in (("tau_g1_bytes", 2, 640, 0xffffffff, 127 * 64), ("tau_g2_bytes", 3, 128, 0xffffffff, 256),
                                          ("lagrange_g1_bytes", 12, 64 * 64, 6, 127 * 64)):
        v = f.kzg_view()
        setattr(v, field, have)
        h = ctypes.c_void_p()
        assert lib.zk_kzg_create(ctypes.byref(h), ctypes.byref(v), 127, level, -1) == 1 and not h
        assert lib.zk_last_error().decode() == "zk_kzg_create: ptau section %d is short: %d bytes, %d needed" % (sec, have, need)
    h = ctypes.c_void_p()
    assert lib.zk_kzg_create(ctypes.byref(h), ctypes.byref(f.kzg_view()), 128, 0xffffffff, -1) == 1
    assert lib.zk_last_error().decode() == "zk_kzg_create: max_coeffs 128 is outside 1 .. 127 (power 6)"
    assert lib.zk_kzg_create(ctypes.byref(h), ctypes.byref(f.kzg_view()), 127, 7, -1) == 1
    assert lib.zk_last_error().decode() == "zk_kzg_create: Lagrange level 7 is above the file's power 6"
    f.close()
