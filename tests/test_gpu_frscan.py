"""Running products over Fr on the GPU: batch inversion, prefix products, the grand product of ratios and the accumulator of
PLONK's permutation argument.  Exact arithmetic: every expected value comes from Python integers (pow(x, -1, R), running
products), w is oracle.bn254.fr_root(log_n), and the comparison is byte for byte.  The vectors depend on n only, so one
oracle serves every ZKHIP_SCAN_SEG setting and equal bytes across the settings follow from equality with it."""
import ctypes
import functools
import random

import numpy as np
import pytest

from oracle import bn254 as bn

pytestmark = pytest.mark.gpu

R = bn.R_MOD
DEFAULT_SEG = 8                                        # ZKHIP_SCAN_SEG when the variable is not set
SEGS = {"seg1": "1", "seg3": "3", "default": None}
TAU, ALPHA, BETA = 0x1F3A9C5E77D1B2A49E0C6F5D3B8A17264C9E0F1D2B3A4958, 0x2B7E151628AED2A6ABF7158809CF4F3C, 0x3243F6A8885A308D313198A2E0370734


def le(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8)


def ints(rows):
    b = bytes(rows)
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def set_seg(monkeypatch, name):
    if SEGS[name] is None:
        monkeypatch.delenv("ZKHIP_SCAN_SEG", raising=False)
    else:
        monkeypatch.setenv("ZKHIP_SCAN_SEG", SEGS[name])


def seg_of(name):
    return int(SEGS[name]) if SEGS[name] else DEFAULT_SEG


def tier_sizes(seg):
    """n = 1, 2, 3 and b - 1, b, b + 1, 2 b + 1 around every boundary b of the scan at `seg` elements a lane: a lane's
    segment, a wave (64 lanes), a workgroup (4 waves) and, at seg = 1 only, the carry pass, whose lanes take one workgroup
    total each up to 256 workgroups and more beyond"""
    out = [1, 2, 3]
    for b in (seg, 64 * seg, 256 * seg) + ((65536,) if seg == 1 else ()):
        out += [n for n in (b - 1, b, b + 1, 2 * b + 1) if n >= 1]
    return sorted(set(out))


CASES = [pytest.param(name, n, id="%s-%d" % (name, n)) for name in SEGS for n in tier_sizes(seg_of(name))]
# both sides of every lane, wave and workgroup boundary of the three settings
EDGES = sorted({b + d for s in (1, 3, DEFAULT_SEG) for b in (s, 64 * s, 256 * s) for d in (-1, 0)})


def inverses(v):
    """1 / v[i] for non-zero v[i], 0 for 0, by one pow(x, -1, R)"""
    pre, t = [], 1
    for x in v:
        pre.append(t)
        if x:
            t = t * x % R
    inv, out = pow(t, -1, R), [0] * len(v)
    for i in range(len(v) - 1, -1, -1):
        if v[i]:
            out[i] = inv * pre[i] % R
            inv = inv * v[i] % R
    return out


def running(v):
    """(inclusive, exclusive) running products"""
    inc, t = [], 1
    for x in v:
        t = t * x % R
        inc.append(t)
    return inc, [1] + inc[:-1]


def ratios(num, den):
    """(z, last)"""
    inv, z, t = inverses(den), [], 1
    for a, b in zip(num, inv):
        z.append(t)
        t = t * a % R * b % R
    return z, t


@functools.lru_cache(maxsize=None)
def vector(n, zeros):
    """n values and their oracle results: random, with 1 and r - 1 (and 0 when asked) at index 0, at n - 1 and on both sides
    of every tier boundary.  zeros: (values, inverses, how many zeros); else (values, inclusive, exclusive)"""
    rng = random.Random(1000 * n + zeros)
    v = [rng.getrandbits(253) for _ in range(n)] if n > 5000 else [rng.randrange(R) for _ in range(n)]      # 2^253 < r
    special = (0, 1, R - 1) if zeros else (1, R - 1)
    for k, i in enumerate([0, n - 1] + EDGES):
        if 0 <= i < n:
            v[i] = special[(k + i) % len(special)]
    if zeros:
        return v, inverses(v), sum(1 for x in v if x == 0)
    return (v,) + running(v)


@functools.lru_cache(maxsize=None)
def fraction(n):
    """(num, den, z, last): den without zeros"""
    num, den = vector(n, 0)[0], list(reversed(vector(n + 1, 0)[0]))[:n]
    return (num, den) + ratios(num, den)


# ---------------------------------------------------------------- batch inversion
@pytest.mark.parametrize("name,n", CASES)
def test_batch_inverse_matches_the_oracle(zk, monkeypatch, name, n):
    set_seg(monkeypatch, name)
    v, want, nz = vector(n, 1)
    out, zeros = zk.fr_batch_inverse(v)
    got = ints(out)
    assert got == want and zeros == nz
    assert all((a * b) % R == 1 for a, b in zip(v, got) if a) and all(b == 0 for a, b in zip(v, got) if not a)


@pytest.mark.parametrize("name", list(SEGS))
def test_batch_inverse_of_constant_vectors_and_nothing(zk, monkeypatch, name):
    set_seg(monkeypatch, name)
    n = 256 * seg_of(name) + 5
    out, zeros = zk.fr_batch_inverse([0] * n)
    assert not out.any() and zeros == n
    out, zeros = zk.fr_batch_inverse([1] * n)
    assert ints(out) == [1] * n and zeros == 0
    out, zeros = zk.fr_batch_inverse([R - 1] * n)
    assert ints(out) == [R - 1] * n and zeros == 0
    out, zeros = zk.fr_batch_inverse([])
    assert out.size == 0 and zeros == 0


def test_batch_inverse_in_place_and_without_a_count(zk):
    lib = zk.load_library()
    v, want, nz = vector(771, 1)
    buf = le(v).copy()
    p = ctypes.c_void_p(buf.ctypes.data)
    assert lib.zk_fr_batch_inverse(p, p, 771, None, -1) == 0, lib.zk_last_error()
    assert ints(buf) == want
    zeros = ctypes.c_uint64(99)
    assert lib.zk_fr_batch_inverse(None, None, 0, ctypes.byref(zeros), -1) == 0 and zeros.value == 0


def test_c_entries_refuse_values_not_below_r_and_bad_knobs(zk, monkeypatch):
    lib = zk.load_library()
    bad = le([1, 2, 3, 4, 5, R, 7, R + 1]).copy()
    good = le([1] * 8).copy()
    out, last = np.zeros(8 * 32, dtype=np.uint8), np.zeros(32, dtype=np.uint8)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)       # noqa: E731

    def err(rc):
        assert rc == 1
        return lib.zk_last_error().decode()

    assert err(lib.zk_fr_batch_inverse(P(out), P(bad), 8, None, -1)) == "zk_fr_batch_inverse: value 5 is not below r"
    assert err(lib.zk_fr_prefix_product(P(out), P(bad), 8, 0, -1)) == "zk_fr_prefix_product: value 5 is not below r"
    assert err(lib.zk_fr_grand_product(P(out), P(last), P(bad), P(good), 8, -1)) == "zk_fr_grand_product: numerator 5 is not below r"
    assert err(lib.zk_fr_grand_product(P(out), P(last), P(good), P(bad), 8, -1)) == "zk_fr_grand_product: denominator 5 is not below r"
    assert err(lib.zk_fr_prefix_product(P(out), P(good), 8, 2, -1)) == "zk_fr_prefix_product: flags 2 is unknown"
    assert err(lib.zk_fr_prefix_product(P(out), P(good), 8, 3, -1)) == "zk_fr_prefix_product: flags 3 is unknown"
    one, two, big = le([1]).copy(), le([1, 2]).copy(), le([R]).copy()
    w, gg = np.concatenate([good, bad]), np.concatenate([good, good])      # 2 columns of 8 rows
    assert err(lib.zk_plonk_permutation_product(P(out), P(last), P(w), P(gg), 2, 3, P(two), P(one), P(one), -1)) \
        == "zk_plonk_permutation_product: wires: column 1, row 5 is not below r"
    assert err(lib.zk_plonk_permutation_product(P(out), P(last), P(gg), P(w), 2, 3, P(two), P(one), P(one), -1)) \
        == "zk_plonk_permutation_product: sigmas: column 1, row 5 is not below r"
    assert err(lib.zk_plonk_permutation_product(P(out), P(last), P(good), P(good), 1, 3, P(big), P(one), P(one), -1)) \
        == "zk_plonk_permutation_product: shift 0 is not below r"
    assert err(lib.zk_plonk_permutation_product(P(out), P(last), P(good), P(good), 1, 3, P(one), P(big), P(one), -1)) \
        == "zk_plonk_permutation_product: beta is not below r"
    assert err(lib.zk_plonk_permutation_product(P(out), P(last), P(good), P(good), 1, 3, P(one), P(one), P(big), -1)) \
        == "zk_plonk_permutation_product: gamma is not below r"
    assert err(lib.zk_plonk_permutation_product(P(out), P(last), P(good), P(good), 9, 3, P(one), P(one), P(one), -1)) \
        == "zk_plonk_permutation_product: cols 9 is outside 1 .. 8"
    assert err(lib.zk_plonk_permutation_product(P(out), P(last), P(good), P(good), 1, 29, P(one), P(one), P(one), -1)) \
        == "zk_plonk_permutation_product: log_n 29 is above 28"
    for value in ("0", "4097", "x", "16 "):
        monkeypatch.setenv("ZKHIP_SCAN_SEG", value)
        assert err(lib.zk_fr_batch_inverse(P(out), P(good), 8, None, -1)) == "ZKHIP_SCAN_SEG: a number of elements per lane from 1 to 4096 expected"
    monkeypatch.setenv("ZKHIP_SCAN_SEG", "4096")
    assert lib.zk_fr_prefix_product(P(out), P(good), 8, 0, -1) == 0 and ints(out) == [1] * 8


# ---------------------------------------------------------------- prefix products
@pytest.mark.parametrize("name,n", CASES)
def test_prefix_product_matches_the_oracle(zk, monkeypatch, name, n):
    set_seg(monkeypatch, name)
    v, inc, exc = vector(n, 0)
    assert ints(zk.fr_prefix_product(v)) == inc
    assert ints(zk.fr_prefix_product(le(v), exclusive=True)) == exc


@pytest.mark.parametrize("name", list(SEGS))
def test_prefix_product_with_a_zero_in_the_middle(zk, monkeypatch, name):
    set_seg(monkeypatch, name)
    seg = seg_of(name)
    for at in (0, seg, 64 * seg - 1, 256 * seg, 300 * seg + 1):
        n = 520 * seg + 3
        v = list(vector(n, 0)[0])
        v[at] = 0
        inc, exc = running(v)
        got_inc, got_exc = ints(zk.fr_prefix_product(v)), ints(zk.fr_prefix_product(v, exclusive=True))
        assert got_inc == inc and got_exc == exc
        assert all(got_inc[:at]) and not any(got_inc[at:]) and all(got_exc[:at + 1]) and not any(got_exc[at + 1:])
    assert ints(zk.fr_prefix_product([1] * n)) == [1] * n
    assert ints(zk.fr_prefix_product([R - 1] * n)) == [R - 1 if i % 2 == 0 else 1 for i in range(n)]


# ---------------------------------------------------------------- grand products
@pytest.mark.parametrize("name,n", CASES)
def test_grand_product_matches_the_oracle(zk, monkeypatch, name, n):
    set_seg(monkeypatch, name)
    num, den, want, last = fraction(n)
    z, got_last = zk.fr_grand_product(num, den)
    assert ints(z) == want and got_last == last
    z, got_last = zk.fr_grand_product(le(den), le(den))
    assert ints(z) == [1] * n and got_last == 1


@pytest.mark.parametrize("name", list(SEGS))
def test_grand_product_zero_numerators_and_denominators(zk, monkeypatch, name):
    set_seg(monkeypatch, name)
    seg = seg_of(name)
    n = 520 * seg + 3
    num, den, _, _ = fraction(n)
    num, mid = list(num), 256 * seg - 1
    num[mid] = 0
    want, last = ratios(num, den)
    z, got_last = zk.fr_grand_product(num, den)
    assert ints(z) == want and got_last == last == 0 and all(want[:mid + 1]) and not any(want[mid + 1:])
    for where in ((0,), (mid,), (n - 1,), (mid + 1, n - 1), (0, mid), (70 * seg, 64 * seg + 1)):
        d = list(den)
        for i in where:
            d[i] = 0
        with pytest.raises(zk.ZkHipError, match="^zk_fr_grand_product: denominator %d is zero$" % min(where)):
            zk.fr_grand_product(num, d)
    z, got_last = zk.fr_grand_product([], [])
    assert z.size == 0 and got_last == 1
    lib, last32 = zk.load_library(), np.zeros(32, dtype=np.uint8)
    assert lib.zk_fr_grand_product(None, ctypes.c_void_p(last32.ctypes.data), None, None, 0, -1) == 0 and ints(last32) == [1]


# ---------------------------------------------------------------- the permutation argument
def circuit(rng, cols, log_n, identity=False):
    """(wires, sigmas, shifts, cycles): a random partition of the cols * n cells into cycles, one value a cycle, sigma the
    cycle's successor as the value shifts[j'] w^i'"""
    n, w = 1 << log_n, bn.fr_root(log_n)
    shifts = list(range(1, cols + 1))
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * w % R
    cells = [(j, i) for j in range(cols) for i in range(n)]
    order = list(cells)
    if not identity:
        rng.shuffle(order)
    wires, sigmas, cycles, at = [[0] * n for _ in range(cols)], [[0] * n for _ in range(cols)], [], 0
    while at < len(order):
        size = 1 if identity else min(len(order) - at, rng.choice((1, 1, 2, 3, 5, 17)))
        cyc, value = order[at:at + size], rng.randrange(R)
        for k, (j, i) in enumerate(cyc):
            nj, ni = cyc[(k + 1) % size]
            wires[j][i], sigmas[j][i] = value, shifts[nj] * pw[ni] % R
        cycles.append(cyc)
        at += size
    return wires, sigmas, shifts, cycles


def accumulator(wires, sigmas, shifts, beta, gamma, log_n):
    n, cols, w = 1 << log_n, len(wires), bn.fr_root(log_n)
    num, den, x = [], [], beta
    for i in range(n):
        a = b = 1
        for j in range(cols):
            a = a * ((wires[j][i] + x * shifts[j] + gamma) % R) % R
            b = b * ((wires[j][i] + beta * sigmas[j][i] + gamma) % R) % R
        num.append(a)
        den.append(b)
        x = x * w % R
    return ratios(num, den)


PERM_CASES = [pytest.param(name, cols, log_n, id="%s-cols%d-2p%d" % (name, cols, log_n))
              for name in SEGS for cols in (1, 3, 8) for log_n in (0, 1, 3, 6, 10)] + [pytest.param("seg1", 3, 17, id="seg1-cols3-2p17-carry")]


@pytest.mark.parametrize("name,cols,log_n", PERM_CASES)
def test_permutation_product_matches_the_oracle(zk, monkeypatch, name, cols, log_n):
    set_seg(monkeypatch, name)
    rng = random.Random(100 * cols + log_n)
    wires, sigmas, shifts, cycles = circuit(rng, cols, log_n)
    beta, gamma = rng.randrange(1, R), rng.randrange(1, R)
    want, last = accumulator(wires, sigmas, shifts, beta, gamma, log_n)
    assert last == 1
    z, got_last = zk.plonk_permutation_product(wires, sigmas, shifts, beta, gamma)
    assert ints(z) == want and got_last == 1
    long = [c for c in cycles if len(c) >= 2]
    if long:                                            # one wire of a cycle changed: the product no longer closes
        j, i = long[len(long) // 2][0]
        wires[j][i] = (wires[j][i] + 1) % R
        want, last = accumulator(wires, sigmas, shifts, beta, gamma, log_n)
        assert last != 1
        z, got_last = zk.plonk_permutation_product(np.stack([le(c) for c in wires]), np.stack([le(c) for c in sigmas]), le(shifts), beta, gamma)
        assert ints(z) == want and got_last == last


@pytest.mark.parametrize("name", list(SEGS))
def test_permutation_product_special_challenges_and_zero_denominators(zk, monkeypatch, name):
    set_seg(monkeypatch, name)
    rng = random.Random(5)
    cols, log_n = 3, 10
    n = 1 << log_n
    wires, sigmas, shifts, _ = circuit(rng, cols, log_n, identity=True)
    beta, gamma = rng.randrange(1, R), rng.randrange(1, R)
    z, last = zk.plonk_permutation_product(wires, sigmas, shifts, beta, gamma)
    assert ints(z) == [1] * n and last == 1                # the identity permutation
    wires, sigmas, shifts, _ = circuit(rng, cols, log_n)
    z, last = zk.plonk_permutation_product(wires, sigmas, shifts, 0, gamma)
    assert ints(z) == [1] * n and last == 1                # beta = 0: num = den
    want, want_last = accumulator(wires, sigmas, shifts, beta, 0, log_n)
    z, last = zk.plonk_permutation_product(wires, sigmas, shifts, beta, 0)
    assert ints(z) == want and last == want_last == 1      # gamma = 0
    for j, row in ((0, 0), (1, 517), (2, n - 1)):
        g = -(wires[j][row] + beta * sigmas[j][row]) % R
        den_rows = [i for i in range(n) if any((wires[c][i] + beta * sigmas[c][i] + g) % R == 0 for c in range(cols))]
        with pytest.raises(zk.ZkHipError, match="^zk_plonk_permutation_product: row %d has a zero denominator$" % min(den_rows)):
            zk.plonk_permutation_product(wires, sigmas, shifts, beta, g)
        assert row in den_rows


def test_round_two_commits_to_the_accumulator(zk, tmp_path):
    """the commitment of the accumulator's evaluations in the Lagrange basis is [Z(tau)] G"""
    path = str(tmp_path / "p6.ptau")
    zk.write_trapdoor_ptau(6, TAU, ALPHA, BETA, path)
    rng = random.Random(6)
    wires, sigmas, shifts, _ = circuit(rng, 3, 6)
    beta, gamma = rng.randrange(1, R), rng.randrange(1, R)
    z, last = zk.plonk_permutation_product(wires, sigmas, shifts, beta, gamma)
    assert last == 1
    coeffs, at_tau = bn.ntt(ints(z), inverse=True), 0
    for c in reversed(coeffs):
        at_tau = (c + TAU * at_tau) % R
    with zk.Kzg.from_ptau(path, lagrange_log_n=6) as k:
        assert bytes(k.commit(z, basis="lagrange")) == bn.g1_to_bytes(bn.G1.mul(bn.G1_GEN, at_tau))
