"""Three-column PLONK instances from a seed, and two independent oracles for the quotient t of round 3, in Python integers
(helper of test_plonk_quotient_host.py and test_gpu_plonk_quotient.py; not collected).

An instance: a random partition of the 3n cells into copy cycles with equal values on a cycle, random q_L, q_R, q_M, q_O,
random public inputs on the first two rows, q_C chosen so that every gate holds, sigma from the cycles with the column
shifts (1, 2, 3), z by the recurrence of the permutation argument, and optional blinding by random multiples of Z_H.
Oracle A multiplies the polynomials out (schoolbook) and divides by X^n - 1 by long division; oracle B evaluates on the
coset g * (4n-th roots of unity), divides pointwise and interpolates.  They share only the instance and oracle.bn254.

Instances with CHOSEN coset evaluations (constant_instance, even_point_instance, extreme_instance: helpers of
test_gpu_extreme_operands_plonk.py) break the gate identity on purpose; oracle B is their reference."""
import random

from oracle.bn254 import R_MOD as R, fr_root, ntt

K1, K2 = 2, 3
BLIND = (2, 2, 2, 3)


def le(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def ints(buf):
    b = bytes(buf)
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def t_len_of(coeffs):
    k = len(coeffs)
    while k and coeffs[k - 1] == 0:
        k -= 1
    return k


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


class Instance:
    """Fields: n, log_n, alpha, beta, gamma; the circuit by values at w^j (ql_v .. s3_v) and by coefficients (ql .. s3);
    wires by values (a_v, b_v, c_v); a, b, c, z, pi by coefficients (a, b, c, z blinded when asked)."""
    CIRCUIT = ("ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3")

    def circuit(self, basis="monomial"):
        return [getattr(self, k + ("_v" if basis == "lagrange" else "")) for k in self.CIRCUIT]


def make(seed, log_n, blind=None, alpha=None, beta=None, gamma=None, break_gate=None, intt=None, public=True):
    """blind: None, or the number of blinding coefficients of a, b, c, z (BLIND is the usual (2, 2, 2, 3)).  break_gate: a
    row whose q_C is moved by one after the witness was made, so that its gate fails.  intt: the inverse transform to use
    for values -> coefficients (ints in, ints out); oracle.bn254.ntt otherwise.  public False: PI = 0."""
    rng = random.Random(seed)
    inv_ntt = intt or (lambda v: ntt(v, inverse=True))
    n = 1 << log_n
    w = fr_root(log_n)
    I = Instance()
    I.n, I.log_n = n, log_n
    I.alpha = rng.randrange(1, R) if alpha is None else alpha
    I.beta = rng.randrange(1, R) if beta is None else beta
    I.gamma = rng.randrange(1, R) if gamma is None else gamma
    # copy cycles: a shuffled list of the 3n cells cut into runs of 1 .. 4
    cells = list(range(3 * n))
    rng.shuffle(cells)
    value, nxt, at = [0] * (3 * n), list(range(3 * n)), 0
    while at < 3 * n:
        k = min(rng.randrange(1, 5), 3 * n - at)
        v = rng.randrange(R)
        run = cells[at:at + k]
        for j, cell in enumerate(run):
            value[cell] = v
            nxt[cell] = run[(j + 1) % k]
        at += k
    I.a_v, I.b_v, I.c_v = value[:n], value[n:2 * n], value[2 * n:]
    I.ql_v, I.qr_v, I.qm_v, I.qo_v = ([rng.randrange(R) for _ in range(n)] for _ in range(4))
    pi_v = [rng.randrange(R) if i < 2 and public else 0 for i in range(n)]
    I.qc_v = [(-(I.ql_v[i] * I.a_v[i] + I.qr_v[i] * I.b_v[i] + I.qm_v[i] * I.a_v[i] * I.b_v[i] + I.qo_v[i] * I.c_v[i] + pi_v[i])) % R for i in range(n)]
    if break_gate is not None:
        I.qc_v[break_gate] = (I.qc_v[break_gate] + 1) % R
    shifts = (1, K1, K2)
    wp = [1] * n
    for i in range(1, n):
        wp[i] = wp[i - 1] * w % R
    sig = [shifts[nxt[cell] // n] * wp[nxt[cell] % n] % R for cell in range(3 * n)]
    I.s1_v, I.s2_v, I.s3_v = sig[:n], sig[n:2 * n], sig[2 * n:]
    z_v = [1] * n
    for i in range(n - 1):
        num = den = 1
        for j in range(3):
            num = num * (value[j * n + i] + I.beta * shifts[j] * wp[i] + I.gamma) % R
            den = den * (value[j * n + i] + I.beta * sig[j * n + i] + I.gamma) % R
        z_v[i + 1] = z_v[i] * num % R * pow(den, -1, R) % R
    I.z_v = z_v
    for k in Instance.CIRCUIT:
        setattr(I, k, inv_ntt(getattr(I, k + "_v")))
    I.pi = inv_ntt(pi_v)
    polys = [inv_ntt(v) for v in (I.a_v, I.b_v, I.c_v, z_v)]
    if blind:
        for p, k in zip(polys, blind):                 # + (r_0 + r_1 X + ..) (X^n - 1), the top coefficient not zero
            if not k:
                continue
            r = [rng.randrange(R) for _ in range(k - 1)] + [rng.randrange(1, R)]
            p.extend([0] * k)
            for j, rj in enumerate(r):
                p[j] = (p[j] - rj) % R
                p[n + j] = (p[n + j] + rj) % R
    I.a, I.b, I.c, I.z = polys
    return I


# ---------------------------------------------------------------- instances with chosen coset evaluations
# What the quotient kernel multiplies are evaluations on the coset g * (4n-th roots of unity), which make() does not choose.
# These builders do: a constant polynomial takes its value at all 4n points; 2n coefficients can take chosen values at every
# second point (those points are the coset g * (2n-th roots)), n coefficients at every fourth.  Such instances break the gate
# identity, which is defined behaviour: t is the interpolant of num / Z_H (oracle_b).  Each builder asserts from coset_ext
# that the evaluations are the ones it names and keeps them (I.ext) for oracle_b on the same g.
VECTORS = Instance.CIRCUIT + ("a", "b", "c", "z", "pi")


def from_polys(log_n, polys, challenges, g=5):
    """polys: name -> coefficients for the 13 VECTORS (circuit vectors and pi at most n, padded here; a, b, c, z as given)."""
    n = 1 << log_n
    I = Instance()
    I.n, I.log_n = n, log_n
    I.alpha, I.beta, I.gamma = (int(v) % R for v in challenges)
    for k in VECTORS:
        p = [int(v) % R for v in polys[k]]
        if k in Instance.CIRCUIT or k == "pi":
            assert 1 <= len(p) <= n, k
            p = p + [0] * (n - len(p))
        setattr(I, k, p)
    lens = [len(getattr(I, k)) for k in "abcz"]
    assert all(1 <= k <= 2 * n for k in lens) and sum(lens) <= 5 * n + 3, lens
    for k in Instance.CIRCUIT:                            # the Lagrange basis: values at w^j
        setattr(I, k + "_v", ntt(getattr(I, k)))
    I.ext = (g, {k: coset_ext(getattr(I, k), log_n + 2, g) for k in VECTORS})
    return I


def _identity_sigma():
    return {"s1": [0, 1], "s2": [0, K1], "s3": [0, K2]}


def constant_instance(log_n, values, challenges, sigma_identity=False, g=5):
    """Every vector a constant polynomial: values is name -> standard value over VECTORS (missing: 0), or one value for all
    13.  The device then holds ONE chosen word per vector at every point of every lane.  sigma_identity: s1, s2, s3 are
    X, k1 X, k2 X instead (P = Q wherever z is a constant)."""
    if not isinstance(values, dict):
        values = {k: values for k in VECTORS}
    polys = {k: [values.get(k, 0)] for k in VECTORS}
    if sigma_identity:
        polys.update(_identity_sigma())
    I = from_polys(log_n, polys, challenges, g)
    for k in VECTORS:
        if not (sigma_identity and k in ("s1", "s2", "s3")):
            assert I.ext[1][k] == [values.get(k, 0) % R] * (4 << log_n), k
    return I


def empty_circuit(log_n, challenges=(3, 5, 7), g=5):
    """Everything 0, z = 1, sigma the identity: num vanishes identically, t = 0 and t_len = 0."""
    return constant_instance(log_n, {"z": 1}, challenges, sigma_identity=True, g=g)


def interpolate_on_coset(values, g):
    """The len(values) = 2^k coefficients of the polynomial with p(g w^j) = values[j], w the root of that size."""
    co = ntt([int(v) % R for v in values], inverse=True)
    gi, x, out = pow(g, -1, R), 1, []
    for v in co:
        out.append(v * x % R)
        x = x * gi % R
    return out


def even_point_instance(log_n, a_even, b_even, fourth, values, challenges, g=5):
    """a and b of 2n coefficients with the standard values a_even[k], b_even[k] at the even coset points x_(2k); the circuit
    vectors named in `fourth` (name -> n values) with those values at every fourth point x_(4k); the rest constants from
    `values` (name -> value, missing: 0).  Lengths 2n + 2n + 1 + 1 <= 5n + 3."""
    n = 1 << log_n
    assert len(a_even) == len(b_even) == 2 * n and all(k in Instance.CIRCUIT and len(v) == n for k, v in fourth.items())
    polys = {k: [values.get(k, 0)] for k in VECTORS}
    polys["a"], polys["b"] = interpolate_on_coset(a_even, g), interpolate_on_coset(b_even, g)
    for k, v in fourth.items():
        polys[k] = interpolate_on_coset(v, g)
    I = from_polys(log_n, polys, challenges, g)
    E = I.ext[1]
    assert E["a"][0::2] == [v % R for v in a_even] and E["b"][0::2] == [v % R for v in b_even]
    for k in VECTORS:
        if k in fourth:
            assert E[k][0::4] == [v % R for v in fourth[k]], k
        elif k not in ("a", "b"):
            assert E[k] == [values.get(k, 0) % R] * (4 * n), k
    return I


CONSTANT_FAMILIES = ("const_tmax", "const_top", "const_one", "dealt0", "dealt1", "dealt2", "beta0", "const_tmax_nopi", "z_one", "alpha0")


def constant_t_len(name, n):
    """t_len of a constant family.  Broken gates fill the interpolant: 4n, but for alpha = 0 (C / Z_H takes four values: the
    coefficients 0, n, 2n, 3n only) and z = 1 (no boundary term; the permutation term has degree 3 in X over Z_H)."""
    return {"alpha0": 3 * n + 1, "z_one": min(4 * n, 3 * n + 4)}.get(name, 4 * n)


EXTREME_FAMILIES = CONSTANT_FAMILIES + ("even_alternating", "even_mask01", "empty", "sigma_identity", "longest")


def extreme_instance(name, log_n, g=5):
    """The instances of tests/test_gpu_extreme_operands_plonk.py by name (DESIGN.md section 10 says what each aims at).
    Values are extreme_inputs.held(t): the device word has the limbs of t (T_MAX: eight limbs of 2^29 - 1)."""
    import extreme_inputs as xi
    n = 1 << log_n
    tmax, top, one = xi.held(xi.T_MAX), xi.held(R - 1), xi.held(1)
    three = (tmax, top, one)
    if name in ("const_tmax", "const_top", "const_one"):
        v = {"const_tmax": tmax, "const_top": top, "const_one": one}[name]
        return constant_instance(log_n, v, (v, v, v), g=g)
    if name.startswith("dealt"):                          # the three values dealt round the vectors and the challenges
        k = int(name[5:])
        return constant_instance(log_n, {v: three[(i + k) % 3] for i, v in enumerate(VECTORS)}, [three[(13 + i + k) % 3] for i in range(3)], g=g)
    if name == "beta0":                                   # f_j = a + gamma = 2 T_MAX exactly, no product in between
        return constant_instance(log_n, tmax, (tmax, 0, tmax), g=g)
    if name == "const_tmax_nopi":
        return constant_instance(log_n, {k: tmax for k in VECTORS if k != "pi"}, (tmax, tmax, tmax), g=g)
    if name == "z_one":                                   # the boundary term is zero, sigma is not the identity
        return constant_instance(log_n, {k: 1 if k == "z" else tmax for k in VECTORS}, (tmax, top, one), g=g)
    if name == "alpha0":                                  # the gate term alone
        return constant_instance(log_n, tmax, (0, tmax, tmax), g=g)
    if name == "empty":
        return empty_circuit(log_n, (tmax, top, one), g=g)
    if name == "sigma_identity":                          # P = Q != 0 at every point: t = alpha^2 (c - 1) L1 / Z_H interpolated
        return constant_instance(log_n, {"a": top, "b": tmax, "c": top, "z": tmax}, (tmax, top, tmax), sigma_identity=True, g=g)
    if name == "even_alternating":                        # neighbouring even lanes hold r - 1 and 1, a against b in opposite phase
        alt = xi.held_rows([R - 1, 1] * n)
        return even_point_instance(log_n, alt, alt[1:] + alt[:1], {"ql": alt[:n], "qm": alt[1:n + 1], "s1": alt[:n]},
                                   {k: tmax for k in VECTORS}, (top, tmax, top), g=g)
    if name == "even_mask01":
        rng = random.Random(7100 + log_n)
        mask = lambda k: xi.held_rows([(R - 1) * rng.randrange(2) for _ in range(k)])      # noqa: E731
        return even_point_instance(log_n, mask(2 * n), mask(2 * n), {"qr": mask(n), "qo": mask(n), "s2": mask(n), "qc": mask(n)},
                                   {k: top for k in VECTORS}, (tmax, top, top), g=g)
    if name == "longest":                                 # the largest legal lengths: 2n + 2n + n + 3 = 5n + 3, top coefficients r - 1
        rng = random.Random(7200 + log_n)
        rand = lambda k: [rng.randrange(R) for _ in range(k - 1)] + [R - 1]                # noqa: E731
        polys = {k: rand(n) for k in Instance.CIRCUIT + ("pi", "c")}
        polys.update(a=rand(2 * n), b=rand(2 * n), z=rand(3))
        return from_polys(log_n, polys, (tmax, top, one), g=g)
    raise KeyError(name)


# ---------------------------------------------------------------- oracle A: schoolbook and long division
def _mul(p, q):
    out = [0] * (len(p) + len(q) - 1)
    for i, pi in enumerate(p):
        if pi:
            for j, qj in enumerate(q):
                out[i + j] += pi * qj
    return [v % R for v in out]


def _add(*ps):
    out = [0] * max(len(p) for p in ps)
    for p in ps:
        for i, v in enumerate(p):
            out[i] += v
    return [v % R for v in out]


def _scale(p, k):
    return [v * k % R for v in p]


def numerator(I):
    """num(X) by coefficients"""
    n, be, ga, al = I.n, I.beta, I.gamma, I.alpha
    w = fr_root(I.log_n)
    gate = _add(_mul(I.ql, I.a), _mul(I.qr, I.b), _mul(I.qm, _mul(I.a, I.b)), _mul(I.qo, I.c), I.qc, I.pi)
    p1 = _mul(_mul(_add(I.a, [ga, be]), _add(I.b, [ga, be * K1 % R])), _mul(_add(I.c, [ga, be * K2 % R]), I.z))
    zw, x = [], 1
    for v in I.z:
        zw.append(v * x % R)
        x = x * w % R
    p2 = _mul(_mul(_add(I.a, _scale(I.s1, be), [ga]), _add(I.b, _scale(I.s2, be), [ga])), _mul(_add(I.c, _scale(I.s3, be), [ga]), zw))
    l1 = [pow(n, -1, R)] * n
    bound = _mul(_add(I.z, [R - 1]), l1)
    return _add(gate, _scale(_add(p1, _scale(p2, R - 1)), al), _scale(bound, al * al % R))


def num_at(I, x):
    """num(x) from the polynomials' values at x (Horner), for an x outside H"""
    n, be, ga, al = I.n, I.beta, I.gamma, I.alpha
    v = {k: horner(getattr(I, k), x) for k in Instance.CIRCUIT + ("a", "b", "c", "z", "pi")}
    zw = horner(I.z, x * fr_root(I.log_n) % R)
    gate = v["ql"] * v["a"] + v["qr"] * v["b"] + v["qm"] * v["a"] * v["b"] + v["qo"] * v["c"] + v["qc"] + v["pi"]
    p1 = (v["a"] + be * x + ga) * (v["b"] + be * K1 * x + ga) * (v["c"] + be * K2 * x + ga) * v["z"]
    p2 = (v["a"] + be * v["s1"] + ga) * (v["b"] + be * v["s2"] + ga) * (v["c"] + be * v["s3"] + ga) * zw
    l1 = (pow(x, n, R) - 1) * pow(n * (x - 1), -1, R)
    return (gate + al * (p1 - p2) + al * al * (v["z"] - 1) * l1) % R


def oracle_a(I):
    """(t, remainder): num = t (X^n - 1) + remainder by long division; t padded with zeros to 4n coefficients"""
    n = I.n
    p = numerator(I)
    q = [0] * max(len(p) - n, 0)
    for k in range(len(p) - 1, n - 1, -1):
        q[k - n] = p[k]
        p[k - n] = (p[k - n] + p[k]) % R
    rem = p[:n]
    assert len(q) <= 4 * n or not any(q[4 * n:]), "t has more than 4n coefficients"
    q = q[:4 * n]
    return q + [0] * (4 * n - len(q)), rem


# ---------------------------------------------------------------- oracle B: the coset route
def coset_ext(coeffs, log_m, g):
    m = 1 << log_m
    v, x = [], 1
    for c in coeffs:
        v.append(c * x % R)
        x = x * g % R
    return ntt(v + [0] * (m - len(v)))


def oracle_b(I, g=5):
    """the 4n coefficients of the interpolant of num / Z_H on the coset g * (4n-th roots of unity)"""
    n, be, ga, al = I.n, I.beta, I.gamma, I.alpha
    m, lm = 4 * n, I.log_n + 2
    kept = getattr(I, "ext", None)                      # the builders above keep what they asserted: the same coset_ext calls
    E = kept[1] if kept and kept[0] == g else {k: coset_ext(getattr(I, k), lm, g) for k in Instance.CIRCUIT + ("a", "b", "c", "z", "pi")}
    wm = fr_root(lm)
    zh = [pow((pow(g, n, R) * pow(wm, n * j, R) - 1) % R, -1, R) for j in range(4)]
    ev, x, xs = [], g, []
    for i in range(m):
        xs.append(x)
        x = x * wm % R
    linv = _batch_inverse([n * (xi - 1) % R for xi in xs])      # L1 / Z_H = 1 / (n (x - 1))
    for i in range(m):
        a, b, c, z, zw, xi = E["a"][i], E["b"][i], E["c"][i], E["z"][i], E["z"][(i + 4) % m], xs[i]
        gate = E["ql"][i] * a + E["qr"][i] * b + E["qm"][i] * a * b + E["qo"][i] * c + E["qc"][i] + E["pi"][i]
        p1 = (a + be * xi + ga) * (b + be * K1 * xi + ga) % R * (c + be * K2 * xi + ga) % R * z
        p2 = (a + be * E["s1"][i] + ga) * (b + be * E["s2"][i] + ga) % R * (c + be * E["s3"][i] + ga) % R * zw
        ev.append(((gate + al * (p1 - p2)) * zh[i % 4] + al * al * (z - 1) * linv[i]) % R)
    co = ntt(ev, inverse=True)
    gi, x, out = pow(g, -1, R), 1, []
    for v in co:
        out.append(v * x % R)
        x = x * gi % R
    return out


def _batch_inverse(v):
    pre, acc = [], 1
    for x in v:
        pre.append(acc)
        acc = acc * x % R
    inv = pow(acc, -1, R)
    out = [0] * len(v)
    for i in range(len(v) - 1, -1, -1):
        out[i] = pre[i] * inv % R
        inv = inv * v[i] % R
    return out
