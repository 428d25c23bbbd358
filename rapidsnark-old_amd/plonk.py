"""PLONK round 3 on the GPU (include/zkhip.h, section "PLONK quotient and coset transforms"): transforms on a coset of the
roots of unity and the quotient t = num / Z_H of a three-column circuit.  The arithmetic is libzkhip's; this module checks
shapes and ranges before any library call and turns Python values into the byte layout the library takes: scalars 32
bytes little-endian in standard form."""
import ctypes as C

import numpy as np

from . import lib as L
from .frscan import _one
from .kzg import _scalars
from .zkey import R_MOD

MIN_LOG_N, MAX_LOG_N, MAX_LOG_M = 1, 25, 28
_BASES = {"monomial": L.ZK_KZG_MONOMIAL, "lagrange": L.ZK_KZG_LAGRANGE}
_CIRCUIT = ("ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3")


def _shift(shift):
    """None, or one value that is not zero -> its 32 bytes"""
    if shift is None:
        return None
    b = _one(shift, "shift")
    if not b.any():
        raise ValueError("shift is zero")
    return b


def fr_coset_ntt(values, log_m=None, shift=None, inverse=False, device=-1):
    """numpy uint8 [2^log_m * 32] (zk_fr_coset_ntt).  Forward: values are n_in <= 2^log_m coefficients of p, out[i] =
    p(g w^i), w zk_fr_ntt's root for 2^log_m.  Inverse: values are 2^log_m evaluations, out[i] = coefficient i.  shift None:
    g = 1.  log_m None: the smallest size that holds the values."""
    a = _scalars(values, "values")
    n_in = a.size // 32
    if n_in < 1:
        raise ValueError("values: at least one value expected")
    if log_m is None:
        log_m = (n_in - 1).bit_length()
    log_m = int(log_m)
    if not 0 <= log_m <= MAX_LOG_M:
        raise ValueError("log_m %d is outside 0 .. %d" % (log_m, MAX_LOG_M))
    m = 1 << log_m
    if inverse and n_in != m:
        raise ValueError("n_in %d is not 2^log_m = %d" % (n_in, m))
    if n_in > m:
        raise ValueError("n_in %d is outside 1 .. 2^log_m = %d" % (n_in, m))
    g = _shift(shift)
    out = np.zeros(m * 32, dtype=np.uint8)
    L.check(L.load_library().zk_fr_coset_ntt(L._ptr(out), L._ptr(a), n_in, log_m, L._ptr(g) if g is not None else None, 1 if inverse else 0, device))
    return out


def _circuit_rows(vectors):
    """the eight circuit vectors -> (rows, n, log_n); one length, a power of two, log_n in range"""
    vecs = [_scalars(v, name) for name, v in zip(_CIRCUIT, vectors)]
    n = vecs[0].size // 32
    for name, v in zip(_CIRCUIT, vecs):
        if v.size != n * 32:
            raise ValueError("%s has %d rows, ql has %d: the eight circuit vectors must have one length" % (name, v.size // 32, n))
    if n < 1 or n & (n - 1):
        raise ValueError("n = %d is not a power of two" % n)
    log_n = n.bit_length() - 1
    if not MIN_LOG_N <= log_n <= MAX_LOG_N:
        raise ValueError("log_n %d is outside %d .. %d" % (log_n, MIN_LOG_N, MAX_LOG_N))
    return vecs, n, log_n


def _view(vectors, k1, k2, basis, shift=None, min_log_n=MIN_LOG_N):
    """(view, keep, n, log_n): a zk_plonk_circuit_view over the checked arguments, and the arrays it points into, which the
    caller holds while the library reads it"""
    if basis not in _BASES:
        raise ValueError("basis %r is unknown: 'monomial' or 'lagrange'" % (basis,))
    vecs, n, log_n = _circuit_rows(vectors)
    if log_n < min_log_n:
        raise ValueError("log_n %d is outside %d .. %d" % (log_n, min_log_n, MAX_LOG_N))
    kb1, kb2 = _one(k1, "k1"), _one(k2, "k2")
    g = _shift(shift)
    if g is not None and pow(int.from_bytes(g.tobytes(), "little") % R_MOD, 4 * n, R_MOD) == 1:
        raise ValueError("shift^(4n) is 1: Z_H vanishes on the coset")
    v = L.zk_plonk_circuit_view()
    v.log_n, v.basis = log_n, _BASES[basis]
    for name, a in zip(_CIRCUIT, vecs):
        setattr(v, name, a.ctypes.data)
    C.memmove(v.k1, kb1.ctypes.data, 32)
    C.memmove(v.k2, kb2.ctypes.data, 32)
    v.shift = g.ctypes.data if g is not None else None
    return v, (vecs, g), n, log_n


class _Object:
    """A library object behind a handle: closed by close(), by leaving a with block or by the collector.  A class names
    itself (_name), its destroy and info entries, its plan type and the plan's fields its info() leaves out."""
    _h = None
    _owned = ()                                         # objects made for this one, closed with it
    _drop = ("size", "reserved")

    def _handle(self):
        if not self._h:
            raise L.ZkHipError("the %s object is closed" % self._name)
        return self._h

    def _plan_dict(self):
        h = self._handle()
        plan = self._plan()
        plan.size = C.sizeof(plan)
        L.check(getattr(L.load_library(), self._info)(h, C.byref(plan)))
        return plan, {name: int(getattr(plan, name)) for name, _ in plan._fields_ if name not in self._drop}

    def close(self):
        if self._h:
            getattr(L.load_library(), self._destroy)(self._h)
            self._h = C.c_void_p()
        for o in self._owned:
            o.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _KzgObject(_Object):
    """.. on a Kzg's device, whose points it uses"""

    def _handle(self):
        h = super()._handle()
        self.kzg._handle()                              # a closed Kzg: its points are gone
        return h


def fr_poly_eval(coeffs, zs, device=-1):
    """a list of m ints p_k(z_k) (zk_fr_poly_eval): coeffs one polynomial (ints, or a flat byte array) or several of one
    length (a sequence of int sequences, or a 2-d uint8 array), zs one point each.  Nothing is committed to."""
    from .kzg import _polys
    a, n, m = _polys(coeffs, "coeffs")
    zb = _scalars([zs] if isinstance(zs, (int, np.integer)) else zs, "zs")
    if zb.size != m * 32:
        raise ValueError("zs: %d values for %d polynomials" % (zb.size // 32, m))
    ys = np.zeros(m * 32, dtype=np.uint8)
    L.check(L.load_library().zk_fr_poly_eval(L._ptr(ys), L._ptr(a), n, m, L._ptr(zb), device))
    yb = ys.tobytes()
    return [int.from_bytes(yb[i * 32:(i + 1) * 32], "little") for i in range(m)]


class PlonkOpening(_KzgObject):
    """Rounds 4 and 5 of a three-column PLONK proof on a Kzg's device (zk_plonk_opening): the eight circuit polynomials by
    coefficients, resident, and room for a proof's vectors.  basis "lagrange": values at w^j, converted once.  The object
    keeps a reference to the Kzg, whose points and multiplication it uses.  It is NOT checked that 1, k1, k2 name disjoint
    cosets."""
    _name, _destroy, _info, _plan = "PlonkOpening", "zk_plonk_opening_destroy", "zk_plonk_opening_info", L.zk_plonk_opening_plan

    def __init__(self, kzg, ql, qr, qm, qo, qc, s1, s2, s3, k1, k2, basis="monomial"):
        from .kzg import Kzg
        if not isinstance(kzg, Kzg):
            raise TypeError("a Kzg expected")
        v, keep, n, log_n = _view((ql, qr, qm, qo, qc, s1, s2, s3), k1, k2, basis)
        if n + 6 > kzg.max_coeffs:
            raise ValueError("n + 6 = %d exceeds the kzg's max_coeffs = %d" % (n + 6, kzg.max_coeffs))
        self._h = C.c_void_p()
        self.kzg, self.n, self.log_n, self.max_coeffs, self.device = kzg, n, log_n, kzg.max_coeffs, kzg.device
        kh = kzg._handle()
        L.check(L.load_library().zk_plonk_opening_create(C.byref(self._h), kh, C.byref(v), -1))

    def _vectors(self, names, lens, vectors):
        rows = [_scalars(v, name) for name, v in zip(names, vectors)]
        for name, r in zip(lens, rows):
            if not 1 <= r.size // 32 <= self.max_coeffs:
                raise ValueError("%s %d is outside 1 .. max_coeffs = %d" % (name, r.size // 32, self.max_coeffs))
        return rows

    def evaluate(self, a, b, c, z, zeta):
        """[a(zeta), b(zeta), c(zeta), s1(zeta), s2(zeta), z(zeta w)] as ints (zk_plonk_evaluate).  The vectors, zeta and the
        values stay in the object for open()."""
        rows = self._vectors("abcz", ("a_len", "b_len", "c_len", "z_len"), (a, b, c, z))
        zb = _one(zeta, "zeta")
        h = self._handle()
        ev = np.zeros(6 * 32, dtype=np.uint8)
        args = []
        for r in rows:
            args += [L._ptr(r), r.size // 32]
        L.check(L.load_library().zk_plonk_evaluate(h, L._ptr(ev), *args, L._ptr(zb)))
        eb = ev.tobytes()
        return [int.from_bytes(eb[i * 32:(i + 1) * 32], "little") for i in range(6)]

    def open(self, t_lo, t_mid, t_hi, alpha, beta, gamma, v, pi_zeta=0, want_f=False):
        """(W_zeta, W_zeta_omega, r_zeta[, F]) (zk_plonk_open): the two opening proofs (numpy uint8 [64] each), r(zeta) as an
        int (0 exactly when the round-3 identity holds at zeta; NOT judged here) and, when want_f, F's coefficients (numpy
        uint8 [f_len * 32]).  It consumes the evaluation evaluate() left."""
        rows = self._vectors(("t_lo", "t_mid", "t_hi"), ("lo_len", "mid_len", "hi_len"), (t_lo, t_mid, t_hi))
        sc = [_one(x, name) for name, x in zip(("alpha", "beta", "gamma", "v", "pi_zeta"), (alpha, beta, gamma, v, pi_zeta))]
        h = self._handle()
        wz, wzw, rz = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8), np.zeros(32, dtype=np.uint8)
        f = np.zeros(self.max_coeffs * 32, dtype=np.uint8) if want_f else None
        f_len = C.c_uint64(0)
        args = []
        for r in rows:
            args += [L._ptr(r), r.size // 32]
        L.check(L.load_library().zk_plonk_open(h, L._ptr(wz), L._ptr(wzw), L._ptr(rz), L._ptr(f) if want_f else None, C.byref(f_len), *args,
                                               L._ptr(sc[4]), L._ptr(sc[0]), L._ptr(sc[1]), L._ptr(sc[2]), L._ptr(sc[3])))
        out = (wz, wzw, int.from_bytes(rz.tobytes(), "little"))
        return out + (f[:int(f_len.value) * 32],) if want_f else out

    def info(self):
        """zk_plonk_opening_info -> dict: log_n, device_bytes, seg (ZKHIP_OPEN_SEG in effect), last_launches, pending"""
        return self._plan_dict()[1]


class PlonkCircuit(_Object):
    """What does not change from proof to proof of a three-column PLONK circuit, on a device (zk_plonk_circuit): the eight
    polynomials extended to the coset shift * (4n-th roots of unity).  basis "monomial": coefficients; "lagrange": values at
    w^j, what plonk_permutation_product takes.  It is NOT checked that 1, k1, k2 name disjoint cosets."""
    _name, _destroy, _info, _plan = "PlonkCircuit", "zk_plonk_circuit_destroy", "zk_plonk_circuit_info", L.zk_plonk_circuit_plan

    def __init__(self, ql, qr, qm, qo, qc, s1, s2, s3, k1, k2, basis="monomial", shift=None, device=-1):
        v, keep, n, log_n = _view((ql, qr, qm, qo, qc, s1, s2, s3), k1, k2, basis, shift)
        self.n, self.log_n, self.device = n, log_n, int(device)
        self._h = C.c_void_p()
        L.check(L.load_library().zk_plonk_circuit_create(C.byref(self._h), C.byref(v), device))

    def quotient(self, a, b, c, z, alpha, beta, gamma, pi=None):
        """(t, t_len): t a numpy uint8 array of 4n rows, the coefficients of t = num / Z_H with zeros from t_len on; t_len one
        more than the index of the highest non-zero coefficient (zk_plonk_quotient).  a, b, c, z: coefficients, 1 .. 2n of
        each and at most 5n + 3 together; pi: n coefficients or None.  A t_len above the caller's bound (3n - 3 unblinded,
        3n + 6 with the usual blinding) is a necessary sign of a bad witness; it does NOT replace a gate check."""
        n = self.n
        polys = [_scalars(v, name) for name, v in zip("abcz", (a, b, c, z))]
        lens = [p.size // 32 for p in polys]
        for name, k in zip("abcz", lens):
            if not 1 <= k <= 2 * n:
                raise ValueError("%s_len %d is outside 1 .. 2n = %d" % (name, k, 2 * n))
        if sum(lens) > 5 * n + 3:
            raise ValueError("a_len + b_len + c_len + z_len = %d exceeds 5n + 3 = %d: t would have more than 4n coefficients" % (sum(lens), 5 * n + 3))
        pb = None
        if pi is not None:
            pb = _scalars(pi, "pi")
            if pb.size != n * 32:
                raise ValueError("pi: %d values, n = %d expected" % (pb.size // 32, n))
        ab, bb, gb = _one(alpha, "alpha"), _one(beta, "beta"), _one(gamma, "gamma")
        h = self._handle()
        t = np.zeros(4 * n * 32, dtype=np.uint8)
        t_len = C.c_uint64(0)
        L.check(L.load_library().zk_plonk_quotient(h, L._ptr(t), C.byref(t_len), L._ptr(polys[0]), lens[0], L._ptr(polys[1]), lens[1], L._ptr(polys[2]), lens[2],
                                                   L._ptr(polys[3]), lens[3], L._ptr(pb) if pb is not None else None, L._ptr(ab), L._ptr(bb), L._ptr(gb)))
        return t, int(t_len.value)

    def info(self):
        """zk_plonk_circuit_info -> dict: log_n, points (4n), device_bytes, seg (ZKHIP_QUOT_SEG in effect), last_launches"""
        return self._plan_dict()[1]


# ---------------------------------------------------------------- the prover and the verifier
# include/zkhip.h, section "PLONK prover and verifier": the five rounds chained on the device, the Keccak-256 transcript
# and the verifier.  Parity with snarkjs is unpinned (no file made by snarkjs was at hand): the layout is the header's.
PROOF_BYTES, BLINDS, MIN_PROVER_LOG_N = 768, 11, 3
Q_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
_Q_RINV = pow(1 << 256, -1, Q_MOD)
_POINTS = ("A", "B", "C", "Z", "T1", "T2", "T3", "Wxi", "Wxiw")         # snarkjs's names, the proof's order
_EVALS = ("eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw")


def keccak256(data):
    """32 bytes: Keccak-256 with the original 0x01 padding (zk_keccak256).  No device."""
    a = L._buf(bytes(data))
    out = np.zeros(32, dtype=np.uint8)
    L.check(L.load_library().zk_keccak256(L._ptr(out), L._ptr(a) if a.size else None, a.size))
    return out.tobytes()


def _affine(b):
    """64 bytes in the .ptau encoding -> (x, y) standard ints, None for infinity"""
    if not any(b):
        return None
    return (int.from_bytes(b[:32], "little") * _Q_RINV % Q_MOD, int.from_bytes(b[32:], "little") * _Q_RINV % Q_MOD)


class PlonkProof:
    """768 bytes: [a] [b] [c] [z] [t_lo] [t_mid] [t_hi] [W_zeta] [W_zeta_omega] in the .ptau encoding, then a(zeta), b(zeta),
    c(zeta), s1(zeta), s2(zeta), z(zeta w) as 32 bytes little-endian."""

    def __init__(self, data):
        data = bytes(data)
        if len(data) != PROOF_BYTES:
            raise ValueError("a proof of %d bytes expected, got %d" % (PROOF_BYTES, len(data)))
        self._b = data

    def to_bytes(self):
        return self._b

    @property
    def points(self):
        return [self._b[i * 64:(i + 1) * 64] for i in range(9)]

    @property
    def evals(self):
        return [int.from_bytes(self._b[576 + i * 32:576 + (i + 1) * 32], "little") for i in range(6)]

    def to_json(self):
        """snarkjs's proof.json: its field names, decimal strings, projective points with z = 1 (infinity: 0, 1, 0)"""
        import json
        d = {}
        for name, p in zip(_POINTS, self.points):
            xy = _affine(p)
            d[name] = ["0", "1", "0"] if xy is None else [str(xy[0]), str(xy[1]), "1"]
        for name, v in zip(_EVALS, self.evals):
            d[name] = str(v)
        d["protocol"], d["curve"] = "plonk", "bn128"
        return json.dumps(d, indent=1)

    def __eq__(self, other):
        return isinstance(other, PlonkProof) and self._b == other._b

    def __hash__(self):
        return hash(self._b)


_COMMITMENTS = ("qm", "ql", "qr", "qo", "qc", "s1", "s2", "s3")          # the transcript's order
_KEY_POINTS = ("Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3")           # snarkjs's names for them


def root_of_unity(power):
    """zk_fr_ntt's root for 2^power (the `w` of a key file): 5^((r - 1) / 2^28) squared 28 - power times"""
    return pow(pow(5, (R_MOD - 1) >> 28, R_MOD), 1 << (28 - power), R_MOD)


def _coords_to_bytes(coords, what):
    """standard coordinates below 2^256 -> the .ptau encoding; one that is not below q goes as written, for the library to refuse"""
    out = b""
    for x in coords:
        if not 0 <= x < 1 << 256:
            raise ValueError("%s: a coordinate is not in 0 .. 2^256 - 1" % what)
        out += (x * (1 << 256) % Q_MOD if x < Q_MOD else x).to_bytes(32, "little")
    return out


def _g1_bytes(p, what):
    """64 bytes in the .ptau encoding, or (x, y) standard ints, or None (infinity) -> 64 bytes"""
    if p is None:
        return bytes(64)
    if isinstance(p, (bytes, bytearray, memoryview, np.ndarray)):
        b = bytes(p)
        if len(b) != 64:
            raise ValueError("%s: a point of 64 bytes expected, got %d" % (what, len(b)))
        return b
    x, y = p
    return _coords_to_bytes((int(x), int(y)), what)


def _g2_bytes(p, what):
    """128 bytes, or ((xa, xb), (ya, yb)), or None -> 128 bytes"""
    if p is None:
        return bytes(128)
    if isinstance(p, (bytes, bytearray, memoryview, np.ndarray)):
        b = bytes(p)
        if len(b) != 128:
            raise ValueError("%s: a point of 128 bytes expected, got %d" % (what, len(b)))
        return b
    (xa, xb), (ya, yb) = p
    return _coords_to_bytes((int(xa), int(xb), int(ya), int(yb)), what)


def _dec(v, what):
    if isinstance(v, bool) or not isinstance(v, (str, int)) or (isinstance(v, str) and not v.isdigit()):
        raise ValueError("%s is not a decimal integer below 2^256" % what)
    x = int(v)
    if not 0 <= x < 1 << 256:
        raise ValueError("%s is not a decimal integer below 2^256" % what)
    return x


def _json_g1(v, what):
    """[x, y] or [x, y, z] -> 64 bytes; z = 0 is infinity, any other z divides x and y (as `verifier` reads a point)"""
    if not isinstance(v, list) or len(v) < 2:
        raise ValueError("%s is not an array of at least 2 elements" % what)
    c = [_dec(t, "%s[%d]" % (what, i)) for i, t in enumerate(v[:3])]
    if len(c) == 3 and all(t < Q_MOD for t in c):
        if c[2] == 0:
            return bytes(64)
        zi = pow(c[2], -1, Q_MOD)
        c = [c[0] * zi % Q_MOD, c[1] * zi % Q_MOD]
    return _coords_to_bytes(c[:2], what)


def _json_g2(v, what):
    if not isinstance(v, list) or len(v) < 2 or not all(isinstance(t, list) and len(t) >= 2 for t in v[:3]):
        raise ValueError("%s is not an array of at least 2 pairs" % what)
    c = [[_dec(t, "%s[%d][%d]" % (what, i, j)) for j, t in enumerate(pair[:2])] for i, pair in enumerate(v[:3])]
    if len(c) == 3 and all(t < Q_MOD for pair in c for t in pair):
        za, zb = c[2]
        if za == 0 and zb == 0:
            return bytes(128)
        d = pow(za * za + zb * zb, -1, Q_MOD)                       # 1 / (za + zb u) = (za - zb u) / (za^2 + zb^2)
        ia, ib = za * d % Q_MOD, -zb * d % Q_MOD
        c = [[(a * ia - b * ib) % Q_MOD, (a * ib + b * ia) % Q_MOD] for a, b in c[:2]]
    return _coords_to_bytes(c[0] + c[1], what)


class PlonkVKey:
    """What a verifier needs (zk_plonk_vkey): log_n, n_public, k1, k2, the eight commitments and [tau]G2.  A key a prover
    made keeps the Kzg whose [tau]G2 it names, for plonk_verify; one read from a key file or made from parts has kzg = None
    and is what a PlonkVerifier takes.  The key file has snarkjs's field names (to_json); it names a key of THIS project's
    compile and transcript: parity with snarkjs is unpinned."""

    def __init__(self, kzg, c):
        self.kzg, self._c = kzg, c

    @classmethod
    def from_parts(cls, log_n, n_public, k1, k2, commitments, tau_g2):
        """commitments: eight points in the transcript's order qm ql qr qo qc s1 s2 s3 (or a dict by those names), each 64
        bytes in the .ptau encoding, (x, y) standard ints or None for infinity; tau_g2: 128 bytes or ((xa, xb), (ya, yb)).
        Nothing is judged here but the shapes: a bad key is zk_plonk_verifier_create's to refuse."""
        if isinstance(commitments, dict):
            commitments = [commitments[name] for name in _COMMITMENTS]
        commitments = list(commitments)
        if len(commitments) != 8:
            raise ValueError("commitments: %d points, 8 expected" % len(commitments))
        c = L.zk_plonk_vkey()
        c.size = C.sizeof(c)
        log_n, n_public = int(log_n), int(n_public)
        if not 0 <= log_n < 1 << 32 or not 0 <= n_public < 1 << 64:
            raise ValueError("log_n or n_public is out of range")
        c.log_n, c.n_public = log_n, n_public
        for name, v in (("k1", k1), ("k2", k2)):
            v = int(v)
            if not 0 <= v < 1 << 256:
                raise ValueError("%s is not in 0 .. 2^256 - 1" % name)
            C.memmove(getattr(c, name), v.to_bytes(32, "little"), 32)
        for name, p in zip(_COMMITMENTS, commitments):
            C.memmove(getattr(c, name), _g1_bytes(p, name), 64)
        C.memmove(c.tau_g2, _g2_bytes(tau_g2, "tau_g2"), 128)
        return cls(None, c)

    def to_json(self):
        """verification_key.json with snarkjs's field names for PLONK: protocol, curve, nPublic, power, k1, k2, Qm Ql Qr Qo Qc
        S1 S2 S3, X_2, w; decimal strings, projective points with z = 1 (infinity: 0 1 0)"""
        import json
        d = {"protocol": "plonk", "curve": "bn128", "nPublic": self.n_public, "power": self.log_n, "k1": str(self.k1), "k2": str(self.k2)}
        for key, name in zip(_KEY_POINTS, _COMMITMENTS):
            xy = _affine(bytes(getattr(self._c, name)))
            d[key] = ["0", "1", "0"] if xy is None else [str(xy[0]), str(xy[1]), "1"]
        t = self.tau_g2
        if not any(t):
            d["X_2"] = [["0", "0"], ["1", "0"], ["0", "0"]]
        else:
            v = [str(int.from_bytes(t[i * 32:(i + 1) * 32], "little") * _Q_RINV % Q_MOD) for i in range(4)]
            d["X_2"] = [v[0:2], v[2:4], ["1", "0"]]
        d["w"] = str(root_of_unity(self.log_n)) if 0 <= self.log_n <= 28 else "0"
        return json.dumps(d, indent=1)

    @classmethod
    def from_json(cls, text):
        """The key of to_json, of the program plonkvkey, or of snarkjs (third coordinates honoured as `verifier` does).
        Refused by name: another protocol or curve, a power outside 0 .. 28, a w that is not this library's root for the
        power."""
        import json
        try:
            d = json.loads(text)
        except ValueError as e:
            raise ValueError("the key is not JSON (%s)" % e)
        if not isinstance(d, dict):
            raise ValueError("the key is not a JSON object")
        if d.get("protocol") != "plonk":
            raise ValueError("protocol \"%s\" is not plonk" % d.get("protocol"))
        if d.get("curve") not in ("bn128", "bn254"):
            raise ValueError("curve \"%s\" is not bn128" % d.get("curve"))
        for key in ("nPublic", "power", "k1", "k2", "X_2", "w") + _KEY_POINTS:
            if key not in d:
                raise ValueError("the key has no \"%s\"" % key)
        power, n_public = _dec(d["power"], "power"), _dec(d["nPublic"], "nPublic")
        if power > 28:
            raise ValueError("power %d is outside 0 .. 28" % power)
        if _dec(d["w"], "w") != root_of_unity(power):
            raise ValueError("w is not this library's root of unity for power %d" % power)
        if n_public >= 1 << 64:
            raise ValueError("nPublic is not below 2^64")
        return cls.from_parts(power, n_public, _dec(d["k1"], "k1"), _dec(d["k2"], "k2"), [_json_g1(d[k], k) for k in _KEY_POINTS], _json_g2(d["X_2"], "X_2"))

    log_n = property(lambda self: int(self._c.log_n))
    n = property(lambda self: 1 << int(self._c.log_n))
    n_public = property(lambda self: int(self._c.n_public))
    k1 = property(lambda self: int.from_bytes(bytes(self._c.k1), "little"))
    k2 = property(lambda self: int.from_bytes(bytes(self._c.k2), "little"))
    tau_g2 = property(lambda self: bytes(self._c.tau_g2))

    @property
    def commitments(self):
        """name -> 64 bytes, the transcript's order"""
        return {name: bytes(getattr(self._c, name)) for name in ("qm", "ql", "qr", "qo", "qc", "s1", "s2", "s3")}


def _maps(maps, n, n_witness):
    out = []
    for name, m in zip(("a_map", "b_map", "c_map"), maps):
        a = np.ascontiguousarray(np.asarray(m, dtype=np.int64).reshape(-1))
        if a.size != n:
            raise ValueError("%s has %d indices, n = %d expected" % (name, a.size, n))
        bad = np.nonzero((a < 0) | (a >= n_witness))[0]
        if bad.size:
            raise ValueError("%s %d is %d, not below n_witness = %d" % (name, int(bad[0]), int(a[bad[0]]), n_witness))
        out.append(a.astype(np.uint32))
    return out


class PlonkProver(_KzgObject):
    """A three-column PLONK prover for one circuit on a Kzg's device (zk_plonk_prover): everything that does not change from
    proof to proof stays resident, a proof uploads the witness and nothing else per row.  Row i's wires are
    witness[a_map[i]], witness[b_map[i]], witness[c_map[i]].  The object keeps a reference to the Kzg."""
    _name, _destroy, _info, _plan = "PlonkProver", "zk_plonk_prover_destroy", "zk_plonk_prover_info", L.zk_plonk_prover_plan
    _drop = ("size", "round_launches")

    def __init__(self, kzg, ql, qr, qm, qo, qc, s1, s2, s3, k1, k2, a_map, b_map, c_map, n_witness, n_public=0, basis="monomial", shift=None):
        from .kzg import Kzg
        if not isinstance(kzg, Kzg):
            raise TypeError("a Kzg expected")
        v, keep, n, log_n = _view((ql, qr, qm, qo, qc, s1, s2, s3), k1, k2, basis, shift, MIN_PROVER_LOG_N)
        if n + 6 > kzg.max_coeffs:
            raise ValueError("n + 6 = %d exceeds the kzg's max_coeffs = %d" % (n + 6, kzg.max_coeffs))
        n_witness, n_public = int(n_witness), int(n_public)
        if n_witness < 1:
            raise ValueError("n_witness is %d: at least one value expected" % n_witness)
        if not 0 <= n_public <= n:
            raise ValueError("n_public %d is outside 0 .. n = %d" % (n_public, n))
        maps = _maps((a_map, b_map, c_map), n, n_witness)
        self._h = C.c_void_p()
        self.kzg, self.n, self.log_n, self.n_witness, self.n_public, self.device = kzg, n, log_n, n_witness, n_public, kzg.device
        kh = kzg._handle()
        L.check(L.load_library().zk_plonk_prover_create(C.byref(self._h), kh, C.byref(v), L._ptr(maps[0]), L._ptr(maps[1]), L._ptr(maps[2]), n_witness,
                                                        n_public, -1))

    r1cs = None                                         # the PlonkR1cs of a prover made by from_r1cs

    @classmethod
    def from_r1cs(cls, kzg, r1cs, shift=None):
        """A prover over a compiled circuit (zk_plonk_prover_create_r1cs).  r1cs: a PlonkR1cs, which the prover borrows, or a
        .r1cs path or bytes, compiled here with k1 = 2, k2 = 3 on the kzg's device and closed with the prover."""
        from .kzg import Kzg
        if not isinstance(kzg, Kzg):
            raise TypeError("a Kzg expected")
        g = _shift(shift)
        own = not isinstance(r1cs, PlonkR1cs)
        c = PlonkR1cs(r1cs, device=kzg.device) if own else r1cs
        try:
            if c.n + 6 > kzg.max_coeffs:
                raise ValueError("n + 6 = %d exceeds the kzg's max_coeffs = %d" % (c.n + 6, kzg.max_coeffs))
            self = cls.__new__(cls)
            self._h = C.c_void_p()
            self.kzg, self.n, self.log_n, self.n_witness, self.n_public, self.device = kzg, c.n, c.log_n, c.n_witness, c.n_public, kzg.device
            self.r1cs, self._owned = c, (c,) if own else ()
            L.check(L.load_library().zk_plonk_prover_create_r1cs(C.byref(self._h), kzg._handle(), c._handle(), L._ptr(g) if g is not None else None, -1))
        except Exception:
            if own:
                c.close()
            raise
        return self

    def prove_r1cs(self, wtns, blind=None):
        """-> PlonkProof (zk_plonk_prove_r1cs) from a circom witness: a .wtns path or bytes, or the raw values (a numpy uint8
        array or a PinnedBuffer), as R1cs.check takes it.  The device extends it; the publics are its values 1 .. n_public.
        blind and ZKHIP_SELFVERIFY: as prove."""
        import os
        if self.r1cs is None:
            if not self._h:
                raise L.ZkHipError("the PlonkProver object is closed")
            raise L.ZkHipError("zk_plonk_prove_r1cs: the prover was not made from an r1cs (zk_plonk_prover_create_r1cs)")
        a, n_vars = self.r1cs._values(wtns)
        bb = None
        if blind is not None:
            bb = _scalars(blind, "blind")
            if bb.size != BLINDS * 32:
                raise ValueError("blind: %d values, %d expected" % (bb.size // 32, BLINDS))
        h = self._handle()
        self.r1cs._handle()
        out = np.zeros(PROOF_BYTES, dtype=np.uint8)
        L.check(L.load_library().zk_plonk_prove_r1cs(h, L._ptr(out), C.c_void_p(a.ctypes.data) if a.size else None, n_vars,
                                                     L._ptr(bb) if bb is not None else None))
        proof = PlonkProof(out.tobytes())
        if os.environ.get("ZKHIP_SELFVERIFY") == "1":
            verdict = plonk_verify(self.vkey(), proof, np.array(a[32:32 * (1 + self.n_public)]))
            if verdict != 0:
                raise L.ZkHipError("ZKHIP_SELFVERIFY: the proof does not verify (verdict %d)" % verdict)
        return proof

    def prove(self, witness, publics=None, blind=None):
        """-> PlonkProof (zk_plonk_prove).  publics None: witness[1 : 1 + n_public], circom's layout.  blind None: eleven
        scalars from the OS generator; given (FOR TESTS ONLY): b1 .. b11.  ZKHIP_SELFVERIFY=1: the proof is verified before
        it is returned."""
        import os
        w = _scalars(witness, "witness")
        if w.size != self.n_witness * 32:
            raise ValueError("witness: %d values, n_witness = %d expected" % (w.size // 32, self.n_witness))
        if publics is None:
            if 1 + self.n_public > self.n_witness:
                raise ValueError("publics: the witness has no %d values after its first" % self.n_public)
            pb = w[32:32 * (1 + self.n_public)].copy()
        else:
            pb = _scalars(publics, "publics")
            if pb.size != self.n_public * 32:
                raise ValueError("publics: %d values, n_public = %d expected" % (pb.size // 32, self.n_public))
        bb = None
        if blind is not None:
            bb = _scalars(blind, "blind")
            if bb.size != BLINDS * 32:
                raise ValueError("blind: %d values, %d expected" % (bb.size // 32, BLINDS))
        h = self._handle()
        out = np.zeros(PROOF_BYTES, dtype=np.uint8)
        L.check(L.load_library().zk_plonk_prove(h, L._ptr(out), L._ptr(w), L._ptr(pb) if self.n_public else None, L._ptr(bb) if bb is not None else None))
        proof = PlonkProof(out.tobytes())
        if os.environ.get("ZKHIP_SELFVERIFY") == "1":
            verdict = plonk_verify(self.vkey(), proof, pb)
            if verdict != 0:
                raise L.ZkHipError("ZKHIP_SELFVERIFY: the proof does not verify (verdict %d)" % verdict)
        return proof

    # ---- many witnesses a call (include/zkhip.h: zk_plonk_prove_many and its neighbours)
    def _many_blinds(self, blinds, m):
        """None, or m rows of eleven scalars (or their m x 11 x 32 bytes) -> bytes or None.  Values are the library's to judge"""
        if blinds is None:
            return None
        if isinstance(blinds, (bytes, bytearray, memoryview)) or (isinstance(blinds, np.ndarray) and blinds.dtype == np.uint8):
            bb = L._buf(blinds)
            if bb.size != m * BLINDS * 32:
                raise ValueError("blinds: %d bytes, %d rows of %d scalars expected" % (bb.size, m, BLINDS))
            return bb
        blinds = list(blinds)
        if len(blinds) != m:
            raise ValueError("blinds: %d rows for %d witnesses" % (len(blinds), m))
        rows = []
        for i, row in enumerate(blinds):
            r = _scalars(row, "blinds[%d]" % i, below_r=False)
            if r.size != BLINDS * 32:
                raise ValueError("blinds[%d]: %d values, %d expected" % (i, r.size // 32, BLINDS))
            rows.append(r)
        return np.concatenate(rows) if rows else np.zeros(0, dtype=np.uint8)

    def _many_result(self, out, status, publics_of):
        """the call's bytes -> (list of PlonkProof or None, status); ZKHIP_SELFVERIFY=1: the proofs made go through ONE verify call"""
        import os
        m = status.size
        proofs = [PlonkProof(out[i * PROOF_BYTES:(i + 1) * PROOF_BYTES].tobytes()) if status[i] == 0 else None for i in range(m)]
        made = [i for i in range(m) if status[i] == 0]
        if made and os.environ.get("ZKHIP_SELFVERIFY") == "1":
            with PlonkVerifier(self.vkey(), device=self.device) as v:
                verdicts = v.verify([proofs[i] for i in made], [publics_of(i) for i in made] if self.n_public else None)
            bad = [j for j in range(len(made)) if verdicts[j] != 0]
            if bad:
                raise L.ZkHipError("ZKHIP_SELFVERIFY: proof %d does not verify (verdict %d)" % (made[bad[0]], int(verdicts[bad[0]])))
        return proofs, status

    def prove_many(self, witnesses, publics=None, blinds=None):
        """-> (list of PlonkProof or None, numpy uint32 [m] status) (zk_plonk_prove_many): m witnesses of the circuit in one call,
        proof i what prove(witnesses[i], publics[i], blinds[i]) gives.  A witness the prover refuses gives None and a status that
        is not 0 (1: a zero denominator, 2: the copies, 3: the gates, 4: a value not below r) and does not take the others with
        it.  publics None: each witness's values 1 .. n_public.  blinds None: drawn; given (FOR TESTS ONLY): m rows of eleven.
        ZKHIP_PLONK_PROVE_BATCH sets how many proofs share a round's multiplication.  ZKHIP_SELFVERIFY=1: the proofs made are
        verified, in ONE PlonkVerifier.verify call, before they are returned."""
        witnesses = list(witnesses)
        m = len(witnesses)
        ws = []
        for i, w in enumerate(witnesses):
            a = _scalars(w, "witnesses[%d]" % i, below_r=False)
            if a.size != self.n_witness * 32:
                raise ValueError("witnesses[%d]: %d values, n_witness = %d expected" % (i, a.size // 32, self.n_witness))
            ws.append(a)
        if publics is None:
            if 1 + self.n_public > self.n_witness:
                raise ValueError("publics: a witness has no %d values after its first" % self.n_public)
            ps = [w[32:32 * (1 + self.n_public)] for w in ws]
        else:
            publics = list(publics)
            if len(publics) != m:
                raise ValueError("publics: %d rows for %d witnesses" % (len(publics), m))
            ps = []
            for i, row in enumerate(publics):
                a = _scalars(row, "publics[%d]" % i, below_r=False)
                if a.size != self.n_public * 32:
                    raise ValueError("publics[%d]: %d values, n_public = %d expected" % (i, a.size // 32, self.n_public))
                ps.append(a)
        bb = self._many_blinds(blinds, m)
        h = self._handle()
        wb = np.concatenate(ws) if ws else np.zeros(0, dtype=np.uint8)
        pb = np.concatenate(ps) if ps and self.n_public else None
        out = np.zeros(m * PROOF_BYTES, dtype=np.uint8)
        status = np.full(m, 0xFFFFFFFF, dtype=np.uint32)
        L.check(L.load_library().zk_plonk_prove_many(h, m, L._ptr(out) if m else None, L._ptr(status) if m else None, L._ptr(wb) if m else None,
                                                     L._ptr(pb) if pb is not None and m else None, L._ptr(bb) if bb is not None and m else None))
        return self._many_result(out, status, lambda i: ps[i])

    def prove_r1cs_many(self, wtns, blinds=None):
        """-> (list of PlonkProof or None, status) (zk_plonk_prove_r1cs_many) from m circom witnesses, each as prove_r1cs takes
        its one; the device extends each.  blinds and ZKHIP_SELFVERIFY: as prove_many."""
        if self.r1cs is None:
            if not self._h:
                raise L.ZkHipError("the PlonkProver object is closed")
            raise L.ZkHipError("zk_plonk_prove_r1cs_many: the prover was not made from an r1cs (zk_plonk_prover_create_r1cs)")
        vals = [self.r1cs._values(w) for w in wtns]
        m = len(vals)
        for i, (a, n_vars) in enumerate(vals):
            if n_vars != vals[0][1]:
                raise ValueError("wtns[%d] has %d values, wtns[0] has %d: the witnesses must have one length" % (i, n_vars, vals[0][1]))
            if a.size < n_vars * 32:
                raise ValueError("wtns[%d]: %d bytes for %d values" % (i, a.size, n_vars))
        n_vars = vals[0][1] if m else self.r1cs.n_wires
        bb = self._many_blinds(blinds, m)
        h = self._handle()
        self.r1cs._handle()
        wb = np.concatenate([a[:n_vars * 32] for a, _ in vals]) if m else np.zeros(0, dtype=np.uint8)
        out = np.zeros(m * PROOF_BYTES, dtype=np.uint8)
        status = np.full(m, 0xFFFFFFFF, dtype=np.uint32)
        L.check(L.load_library().zk_plonk_prove_r1cs_many(h, m, L._ptr(out) if m else None, L._ptr(status) if m else None, L._ptr(wb) if wb.size else None,
                                                          n_vars, L._ptr(bb) if bb is not None and m else None))
        return self._many_result(out, status, lambda i: np.array(vals[i][0][32:32 * (1 + self.n_public)]))

    def commit_many(self, coeffs):
        """list of k commitments, 64 bytes each (zk_plonk_prover_commit_many): k polynomials of at most n + 6 coefficients each
        (sequences of ints, or uint8 rows), through the prover's table and its batched multiplication."""
        n6 = self.n + 6
        rows = []
        for i, c in enumerate(coeffs):
            a = _scalars(c, "coeffs[%d]" % i, below_r=False)
            if not 1 <= a.size // 32 <= n6:
                raise ValueError("coeffs[%d]: %d coefficients, 1 .. n + 6 = %d expected" % (i, a.size // 32, n6))
            rows.append(np.concatenate([a, np.zeros(n6 * 32 - a.size, dtype=np.uint8)]))
        if not rows:
            raise ValueError("coeffs: at least one polynomial expected")
        h = self._handle()
        cb = np.concatenate(rows)
        out = np.zeros(len(rows) * 64, dtype=np.uint8)
        L.check(L.load_library().zk_plonk_prover_commit_many(h, L._ptr(out), L._ptr(cb), len(rows)))
        ob = out.tobytes()
        return [ob[i * 64:(i + 1) * 64] for i in range(len(rows))]

    def many_info(self):
        """zk_plonk_prover_many_info -> dict: batch (the chunk width in effect), table_batch, window_bits, table_rows,
        table_bytes, slot_bytes, msm_bytes, and of the last many-call last_chunks, last_multiplications, last_launches,
        last_drains, last_refused"""
        h = self._handle()
        plan = L.zk_plonk_prover_many_plan()
        plan.size = C.sizeof(plan)
        L.check(L.load_library().zk_plonk_prover_many_info(h, C.byref(plan)))
        return {name: int(getattr(plan, name)) for name, _ in plan._fields_ if name not in ("size", "reserved", "reserved2")}

    def vkey(self):
        """-> PlonkVKey (zk_plonk_prover_vkey): log_n, n_public, k1, k2, the eight commitments and [tau]G2"""
        h = self._handle()
        c = L.zk_plonk_vkey()
        c.size = C.sizeof(c)
        L.check(L.load_library().zk_plonk_prover_vkey(h, C.byref(c)))
        return PlonkVKey(self.kzg, c)

    def info(self):
        """zk_plonk_prover_info -> dict: log_n, n_witness, n_public, device_bytes, the four knobs in effect, last_launches and
        round_launches (a list of five)"""
        plan, d = self._plan_dict()
        d["round_launches"] = [int(x) for x in plan.round_launches]
        return d


class PlonkR1cs(_Object):
    """A circom .r1cs compiled on a device to a three-column PLONK circuit (zk_plonk_r1cs; include/zkhip.h, section "PLONK
    from an R1CS", states the layout): .vectors, the eight vectors ql qr qm qo qc s1 s2 s3 as values over the domain (a list of
    numpy uint8 [n * 32]), .maps (three numpy uint32 [n]), and extend(wtns), the witness a proof needs.  Custom gates are
    refused as by R1cs.  k1, k2 must name, with 1, three different cosets of the n-th roots of unity."""
    _name, _destroy, _info, _plan = "PlonkR1cs", "zk_plonk_r1cs_destroy", "zk_plonk_r1cs_info", L.zk_plonk_r1cs_plan

    def __init__(self, path_or_bytes, k1=2, k2=3, device=-1):
        from .r1cs import open_r1cs
        kb1, kb2 = _one(k1, "k1"), _one(k2, "k2")
        self.header, sec = open_r1cs(path_or_bytes)
        h = self.header
        keep = np.frombuffer(sec, dtype=np.uint8)
        v = L.zk_r1cs_view(h.nWires, h.nPubOut, h.nPubIn, h.nPrvIn, h.nConstraints, keep.ctypes.data if keep.size else None, keep.size)
        self._h = C.c_void_p()
        self.k1, self.k2, self.device = int(k1), int(k2), int(device)
        self._circuit = None
        L.check(L.load_library().zk_plonk_r1cs_create(C.byref(self._h), C.byref(v), L._ptr(kb1), L._ptr(kb2), device))
        d = self.info()
        self.log_n, self.n, self.rows = d["log_n"], 1 << d["log_n"], d["rows"]
        self.n_public, self.n_wires, self.n_additions, self.n_witness = d["n_public"], d["n_wires"], d["n_additions"], d["n_witness"]

    def _fetch(self):
        if self._circuit is None:
            h = self._handle()
            n = self.n
            vec = np.zeros(8 * n * 32, dtype=np.uint8)
            maps = [np.zeros(n, dtype=np.uint32) for _ in range(3)]
            L.check(L.load_library().zk_plonk_r1cs_circuit(h, L._ptr(vec), *[L._ptr(m) for m in maps]))
            self._circuit = ([vec[j * n * 32:(j + 1) * n * 32] for j in range(8)], maps)
        return self._circuit

    vectors = property(lambda self: self._fetch()[0])
    maps = property(lambda self: self._fetch()[1])

    def _values(self, wtns):
        from .r1cs import R1cs
        return R1cs._values(self, wtns)

    def extend(self, wtns):
        """numpy uint8 [n_witness * 32]: the circom witness (a .wtns path or bytes, or its raw values) and, after it, the
        values of the wires the addition gates introduced (zk_plonk_r1cs_extend)"""
        h = self._handle()
        a, n_vars = self._values(wtns)
        out = np.zeros(self.n_witness * 32, dtype=np.uint8)
        L.check(L.load_library().zk_plonk_r1cs_extend(h, L._ptr(out), C.c_void_p(a.ctypes.data) if a.size else None, n_vars))
        return out

    def info(self):
        """zk_plonk_r1cs_info -> dict: log_n, rows (N), n_public, n_wires, n_additions, n_witness, terms, device_bytes, seg
        (ZKHIP_R1CS_SEG in effect), sort_passes, last_launches"""
        return self._plan_dict()[1]


def plonk_verify(vkey, proof, publics=(), kzg=None):
    """VERIFY_OK (0) / VERIFY_INVALID (1) / VERIFY_MALFORMED (2) for one proof (zk_plonk_verify).  proof: a PlonkProof or
    its 768 bytes.  The pairing product runs on the device of the key's Kzg (or the one given)."""
    if not isinstance(vkey, PlonkVKey):
        raise TypeError("a PlonkVKey expected (PlonkProver.vkey())")
    pr = proof if isinstance(proof, PlonkProof) else PlonkProof(proof)
    # values that are not below r are the library's to refuse (MALFORMED): they must only fit 32 bytes
    pb = _scalars(publics, "publics", below_r=False)
    if pb.size != vkey.n_public * 32:
        raise ValueError("publics: %d values, n_public = %d expected" % (pb.size // 32, vkey.n_public))
    k = kzg if kzg is not None else vkey.kzg
    if k is None:
        raise ValueError("the key names no Kzg (it was read from a key file or made from parts): pass kzg=, or verify with PlonkVerifier(vkey), "
                         "which needs the key alone")
    h = k._handle()
    a = L._buf(pr.to_bytes())
    verdict = np.full(1, 255, dtype=np.uint8)
    L.check(L.load_library().zk_plonk_verify(h, C.byref(vkey._c), L._ptr(a), L._ptr(pb) if vkey.n_public else None, L._ptr(verdict)))
    return int(verdict[0])


class PlonkVerifier(_Object):
    """A verifier for one key, made from the key alone (zk_plonk_verifier): no Kzg and no .ptau.  verify() judges m proofs a
    call, each with its own verdict, and everything per proof (the checks, the Keccak transcript, the scalars, the nineteen
    products, the pairing) runs on the device.  ZKHIP_PLONK_VERIFY_CHUNK bounds the memory of a call and changes no
    verdict.  verify_batch() gives the same verdicts from one pairing equation a group of proofs (a random combination with
    scalars the library draws), several times faster when invalid proofs are rare."""
    _name, _destroy, _info, _plan = "PlonkVerifier", "zk_plonk_verifier_destroy", "zk_plonk_verifier_info", L.zk_plonk_verifier_plan
    _drop = ("size",)

    def __init__(self, vkey, device=-1):
        if not isinstance(vkey, PlonkVKey):
            raise TypeError("a PlonkVKey expected (PlonkProver.vkey(), PlonkVKey.from_json or PlonkVKey.from_parts)")
        self._h = C.c_void_p()
        self.vkey, self.log_n, self.n_public, self.device = vkey, vkey.log_n, vkey.n_public, int(device)
        L.check(L.load_library().zk_plonk_verifier_create(C.byref(self._h), C.byref(vkey._c), device))

    def _inputs(self, proofs, publics):
        """-> (proof bytes, public bytes or None, m)"""
        if isinstance(proofs, np.ndarray):
            if proofs.dtype != np.uint8 or proofs.ndim != 2 or proofs.shape[1] != PROOF_BYTES:
                raise ValueError("proofs: a uint8 array of m rows of %d bytes expected" % PROOF_BYTES)
            a = np.ascontiguousarray(proofs).reshape(-1)
        else:
            rows = [p.to_bytes() if isinstance(p, PlonkProof) else PlonkProof(p).to_bytes() for p in proofs]
            a = np.frombuffer(b"".join(rows), dtype=np.uint8)
        m = a.size // PROOF_BYTES
        if self.n_public == 0:
            if publics is not None and any(len(row) for row in publics):
                raise ValueError("publics: the key has no public inputs")
            return a, None, m
        if publics is None:
            raise ValueError("publics: %d rows of n_public = %d values expected" % (m, self.n_public))
        # values that are not below r are the library's to call MALFORMED: they must only fit 32 bytes
        if isinstance(publics, np.ndarray) and publics.dtype == np.uint8:
            pb = np.ascontiguousarray(publics).reshape(-1)
            if pb.size != m * self.n_public * 32:
                raise ValueError("publics: %d bytes, %d rows of n_public = %d values expected" % (pb.size, m, self.n_public))
            return a, pb, m
        publics = list(publics)
        if len(publics) != m:
            raise ValueError("publics: %d rows for %d proofs" % (len(publics), m))
        rows = []
        for i, row in enumerate(publics):
            r = _scalars(row, "publics[%d]" % i, below_r=False)
            if r.size != self.n_public * 32:
                raise ValueError("publics[%d]: %d values, n_public = %d expected" % (i, r.size // 32, self.n_public))
            rows.append(r)
        return a, (np.concatenate(rows) if rows else np.zeros(0, dtype=np.uint8)), m

    def verify(self, proofs, publics=None):
        """numpy uint8 [m]: VERIFY_OK (0) / VERIFY_INVALID (1) / VERIFY_MALFORMED (2) a proof, what plonk_verify gives it
        (zk_plonk_verifier_verify).  proofs: a list of PlonkProof or of 768 bytes each, or a uint8 array (m, 768).  publics: m
        rows of n_public ints (or a uint8 array of m x n_public x 32 bytes); None when the key has no public inputs."""
        a, pb, m = self._inputs(proofs, publics)
        h = self._handle()
        verdict = np.full(m, 255, dtype=np.uint8)
        L.check(L.load_library().zk_plonk_verifier_verify(h, L._ptr(a) if m else None, L._ptr(pb) if pb is not None and m else None, m,
                                                          L._ptr(verdict) if m else None))
        return verdict

    @staticmethod
    def _batch_scalars(scalars, m):
        """-> m x 16 bytes little-endian (uint8 array), or None when the library is to draw them"""
        if scalars is None:
            return None
        if isinstance(scalars, (bytes, bytearray, np.ndarray)):
            sc = L._buf(scalars)
            if sc.size != m * 16:
                raise ValueError("scalars: %d bytes, %d scalars of 16 bytes expected" % (sc.size, m))
            values = [int.from_bytes(sc[i * 16:(i + 1) * 16].tobytes(), "little") for i in range(m)]
        else:
            values = [int(x) for x in scalars]
            if len(values) != m:
                raise ValueError("scalars: %d values for %d proofs" % (len(values), m))
            for i, x in enumerate(values):
                if not 0 <= x < 1 << 128:
                    raise ValueError("scalars[%d] is not below 2^128" % i)
            sc = np.frombuffer(b"".join(x.to_bytes(16, "little") for x in values), dtype=np.uint8)
        for i, x in enumerate(values):
            if x == 0:
                raise ValueError("scalars[%d] is zero" % i)
        return sc

    def verify_batch(self, proofs, publics=None, scalars=None):
        """(numpy uint8 [m] verdicts, report dict): verify()'s verdicts by random combination (zk_plonk_verifier_verify_batch):
        one equation a group of ZKHIP_PLONK_VERIFY_GROUP proofs, the proofs of a failing group one by one.  proofs and
        publics as verify() takes them.  scalars is FOR TESTS ONLY (m ints below 2^128, none zero, or m x 16 bytes
        little-endian); None: the library draws them.  Scalars a prover can predict are unsound.  report: group, groups,
        groups_failed, proofs_rechecked, malformed, launches, chunks."""
        a, pb, m = self._inputs(proofs, publics)
        sc = self._batch_scalars(scalars, m)
        h = self._handle()
        verdict = np.full(m, 255, dtype=np.uint8)
        rep = L.zk_plonk_batch_report()
        rep.size = C.sizeof(rep)
        L.check(L.load_library().zk_plonk_verifier_verify_batch(h, L._ptr(a) if m else None, L._ptr(pb) if pb is not None and m else None, m,
                                                                L._ptr(sc) if sc is not None and m else None, L._ptr(verdict) if m else None, C.byref(rep)))
        return verdict, {name: int(getattr(rep, name)) for name, _ in rep._fields_ if name != "size"}

    def batch_sums(self, proofs, publics, scalars):
        """list of (L, W), a pair of 64 bytes a group in the order the groups are formed (64 zero bytes each for a group with
        no well-formed proof): the two sums of verify_batch()'s equation, no pairing run (zk_plonk_verifier_batch_sums).  For
        tests; scalars must be given."""
        a, pb, m = self._inputs(proofs, publics)
        if scalars is None:
            raise ValueError("scalars: %d values expected" % m)
        sc = self._batch_scalars(scalars, m)
        h = self._handle()
        sums = np.zeros(max(m, 1) * 128, dtype=np.uint8)             # a group holds a proof at least
        n = C.c_uint64(0)
        L.check(L.load_library().zk_plonk_verifier_batch_sums(h, L._ptr(a) if m else None, L._ptr(pb) if pb is not None and m else None, m,
                                                              L._ptr(sc) if m else None, L._ptr(sums), max(m, 1), C.byref(n)))
        raw = sums.tobytes()
        return [(raw[g * 128:g * 128 + 64], raw[g * 128 + 64:g * 128 + 128]) for g in range(n.value)]

    def challenges(self, proofs, publics=None):
        """(m lists of six ints beta gamma alpha zeta v u, numpy uint8 [m] status): the first kernel alone
        (zk_plonk_verifier_challenges).  status 0: well-formed; 2: malformed, and the row is all zero.  For tests of the device
        transcript on inputs that are no valid proofs, and for finding the first difference against another implementation."""
        a, pb, m = self._inputs(proofs, publics)
        h = self._handle()
        ch = np.zeros(m * 6 * 32, dtype=np.uint8)
        status = np.full(m, 255, dtype=np.uint8)
        L.check(L.load_library().zk_plonk_verifier_challenges(h, L._ptr(a) if m else None, L._ptr(pb) if pb is not None and m else None, m,
                                                              L._ptr(ch) if m else None, L._ptr(status) if m else None))
        raw = ch.tobytes()
        return [[int.from_bytes(raw[(i * 6 + j) * 32:(i * 6 + j + 1) * 32], "little") for j in range(6)] for i in range(m)], status

    def info(self):
        """zk_plonk_verifier_info -> dict: log_n, n_public, device_bytes, chunk (ZKHIP_PLONK_VERIFY_CHUNK in effect),
        last_launches, last_chunks"""
        return self._plan_dict()[1]


class PlonkVerifierSet(_Object):
    """A verifier over a key set (zk_plonk_verifier_set): proofs under many keys that share one [tau]G2, proof i under key
    key_of[i], in one call.  The set copies the keys; on its device it keeps one pair of line tables and the generator once,
    and a record and the eight commitments a key.  verify() gives every proof the verdict PlonkVerifier(vkeys[key_of[i]])
    gives it, four launches a chunk whatever the keys; verify_batch() the same verdicts from one pairing equation a group of
    proofs, whatever keys the group holds."""
    _name, _destroy, _info, _plan = "PlonkVerifierSet", "zk_plonk_verifier_set_destroy", "zk_plonk_verifier_set_info", L.zk_plonk_verifier_set_plan
    _drop = ("size",)

    def __init__(self, vkeys, device=-1):
        vkeys = list(vkeys)
        for i, vk in enumerate(vkeys):
            if not isinstance(vk, PlonkVKey):
                raise TypeError("vkeys[%d]: a PlonkVKey expected (PlonkProver.vkey(), PlonkVKey.from_json or PlonkVKey.from_parts)" % i)
        if not 1 <= len(vkeys) <= 65536:
            raise ValueError("vkeys: %d keys, 1 to 65536 expected" % len(vkeys))
        self._h = C.c_void_p()
        self.vkeys, self.n_public, self.device = vkeys, [vk.n_public for vk in vkeys], int(device)
        ptrs = (C.POINTER(L.zk_plonk_vkey) * len(vkeys))(*[C.pointer(vk._c) for vk in vkeys])
        L.check(L.load_library().zk_plonk_verifier_set_create(C.byref(self._h), ptrs, len(vkeys), device))

    def _inputs(self, proofs, key_of, publics):
        """-> (proof bytes, key_of as uint32, the ragged public bytes, m): every shape is checked here, before any call"""
        if isinstance(proofs, np.ndarray):
            if proofs.dtype != np.uint8 or proofs.ndim != 2 or proofs.shape[1] != PROOF_BYTES:
                raise ValueError("proofs: a uint8 array of m rows of %d bytes expected" % PROOF_BYTES)
            a = np.ascontiguousarray(proofs).reshape(-1)
        else:
            rows = [p.to_bytes() if isinstance(p, PlonkProof) else PlonkProof(p).to_bytes() for p in proofs]
            a = np.frombuffer(b"".join(rows), dtype=np.uint8)
        m = a.size // PROOF_BYTES
        keys = np.asarray(key_of if isinstance(key_of, np.ndarray) else [int(k) for k in key_of], dtype=np.int64).reshape(-1)
        if keys.size != m:
            raise ValueError("key_of: %d entries for %d proofs" % (keys.size, m))
        out = np.nonzero((keys < 0) | (keys >= len(self.n_public)))[0]
        if out.size:
            raise ValueError("key_of[%d] = %d, the set holds %d keys" % (out[0], keys[out[0]], len(self.n_public)))
        widths = np.asarray(self.n_public, dtype=np.int64)[keys]
        total = int(widths.sum()) * 32
        if publics is None:
            if total:
                raise ValueError("publics: %d rows expected, proof i's of n_public(key_of[i]) values" % m)
            pb = np.zeros(0, dtype=np.uint8)
        elif isinstance(publics, (bytes, bytearray)) or (isinstance(publics, np.ndarray) and publics.dtype == np.uint8):
            pb = L._buf(publics)
            if pb.size != total:
                raise ValueError("publics: %d bytes, %d expected (%d values of 32 bytes)" % (pb.size, total, total // 32))
        else:
            publics = list(publics)
            if len(publics) != m:
                raise ValueError("publics: %d rows for %d proofs" % (len(publics), m))
            rows = []
            for i, row in enumerate(publics):
                # values that are not below r are the library's to call MALFORMED: they must only fit 32 bytes
                r = _scalars(row, "publics[%d]" % i, below_r=False)
                if r.size != widths[i] * 32:
                    raise ValueError("publics[%d]: %d values, n_public = %d expected for key %d" % (i, r.size // 32, widths[i], keys[i]))
                rows.append(r)
            pb = np.concatenate(rows) if rows else np.zeros(0, dtype=np.uint8)
        return a, keys.astype(np.uint32), np.ascontiguousarray(pb, dtype=np.uint8), m

    def verify(self, proofs, key_of, publics=None):
        """numpy uint8 [m]: what PlonkVerifier(vkeys[key_of[i]]).verify gives proof i (zk_plonk_verifier_set_verify).  proofs: as
        PlonkVerifier.verify takes them; key_of: m indices into the set; publics: m rows, row i of n_public(key_of[i]) ints
        (empty for a key without public inputs), or the flat ragged bytes; None when no proof has public inputs."""
        a, ko, pb, m = self._inputs(proofs, key_of, publics)
        h = self._handle()
        verdict = np.full(m, 255, dtype=np.uint8)
        L.check(L.load_library().zk_plonk_verifier_set_verify(h, L._ptr(a) if m else None, L._ptr(ko) if m else None, L._ptr(pb) if pb.size else None, pb.size, m,
                                                              L._ptr(verdict) if m else None))
        return verdict

    def verify_batch(self, proofs, key_of, publics=None, scalars=None):
        """(numpy uint8 [m] verdicts, report dict): verify()'s verdicts by random combination
        (zk_plonk_verifier_set_verify_batch): one equation a group of ZKHIP_PLONK_VERIFY_GROUP proofs of the key-ordered chunk,
        the proofs of a failing group one by one.  scalars is FOR TESTS ONLY, as PlonkVerifier.verify_batch's, in the caller's
        order; None: the library draws them.  Scalars a prover can predict are unsound, across keys too.  report: group,
        launches, chunks, groups, groups_failed, segments, proofs_rechecked, malformed."""
        a, ko, pb, m = self._inputs(proofs, key_of, publics)
        sc = PlonkVerifier._batch_scalars(scalars, m)
        h = self._handle()
        verdict = np.full(m, 255, dtype=np.uint8)
        rep = L.zk_plonk_set_batch_report()
        rep.size = C.sizeof(rep)
        L.check(L.load_library().zk_plonk_verifier_set_verify_batch(h, L._ptr(a) if m else None, L._ptr(ko) if m else None, L._ptr(pb) if pb.size else None, pb.size,
                                                                    m, L._ptr(sc) if sc is not None and m else None, L._ptr(verdict) if m else None, C.byref(rep)))
        return verdict, {name: int(getattr(rep, name)) for name, _ in rep._fields_ if name != "size"}

    def batch_sums(self, proofs, key_of, publics, scalars):
        """list of (L, W), a pair of 64 bytes a group in the order the groups are formed (64 zero bytes each for a group with
        no well-formed proof): the two sums of verify_batch()'s equation, no pairing run (zk_plonk_verifier_set_batch_sums).
        For tests; scalars must be given."""
        a, ko, pb, m = self._inputs(proofs, key_of, publics)
        if scalars is None:
            raise ValueError("scalars: %d values expected" % m)
        sc = PlonkVerifier._batch_scalars(scalars, m)
        h = self._handle()
        sums = np.zeros(max(m, 1) * 128, dtype=np.uint8)             # a group holds a proof at least
        n = C.c_uint64(0)
        L.check(L.load_library().zk_plonk_verifier_set_batch_sums(h, L._ptr(a) if m else None, L._ptr(ko) if m else None, L._ptr(pb) if pb.size else None, pb.size, m,
                                                                  L._ptr(sc) if m else None, L._ptr(sums), max(m, 1), C.byref(n)))
        raw = sums.tobytes()
        return [(raw[g * 128:g * 128 + 64], raw[g * 128 + 64:g * 128 + 128]) for g in range(n.value)]

    def info(self):
        """zk_plonk_verifier_set_info -> dict: n_keys, max_n_public, device_bytes, chunk (ZKHIP_PLONK_VERIFY_CHUNK in effect),
        last_launches, last_chunks"""
        return self._plan_dict()[1]
