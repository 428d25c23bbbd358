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


class PlonkCircuit:
    """What does not change from proof to proof of a three-column PLONK circuit, on a device (zk_plonk_circuit): the eight
    polynomials extended to the coset shift * (4n-th roots of unity).  basis "monomial": coefficients; "lagrange": values at
    w^j, what plonk_permutation_product takes.  It is NOT checked that 1, k1, k2 name disjoint cosets."""

    def __init__(self, ql, qr, qm, qo, qc, s1, s2, s3, k1, k2, basis="monomial", shift=None, device=-1):
        if basis not in _BASES:
            raise ValueError("basis %r is unknown: 'monomial' or 'lagrange'" % (basis,))
        vecs = [_scalars(v, name) for name, v in zip(_CIRCUIT, (ql, qr, qm, qo, qc, s1, s2, s3))]
        n = vecs[0].size // 32
        for name, v in zip(_CIRCUIT, vecs):
            if v.size != n * 32:
                raise ValueError("%s has %d rows, ql has %d: the eight circuit vectors must have one length" % (name, v.size // 32, n))
        if n < 1 or n & (n - 1):
            raise ValueError("n = %d is not a power of two" % n)
        log_n = n.bit_length() - 1
        if not MIN_LOG_N <= log_n <= MAX_LOG_N:
            raise ValueError("log_n %d is outside %d .. %d" % (log_n, MIN_LOG_N, MAX_LOG_N))
        kb1, kb2 = _one(k1, "k1"), _one(k2, "k2")
        g = _shift(shift)
        if g is not None and pow(int.from_bytes(g.tobytes(), "little") % R_MOD, 4 * n, R_MOD) == 1:
            raise ValueError("shift^(4n) is 1: Z_H vanishes on the coset")
        self.n, self.log_n, self.device = n, log_n, int(device)
        self._h = C.c_void_p()
        v = L.zk_plonk_circuit_view()
        v.log_n, v.basis = log_n, _BASES[basis]
        for name, a in zip(_CIRCUIT, vecs):
            setattr(v, name, a.ctypes.data)
        C.memmove(v.k1, kb1.ctypes.data, 32)
        C.memmove(v.k2, kb2.ctypes.data, 32)
        v.shift = g.ctypes.data if g is not None else None
        L.check(L.load_library().zk_plonk_circuit_create(C.byref(self._h), C.byref(v), device))

    def _handle(self):
        if not self._h:
            raise L.ZkHipError("the PlonkCircuit object is closed")
        return self._h

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
        plan = L.zk_plonk_circuit_plan()
        plan.size = C.sizeof(plan)
        L.check(L.load_library().zk_plonk_circuit_info(self._handle(), C.byref(plan)))
        return {name: int(getattr(plan, name)) for name, _ in plan._fields_ if name != "size"}

    def close(self):
        if self._h:
            L.load_library().zk_plonk_circuit_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
