"""KZG polynomial commitments over a .ptau on the GPU (include/zkhip.h, section "KZG polynomial commitments over a .ptau"):
commit, open, verify.  The arithmetic is libzkhip's; this module checks shapes and ranges before any library call and
turns Python values into the byte layouts the library takes: scalars 32 bytes little-endian in standard form, points
affine Montgomery (x | y, 64 bytes, all-zero = infinity)."""
import ctypes as C

import numpy as np

from . import lib as L
from .zkey import R_MOD

VERIFY_OK, VERIFY_INVALID, VERIFY_MALFORMED = 0, 1, 2
_BASES = {"monomial": L.ZK_KZG_MONOMIAL, "lagrange": L.ZK_KZG_LAGRANGE}


def _scalars(values, what, below_r=True):
    """a sequence of ints, or a uint8 array / bytes of 32-byte rows -> contiguous numpy uint8 [n * 32].  Ints must lie in
    0 .. r - 1; rows are passed as they are (the library names a row that is not below r)."""
    if isinstance(values, (bytes, bytearray, memoryview)) or (isinstance(values, np.ndarray) and values.dtype == np.uint8):
        a = L._buf(values)
        if a.size % 32:
            raise ValueError("%s: rows of 32 bytes expected, got %d bytes" % (what, a.size))
        return a
    out = bytearray()
    for i, v in enumerate(values):
        x = int(v)
        if not 0 <= x < (R_MOD if below_r else 1 << 256):
            raise ValueError("%s: value %d is not in 0 .. r - 1" % (what, i))
        out += x.to_bytes(32, "little")
    return np.frombuffer(bytes(out), dtype=np.uint8)


def _polys(coeffs, what):
    """one polynomial (ints, or a 1-d byte array) or several (a sequence of int sequences, or a 2-d uint8 array of m rows
    of n * 32 bytes) -> (bytes, n, m)"""
    if isinstance(coeffs, np.ndarray) and coeffs.dtype == np.uint8 and coeffs.ndim >= 2:
        m = coeffs.shape[0]
        a = _scalars(np.ascontiguousarray(coeffs), what)
        if m == 0 or a.size == 0:
            raise ValueError("%s: at least one polynomial of at least one coefficient expected" % what)
        return a, a.size // 32 // m, m
    if not isinstance(coeffs, (bytes, bytearray, memoryview, np.ndarray)) and len(coeffs) and not isinstance(coeffs[0], (int, np.integer)):
        rows = [_scalars(r, what) for r in coeffs]
        if any(r.size != rows[0].size for r in rows):
            raise ValueError("%s: the polynomials must have one length" % what)
        if rows[0].size == 0:
            raise ValueError("%s: at least one coefficient expected" % what)
        return np.concatenate(rows), rows[0].size // 32, len(rows)
    a = _scalars(coeffs, what)
    if a.size == 0:
        raise ValueError("%s: at least one coefficient expected" % what)
    return a, a.size // 32, 1


def _points(b, what):
    a = L._buf(b)
    if a.size % 64:
        raise ValueError("%s: points of 64 bytes expected, got %d bytes" % (what, a.size))
    return a


def fr_poly_divide(coeffs, z, device=-1):
    """(q, y) with q = (p - p(z)) / (X - z) and y = p(z) for p = sum coeffs[i] X^i (zk_fr_poly_divide): q a numpy uint8 array
    of (n - 1) * 32 bytes, y an int."""
    a = _scalars(coeffs, "coeffs")
    if a.size == 0:
        raise ValueError("coeffs: at least one coefficient expected")
    zb = _scalars([z] if isinstance(z, (int, np.integer)) else z, "z")
    if zb.size != 32:
        raise ValueError("z: one value expected")
    n = a.size // 32
    q = np.zeros((n - 1) * 32, dtype=np.uint8)
    y = np.zeros(32, dtype=np.uint8)
    L.check(L.load_library().zk_fr_poly_divide(L._ptr(q) if n > 1 else None, L._ptr(y), L._ptr(a), n, L._ptr(zb), device))
    return q, int.from_bytes(y.tobytes(), "little")


class Kzg:
    """The reference string of a .ptau on a device (zk_kzg).  It is NOT checked that the file's points are the powers of
    one tau: ptau_check does that."""

    def __init__(self, ptau, max_coeffs=None, lagrange_log_n=None, device=-1):
        from .ptau import PtauFile
        if not isinstance(ptau, PtauFile):
            raise TypeError("a PtauFile expected (Kzg.from_ptau takes a path)")
        full = (2 << ptau.power) - 1
        max_coeffs = full if max_coeffs is None else int(max_coeffs)
        if not 1 <= max_coeffs <= full or max_coeffs >= 1 << 31:
            raise ValueError("max_coeffs %d is outside 1 .. %d (power %d)" % (max_coeffs, min(full, (1 << 31) - 1), ptau.power))
        if lagrange_log_n is not None:
            lagrange_log_n = int(lagrange_log_n)
            if not 0 <= lagrange_log_n <= ptau.power:
                raise ValueError("lagrange_log_n %d is outside 0 .. %d (the file's power)" % (lagrange_log_n, ptau.power))
            if 12 not in ptau.sections:
                raise ValueError("a Lagrange level needs a prepared file (ptau section 12 is absent)")
        self.max_coeffs, self.lagrange_log_n, self.power, self.device = max_coeffs, lagrange_log_n, ptau.power, int(device)
        self._h = C.c_void_p()
        v = ptau.kzg_view()
        level = L.ZK_KZG_NO_LAGRANGE if lagrange_log_n is None else lagrange_log_n
        L.check(L.load_library().zk_kzg_create(C.byref(self._h), C.byref(v), max_coeffs, level, device))

    @classmethod
    def from_ptau(cls, path_or_ptau, max_coeffs=None, lagrange_log_n=None, device=-1):
        from .ptau import PtauFile
        if isinstance(path_or_ptau, PtauFile):
            return cls(path_or_ptau, max_coeffs, lagrange_log_n, device)
        f = PtauFile(path_or_ptau)
        try:
            return cls(f, max_coeffs, lagrange_log_n, device)      # the object keeps nothing of the file
        finally:
            f.close()

    def _handle(self):
        if not self._h:
            raise L.ZkHipError("the Kzg object is closed")
        return self._h

    def commit(self, coeffs, basis="monomial"):
        """-> numpy uint8 [m * 64]: the commitments of m polynomials (one when coeffs is a flat vector)."""
        if basis not in _BASES:
            raise ValueError("basis %r is unknown: 'monomial' or 'lagrange'" % (basis,))
        a, n, m = _polys(coeffs, "coeffs")
        if basis == "lagrange":
            if self.lagrange_log_n is None:
                raise ValueError("the object holds no Lagrange level")
            if n != 1 << self.lagrange_log_n:
                raise ValueError("n = %d, the Lagrange level holds %d points" % (n, 1 << self.lagrange_log_n))
        elif n > self.max_coeffs:
            raise ValueError("n = %d exceeds max_coeffs = %d" % (n, self.max_coeffs))
        h = self._handle()
        out = np.zeros(m * 64, dtype=np.uint8)
        L.check(L.load_library().zk_kzg_commit(h, L._ptr(out), L._ptr(a), n, m, _BASES[basis]))
        return out

    def open(self, coeffs, zs):
        """-> (ys, proofs): a list of m ints p_k(z_k) and numpy uint8 [m * 64], the commitments of (p_k - y_k) / (X - z_k)."""
        a, n, m = _polys(coeffs, "coeffs")
        zb = _scalars([zs] if isinstance(zs, (int, np.integer)) else zs, "zs")
        if zb.size != m * 32:
            raise ValueError("zs: %d values for %d polynomials" % (zb.size // 32, m))
        if n > self.max_coeffs:
            raise ValueError("n = %d exceeds max_coeffs = %d" % (n, self.max_coeffs))
        h = self._handle()
        ys = np.zeros(m * 32, dtype=np.uint8)
        proofs = np.zeros(m * 64, dtype=np.uint8)
        L.check(L.load_library().zk_kzg_open(h, L._ptr(ys), L._ptr(proofs), L._ptr(a), n, m, L._ptr(zb)))
        yb = ys.tobytes()
        return [int.from_bytes(yb[i * 32:(i + 1) * 32], "little") for i in range(m)], proofs

    def _openings(self, commitments, zs, ys, proofs):
        c, p = _points(commitments, "commitments"), _points(proofs, "proofs")
        # values that are not below r are the device's to refuse (MALFORMED): they must only fit 32 bytes
        z, y = _scalars(zs, "zs", below_r=False), _scalars(ys, "ys", below_r=False)
        m = c.size // 64
        if p.size != m * 64 or z.size != m * 32 or y.size != m * 32:
            raise ValueError("%d commitments, %d zs, %d ys, %d proofs: one of each per opening expected" % (m, z.size // 32, y.size // 32, p.size // 64))
        return c, z, y, p, m

    def verify(self, commitments, zs, ys, proofs):
        """-> numpy uint8 [m]: VERIFY_OK / VERIFY_INVALID / VERIFY_MALFORMED per opening."""
        c, z, y, p, m = self._openings(commitments, zs, ys, proofs)
        h = self._handle()
        verdict = np.full(m, 255, dtype=np.uint8)
        if m:
            L.check(L.load_library().zk_kzg_verify(h, L._ptr(c), L._ptr(z), L._ptr(y), L._ptr(p), m, L._ptr(verdict)))
        return verdict

    def verify_batch(self, commitments, zs, ys, proofs, scalars=None):
        """-> ONE verdict for the batch, by random linear combination.  scalars is FOR TESTS ONLY (m ints in 1 .. 2^128 - 1 or
        m x 16 bytes): scalars that are known before the openings are fixed are unsound."""
        c, z, y, p, m = self._openings(commitments, zs, ys, proofs)
        sc = None
        if scalars is not None:
            if isinstance(scalars, (bytes, bytearray, memoryview, np.ndarray)):
                sc = L._buf(scalars)
            else:
                vals = [int(v) for v in scalars]
                if any(not 0 < v < 1 << 128 for v in vals):
                    raise ValueError("scalars: values in 1 .. 2^128 - 1 expected")
                sc = np.frombuffer(b"".join(v.to_bytes(16, "little") for v in vals), dtype=np.uint8)
            if sc.size != m * 16:
                raise ValueError("scalars: %d x 16 bytes expected, got %d bytes" % (m, sc.size))
        h = self._handle()
        verdict = np.full(1, 255, dtype=np.uint8)
        L.check(L.load_library().zk_kzg_verify_batch(h, L._ptr(c) if m else None, L._ptr(z) if m else None, L._ptr(y) if m else None,
                                                     L._ptr(p) if m else None, m, L._ptr(sc) if sc is not None and m else None, L._ptr(verdict)))
        return int(verdict[0])

    def info(self):
        """zk_kzg_info -> dict"""
        plan = L.zk_kzg_plan()
        plan.size = C.sizeof(plan)
        L.check(L.load_library().zk_kzg_info(self._handle(), C.byref(plan)))
        d = {name: int(getattr(plan, name)) for name, _ in plan._fields_ if name != "size"}
        d["lagrange_log_n"] = None if d["lagrange_log_n"] == L.ZK_KZG_NO_LAGRANGE else d["lagrange_log_n"]
        return d

    def close(self):
        if self._h:
            L.load_library().zk_kzg_destroy(self._h)
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
