"""Running products over Fr on the GPU (include/zkhip.h, section "Grand products and batch inversion over Fr"): batch
inversion, prefix products, the grand product of ratios and the accumulator of PLONK's permutation argument.  The
arithmetic is libzkhip's; this module checks shapes and ranges before any library call and turns Python values into the
byte layout the library takes: scalars 32 bytes little-endian in standard form."""
import ctypes as C

import numpy as np

from . import lib as L
from .kzg import _scalars

MAX_COLS, MAX_LOG_N = 8, 28


def _int(b):
    return int.from_bytes(b.tobytes(), "little")


def _one(value, what):
    b = _scalars([value] if isinstance(value, (int, np.integer)) else value, what)
    if b.size != 32:
        raise ValueError("%s: one value expected" % what)
    return b


def _columns(cols, what):
    """several columns (a sequence of int sequences or of byte rows, or a 2-d uint8 array of rows of n * 32 bytes)
    -> (bytes, number of columns, n)"""
    if isinstance(cols, np.ndarray) and cols.dtype == np.uint8:
        if cols.ndim != 2:
            raise ValueError("%s: a 2-d array of one row of n * 32 bytes per column expected" % what)
        m = cols.shape[0]
        a = _scalars(np.ascontiguousarray(cols), what)
        if m and cols.shape[1] % 32:
            raise ValueError("%s: rows of 32 bytes expected, got %d bytes a column" % (what, cols.shape[1]))
        return a, m, (a.size // 32 // m if m else 0)
    if isinstance(cols, (bytes, bytearray, memoryview)) or (len(cols) and isinstance(cols[0], (int, np.integer))):
        raise ValueError("%s: a list of columns expected" % what)
    rows = [_scalars(c, "%s[%d]" % (what, j)) for j, c in enumerate(cols)]
    if any(r.size != rows[0].size for r in rows):
        raise ValueError("%s: the columns must have one length" % what)
    if not rows:
        return np.zeros(0, dtype=np.uint8), 0, 0
    return np.concatenate(rows), len(rows), rows[0].size // 32


def fr_batch_inverse(values, device=-1):
    """(inverses, zeros): inverses a numpy uint8 array of n * 32 bytes with values[i]^-1 (zero for a zero), zeros how many
    values were zero (zk_fr_batch_inverse)."""
    a = _scalars(values, "values")
    n = a.size // 32
    out = np.zeros(n * 32, dtype=np.uint8)
    zeros = C.c_uint64(0)
    if n:
        L.check(L.load_library().zk_fr_batch_inverse(L._ptr(out), L._ptr(a), n, C.byref(zeros), device))
    return out, int(zeros.value)


def fr_prefix_product(values, exclusive=False, device=-1):
    """numpy uint8 [n * 32]: out[i] = values[0] .. values[i], or 1, values[0], .., values[0] .. values[n-2] when exclusive
    (zk_fr_prefix_product)."""
    a = _scalars(values, "values")
    n = a.size // 32
    out = np.zeros(n * 32, dtype=np.uint8)
    if n:
        L.check(L.load_library().zk_fr_prefix_product(L._ptr(out), L._ptr(a), n, L.ZK_SCAN_EXCLUSIVE if exclusive else 0, device))
    return out


def fr_grand_product(num, den, device=-1):
    """(z, last): z a numpy uint8 array of n * 32 bytes with z[0] = 1 and z[i] = prod_(j<i) num[j] / den[j], last the int
    prod_(j<n) num[j] / den[j] (zk_fr_grand_product).  A zero denominator is the library's error, naming the lowest."""
    a, b = _scalars(num, "num"), _scalars(den, "den")
    if a.size != b.size:
        raise ValueError("%d numerators, %d denominators: one of each per element expected" % (a.size // 32, b.size // 32))
    n = a.size // 32
    z = np.zeros(n * 32, dtype=np.uint8)
    last = np.zeros(32, dtype=np.uint8)
    if not n:
        return z, 1
    L.check(L.load_library().zk_fr_grand_product(L._ptr(z), L._ptr(last), L._ptr(a), L._ptr(b), n, device))
    return z, _int(last)


def plonk_permutation_product(wires, sigmas, shifts, beta, gamma, device=-1):
    """(z, last) of PLONK's permutation argument over cols columns of n = 2^log_n rows (zk_plonk_permutation_product):
    z[0] = 1, z[i+1] = z[i] prod_j (wires[j][i] + beta shifts[j] w^i + gamma) / (wires[j][i] + beta sigmas[j][i] + gamma),
    last = z[n].  wires, sigmas: a list of cols columns or a 2-d uint8 array [cols, n * 32]; sigmas holds the VALUES
    sigma_j(w^i).  It is NOT checked that sigmas is a permutation."""
    w, cols, n = _columns(wires, "wires")
    s, scols, sn = _columns(sigmas, "sigmas")
    if (cols, n) != (scols, sn):
        raise ValueError("wires is %d x %d, sigmas is %d x %d: one shape expected" % (cols, n, scols, sn))
    if not 1 <= cols <= MAX_COLS:
        raise ValueError("cols %d is outside 1 .. %d" % (cols, MAX_COLS))
    if n < 1 or n & (n - 1) or n > 1 << MAX_LOG_N:
        raise ValueError("n = %d is not a power of two from 1 to 2^%d" % (n, MAX_LOG_N))
    sh = _scalars(shifts, "shifts")
    if sh.size != cols * 32:
        raise ValueError("shifts: %d values for %d columns" % (sh.size // 32, cols))
    bb, gb = _one(beta, "beta"), _one(gamma, "gamma")
    z = np.zeros(n * 32, dtype=np.uint8)
    last = np.zeros(32, dtype=np.uint8)
    L.check(L.load_library().zk_plonk_permutation_product(L._ptr(z), L._ptr(last), L._ptr(w), L._ptr(s), cols, n.bit_length() - 1, L._ptr(sh),
                                                           L._ptr(bb), L._ptr(gb), device))
    return z, _int(last)
