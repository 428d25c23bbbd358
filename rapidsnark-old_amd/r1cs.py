"""circom's binary R1CS (.r1cs): header reader, constraint reader and writer, and the GPU witness checker R1cs.

Same container as .zkey / .wtns (binfile.py): magic "r1cs", version 1, sections in any order.
  1 header      u32 n8 (= 32), prime (n8 bytes LE), u32 nWires, nPubOut, nPubIn, nPrvIn, u64 nLabels, u32 nConstraints
  2 constraints per constraint the linear combinations A, B, C; each a u32 term count and that many
                (u32 wire id, n8-byte coefficient LE, standard form) pairs
  3 wire -> label map (u64 per wire; not read)
  4, 5          custom gates (PLONK): refused, Groth16 cannot use them
Wire 0 is the constant 1, wires 1 .. nPubOut + nPubIn are the public signals (the zkey's nPublic).

The reference reads no .r1cs (its prover trusts the witness); the counterpart is snarkjs `wtns check`."""
import collections
import ctypes as C
import struct

import numpy as np

from . import lib as L
from .binfile import container_parts, open_existing
from .synth import R_MOD as BN254_R

TERM_BYTES = 4 + 32
NONE = 0xFFFFFFFF


class R1csHeader:
    __slots__ = ("n8", "prime", "nWires", "nPubOut", "nPubIn", "nPrvIn", "nLabels", "nConstraints")

    @property
    def nPublic(self):
        return self.nPubOut + self.nPubIn


def load_r1cs_header(f) -> R1csHeader:
    """Section 1 of an opened .r1cs (binfile.BinFile); refuses other curves and custom gates."""
    for sec in (4, 5):
        if sec in f.sections:
            raise ValueError("r1cs custom gates (section %d) are not supported: Groth16 cannot use them" % sec)
    h = R1csHeader()
    f.startReadSection(1)
    h.n8 = f.readU32LE()
    if h.n8 != 32:
        raise ValueError("r1cs: only 256-bit fields are supported")
    h.prime = int.from_bytes(f.read(h.n8), "little")
    if h.prime != BN254_R:
        raise ValueError("r1cs curve not supported")
    h.nWires, h.nPubOut, h.nPubIn, h.nPrvIn = (f.readU32LE() for _ in range(4))
    h.nLabels = f.readU64LE()
    h.nConstraints = f.readU32LE()
    f.endReadSection()
    return h


def open_r1cs(path_or_bytes):
    """-> (header, constraints section as a memoryview) of a .r1cs given as path or bytes.  Checks the container only:
    wire ids and coefficients are range-checked on the device (zk_r1cs_create)."""
    if isinstance(path_or_bytes, str):
        with open(path_or_bytes, "rb") as fh:
            path_or_bytes = fh.read()
    data = bytes(path_or_bytes)
    try:
        f = open_existing(data, "r1cs", 1)
    except struct.error:                 # the section table itself is cut off
        raise ValueError("r1cs file is truncated") from None
    end = max((pos + size for lst in f.sections.values() for pos, size in lst), default=12)
    if end > len(data):
        raise ValueError("r1cs file is truncated")
    if 1 not in f.sections or 2 not in f.sections:
        raise ValueError("r1cs has no %s section" % ("header" if 1 not in f.sections else "constraints"))
    try:
        h = load_r1cs_header(f)
    except struct.error:
        raise ValueError("r1cs header section is truncated") from None
    return h, f.getSectionData(2)


def read_constraints(data):
    """Decode section 2 on the host (tests, small circuits): -> (header, [(A, B, C)]), each linear combination a list of
    (wire, value) pairs in file order."""
    h, sec = open_r1cs(data)
    out, pos = [], 0
    for _ in range(h.nConstraints):
        lcs = []
        for _m in range(3):
            (cnt,) = struct.unpack_from("<I", sec, pos)
            pos += 4
            lc = []
            for _t in range(cnt):
                (wire,) = struct.unpack_from("<I", sec, pos)
                lc.append((wire, int.from_bytes(sec[pos + 4:pos + 36], "little")))
                pos += TERM_BYTES
            lcs.append(lc)
        out.append(tuple(lcs))
    if pos != len(sec):
        raise ValueError("r1cs constraints section size mismatch")
    return h, out


def _coef_rows(coefs, nnz):
    """coefficients -> (nnz, 32) uint8, standard form LE: a uint8 array (nnz x 32 or flat) or a sequence of ints < 2^256."""
    if isinstance(coefs, np.ndarray) and coefs.dtype == np.uint8:
        a = np.ascontiguousarray(coefs).reshape(-1, 32)
    else:
        a = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in coefs), dtype=np.uint8).reshape(-1, 32)
    if a.shape[0] != nnz:
        raise ValueError("coefficient count %d != term count %d" % (a.shape[0], nnz))
    return a


def csr_from_rows(rows):
    """[[(wire, value), ...] per row] (or dicts {wire: value}) -> (rowptr, wires, coefs) CSR arrays for write_r1cs."""
    rows = [list(r.items()) if isinstance(r, dict) else list(r) for r in rows]
    rowptr = np.zeros(len(rows) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    wires = np.array([t[0] for r in rows for t in r], dtype=np.uint32)
    coefs = [int(t[1]) for r in rows for t in r]
    return rowptr, wires, coefs


def write_r1cs(A, B, C, n_wires, n_pub_out=0, n_pub_in=0, n_prv_in=None, n_labels=None, prime=BN254_R):
    """-> the bytes of a .r1cs.  A, B, C: (rowptr, wire ids, coefficients) per matrix, one row per constraint; rowptr has
    nConstraints + 1 entries, coefficients as for _coef_rows.  Values are written as given (no reduction, no range check:
    tests write malformed files on purpose).  Vectorised: 2^20 constraints take a few seconds."""
    mats = []
    for rp, wires, coefs in (A, B, C):
        rp = np.asarray(rp, dtype=np.int64)
        wires = np.asarray(wires, dtype=np.uint32).reshape(-1)
        nnz = int(rp[-1]) if rp.size else 0
        if wires.size != nnz:
            raise ValueError("wire id count %d != term count %d" % (wires.size, nnz))
        mats.append((rp, wires, _coef_rows(coefs, nnz)))
    m = mats[0][0].size - 1
    if any(x[0].size - 1 != m for x in mats):
        raise ValueError("A, B and C need the same number of rows")
    counts = np.stack([np.diff(x[0]) for x in mats], axis=1).reshape(-1)           # (constraint, matrix) order
    lc_off = np.zeros(counts.size + 1, dtype=np.int64)                              # in 4-byte words: every field is a multiple of 4 bytes
    np.cumsum(1 + 9 * counts, out=lc_off[1:])
    sec2 = np.zeros(int(lc_off[-1]), dtype="<u4")
    sec2[lc_off[:-1]] = counts
    for k, (rp, wires, coefs) in enumerate(mats):
        nnz = wires.size
        if not nnz:
            continue
        row_len = np.diff(rp)
        start = lc_off[:-1].reshape(-1, 3)[:, k] + 1                               # first term word of each row
        rank = np.arange(nnz, dtype=np.int64) - np.repeat(rp[:-1], row_len)
        at = np.repeat(start, row_len) + 9 * rank
        sec2[at] = wires
        sec2[at[:, None] + np.arange(1, 9)] = coefs.view("<u4").reshape(nnz, 8)
    if n_prv_in is None:
        n_prv_in = max(0, n_wires - 1 - n_pub_out - n_pub_in)
    if n_labels is None:
        n_labels = n_wires
    sec1 = (struct.pack("<I", 32) + int(prime).to_bytes(32, "little")
            + struct.pack("<IIIIQI", n_wires, n_pub_out, n_pub_in, n_prv_in, n_labels, m))
    sec3 = np.arange(n_wires, dtype="<u8").tobytes()
    return b"".join(container_parts(b"r1cs", 1, [(1, sec1), (2, sec2), (3, sec3)]))


def write_r1cs_rows(A, B, C, n_wires, n_public, **kw):
    """write_r1cs over row lists ([(wire, value), ...] or dicts per constraint); the public signals are written as public
    inputs (nPubOut = 0)."""
    return write_r1cs(csr_from_rows(A), csr_from_rows(B), csr_from_rows(C), n_wires, 0, n_public, **kw)


# ---------------------------------------------------------------- the GPU checker (include/zkhip.h, section "R1CS")
R1csReport = collections.namedtuple("R1csReport", "ok failed first_failed a b c one_ok first_unreduced")
R1csReport.__doc__ = """zk_r1cs_report: failed = constraints with A.w * B.w != C.w; first_failed / first_unreduced = lowest index or
None; a, b, c = A.w, B.w, C.w of first_failed (ints, None when nothing fails); one_ok = (w[0] == 1); ok = all of it holds."""


def _report(rep):
    none = lambda v: None if v == NONE else int(v)
    ff = none(rep.first_failed)
    val = lambda x: int.from_bytes(bytes(x), "little") if ff is not None else None
    ok = rep.failed == 0 and bool(rep.one_ok) and rep.first_unreduced == NONE
    return R1csReport(ok, int(rep.failed), ff, val(rep.a), val(rep.b), val(rep.c), bool(rep.one_ok), none(rep.first_unreduced))


class R1cs:
    """A circuit's R1CS resident on one GPU: check(wtns) tests a witness against every constraint, match_zkey(zkey) tests
    that a .zkey was made from this circuit (A and B as linear maps; C is not in a zkey).  The file is parsed on the host
    before the device is touched; without a GPU the constructor raises ZkHipError."""

    def __init__(self, path_or_bytes, device=-1):
        self._lib = L.load_library()
        self.header, sec = open_r1cs(path_or_bytes)
        h = self.header
        keep = np.frombuffer(sec, dtype=np.uint8)
        v = L.zk_r1cs_view(h.nWires, h.nPubOut, h.nPubIn, h.nPrvIn, h.nConstraints, keep.ctypes.data if keep.size else None, keep.size)
        self._h = C.c_void_p()
        L.check(self._lib.zk_r1cs_create(C.byref(self._h), C.byref(v), device))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.zk_r1cs_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def _values(self, wtns):
        """.wtns path / bytes -> (numpy uint8 view of the values, nVars); a numpy uint8 array (e.g. a PinnedBuffer's .array) or
        a PinnedBuffer holds the values themselves."""
        if isinstance(wtns, L.PinnedBuffer):
            wtns = wtns.array
        if isinstance(wtns, np.ndarray):
            a = np.ascontiguousarray(wtns).view(np.uint8).reshape(-1)
            return a, a.size // 32
        f = open_existing(wtns, "wtns", 2)
        f.startReadSection(1)
        n8 = f.readU32LE()
        prime = int.from_bytes(f.read(n8), "little")
        n_vars = f.readU32LE()
        f.endReadSection()
        if n8 != 32 or prime != BN254_R:
            raise ValueError("different wtns curve")
        a = np.frombuffer(f.getSectionData(2), dtype=np.uint8)
        if a.size < min(n_vars, self.header.nWires) * 32:
            raise ValueError("wtns values section is shorter than nVars x 32 bytes")
        return a, n_vars

    def check(self, wtns):
        """Witness in host memory (.wtns path or bytes, raw values as a numpy uint8 array, or a PinnedBuffer) -> R1csReport."""
        a, n_vars = self._values(wtns)
        rep = L.zk_r1cs_report()
        rep.size = C.sizeof(L.zk_r1cs_report)
        L.check(self._lib.zk_r1cs_check(self._h, C.c_void_p(a.ctypes.data) if a.size else None, n_vars, C.byref(rep)))
        return _report(rep)

    def check_dev(self, d_wtns_ptr, n_vars):
        """Witness already in HBM on the checker's device (nVars x 32 B, standard form) -> R1csReport."""
        rep = L.zk_r1cs_report()
        rep.size = C.sizeof(L.zk_r1cs_report)
        L.check(self._lib.zk_r1cs_check_dev(self._h, C.c_void_p(d_wtns_ptr), n_vars, C.byref(rep)))
        return _report(rep)

    def match_zkey(self, zkey):
        """-> (rows_differing, first_row or None): does the .zkey (path or bytes) hold this circuit's A and B?"""
        from .prover import _zkey_view
        keep = []
        _, v = _zkey_view(zkey, keep)
        rows, first = C.c_uint64(0), C.c_uint32(0)
        L.check(self._lib.zk_r1cs_match_zkey(self._h, C.byref(v), C.byref(rows), C.byref(first)))
        return int(rows.value), (None if first.value == NONE else int(first.value))
