"""Is this .zkey the key of this circuit over this Powers of Tau file (include/zkhip.h, section "Is this .zkey the key of
this circuit"; no counterpart in the reference): the arithmetic half of snarkjs `zkey verify` on the GPU.

zkey_verify(r1cs, ptau, zkey) maps the three files, hands them to zk_zkey_verify and returns a ZkeyVerifyReport.  Checked:
every point of the key's sections 2, 3 and 5 to 9; alpha1, beta1, beta2 against the .ptau; gamma2 = the G2 generator;
delta1 and delta2 the same delta; section 4 against the circuit; sections 3 and 5 to 9 against the circuit and the
Lagrange levels of the .ptau.  NOT checked: section 10, the contribution transcript."""
import ctypes as C
import mmap
import struct

import numpy as np

from . import lib as L
from .binfile import BinFile
from .ptau import _open_ptau, _r1cs_view
from .synth import Q_MOD, R_MOD
from .zkey import _section_sizes, load_zkey_header

ITEMS = ("alpha1", "beta1", "beta2", "gamma2", "delta", "coefs", "A", "B1", "B2", "IC", "C", "H")       # ZK_ZV_*
SHAPES = ("nVars", "nPublic", "domain", "ptau_unprepared", "ptau_power")                                # ZK_ZV_SHAPE_*


class ZkeyVerifyReport:
    """What zk_zkey_verify found.  ok; verdict (0 OK, 1 INVALID, 2 MALFORMED); failed / not_checked: sets of the item names
    of ITEMS; shape_failed: set of the names of SHAPES (the files do not fit each other: nothing else was evaluated); for a
    malformed point bad_section, bad_index and bad_kind (1 coordinate >= q, 2 off the curve, 3 not in the subgroup, 4
    infinity); coef_rows_differing and coef_first_row (None: none); delta_is_generator: a phase-2 starting key, not safe to
    prove with.  The contribution transcript is never checked."""

    def __init__(self, rep):
        self.verdict = int(rep.verdict)
        self.ok = self.verdict == 0
        self.failed = {name for i, name in enumerate(ITEMS) if rep.failed >> i & 1}
        self.not_checked = {name for i, name in enumerate(ITEMS) if rep.not_checked >> i & 1}
        self.shape_failed = {name for i, name in enumerate(SHAPES) if rep.shape_failed >> i & 1}
        self.bad_section, self.bad_index, self.bad_kind = int(rep.bad_section), int(rep.bad_index), int(rep.bad_kind)
        self.coef_rows_differing = int(rep.coef_rows_differing)
        self.coef_first_row = None if rep.coef_first_row == 0xFFFFFFFF else int(rep.coef_first_row)
        self.delta_is_generator = bool(rep.delta_is_generator)

    def __repr__(self):
        return "ZkeyVerifyReport(verdict=%d, failed=%r, not_checked=%r, shape_failed=%r, bad=(%d, %d, %d), delta_is_generator=%r)" % (
            self.verdict, sorted(self.failed), sorted(self.not_checked), sorted(self.shape_failed), self.bad_section, self.bad_index,
            self.bad_kind, self.delta_is_generator)


class _ZkeyFile:
    """A .zkey (path: mapped read-only; or bytes) as a zk_zkey_verify_view.  Raises ValueError on a file that is not a
    Groth16 BN254 key or whose sections 3 to 9 are missing or truncated."""

    def __init__(self, path_or_bytes):
        if isinstance(path_or_bytes, str):
            with open(path_or_bytes, "rb") as fh:
                if fh.seek(0, 2) < 12:
                    raise ValueError("zkey file is truncated")
                self._map = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
            data = self._map
        else:
            self._map = None
            data = bytes(path_or_bytes)
        self.raw = np.frombuffer(data, dtype=np.uint8)
        if bytes(self.raw[:4]) != b"zkey":
            raise ValueError("not a zkey file (magic %r)" % bytes(self.raw[:4]))
        try:
            f = BinFile(data, "zkey", 1)
        except struct.error:
            raise ValueError("zkey file is truncated") from None
        self.sections = {sid: lst[0] for sid, lst in f.sections.items()}
        if any(pos + size > self.raw.size for pos, size in self.sections.values()):
            raise ValueError("zkey file is truncated")
        for sid in range(1, 10):
            if sid not in self.sections:
                raise ValueError("zkey has no section %d" % sid)
        try:
            self.header = h = load_zkey_header(f)
        except (IndexError, struct.error) as e:
            raise ValueError("zkey header: %s" % e) from None
        if h.qPrime != Q_MOD or h.rPrime != R_MOD:
            raise ValueError("zkey curve not supported (q and r are not BN254's)")
        if self.sections[4][1] < 4:
            raise ValueError("zkey section 4 is truncated")
        want = _section_sizes(h)
        (self.nCoefs,) = struct.unpack_from("<I", data, self.sections[4][0])
        want[4] = 4 + 44 * self.nCoefs
        for sid in sorted(want):
            if self.sections[sid][1] < want[sid]:
                raise ValueError("zkey section %d is short: %d bytes, the header implies %d" % (sid, self.sections[sid][1], want[sid]))

    def section(self, sid):
        pos, size = self.sections[sid]
        return self.raw[pos:pos + size]

    def view(self):
        """-> zk_zkey_verify_view (pointers into this object's memory: keep it alive while the view is used)"""
        h = self.header
        v = L.zk_zkey_verify_view()
        k = v.key
        k.nVars, k.nPublic, k.domainSize, k.nCoefs = h.nVars, h.nPublic, h.domainSize, self.nCoefs
        s2 = self.section(2)
        at = 4 + 32 + 4 + 32 + 12                                        # the six points follow the two primes and three counts
        for name, nb in (("vk_alpha1", 64), ("vk_beta1", 64), ("vk_beta2", 128), ("vk_gamma2", 128), ("vk_delta1", 64), ("vk_delta2", 128)):
            setattr(v if name == "vk_gamma2" else k, name, s2[at:at + nb].ctypes.data)
            at += nb
        ptr = lambda sid: self.section(sid).ctypes.data if self.sections[sid][1] else None
        v.pointsIC, v.pointsIC_bytes = ptr(3), self.sections[3][1]
        for sid, name in ((4, "coefs"), (5, "pointsA"), (6, "pointsB1"), (7, "pointsB2"), (8, "pointsC"), (9, "pointsH")):
            setattr(k, name, ptr(sid))
            setattr(k, name + "_bytes", self.sections[sid][1])
        return v

    def close(self):
        self.raw = None
        if self._map is not None:
            try:
                self._map.close()
            except BufferError:
                pass
            self._map = None


def _call(r1cs, ptau, zkey, fn):
    _h, rv, keep = _r1cs_view(r1cs)
    pf, own = _open_ptau(ptau)
    zf = None
    try:
        zf = _ZkeyFile(zkey)
        pv, zv = pf.view(), zf.view()
        return fn(rv, pv, zv)
    finally:
        if zf is not None:
            zf.close()
        if own:
            pf.close()
        del keep


def zkey_verify_sizes(r1cs, ptau, zkey):
    """-> zk_zkey_verify_sizes as a dict (log_domain, shape_failed as a set of the names of SHAPES, chunk_points,
    device_bytes: an upper estimate of the HBM the check holds); raises ZkHipError with the library's message (a short
    section, a .r1cs that does not walk), ValueError for a file that is not what its name says.  No device is touched."""
    def fn(rv, pv, zv):
        z = L.zk_zkey_verify_sizes_t()
        L.check(L._need("zk_zkey_verify_sizes")(C.byref(rv), C.byref(pv), C.byref(zv), C.byref(z)))
        return {"log_domain": int(z.log_domain), "shape_failed": {n for i, n in enumerate(SHAPES) if z.shape_failed >> i & 1},
                "chunk_points": int(z.chunk_points), "device_bytes": int(z.device_bytes)}
    return _call(r1cs, ptau, zkey, fn)


def zkey_verify(r1cs, ptau, zkey, s=None, device=-1):
    """Is the .zkey (path or bytes) the key of the circuit (.r1cs: path or bytes) over the .ptau (path, bytes or PtauFile;
    prepared for phase 2, power >= the circuit's): zk_zkey_verify on the GPU -> ZkeyVerifyReport.  s: the scalar of the
    random combinations, drawn by the library after the files are mapped when None (a fixed one is for tests; 0, 1 and
    values >= r are refused).  Shapes that disagree are reported (shape_failed) before a device is touched.  The
    contribution transcript (section 10) is not checked."""
    if s is not None and not 2 <= int(s) < R_MOD:
        raise ValueError("the check scalar must be at least 2 and below r")

    def fn(rv, pv, zv):
        rep = L.zk_zkey_verify_report()
        rep.size = C.sizeof(rep)
        ss = L._scalar32(s) if s is not None else None
        L.check(L._need("zk_zkey_verify")(C.byref(rv), C.byref(pv), C.byref(zv), L._ptr(ss) if ss is not None else None, device, C.byref(rep)))
        return ZkeyVerifyReport(rep)
    return _call(r1cs, ptau, zkey, fn)
