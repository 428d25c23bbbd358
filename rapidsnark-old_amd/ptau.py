"""Powers of Tau files (.ptau) and the Groth16 setup on the GPU (include/zkhip.h, section "Groth16 setup").

Same container as .zkey / .r1cs (binfile.py): magic "ptau", version 1.  Points as in a .zkey: affine, Montgomery LE, 64 B
in G1 and 128 B in G2, all-zero = infinity.
   1 header      u32 n8 (= 32), q (n8 bytes), u32 power, u32 ceremonyPower
   2 tauG1       2^(power+1) - 1 points         3 tauG2, 4 alphaTauG1, 5 betaTauG1: 2^power points each
   6 betaG2      one point                      7 contributions (not read)
  12 .. 15       written by `snarkjs powersoftau prepare phase2`: the Lagrange form of tauG1, tauG2, alphaTauG1, betaTauG1.
                 Each is the concatenation of levels p = 0, 1, ...; level p holds 2^p points from point 2^p - 1 on, point j
                 being [L_j^(2^p)(tau)] (times alpha / beta in 14 / 15).  Section 12 runs to level power + 1 (built from the
                 2^(power+1) - 1 powers that exist: the missing top power counts as infinity), 13 to 15 to level power.

prepare_phase2(src, dst) is `snarkjs powersoftau prepare phase2` on the GPU: sections 12 to 15 from sections 2 to 5, an
inverse DFT over the points themselves (csrc/ptau_prepare.hip), for a ceremony's own output, whose tau nobody knows.

ptau_new(power, path) writes the file a ceremony starts from (`snarkjs powersoftau new`: every point a generator), and
ptau_contribute(src, dst) is the arithmetic of `snarkjs powersoftau contribute` on the GPU (csrc/mulvec.hip): sections 2 to
5 times the powers of a new tau (and alpha, beta), section 6 times beta.  Section 7 is copied, not extended: the result is
a sound file if one contributor forgot their scalars, not a transcript `snarkjs powersoftau verify` accepts.

groth16_setup(r1cs, ptau) makes the phase-2 starting key of snarkjs `groth16 setup` / `zkey new` from these sections on the
GPU (gamma = delta = 1) as the key dict zkgen.write_zkey / zkgen.verification_key take."""
import ctypes as C
import mmap
import os
import secrets
import struct

import numpy as np

from . import lib as L
from . import synth
from .binfile import BinFile, rewrite_mapped, write_container

Q_MOD = synth.Q_MOD
R_MOD = synth.R_MOD
POINT_BYTES = {12: 64, 13: 128, 14: 64, 15: 64}
LAGRANGE = (12, 13, 14, 15)


class PtauFile:
    """A .ptau (path: mapped read-only, never read whole; or bytes): header, sections and level slices.  Raises ValueError
    on a file that is not a BN254 ptau."""

    def __init__(self, path_or_bytes):
        if isinstance(path_or_bytes, str):
            with open(path_or_bytes, "rb") as fh:
                size = fh.seek(0, 2)
                if size < 12:
                    raise ValueError("ptau file is truncated")
                self._map = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
            data = self._map
        else:
            self._map = None
            data = bytes(path_or_bytes)
        self.raw = np.frombuffer(data, dtype=np.uint8)
        if bytes(self.raw[:4]) != b"ptau":
            raise ValueError("not a ptau file (magic %r)" % bytes(self.raw[:4]))
        try:
            f = BinFile(data, "ptau", 1)
        except struct.error:
            raise ValueError("ptau file is truncated") from None
        end = max((pos + size for lst in f.sections.values() for pos, size in lst), default=12)
        if end > len(data):
            raise ValueError("ptau file is truncated")
        self.sections = {sid: lst[0] for sid, lst in f.sections.items()}
        if 1 not in self.sections:
            raise ValueError("ptau has no header section")
        pos, size = self.sections[1]
        if size < 4:
            raise ValueError("ptau header section is truncated")
        (self.n8,) = struct.unpack_from("<I", data, pos)
        if self.n8 != 32:
            raise ValueError("ptau: n8 is %d, only 32-byte fields (BN254) are supported" % self.n8)
        if size < 4 + 32 + 8:
            raise ValueError("ptau header section is truncated")
        self.q = int.from_bytes(bytes(data[pos + 4:pos + 36]), "little")
        if self.q != Q_MOD:
            raise ValueError("ptau curve not supported (q is not BN254's)")
        self.power, self.ceremony_power = struct.unpack_from("<II", data, pos + 36)

    @property
    def prepared(self):
        return all(s in self.sections for s in LAGRANGE)

    def section(self, sid):
        """-> numpy uint8 view of section sid."""
        if sid not in self.sections:
            raise ValueError("ptau has no section %d" % sid)
        pos, size = self.sections[sid]
        return self.raw[pos:pos + size]

    def point(self, sid, i, nbytes):
        s = self.section(sid)
        if s.size < (i + 1) * nbytes:
            raise ValueError("ptau section %d is short" % sid)
        return s[i * nbytes:(i + 1) * nbytes]

    def level(self, sid, p):
        """Level p of Lagrange section sid (12 .. 15): 2^p points, numpy uint8 view."""
        nb = POINT_BYTES[sid]
        s = self.section(sid)
        lo, hi = ((1 << p) - 1) * nb, ((2 << p) - 1) * nb
        if s.size < hi:
            raise ValueError("ptau section %d is short: level %d ends at byte %d of %d" % (sid, p, hi, s.size))
        return s[lo:hi]

    def view(self):
        """-> zk_ptau_view (pointers into this object's memory: keep it alive while the view is used).  Sections 12 to 15
        that are missing stay NULL: the library reports the file as not prepared."""
        v = L.zk_ptau_view()
        v.power = self.power
        v.alpha1 = self.point(4, 0, 64).ctypes.data
        v.beta1 = self.point(5, 0, 64).ctypes.data
        v.beta2 = self.point(6, 0, 128).ctypes.data
        for sid, name in zip(LAGRANGE, ("lagrange_g1", "lagrange_g2", "lagrange_alpha_g1", "lagrange_beta_g1")):
            if sid in self.sections:
                s = self.section(sid)
                setattr(v, name, s.ctypes.data if s.size else None)
                setattr(v, name + "_bytes", s.size)
        return v

    def powers_view(self):
        """-> zk_ptau_powers_view (sections 2 to 5 as pointers into this object's memory).  A missing section stays NULL:
        the library names it."""
        v = L.zk_ptau_powers_view()
        v.power = self.power
        for sid, name in zip((2, 3, 4, 5), ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1")):
            if sid in self.sections:
                s = self.section(sid)
                setattr(v, name, s.ctypes.data if s.size else None)
                setattr(v, name + "_bytes", s.size)
        return v

    def file_view(self):
        """-> zk_ptau_file_view (sections 2 to 6 and 12 to 15 as pointers into this object's memory).  A missing section
        stays NULL: the library names it."""
        v = L.zk_ptau_file_view()
        v.power = self.power
        for sid in (2, 3, 4, 5, 6) + LAGRANGE:
            if sid in self.sections:
                s = self.section(sid)
                v.sec[sid] = s.ctypes.data if s.size else None
                v.sec_bytes[sid] = s.size
        return v

    def kzg_view(self):
        """-> zk_kzg_view (sections 2, 3 and, when the file is prepared, 12 as pointers into this object's memory).  A missing
        section stays NULL: the library names it."""
        v = L.zk_kzg_view()
        v.power = self.power
        for sid, name in ((2, "tau_g1"), (3, "tau_g2"), (12, "lagrange_g1")):
            if sid in self.sections:
                s = self.section(sid)
                setattr(v, name, s.ctypes.data if s.size else None)
                setattr(v, name + "_bytes", s.size)
        return v

    def close(self):
        self.raw = None
        if self._map is not None:
            try:
                self._map.close()
            except BufferError:          # a caller still holds a view of the mapping: it goes with the last view
                pass
            self._map = None


# ---------------------------------------------------------------- a trapdoor .ptau (test and benchmark inputs)
def _fr_rows(values):
    return np.frombuffer(b"".join(int(v % R_MOD).to_bytes(32, "little") for v in values), dtype=np.uint8).copy()


def _lagrange_level(powers, p, zero_top=False):
    """L_j^(2^p)(tau), j < 2^p, standard form: one inverse NTT of tau^0 .. tau^(2^p - 1) (the top power zeroed on request)."""
    n = 1 << p
    x = np.ascontiguousarray(powers[:n * 32]).copy()
    if zero_top:
        x[(n - 1) * 32:] = 0
    if n == 1:
        return x
    return np.frombuffer(L.fr_ntt(x, inverse=True), dtype=np.uint8)


def write_trapdoor_ptau(power, tau, alpha, beta, path, prepared=True):
    """Write a prepared .ptau of `power` (sections 1 to 7 and 12 to 15; prepared=False: sections 1 to 7 only, as a
    ceremony leaves the file, the input of prepare_phase2) whose tau, alpha, beta are KNOWN.  NOT a
    ceremony: anyone who has these numbers can forge proofs for every key made from the file.  It makes test and
    benchmark inputs only: keys whose trapdoor is known, so that proofs can be checked in Fr alone.  Needs a GPU: the
    Lagrange levels are inverse NTTs of the powers of tau (zk_fr_ntt), the points batch fixed-base multiplications
    (zk_fixed_base_g1 / g2), as zkgen does for its keys."""
    from . import zkgen
    if not 1 <= power <= 27:
        raise ValueError("power must be in 1 .. 27")
    g1, g2 = synth.g1_gen_bytes(), synth.g2_gen_bytes()
    n = 1 << power
    pw = zkgen._powers(tau, 2 * n)                                         # tau^0 .. tau^(2n - 1), standard
    a_k = lambda x, k: zkgen._scale(x, k, x.size // 32)
    sections = [
        (1, struct.pack("<I", 32) + int(Q_MOD).to_bytes(32, "little") + struct.pack("<II", power, power)),
        (2, L.fixed_base_g1(g1, pw[:(2 * n - 1) * 32])),
        (3, L.fixed_base_g2(g2, pw[:n * 32])),
        (4, L.fixed_base_g1(g1, a_k(pw[:n * 32], alpha))),
        (5, L.fixed_base_g1(g1, a_k(pw[:n * 32], beta))),
        (6, L.fixed_base_g2(g2, _fr_rows([beta]))),
        (7, struct.pack("<I", 0)),
    ]
    if prepared:
        levels = [_lagrange_level(pw, p, zero_top=(p == power + 1)) for p in range(power + 2)]
        lag = np.concatenate(levels)                                        # section 12's scalars
        lag13 = lag[:((2 * n) - 1) * 32]                                    # levels 0 .. power
        sections += [
            (12, L.fixed_base_g1(g1, lag)),
            (13, L.fixed_base_g2(g2, lag13)),
            (14, L.fixed_base_g1(g1, a_k(lag13, alpha))),
            (15, L.fixed_base_g1(g1, a_k(lag13, beta))),
        ]
    write_container(path, b"ptau", 1, sections)


# ---------------------------------------------------------------- a new file and a contribution to it
def ptau_new(power, path):
    """What `snarkjs powersoftau new bn128 power path` writes (and the program `ptaunew`, byte for byte): sections 2, 4, 5
    filled with the generator of G1, 3 and 6 with that of G2, section 7 a contribution count of zero.  tau = alpha = beta =
    1: contribute before use.  No device is touched."""
    if not 1 <= power <= 28:
        raise ValueError("power must be in 1 .. 28")
    g1 = np.frombuffer(synth.g1_gen_bytes(), dtype=np.uint8)
    g2 = np.frombuffer(synth.g2_gen_bytes(), dtype=np.uint8)
    n = 1 << power
    head = np.frombuffer(b"ptau" + struct.pack("<I", 1), dtype=np.uint8)
    hdr = np.frombuffer(struct.pack("<I", 32) + int(Q_MOD).to_bytes(32, "little") + struct.pack("<II", power, power), dtype=np.uint8)
    rows = [(2, g1, 2 * n - 1), (3, g2, n), (4, g1, n), (5, g1, n), (6, g2, 1)]
    secs = [(1, hdr.size, hdr)] + [(sid, g.size * cnt, None) for sid, g, cnt in rows] + [(7, 4, np.zeros(4, np.uint8))]
    with rewrite_mapped(path, head, secs) as (o, starts):
        for (sid, g, cnt), at in zip(rows, starts[1:6]):
            o[at:at + g.size * cnt].reshape(cnt, g.size)[:] = g
        del o


def ptau_contribute_sizes(src):
    """-> zk_ptau_contribute_sizes as a dict (the byte sizes of the output sections 2 to 6, chunk_points, device_bytes);
    raises ZkHipError with the library's message (unsupported power, prepared file, missing or short section).  No device
    is touched."""
    pf, own = _open_ptau(src)
    try:
        fv = pf.file_view()
        z = L.zk_ptau_contrib_sizes()
        L.check(L.load_library().zk_ptau_contribute_sizes(C.byref(fv), C.byref(z)))
    finally:
        if own:
            pf.close()
    return {name: int(getattr(z, name)) for name, _ in L.zk_ptau_contrib_sizes._fields_}


def ptau_contribute(src, dst, tau=None, alpha=None, beta=None, device=-1):
    """One contribution to a .ptau on the GPU (zk_ptau_contribute), the arithmetic of `snarkjs powersoftau contribute`.
    src: path of a file that is not prepared for phase 2; dst: path.  tau, alpha, beta: ints with 0 < s < r; None draws the
    scalar from `secrets` (2 <= s < r), and a file is safe only if somebody's drawn scalars were forgotten.  dst holds the
    magic and version of src and its sections 1 to 7 in src's order: 1 and 7 byte for byte (the transcript is COPIED, not
    extended), 2 to 6 from the library.  It is written as dst + ".partial" through a mapping and renamed at the end: a
    failure (ZkHipError with the library's message, ValueError for bad scalars or dst = src) leaves neither file."""
    given = []
    for name, s in (("tau", tau), ("alpha", alpha), ("beta", beta)):
        while s is None:
            s = secrets.randbits(254)
            s = s if 2 <= s < R_MOD else None
        s = int(s)
        if not 0 < s < R_MOD:
            raise ValueError("the contribution scalar %s must satisfy 0 < s < r" % name)
        given.append(s)
    if os.path.exists(dst) and os.path.samefile(src, dst):
        raise ValueError("the input and the output are the same file")
    lib = L.load_library()
    pf = PtauFile(src)
    try:
        fv = pf.file_view()
        z = L.zk_ptau_contrib_sizes()
        L.check(lib.zk_ptau_contribute_sizes(C.byref(fv), C.byref(z)))
        made = {2: z.tau_g1_bytes, 3: z.tau_g2_bytes, 4: z.alpha_tau_g1_bytes, 5: z.beta_tau_g1_bytes, 6: z.beta_g2_bytes}
        keep = sorted((pos, size, sid) for sid, (pos, size) in pf.sections.items() if 1 <= sid <= 7)
        secs = [(sid, int(made[sid]), None) if sid in made else (sid, size, pf.raw[pos:pos + size]) for pos, size, sid in keep]
        with rewrite_mapped(dst, pf.raw[:8], secs) as (o, starts):
            where = {sid: at for (sid, _, _), at in zip(secs, starts)}
            out = L.zk_ptau_contrib_out(*(o[where[sid]:].ctypes.data for sid in (2, 3, 4, 5, 6)))
            ss = [L._scalar32(s) for s in given]
            try:
                L.check(lib.zk_ptau_contribute(C.byref(fv), L._ptr(ss[0]), L._ptr(ss[1]), L._ptr(ss[2]), device, C.byref(out)))
            finally:
                for a in ss:
                    a[:] = 0
            del o
    finally:
        pf.close()


# ---------------------------------------------------------------- prepare phase 2
def prepare_sizes(ptau):
    """-> zk_ptau_prepare_sizes as a dict (the byte sizes of sections 12 to 15 and device_bytes); raises ZkHipError with the
    library's message (unsupported power, missing or short section).  No device is touched."""
    pf, own = _open_ptau(ptau)
    try:
        pv = pf.powers_view()
        z = L.zk_ptau_lagrange_sizes()
        L.check(L.load_library().zk_ptau_prepare_sizes(C.byref(pv), C.byref(z)))
    finally:
        if own:
            pf.close()
    return {name: int(getattr(z, name)) for name, _ in L.zk_ptau_lagrange_sizes._fields_}


def prepare_phase2(src, dst, device=-1):
    """`snarkjs powersoftau prepare phase2 src dst` on the GPU.  src: path, bytes or PtauFile; dst: path.  dst holds the
    magic and version of src, its sections 1 to 7 byte for byte in src's order, then sections 12 to 15.  It is written as
    dst + ".partial" through a mapping and renamed at the end: a failure (ZkHipError with the library's message,
    ValueError for a file that is already prepared) leaves neither file."""
    lib = L.load_library()
    pf, own = _open_ptau(src)
    try:
        if pf.prepared:
            raise ValueError("the ptau file is already prepared for phase 2 (it has sections 12 to 15)")
        pv = pf.powers_view()
        z = L.zk_ptau_lagrange_sizes()
        L.check(lib.zk_ptau_prepare_sizes(C.byref(pv), C.byref(z)))
        keep = sorted((pos, size, sid) for sid, (pos, size) in pf.sections.items() if 1 <= sid <= 7)
        secs = [(sid, size, pf.raw[pos:pos + size]) for pos, size, sid in keep]
        secs += [(sid, int(getattr(z, name + "_bytes")), None) for sid, name in
                 zip(LAGRANGE, ("lagrange_g1", "lagrange_g2", "lagrange_alpha_g1", "lagrange_beta_g1"))]
        with rewrite_mapped(dst, pf.raw[:8], secs) as (o, starts):
            out = L.zk_ptau_lagrange_out(*(o[at:].ctypes.data for at in starts[-4:]))
            L.check(lib.zk_ptau_prepare(C.byref(pv), device, C.byref(out)))
            del o
    finally:
        if own:
            pf.close()


# ---------------------------------------------------------------- is the file sound
class PtauReport:
    """What zk_ptau_check found.  ok; verdict (0 OK, 1 INVALID, 2 MALFORMED); failed: the set of section ids (2 .. 6) whose
    equation failed, 0 for a generator; lagrange_failed: {12 .. 15: set of levels}; for a malformed point bad_section,
    bad_index and bad_kind (1 coordinate >= q, 2 off the curve, 3 not in the subgroup, 4 infinity)."""

    def __init__(self, rep, prepared):
        self.verdict = int(rep.verdict)
        self.ok = self.verdict == L.ZK_PTAU_OK
        self.prepared = bool(prepared)
        self.failed = {k for k in range(32) if rep.failed >> k & 1}
        self.lagrange_failed = {sid: {p for p in range(32) if rep.lagrange_failed[i] >> p & 1} for i, sid in enumerate(LAGRANGE)}
        self.bad_section, self.bad_index, self.bad_kind = int(rep.bad_section), int(rep.bad_index), int(rep.bad_kind)

    def __repr__(self):
        return "PtauReport(verdict=%d, failed=%r, lagrange_failed=%r, bad=(%d, %d, %d))" % (
            self.verdict, sorted(self.failed), {k: sorted(v) for k, v in self.lagrange_failed.items() if v},
            self.bad_section, self.bad_index, self.bad_kind)


def ptau_check_sizes(ptau):
    """-> zk_ptau_check_sizes as a dict (prepared, chunk_points, device_bytes); raises ZkHipError with the library's message
    (unsupported power, missing or short section, some but not all of sections 12 to 15).  No device is touched."""
    pf, own = _open_ptau(ptau)
    try:
        fv = pf.file_view()
        z = L.zk_ptau_check_sizes_t()
        L.check(L.load_library().zk_ptau_check_sizes(C.byref(fv), C.byref(z)))
    finally:
        if own:
            pf.close()
    return {name: int(getattr(z, name)) for name, _ in L.zk_ptau_check_sizes_t._fields_}


def ptau_check(ptau, s=None, device=-1):
    """Is the .ptau (path, bytes or PtauFile) sound: zk_ptau_check on the GPU -> PtauReport.  s: the scalar of the random
    combination, drawn by the library when None (a fixed one is for tests).  The contribution transcript is not checked."""
    lib = L.load_library()
    pf, own = _open_ptau(ptau)
    try:
        fv = pf.file_view()
        z = L.zk_ptau_check_sizes_t()
        L.check(lib.zk_ptau_check_sizes(C.byref(fv), C.byref(z)))
        rep = L.zk_ptau_report()
        ss = L._scalar32(s) if s is not None else None
        L.check(lib.zk_ptau_check(C.byref(fv), L._ptr(ss) if ss is not None else None, device, C.byref(rep)))
    finally:
        if own:
            pf.close()
    return PtauReport(rep, z.prepared)


# ---------------------------------------------------------------- the setup
def _r1cs_view(r1cs):
    from .r1cs import open_r1cs
    h, sec = open_r1cs(r1cs)
    keep = np.frombuffer(sec, dtype=np.uint8)
    v = L.zk_r1cs_view(h.nWires, h.nPubOut, h.nPubIn, h.nPrvIn, h.nConstraints, keep.ctypes.data if keep.size else None, keep.size)
    return h, v, keep


def _open_ptau(ptau):
    return (ptau, False) if isinstance(ptau, PtauFile) else (PtauFile(ptau), True)


def setup_sizes(r1cs, ptau):
    """-> zk_groth16_setup_sizes as a dict (nVars, nPublic, domainSize, log_domain, nCoefs); raises ZkHipError with the
    library's message when the files do not fit each other."""
    _h, rv, keep = _r1cs_view(r1cs)
    pf, own = _open_ptau(ptau)
    try:
        pv = pf.view()
        s = L.zk_setup_sizes()
        L.check(L.load_library().zk_groth16_setup_sizes(C.byref(rv), C.byref(pv), C.byref(s)))
    finally:
        if own:
            pf.close()
    del keep
    return {name: int(getattr(s, name)) for name, _ in L.zk_setup_sizes._fields_}


def groth16_setup(r1cs, ptau, device=-1):
    """The phase-2 starting key of snarkjs `groth16 setup circuit.r1cs pot.ptau` on the GPU (gamma = delta = 1): a dict with
    the sections zkgen.write_zkey and zkgen.verification_key take (numpy uint8 arrays).  r1cs: path or bytes; ptau: path,
    bytes or PtauFile (prepared for phase 2, power >= the circuit's log domain)."""
    lib = L.load_library()
    _h, rv, keep = _r1cs_view(r1cs)
    pf, own = _open_ptau(ptau)
    try:
        pv = pf.view()
        s = L.zk_setup_sizes()
        L.check(lib.zk_groth16_setup_sizes(C.byref(rv), C.byref(pv), C.byref(s)))
        nv, npub, n, nc = s.nVars, s.nPublic, s.domainSize, s.nCoefs
        key = {"nVars": nv, "nPublic": npub, "domainSize": n, "nCoefs": nc,
               "coefs": np.zeros(4 + 44 * nc, np.uint8), "pointsIC": np.zeros((npub + 1) * 64, np.uint8),
               "pointsA": np.zeros(nv * 64, np.uint8), "pointsB1": np.zeros(nv * 64, np.uint8), "pointsB2": np.zeros(nv * 128, np.uint8),
               "pointsC": np.zeros((nv - npub - 1) * 64, np.uint8), "pointsH": np.zeros(n * 64, np.uint8)}
        ptr = lambda name: key[name].ctypes.data if key[name].size else None
        out = L.zk_setup_out(ptr("coefs"), ptr("pointsIC"), ptr("pointsA"), ptr("pointsB1"), ptr("pointsB2"), ptr("pointsC"), ptr("pointsH"))
        L.check(lib.zk_groth16_setup(C.byref(rv), C.byref(pv), device, C.byref(out)))
        key["vk_alpha1"] = pf.point(4, 0, 64).copy()
        key["vk_beta1"] = pf.point(5, 0, 64).copy()
        key["vk_beta2"] = pf.point(6, 0, 128).copy()
    finally:
        if own:
            pf.close()
    del keep
    g1, g2 = (np.frombuffer(b, dtype=np.uint8).copy() for b in (synth.g1_gen_bytes(), synth.g2_gen_bytes()))
    key["vk_gamma2"], key["vk_delta1"], key["vk_delta2"] = g2, g1, g2.copy()
    return key
