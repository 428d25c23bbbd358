"""Pairings and Groth16 verification on the GPU (include/zkhip.h, section "Pairing and verification"): the counterpart of
snarkjs `groth16 verify`, which the reference leaves to snarkjs.  The arithmetic is libzkhip's; this module reads the files
(proof.json, public.json, verification_key.json or the key's own sections 2 and 3) into the byte layouts the library takes:
points affine Montgomery, x | y (G2: x.re | x.im | y.re | y.im), all-zero = infinity; public signals 32 bytes little-endian."""
import ctypes as C
import json
import mmap
import struct

import numpy as np

from . import lib as L
from .binfile import BinFile
from .zkey import Q_MOD, R_MOD, load_zkey_header

VERIFY_OK, VERIFY_INVALID, VERIFY_MALFORMED = 0, 1, 2
_MONT = 1 << 256


def _coord(v):
    """a coordinate of a JSON point: a decimal string (or a number), kept as it is when it is not below q so that the
    device check sees it (it must still fit 32 bytes)"""
    x = int(v)
    if not 0 <= x < _MONT:
        raise ValueError("coordinate %r does not fit 256 bits" % (v,))
    return x


def _enc(x):
    # Montgomery form of a reduced value; a value >= q is passed through unreduced: the device refuses it
    return (x * _MONT % Q_MOD if x < Q_MOD else x).to_bytes(32, "little")


def _f2_inv(a, b):
    d = pow((a * a + b * b) % Q_MOD, -1, Q_MOD)
    return a * d % Q_MOD, -b * d % Q_MOD


def g1_bytes(j):
    """[x, y] or [x, y, z] of a snarkjs JSON -> 64 bytes.  z is the projective third coordinate: 0 is infinity, 1 (what
    snarkjs writes) leaves x and y, anything else divides them (x / z, y / z)."""
    x, y = _coord(j[0]), _coord(j[1])
    if len(j) > 2:
        z = _coord(j[2])
        if z % Q_MOD == 0:
            return bytes(64)
        if z != 1:
            zi = pow(z, -1, Q_MOD)
            x, y = x * zi % Q_MOD, y * zi % Q_MOD
    return _enc(x) + _enc(y)


def g2_bytes(j):
    """[[x.re, x.im], [y.re, y.im]] with an optional [z.re, z.im] -> 128 bytes"""
    x, y = [_coord(j[0][0]), _coord(j[0][1])], [_coord(j[1][0]), _coord(j[1][1])]
    if len(j) > 2:
        z = (_coord(j[2][0]), _coord(j[2][1]))
        if z[0] % Q_MOD == 0 and z[1] % Q_MOD == 0:
            return bytes(128)
        if z != (1, 0):
            ia, ib = _f2_inv(*z)
            x = [(x[0] * ia - x[1] * ib) % Q_MOD, (x[0] * ib + x[1] * ia) % Q_MOD]
            y = [(y[0] * ia - y[1] * ib) % Q_MOD, (y[0] * ib + y[1] * ia) % Q_MOD]
    return _enc(x[0]) + _enc(x[1]) + _enc(y[0]) + _enc(y[1])


def load_proof(path):
    """proof.json -> 256 bytes: A 64 | B 128 | C 64 (the layout of zk_proof)"""
    with open(path) as f:
        j = json.load(f)
    if j.get("protocol", "groth16") != "groth16":
        raise ValueError("proof is not groth16")
    return g1_bytes(j["pi_a"]) + g2_bytes(j["pi_b"]) + g1_bytes(j["pi_c"])


def load_public(path):
    """public.json -> nPublic x 32 bytes little-endian; `null` (what the reference's prover writes when nPublic = 0) is
    an empty list.  A signal >= r is kept: the device refuses it."""
    with open(path) as f:
        j = json.load(f)
    out = b""
    for v in ([] if j is None else j):
        x = int(v)
        if not 0 <= x < _MONT:
            raise ValueError("public signal %r does not fit 256 bits" % (v,))
        out += x.to_bytes(32, "little")
    return out


def pairing(g1_bytes_, g2_bytes_, group=1, device=-1):
    """zk_pairing: n G1 points (64 B each) and n G2 points (128 B each), taken in consecutive groups of `group` pairs ->
    numpy uint8 [ceil(n / group) * 384]: per group the final-exponentiated product of its pairings, 12 Fq values of 32 B
    little-endian standard form, c0.c0.re first.  Raises ZkHipError naming the index of a point that is not on its curve
    or not in the subgroup."""
    a, b = L._buf(g1_bytes_), L._buf(g2_bytes_)
    if a.size % 64 or b.size % 128 or a.size // 64 != b.size // 128:
        raise ValueError("n x 64 bytes of G1 points and n x 128 bytes of G2 points expected")
    group = int(group)
    if group < 0 or group >= 1 << 32:
        raise ValueError("group: 0 .. 2^32 - 1")
    n = a.size // 64
    fn = getattr(L.load_library(), "zk_pairing", None)
    if fn is None:
        raise L.ZkHipError("zk_pairing is not in this build of libzkhip.so")
    out = np.zeros(((n + group - 1) // group if group else 0) * 384, dtype=np.uint8)
    L.check(fn(L._ptr(out) if out.size else None, L._ptr(a) if n else None, L._ptr(b) if n else None, n, group, device))
    return out


def pairing_last_path():
    """zk_pairing_last_path: 0 (a lane per group) or 1 (a workgroup per group) for this thread's last pairing(), -1 before the first."""
    return int(L.load_library().zk_pairing_last_path())


class VerificationKey:
    """A Groth16 verification key on the device (zk_vkey): .verify(proofs, publics) -> one verdict per proof."""

    def __init__(self, alpha1, beta2, gamma2, delta2, ic, device=-1):
        ic = bytes(ic)
        if len(alpha1) != 64 or len(beta2) != 128 or len(gamma2) != 128 or len(delta2) != 128 or len(ic) % 64 or not ic:
            raise ValueError("verification key: alpha 64 bytes, beta, gamma, delta 128 bytes each, IC (nPublic + 1) x 64 bytes expected")
        self.alpha1, self.beta2, self.gamma2, self.delta2, self.ic = bytes(alpha1), bytes(beta2), bytes(gamma2), bytes(delta2), ic
        self.n_public = len(ic) // 64 - 1
        self.device = int(device)                     # as given: -1 is the device that was current
        self._h = C.c_void_p()
        lib = L.load_library()
        if not hasattr(lib, "zk_vkey_create"):
            raise L.ZkHipError("zk_vkey_create is not in this build of libzkhip.so")
        keep = [np.frombuffer(b, dtype=np.uint8) for b in (self.alpha1, self.beta2, self.gamma2, self.delta2, self.ic)]
        v = L.zk_vkey_view()
        v.vk_alpha1, v.vk_beta2, v.vk_gamma2, v.vk_delta2, v.IC = (a.ctypes.data for a in keep)
        v.nPublic = self.n_public
        L.check(lib.zk_vkey_create(C.byref(self._h), C.byref(v), device))

    @staticmethod
    def read_zkey(path):
        """(alpha1, beta2, gamma2, delta2, IC) of a .zkey: only the section table and sections 1 to 3 are read"""
        with open(path, "rb") as fh:
            if fh.read(4) != b"zkey":
                raise ValueError("not a zkey file")
            m = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
        try:
            try:
                f = BinFile(m, "zkey", 1)
            except struct.error:
                raise ValueError("zkey file is truncated") from None
            for sid in (1, 2, 3):
                if sid not in f.sections:
                    raise ValueError("zkey has no section %d" % sid)
                if sum(f.sections[sid][0]) > len(m):
                    raise ValueError("zkey file is truncated")
            try:
                h = load_zkey_header(f)
            except struct.error:
                raise ValueError("zkey header is short") from None
            except IndexError as e:                  # section 2 ends before its six points do, or another section is not as it must be
                raise ValueError("zkey header is short" if f.pos > sum(f.sections[2][0]) else "zkey header: %s" % e) from None
            if h.qPrime != Q_MOD or h.rPrime != R_MOD:
                raise ValueError("zkey curve not supported (q and r are not BN254's)")
            ic = bytes(f.getSectionData(3))
            if len(ic) != (h.nPublic + 1) * 64:
                raise ValueError("zkey section 3 holds %d bytes, nPublic = %d implies %d" % (len(ic), h.nPublic, (h.nPublic + 1) * 64))
            return h.vk_alpha1, h.vk_beta2, h.vk_gamma2, h.vk_delta2, ic
        finally:
            f = None
            try:
                m.close()
            except BufferError:          # an exception's traceback still holds a view: the mapping goes with it
                pass

    @staticmethod
    def read_json(path):
        """the same from snarkjs's verification_key.json (vk_alphabeta_12 is ignored: the library computes its own)"""
        with open(path) as f:
            j = json.load(f)
        if j.get("protocol", "groth16") != "groth16":
            raise ValueError("verification key is not groth16")
        if j.get("curve", "bn128") not in ("bn128", "bn254"):
            raise ValueError("verification key curve is not bn128")
        ic = b"".join(g1_bytes(p) for p in j["IC"])
        if "nPublic" in j and int(j["nPublic"]) + 1 != len(j["IC"]):
            raise ValueError("verification key has %d IC points for nPublic = %d" % (len(j["IC"]), int(j["nPublic"])))
        return g1_bytes(j["vk_alpha_1"]), g2_bytes(j["vk_beta_2"]), g2_bytes(j["vk_gamma_2"]), g2_bytes(j["vk_delta_2"]), ic

    @classmethod
    def from_zkey(cls, path, device=-1):
        return cls(*cls.read_zkey(path), device=device)

    @classmethod
    def from_json(cls, path, device=-1):
        return cls(*cls.read_json(path), device=device)

    @classmethod
    def from_file(cls, path, device=-1):
        """a .zkey (by its magic) or a verification_key.json"""
        with open(path, "rb") as f:
            magic = f.read(4)
        return cls.from_zkey(path, device) if magic == b"zkey" else cls.from_json(path, device)

    def verify(self, proofs, publics=b""):
        """proofs: n x 256 bytes; publics: n x nPublic x 32 bytes -> numpy uint8 [n] of VERIFY_OK / VERIFY_INVALID (the
        equation fails) / VERIFY_MALFORMED (a point off its curve, outside the subgroup or at infinity, a value not reduced)"""
        if not self._h:
            raise L.ZkHipError("the verification key is closed")
        p, s = L._buf(proofs), L._buf(publics)
        if p.size % 256:
            raise ValueError("proofs: a multiple of 256 bytes expected")
        n = p.size // 256
        if s.size != n * self.n_public * 32:
            raise ValueError("publics: %d proofs x %d signals x 32 bytes expected, got %d bytes" % (n, self.n_public, s.size))
        out = np.zeros(n, dtype=np.uint8)
        L.check(L.load_library().zk_vkey_verify(self._h, L._ptr(p) if n else None, L._ptr(s) if s.size else None, n, L._ptr(out) if n else None))
        return out

    def verify_batch(self, proofs, publics=b"", scalars=None):
        """zk_vkey_verify_batch: verify()'s arguments -> (verdicts, report).  Groups of ZKHIP_VERIFY_GROUP proofs are checked by
        one random linear combination each and only the proofs of a failing group one by one: the same verdicts as verify()
        except that an INVALID proof is taken for OK with probability at most 2^-128 per group.  report: dict of
        zk_vkey_batch_report (group, groups, groups_failed, proofs_rechecked, malformed, launches).
        scalars is for tests only: n x 16 bytes little-endian, one non-zero scalar per proof.  None, the only sound choice
        outside a test, lets the library draw them from the system's random source."""
        if not self._h:
            raise L.ZkHipError("the verification key is closed")
        p, s = L._buf(proofs), L._buf(publics)
        if p.size % 256:
            raise ValueError("proofs: a multiple of 256 bytes expected")
        n = p.size // 256
        if s.size != n * self.n_public * 32:
            raise ValueError("publics: %d proofs x %d signals x 32 bytes expected, got %d bytes" % (n, self.n_public, s.size))
        r = None
        if scalars is not None:
            r = L._buf(scalars)
            if r.size != n * 16:
                raise ValueError("scalars: %d proofs x 16 bytes expected, got %d bytes" % (n, r.size))
        fn = getattr(L.load_library(), "zk_vkey_verify_batch", None)
        if fn is None:
            raise L.ZkHipError("zk_vkey_verify_batch is not in this build of libzkhip.so")
        out = np.zeros(n, dtype=np.uint8)
        rep = L.zk_vkey_batch_report()
        rep.size = C.sizeof(L.zk_vkey_batch_report)
        L.check(fn(self._h, L._ptr(p) if n else None, L._ptr(s) if s.size else None, n, L._ptr(r) if r is not None and n else None,
                   L._ptr(out) if n else None, C.byref(rep)))
        return out, {name: int(getattr(rep, name)) for name, _ in L.zk_vkey_batch_report._fields_ if name not in ("size", "reserved")}

    def info(self):
        """zk_vkey_info: which path the last verify() took (last_path: 0 a lane per proof, 1 a workgroup per proof), the
        threshold it used, its kernel launches, and the proofs sent down each path since the key was made."""
        if not self._h:
            raise L.ZkHipError("the verification key is closed")
        plan = L.zk_vkey_plan()
        L.check(L.load_library().zk_vkey_info(self._h, C.byref(plan)))
        return {name: int(getattr(plan, name)) for name, _ in L.zk_vkey_plan._fields_ if name != "reserved"}

    def close(self):
        if getattr(self, "_h", None):
            L.load_library().zk_vkey_destroy(self._h)
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


class VerificationKeySet:
    """Proofs under many keys in one call (zk_vkey_set): a handle over VerificationKey objects of one device.
    .verify(proofs, key_of, publics) gives proof i the verdict keys[key_of[i]].verify gives it, and the number of kernel
    launches does not depend on the number of keys.  The set holds references to its keys: they live as long as it does
    (closing one of them while the set is open is the caller's error).  A key may appear twice."""

    def __init__(self, keys):
        keys = list(keys)
        if not keys:
            raise ValueError("a key set needs at least one key")
        for j, k in enumerate(keys):
            if not isinstance(k, VerificationKey):
                raise ValueError("key %d is not a VerificationKey" % j)
            if not k._h:
                raise ValueError("key %d is closed" % j)
        # keys made for the current device (-1) are left to the library, which knows where they are and names both devices
        named = sorted({k.device for k in keys if k.device >= 0})
        if len(named) > 1:
            raise ValueError("the keys of a set are on one device; these are on devices %s" % ", ".join(map(str, named)))
        self.keys = keys
        self.n_public = np.array([k.n_public for k in keys], dtype=np.int64)
        self._h = C.c_void_p()
        fn = getattr(L.load_library(), "zk_vkey_set_create", None)
        if fn is None:
            raise L.ZkHipError("zk_vkey_set_create is not in this build of libzkhip.so")
        arr = (C.c_void_p * len(keys))(*[k._h.value for k in keys])
        L.check(fn(C.byref(self._h), arr, len(keys)))

    def _checked(self, proofs, key_of, publics):
        """verify()'s argument checks -> (proofs, key_of as uint32, publics, n); ValueError before any library call"""
        p, s = L._buf(proofs), L._buf(publics)
        if p.size % 256:
            raise ValueError("proofs: a multiple of 256 bytes expected")
        n = p.size // 256
        ko = np.asarray(key_of)
        if ko.ndim != 1 or ko.size != n:
            raise ValueError("key_of: %d indices expected, one per proof, got %s" % (n, "x".join(map(str, ko.shape)) or "a scalar"))
        if n and ko.dtype.kind not in "iu":
            raise ValueError("key_of: integers expected, got %s" % ko.dtype)
        ko = ko.astype(np.int64) if n else np.zeros(0, dtype=np.int64)
        bad = np.flatnonzero((ko < 0) | (ko >= len(self.keys)))
        if bad.size:
            raise ValueError("key_of[%d] = %d: the set holds %d keys" % (bad[0], ko[bad[0]], len(self.keys)))
        want = int(self.n_public[ko].sum()) * 32
        if s.size != want:
            raise ValueError("publics: %d bytes expected (%d signals of 32 bytes for these keys), got %d bytes" % (want, want // 32, s.size))
        return p, np.ascontiguousarray(ko, dtype=np.uint32), s, n

    def verify(self, proofs, key_of, publics=b""):
        """proofs: n x 256 bytes; key_of: n indices into the set's keys (any integer sequence or array); publics: the
        signals of proof 0, then of proof 1, ...: proof i has keys[key_of[i]].n_public of them, 32 bytes each
        -> numpy uint8 [n] of VERIFY_OK / VERIFY_INVALID / VERIFY_MALFORMED"""
        if not self._h:
            raise L.ZkHipError("the key set is closed")
        p, ko, s, n = self._checked(proofs, key_of, publics)
        out = np.zeros(n, dtype=np.uint8)
        L.check(L.load_library().zk_vkey_set_verify(self._h, L._ptr(p) if n else None, L._ptr(ko) if n else None, L._ptr(s) if s.size else None,
                                                    s.size, n, L._ptr(out) if n else None))
        return out

    def verify_batch(self, proofs, key_of, publics=b"", scalars=None):
        """zk_vkey_set_verify_batch: verify()'s arguments -> (verdicts, report).  Inside a chunk the proofs are ordered by
        key and cut into groups of at most ZKHIP_VERIFY_GROUP proofs under at most ZKHIP_VERIFY_GROUP_KEYS keys; a group is
        checked by one random linear combination across its keys and only the proofs of a failing group one by one: the same
        verdicts as verify() except that an INVALID proof is taken for OK with probability at most 2^-128 per group.
        report: dict of zk_vkey_set_batch_report (group, group_keys, launches, groups, groups_failed, segments,
        proofs_rechecked, malformed).
        scalars is for tests only: n x 16 bytes little-endian, one non-zero scalar per proof.  None, the only sound choice
        outside a test, lets the library draw them from the system's random source."""
        if not self._h:
            raise L.ZkHipError("the key set is closed")
        p, ko, s, n = self._checked(proofs, key_of, publics)
        r = None
        if scalars is not None:
            r = L._buf(scalars)
            if r.size != n * 16:
                raise ValueError("scalars: %d proofs x 16 bytes expected, got %d bytes" % (n, r.size))
        fn = getattr(L.load_library(), "zk_vkey_set_verify_batch", None)
        if fn is None:
            raise L.ZkHipError("zk_vkey_set_verify_batch is not in this build of libzkhip.so")
        out = np.zeros(n, dtype=np.uint8)
        rep = L.zk_vkey_set_batch_report()
        rep.size = C.sizeof(L.zk_vkey_set_batch_report)
        L.check(fn(self._h, L._ptr(p) if n else None, L._ptr(ko) if n else None, L._ptr(s) if s.size else None, s.size, n,
                   L._ptr(r) if r is not None and n else None, L._ptr(out) if n else None, C.byref(rep)))
        return out, {name: int(getattr(rep, name)) for name, _ in L.zk_vkey_set_batch_report._fields_ if name != "size"}

    def info(self):
        """zk_vkey_set_info: n_keys, the path of the last verify() (last_path: 0 a lane per proof, 1 a workgroup per proof),
        its kernel launches, its waves with idle lanes, and the proofs sent down each path since the set was made."""
        if not self._h:
            raise L.ZkHipError("the key set is closed")
        plan = L.zk_vkey_set_plan()
        plan.size = C.sizeof(L.zk_vkey_set_plan)
        L.check(L.load_library().zk_vkey_set_info(self._h, C.byref(plan)))
        return {name: int(getattr(plan, name)) for name, _ in L.zk_vkey_set_plan._fields_ if name != "size"}

    def close(self):
        if getattr(self, "_h", None):
            L.load_library().zk_vkey_set_destroy(self._h)
            self._h = C.c_void_p()
        self.keys = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def groth16_verify(vk_path, public_path, proof_path, device=-1):
    """What `verifier vk public proof` answers: True when the proof verifies.  vk_path: verification_key.json or a .zkey."""
    proof, public = load_proof(proof_path), load_public(public_path)
    key = VerificationKey.read_zkey(vk_path) if open(vk_path, "rb").read(4) == b"zkey" else VerificationKey.read_json(vk_path)
    if len(key[4]) // 64 != len(public) // 32 + 1:
        raise ValueError("verification key has %d IC points for %d public signals" % (len(key[4]) // 64, len(public) // 32))
    with VerificationKey(*key, device=device) as vk:
        return int(vk.verify(proof, public)[0]) == VERIFY_OK
