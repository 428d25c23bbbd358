"""ZKeyUtils::loadHeader mirror (reference src/zkey_utils.hpp:11-36, src/zkey_utils.cpp:17-52), and the phase-2
contribution to a key on the GPU (include/zkhip.h, section "Phase-2 contribution"; no counterpart in the reference)."""
import ctypes as C
import json
import mmap
import os
import secrets
import struct

import numpy as np

from .synth import Q_MOD, R_MOD


class ZkeyHeader:
    __slots__ = ("n8q", "qPrime", "n8r", "rPrime", "nVars", "nPublic", "domainSize", "nCoefs",
                 "vk_alpha1", "vk_beta1", "vk_beta2", "vk_gamma2", "vk_delta1", "vk_delta2")


def load_zkey_header(f) -> ZkeyHeader:
    h = ZkeyHeader()
    f.startReadSection(1)
    if f.readU32LE() != 1:
        raise ValueError("zkey file is not groth16")
    f.endReadSection()
    f.startReadSection(2)
    h.n8q = f.readU32LE()
    h.qPrime = int.from_bytes(f.read(h.n8q), "little")
    h.n8r = f.readU32LE()
    h.rPrime = int.from_bytes(f.read(h.n8r), "little")
    h.nVars = f.readU32LE()
    h.nPublic = f.readU32LE()
    h.domainSize = f.readU32LE()
    h.vk_alpha1 = bytes(f.read(h.n8q * 2))
    h.vk_beta1 = bytes(f.read(h.n8q * 2))
    h.vk_beta2 = bytes(f.read(h.n8q * 4))
    h.vk_gamma2 = bytes(f.read(h.n8q * 4))
    h.vk_delta1 = bytes(f.read(h.n8q * 2))
    h.vk_delta2 = bytes(f.read(h.n8q * 4))
    f.endReadSection()
    h.nCoefs = f.getSectionSize(4) // (12 + h.n8r)      # zkey_utils.cpp:49
    return h


# ---------------------------------------------------------------- phase-2 contribution
def _section_sizes(h):
    """the byte sizes the header implies for sections 3 to 9 (section 4 from its own leading count)"""
    np1 = h.nPublic + 1
    return {3: np1 * 64, 5: h.nVars * 64, 6: h.nVars * 64, 7: h.nVars * 128, 8: (h.nVars - np1) * 64, 9: h.domainSize * 64}


def _vk_json(h, delta2, ic):
    """verification_key.json as `zkeynew` writes it (zkgen.verification_key's content), from Montgomery bytes, on the host"""
    rinv = pow(1 << 256, -1, Q_MOD)
    std = lambda b: [str(int.from_bytes(bytes(b[i:i + 32]), "little") * rinv % Q_MOD) for i in range(0, len(b), 32)]
    g1 = lambda b: std(b) + ["1"]

    def g2(b):
        xa, xb, ya, yb = std(b)
        return [[xa, xb], [ya, yb], ["1", "0"]]

    return {"protocol": "groth16", "curve": "bn128", "nPublic": h.nPublic, "vk_alpha_1": g1(h.vk_alpha1), "vk_beta_2": g2(h.vk_beta2),
            "vk_gamma_2": g2(h.vk_gamma2), "vk_delta_2": g2(delta2), "IC": [g1(ic[i:i + 64]) for i in range(0, len(ic), 64)]}


def zkey_contribute(src, dst, d=None, vk_path=None, device=-1):
    """One phase-2 contribution on the GPU, what `zkeycontribute src dst [vk_path]` does: delta <- delta d in section 2,
    every point of sections 8 and 9 <- d^-1 point; magic, version and sections 1, 3 to 7 and 10 byte for byte, sections
    1 to 10 in src's order.  src: path of a Groth16 BN254 .zkey; dst: path (written as dst + ".partial", renamed at the
    end; a failure leaves neither).  d: the secret, 0 < d < r; None draws it from `secrets` (the caller never sees it:
    that is the point of a contribution; pass d only in tests).  Section 10 is copied, not extended: the result is a sound
    proving key, not a verifiable ceremony transcript.  vk_path: the verification key with the new vk_delta_2, as JSON.
    Raises ValueError for a file that is not such a key or a d out of range, ZkHipError with the library's message (a point
    off the curve names its section and index)."""
    from . import lib as L
    from .binfile import BinFile, rewrite_mapped
    if d is None:
        d = 0
        while not 0 < d < R_MOD:
            d = secrets.randbits(254)
    d = int(d)
    if not 0 < d < R_MOD:
        raise ValueError("the contribution scalar must satisfy 0 < d < r")
    if os.path.exists(dst) and os.path.samefile(src, dst):
        raise ValueError("the input and the output are the same file")
    lib = L.load_library()
    with open(src, "rb") as fh:
        m_in = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
    raw = np.frombuffer(m_in, dtype=np.uint8)
    try:
        if bytes(raw[:4]) != b"zkey":
            raise ValueError("not a zkey file (magic %r)" % bytes(raw[:4]))
        try:
            f = BinFile(m_in, "zkey", 1)
        except struct.error:
            raise ValueError("zkey file is truncated") from None
        sections = {sid: lst[0] for sid, lst in f.sections.items()}
        for sid in range(1, 11):
            if sid not in sections:
                raise ValueError("zkey has no section %d" % sid)
            if sum(sections[sid]) > raw.size:
                raise ValueError("zkey file is truncated")
        try:
            h = load_zkey_header(f)
        except (IndexError, struct.error) as e:
            raise ValueError("zkey header: %s" % e) from None
        if h.qPrime != Q_MOD or h.rPrime != R_MOD:
            raise ValueError("zkey curve not supported (q and r are not BN254's)")
        want = _section_sizes(h)
        want[4] = 4 + 44 * struct.unpack_from("<I", m_in, sections[4][0])[0] if sections[4][1] >= 4 else 4
        for sid in sorted(want):
            if sections[sid][1] != want[sid]:
                raise ValueError("zkey section %d is %s: %d bytes, the header implies %d"
                                 % (sid, "short" if sections[sid][1] < want[sid] else "long", sections[sid][1], want[sid]))
        sec = lambda sid: raw[sections[sid][0]:sections[sid][0] + sections[sid][1]]
        s2 = sec(2)
        d1_at, d2_at = s2.size - 128 - 64, s2.size - 128          # delta1, delta2: the last two points of section 2
        zv = L.zk_zkey_contrib_view()
        zv.vk_delta1, zv.vk_delta2 = s2[d1_at:].ctypes.data, s2[d2_at:].ctypes.data
        for sid, name in ((8, "pointsC"), (9, "pointsH")):
            setattr(zv, name, sec(sid).ctypes.data if sections[sid][1] else None)
            setattr(zv, name + "_bytes", sections[sid][1])
        z = L.zk_zkey_contrib_sizes()
        L.check(lib.zk_zkey_contribute_sizes(C.byref(zv), C.byref(z)))
        order = sorted((sections[sid][0], sid) for sid in range(1, 11))
        secs = [(sid, sections[sid][1], None if sid in (8, 9) else sec(sid)) for _, sid in order]
        try:
            with rewrite_mapped(dst, raw[:8], secs) as (o, starts):
                where = {sid: at for (sid, _, _), at in zip(secs, starts)}
                out = L.zk_zkey_contrib_out()
                out.vk_delta1 = o[where[2] + d1_at:].ctypes.data
                out.vk_delta2 = o[where[2] + d2_at:].ctypes.data
                out.pointsC = o[where[8]:].ctypes.data if sections[8][1] else None
                out.pointsH = o[where[9]:].ctypes.data if sections[9][1] else None
                dd = np.frombuffer(d.to_bytes(32, "little"), dtype=np.uint8).copy()
                try:
                    L.check(lib.zk_zkey_contribute(C.byref(zv), C.c_void_p(dd.ctypes.data), device, C.byref(out)))
                finally:
                    dd[:] = 0
                if vk_path is not None:
                    vk = _vk_json(h, bytes(o[where[2] + d2_at:where[2] + d2_at + 128]), bytes(sec(3)))
                    with open(vk_path + ".partial", "w") as fv:
                        json.dump(vk, fv, indent=1)
                    os.replace(vk_path + ".partial", vk_path)
                del o
        except BaseException:
            if vk_path is not None and os.path.exists(vk_path + ".partial"):
                os.remove(vk_path + ".partial")
            raise
    finally:
        del raw
        try:
            m_in.close()
        except BufferError:
            pass
