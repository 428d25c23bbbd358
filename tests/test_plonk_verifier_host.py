"""The PLONK verifier object and the key file without a device: the header declares the new entries with their exact
prototypes and says what the key file is; every export is bound and re-exported; a key made from parts goes through
to_json / from_json unchanged and has snarkjs's field names; the reader honours a third coordinate and refuses a wrong w,
another protocol and another curve by name; and the C entries refuse null and bad arguments before a device is touched."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import plonk_instance as pi
import plonk_prover_instance as pp
from conftest import ROOT
from oracle import bn254 as bn

HEADER = os.path.join(ROOT, "include", "zkhip.h")
ENTRIES = {"zk_plonk_verifier_create": 3, "zk_plonk_verifier_destroy": 1, "zk_plonk_verifier_info": 2, "zk_plonk_verifier_verify": 5,
           "zk_plonk_verifier_challenges": 6}
R, Q = bn.R_MOD, bn.Q_MOD
TAU = 0x1F3A9C5E77D1B2A49E0C6F5D3B8A17264C9E0F1D2B3A4958
FIELDS = ["protocol", "curve", "nPublic", "power", "k1", "k2", "Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3", "X_2", "w"]


def test_header_declares_the_entries():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    for decl in ("typedef struct zk_plonk_verifier zk_plonk_verifier;",
                 "int zk_plonk_verifier_create(zk_plonk_verifier **out, const zk_plonk_vkey *vk, int32_t device);",
                 "void zk_plonk_verifier_destroy(zk_plonk_verifier *v);",
                 "int zk_plonk_verifier_info(zk_plonk_verifier *v, zk_plonk_verifier_plan *plan);",
                 "int zk_plonk_verifier_verify(zk_plonk_verifier *v, const uint8_t *proofs, const uint8_t *publics, uint64_t m, uint8_t *verdict);",
                 "int zk_plonk_verifier_challenges(zk_plonk_verifier *v, const uint8_t *proofs, const uint8_t *publics, uint64_t m, "
                 "uint8_t *challenges, uint8_t *status);",
                 "int zk_plonk_verify(zk_kzg *kzg, const zk_plonk_vkey *vk, const uint8_t proof[ZK_PLONK_PROOF_BYTES], const uint8_t *publics, "
                 "uint8_t *verdict);"):
        assert decl in flat, decl
    section = text[text.index("PLONK prover and verifier"):text.index("PLONK from an R1CS")]
    for words in ("no zk_kzg and no .ptau", "zk_plonk_verifier_create: vk->size is not sizeof(zk_plonk_vkey)",
                  "zk_plonk_verifier_create: log_n 2 is outside 3 .. 25", "zk_plonk_verifier_create: n_public 9 exceeds n = 8",
                  "zk_plonk_verifier_create: k1 is not below r", "zk_plonk_verifier_create: a commitment of the key is not a point of the curve",
                  "zk_plonk_verifier_create: the key's [tau]G2 is not a point of the twist in the subgroup",
                  "Free HBM is checked before anything is allocated", "Calls on one object are serialised",
                  "zk_plonk_verifier_verify: m is not below", "ZKHIP_PLONK_VERIFY_CHUNK: a number of proofs from 1 to 2^20 expected",
                  "changes no verdict", "m = 0 is legal", "status[i] = 0, or ZK_VERIFY_MALFORMED with the row left all zero",
                  "Qm Ql Qr Qo Qc S1 S2 S3", "X_2, w", "parity with snarkjs is UNPINNED", "not promised to verify"):
        assert words in section, words


def test_every_export_is_bound_and_re_exported():
    from rapidsnark_old_amd import lib as L
    import rapidsnark_old_amd as zk
    lib = L.load_library()
    for name, nargs in ENTRIES.items():
        assert name in L.EXPORTS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert lib.zk_plonk_verifier_destroy.restype is None
    assert ctypes.sizeof(L.zk_plonk_verifier_plan) == 40 and L.zk_plonk_verifier_plan.last_chunks.offset == 36
    assert [n for n, _ in L.zk_plonk_verifier_plan._fields_] == ["size", "log_n", "n_public", "device_bytes", "chunk", "last_launches", "last_chunks"]
    assert zk.PlonkVerifier is zk.plonk.PlonkVerifier and zk.PlonkVKey is zk.plonk.PlonkVKey
    for name in ("to_json", "from_json", "from_parts"):
        assert hasattr(zk.PlonkVKey, name), name
    for name in ("verify", "challenges", "info", "close", "__enter__", "__exit__"):
        assert hasattr(zk.PlonkVerifier, name), name
    assert zk.plonk.root_of_unity(28) == bn.ROOT_2_28 and zk.plonk.root_of_unity(4) == bn.fr_root(4)


def key_parts():
    """the commitments of a small circuit at a known tau, one slot at infinity"""
    c = pp.build(6103, 3)
    pts = pp.vkey_points(c.inst, TAU)
    pts[4] = None
    return pts, bn.G2.mul(bn.G2_GEN, TAU)


def test_a_key_from_parts_round_trips_through_json():
    import rapidsnark_old_amd as zk
    pts, tau_g2 = key_parts()
    vk = zk.PlonkVKey.from_parts(3, 2, pi.K1, pi.K2, pts, tau_g2)
    assert vk.kzg is None and (vk.log_n, vk.n, vk.n_public, vk.k1, vk.k2) == (3, 8, 2, pi.K1, pi.K2)
    assert list(vk.commitments.values()) == [bn.g1_to_bytes(P) for P in pts] and vk.tau_g2 == bn.g2_to_bytes(tau_g2)
    text = vk.to_json()
    d = json.loads(text)
    assert list(d) == FIELDS
    assert (d["protocol"], d["curve"], d["nPublic"], d["power"], d["k1"], d["k2"]) == ("plonk", "bn128", 2, 3, str(pi.K1), str(pi.K2))
    assert d["w"] == str(bn.fr_root(3))
    for name, P in zip(FIELDS[6:14], pts):
        assert d[name] == (["0", "1", "0"] if P is None else [str(P[0]), str(P[1]), "1"]), name
    (xa, xb), (ya, yb) = tau_g2
    assert d["X_2"] == [[str(xa), str(xb)], [str(ya), str(yb)], ["1", "0"]]
    back = zk.PlonkVKey.from_json(text)
    assert bytes(back._c) == bytes(vk._c) and back.kzg is None and back.to_json() == text
    by_name = zk.PlonkVKey.from_parts(3, 2, pi.K1, pi.K2, dict(zip(("qm", "ql", "qr", "qo", "qc", "s1", "s2", "s3"), pts)), bn.g2_to_bytes(tau_g2))
    assert bytes(by_name._c) == bytes(vk._c)
    with pytest.raises(ValueError, match="commitments: 7 points, 8 expected"):
        zk.PlonkVKey.from_parts(3, 2, pi.K1, pi.K2, pts[:7], tau_g2)
    with pytest.raises(ValueError, match="the key names no Kzg .*PlonkVerifier"):
        zk.plonk_verify(back, bytes(768), [1, 2])


def test_the_reader_honours_a_third_coordinate_and_refuses_by_name():
    import rapidsnark_old_amd as zk
    pts, tau_g2 = key_parts()
    vk = zk.PlonkVKey.from_parts(3, 2, pi.K1, pi.K2, pts, tau_g2)
    d = json.loads(vk.to_json())
    # z = 7 in G1, z = 3 + 5 u in G2: x and y are divided by it; bare numbers are read as strings are
    z = 7
    x, y = pts[1]
    d["Ql"] = [str(x * z % Q), str(y * z % Q), str(z)]
    d["Qr"] = [int(v) for v in d["Qr"]]
    za, zb = 3, 5
    mul2 = lambda a, b: ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)     # noqa: E731
    d["X_2"] = [[str(v) for v in mul2(tau_g2[0], (za, zb))], [str(v) for v in mul2(tau_g2[1], (za, zb))], [str(za), str(zb)]]
    d["Qo"] = [str(pts[3][0]), str(pts[3][1])]           # no third coordinate: affine
    d["vk_extra"] = "ignored"
    assert bytes(zk.PlonkVKey.from_json(json.dumps(d))._c) == bytes(vk._c)
    d["S2"] = ["5", "6", "0"]                            # z = 0: infinity
    assert zk.PlonkVKey.from_json(json.dumps(d)).commitments["s2"] == bytes(64)
    d["S2"] = [str(Q), "6", "1"]                         # not below q: passed as written, for the library to refuse
    assert zk.PlonkVKey.from_json(json.dumps(d)).commitments["s2"][:32] == Q.to_bytes(32, "little")

    def refused(change, text):
        e = json.loads(vk.to_json())
        change(e)
        with pytest.raises(ValueError, match=text):
            zk.PlonkVKey.from_json(json.dumps(e))

    refused(lambda e: e.update(w=str(bn.fr_root(4))), "^w is not this library's root of unity for power 3$")
    refused(lambda e: e.update(w="1"), "^w is not this library's root of unity for power 3$")
    refused(lambda e: e.update(power=4), "^w is not this library's root of unity for power 4$")
    refused(lambda e: e.update(power=29), "^power 29 is outside 0 .. 28$")
    refused(lambda e: e.update(protocol="groth16"), "^protocol \"groth16\" is not plonk$")
    refused(lambda e: e.update(curve="bls12381"), "^curve \"bls12381\" is not bn128$")
    refused(lambda e: e.pop("S3"), "^the key has no \"S3\"$")
    refused(lambda e: e.update(Qm=["1"]), "^Qm is not an array of at least 2 elements$")
    refused(lambda e: e.update(k1="12x"), "^k1 is not a decimal integer below 2\\^256$")
    with pytest.raises(ValueError, match="the key is not JSON"):
        zk.PlonkVKey.from_json("{")
    e = json.loads(vk.to_json())
    e["curve"] = "bn254"
    assert bytes(zk.PlonkVKey.from_json(json.dumps(e))._c) == bytes(vk._c)


def test_c_entries_refuse_bad_arguments_before_a_device_is_touched():
    import rapidsnark_old_amd as zk
    from rapidsnark_old_amd import lib as L
    lib = L.load_library()
    P = lambda a: ctypes.c_void_p(a.ctypes.data)         # noqa: E731
    pts, tau_g2 = key_parts()
    h = ctypes.c_void_p()

    def create(vk):
        assert lib.zk_plonk_verifier_create(ctypes.byref(h), ctypes.byref(vk._c) if vk is not None else None, -1) == 1 and not h
        return lib.zk_last_error().decode()

    good = lambda **kw: zk.PlonkVKey.from_parts(kw.get("log_n", 3), kw.get("n_public", 2), kw.get("k1", pi.K1), kw.get("k2", pi.K2), kw.get("pts", pts), tau_g2)   # noqa: E731
    assert create(None) == "null argument"
    assert lib.zk_plonk_verifier_create(None, ctypes.byref(good()._c), -1) == 1 and lib.zk_last_error().decode() == "null argument"
    short = good()
    short._c.size = 8
    assert create(short) == "zk_plonk_verifier_create: vk->size is not sizeof(zk_plonk_vkey)"
    assert create(good(log_n=2)) == "zk_plonk_verifier_create: log_n 2 is outside 3 .. 25"
    assert create(good(log_n=26)) == "zk_plonk_verifier_create: log_n 26 is outside 3 .. 25"
    assert create(good(n_public=9)) == "zk_plonk_verifier_create: n_public 9 exceeds n = 8"
    assert create(good(k1=R)) == "zk_plonk_verifier_create: k1 is not below r"
    assert create(good(k2=(1 << 256) - 1)) == "zk_plonk_verifier_create: k2 is not below r"
    assert create(good(pts=pts[:6] + [(1, 3)] + pts[7:])) == "zk_plonk_verifier_create: a commitment of the key is not a point of the curve"
    assert create(good(pts=[(Q, 2)] + pts[1:])) == "zk_plonk_verifier_create: a commitment of the key is not a point of the curve"
    buf, out = np.zeros(768, dtype=np.uint8), np.zeros(192, dtype=np.uint8)
    assert lib.zk_plonk_verifier_verify(None, P(buf), P(buf), 1, P(out)) == 1 and lib.zk_last_error().decode() == "null argument"
    assert lib.zk_plonk_verifier_challenges(None, P(buf), P(buf), 1, P(out), P(out)) == 1 and lib.zk_last_error().decode() == "null argument"
    plan = L.zk_plonk_verifier_plan()
    assert lib.zk_plonk_verifier_info(None, ctypes.byref(plan)) == 1 and lib.zk_last_error().decode() == "null argument"
    lib.zk_plonk_verifier_destroy(None)
    with pytest.raises(TypeError, match="a PlonkVKey expected"):
        zk.PlonkVerifier(bytes(768))
