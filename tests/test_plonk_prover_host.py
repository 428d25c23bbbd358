"""The PLONK prover and verifier without a device: zk_keccak256 against the known answers and a second implementation; the
header declares the entries with their exact prototypes and states the transcript and the refusals; every export is bound
and re-exported; the refusals that need no device carry the header's text; and the reference prover of
tests/plonk_prover_instance.py, which the device tests compare with byte for byte, makes proofs its own pairing-free
verifier accepts and refuses once a value is changed."""
import ctypes
import json
import os
import random
import re

import numpy as np
import pytest

import plonk_instance as pi
import plonk_prover_instance as pp
from oracle import bn254 as bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkhip.h")
ENTRIES = {"zk_keccak256": 3, "zk_plonk_prover_create": 9, "zk_plonk_prover_destroy": 1, "zk_plonk_prover_vkey": 2, "zk_plonk_prover_info": 2,
           "zk_plonk_prove": 5, "zk_plonk_verify": 5}
R = pi.R
TAU = 0x1F3A9C5E77D1B2A49E0C6F5D3B8A17264C9E0F1D2B3A4958
EMPTY = "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
ABC = "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"


# ---------------------------------------------------------------- Keccak-256
def test_keccak256_known_answers():
    import rapidsnark_old_amd as zk
    assert zk.keccak256(b"").hex() == EMPTY and zk.keccak256(b"abc").hex() == ABC
    assert pp.keccak256(b"").hex() == EMPTY and pp.keccak256(b"abc").hex() == ABC


@pytest.mark.parametrize("n", [0, 1, 135, 136, 137, 272])      # the rate is 136 bytes: an empty, a full and a second block
def test_keccak256_agrees_with_the_python_one(n):
    import rapidsnark_old_amd as zk
    rng = random.Random(6000 + n)
    data = bytes(rng.randrange(256) for _ in range(n))
    assert zk.keccak256(data) == pp.keccak256(data)
    assert zk.keccak256(bytearray(data)) == pp.keccak256(data)


def test_keccak256_c_entry():
    from rapidsnark_old_amd import lib as L
    lib = L.load_library()
    out = np.zeros(32, dtype=np.uint8)
    assert lib.zk_keccak256(ctypes.c_void_p(out.ctypes.data), None, 0) == 0 and out.tobytes().hex() == EMPTY
    assert lib.zk_keccak256(None, None, 0) == 1 and lib.zk_last_error().decode() == "null argument"
    assert lib.zk_keccak256(ctypes.c_void_p(out.ctypes.data), None, 3) == 1 and lib.zk_last_error().decode() == "null argument"


# ---------------------------------------------------------------- header and binding
def test_header_declares_the_entries():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    for decl in ("int zk_keccak256(uint8_t out32[32], const uint8_t *data, uint64_t len);",
                 "typedef struct zk_plonk_prover zk_plonk_prover;",
                 "int zk_plonk_prover_create(zk_plonk_prover **out, zk_kzg *kzg, const zk_plonk_circuit_view *view, const uint32_t *a_map, "
                 "const uint32_t *b_map, const uint32_t *c_map, uint64_t n_witness, uint64_t n_public, int32_t device);",
                 "void zk_plonk_prover_destroy(zk_plonk_prover *p);",
                 "int zk_plonk_prover_vkey(zk_plonk_prover *p, zk_plonk_vkey *vk);",
                 "int zk_plonk_prover_info(zk_plonk_prover *p, zk_plonk_prover_plan *plan);",
                 "int zk_plonk_prove(zk_plonk_prover *p, uint8_t proof[ZK_PLONK_PROOF_BYTES], const uint8_t *witness, const uint8_t *publics, "
                 "const uint8_t *blind);",
                 "int zk_plonk_verify(zk_kzg *kzg, const zk_plonk_vkey *vk, const uint8_t proof[ZK_PLONK_PROOF_BYTES], const uint8_t *publics, "
                 "uint8_t *verdict);",
                 "#define ZK_PLONK_PROOF_BYTES 768", "#define ZK_PLONK_BLINDS 11"):
        assert decl in flat, decl
    section = text[text.index("PLONK prover and verifier"):]
    for words in ("ORIGINAL padding byte 0x01", "not SHA-3's 0x06", "32 bytes BIG-endian, standard form", "infinity as 64 zero bytes",
                  "big-endian integer, reduced mod r", "parity with snarkjs is UNPINNED",
                  "beta  = H([qM], [qL], [qR], [qO], [qC], [s1], [s2], [s3], publics[0 .. n_public), [a], [b], [c])", "gamma = H(beta)",
                  "alpha = H(beta, gamma, [z])", "zeta  = H(alpha, [t_lo], [t_mid], [t_hi])", "v     = H(zeta, a', b', c', s1', s2', z'w)",
                  "u     = H([W_zeta], [W_zeta_omega])", "c5d24601 86f7233c", "4e03657a ea45a94f",
                  "a += (b1 X + b2) Z_H", "z += (b7 X^2 + b8 X + b9) Z_H", "t_lo + b10 X^n,  t_mid - b10 + b11 X^n,  t_hi - b11",
                  "zk_plonk_prover_create: log_n 2 is outside 3 .. 25", "exceeds the kzg's max_coeffs =", "is 12, not below n_witness = 12",
                  "zk_plonk_prover_create: qm 5 is not below r", "zk_plonk_prove: witness 5 is not below r",
                  "zk_plonk_prove: the copy constraints do not hold", "zk_plonk_prove: the witness does not satisfy the gates", "NO proof byte is written",
                  "zk_plonk_verify: the key's [tau]G2 is not the kzg's", "E  = (r0 + v a' + v^2 b' + v^3 c' + v^4 s1' + v^5 s2' + u z'w) [1]",
                  "e(W_zeta + u W_zeta_omega, [tau]G2) = e(zeta W_zeta + u zeta w W_zeta_omega + F - E, G2)"):
        assert words in section, words


def test_every_export_is_bound_and_re_exported():
    from rapidsnark_old_amd import lib as L
    import rapidsnark_old_amd as zk
    lib = L.load_library()
    for name, nargs in ENTRIES.items():
        assert name in L.EXPORTS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert ctypes.sizeof(L.zk_plonk_vkey) == 4 + 4 + 8 + 64 + 8 * 64 + 128 and ctypes.sizeof(L.zk_plonk_prover_plan) == 72
    assert L.zk_plonk_vkey.tau_g2.offset == 592 and L.zk_plonk_prover_plan.round_launches.offset == 52
    for name in ("PlonkProver", "PlonkProof", "PlonkVKey", "plonk_verify", "keccak256"):
        assert getattr(zk, name) is getattr(zk.plonk, name), name
    assert zk.plonk.PROOF_BYTES == pp.PROOF_BYTES == 768 and zk.plonk.Q_MOD == bn.Q_MOD


def test_c_entries_refuse_bad_arguments_before_a_device_is_touched():
    from rapidsnark_old_amd import lib as L
    lib = L.load_library()
    P = lambda a: ctypes.c_void_p(a.ctypes.data)       # noqa: E731
    h = ctypes.c_void_p()
    v = L.zk_plonk_circuit_view()
    m = np.zeros(8, dtype=np.uint32)
    assert lib.zk_plonk_prover_create(ctypes.byref(h), None, ctypes.byref(v), P(m), P(m), P(m), 1, 0, -1) == 1
    assert lib.zk_last_error().decode() == "null argument" and not h
    assert lib.zk_plonk_prover_create(None, None, None, None, None, None, 1, 0, -1) == 1 and lib.zk_last_error().decode() == "null argument"
    buf = np.zeros(768, dtype=np.uint8)
    assert lib.zk_plonk_prove(None, P(buf), P(buf), P(buf), None) == 1 and lib.zk_last_error().decode() == "null argument"
    vk = L.zk_plonk_vkey()
    assert lib.zk_plonk_prover_vkey(None, ctypes.byref(vk)) == 1 and lib.zk_last_error().decode() == "null argument"
    plan = L.zk_plonk_prover_plan()
    assert lib.zk_plonk_prover_info(None, ctypes.byref(plan)) == 1 and lib.zk_last_error().decode() == "null argument"
    verdict = np.zeros(1, dtype=np.uint8)
    assert lib.zk_plonk_verify(None, ctypes.byref(vk), P(buf), None, P(verdict)) == 1 and lib.zk_last_error().decode() == "null argument"
    lib.zk_plonk_prover_destroy(None)


def test_python_refuses_bad_arguments_before_any_library_call(monkeypatch):
    from rapidsnark_old_amd import lib as L, plonk as P, kzg as K

    def never(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(L, "load_library", never)
    q = [1, 2, 3, 4, 5, 6, 7, 8]
    ok, m = [q] * 8, [0] * 8
    with pytest.raises(TypeError, match="a Kzg expected"):
        P.PlonkProver(None, *ok, 2, 3, m, m, m, 1)
    k = K.Kzg.__new__(K.Kzg)                            # never made on a device: the checks that come first still answer
    k.max_coeffs, k.device, k._h = 13, 0, None
    with pytest.raises(ValueError, match="basis 'evaluation' is unknown"):
        P.PlonkProver(k, *ok, 2, 3, m, m, m, 1, basis="evaluation")
    with pytest.raises(ValueError, match="qo has 16 rows, ql has 8"):
        P.PlonkProver(k, q, q, q, q * 2, q, q, q, q, 2, 3, m, m, m, 1)
    with pytest.raises(ValueError, match="log_n 2 is outside 3 .. 25"):
        P.PlonkProver(k, *([q[:4]] * 8), 2, 3, m[:4], m[:4], m[:4], 1)
    with pytest.raises(ValueError, match="s2: value 2 is not in 0 .. r - 1"):
        P.PlonkProver(k, q, q, q, q, q, q, [1, 2, R, 4, 5, 6, 7, 8], q, 2, 3, m, m, m, 1)
    with pytest.raises(ValueError, match="shift is zero"):
        P.PlonkProver(k, *ok, 2, 3, m, m, m, 1, shift=0)
    with pytest.raises(ValueError, match="shift\\^\\(4n\\) is 1"):
        P.PlonkProver(k, *ok, 2, 3, m, m, m, 1, shift=bn.fr_root(5))
    with pytest.raises(ValueError, match="n \\+ 6 = 14 exceeds the kzg's max_coeffs = 13"):
        P.PlonkProver(k, *ok, 2, 3, m, m, m, 1)
    k.max_coeffs = 14
    with pytest.raises(ValueError, match="n_witness is 0"):
        P.PlonkProver(k, *ok, 2, 3, m, m, m, 0)
    with pytest.raises(ValueError, match="n_public 9 is outside 0 .. n = 8"):
        P.PlonkProver(k, *ok, 2, 3, m, m, m, 1, 9)
    with pytest.raises(ValueError, match="c_map has 7 indices, n = 8 expected"):
        P.PlonkProver(k, *ok, 2, 3, m, m, m[:7], 1)
    with pytest.raises(ValueError, match="b_map 5 is 12, not below n_witness = 12"):
        P.PlonkProver(k, *ok, 2, 3, m, [0, 1, 2, 3, 4, 12, 13, 0], m, 12)
    with pytest.raises(ValueError, match="a_map 0 is -1, not below n_witness = 12"):
        P.PlonkProver(k, *ok, 2, 3, [-1] + m[1:], m, m, 12)
    with pytest.raises(L.ZkHipError, match="the Kzg object is closed"):
        P.PlonkProver(k, *ok, 2, 3, m, m, m, 12)
    p = P.PlonkProver.__new__(P.PlonkProver)
    p.kzg, p.n, p.log_n, p.n_witness, p.n_public, p._h = k, 8, 3, 4, 2, None
    with pytest.raises(ValueError, match="witness: 3 values, n_witness = 4 expected"):
        p.prove([1, 2, 3])
    with pytest.raises(ValueError, match="witness: value 1 is not in 0 .. r - 1"):
        p.prove([1, R, 3, 4])
    with pytest.raises(ValueError, match="publics: 1 values, n_public = 2 expected"):
        p.prove([1, 2, 3, 4], [5])
    with pytest.raises(ValueError, match="blind: 10 values, 11 expected"):
        p.prove([1, 2, 3, 4], blind=[0] * 10)
    with pytest.raises(ValueError, match="blind: value 10 is not in 0 .. r - 1"):
        p.prove([1, 2, 3, 4], blind=[0] * 10 + [R])
    with pytest.raises(L.ZkHipError, match="the PlonkProver object is closed"):
        p.prove([1, 2, 3, 4])
    p.n_witness = 2
    with pytest.raises(ValueError, match="publics: the witness has no 2 values after its first"):
        p.prove([1, 2])
    for call in (p.vkey, p.info):
        with pytest.raises(L.ZkHipError, match="the PlonkProver object is closed"):
            call()
    with pytest.raises(ValueError, match="a proof of 768 bytes expected, got 767"):
        P.PlonkProof(bytes(767))
    with pytest.raises(TypeError, match="a PlonkVKey expected"):
        P.plonk_verify(None, bytes(768), [])
    vk = P.PlonkVKey(k, L.zk_plonk_vkey())
    vk._c.n_public = 2
    with pytest.raises(ValueError, match="publics: 1 values, n_public = 2 expected"):
        P.plonk_verify(vk, bytes(768), [1])
    with pytest.raises(L.ZkHipError, match="the Kzg object is closed"):
        P.plonk_verify(vk, bytes(768), [1, R])             # a value that is not below r is the library's to refuse


def test_proof_json_has_snarkjs_fields():
    from rapidsnark_old_amd import plonk as P
    c = pp.build(6103, 3)
    ref = pp.prove(c, list(range(1, 12)), TAU)
    proof = P.PlonkProof(ref.to_bytes())
    d = json.loads(proof.to_json())
    assert list(d) == ["A", "B", "C", "Z", "T1", "T2", "T3", "Wxi", "Wxiw", "eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw", "protocol", "curve"]
    assert d["protocol"] == "plonk" and d["curve"] == "bn128"
    for name, pt in zip(("A", "B", "C", "Z", "T1", "T2", "T3", "Wxi", "Wxiw"), ref.points):
        assert d[name] == [str(pt[0]), str(pt[1]), "1"], name
    assert [int(d[k]) for k in ("eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw")] == ref.evals == proof.evals
    assert proof.to_bytes() == ref.to_bytes() and proof == P.PlonkProof(bytearray(ref.to_bytes()))
    assert json.loads(P.PlonkProof(bytes(768)).to_json())["A"] == ["0", "1", "0"]


# ---------------------------------------------------------------- the reference prover and verifier
def test_the_builder_deduplicates_and_shuffles():
    for layout in ("plain", "circom"):
        c = pp.build(6203, 3, 2, layout)
        I = c.inst
        cells = I.a_v + I.b_v + I.c_v
        assert c.n_witness == len(c.witness) < 24 + (3 if layout == "circom" else 0)
        for j, (m, v) in enumerate(zip(c.maps, (I.a_v, I.b_v, I.c_v))):
            assert [c.witness[i] for i in m] == v, j
        used = set(c.maps[0]) | set(c.maps[1]) | set(c.maps[2])
        assert c.n_witness - 1 in used and len(used) == len(set(cells))
        if layout == "plain":
            assert 0 in used and c.witness != sorted(c.witness)
        else:
            assert c.witness[0] == 1 and c.witness[1:3] == c.publics
        assert c.publics == [(R - v) % R for v in bn.ntt(I.pi)[:2]]


@pytest.mark.parametrize("blind", ["random", "zero"])
@pytest.mark.parametrize("n_public", [0, 2])
@pytest.mark.parametrize("log_n", [3, 4])
def test_the_reference_prover_passes_the_reference_verifier(log_n, n_public, blind):
    c = pp.build(6300 + log_n, log_n, n_public)
    rng = random.Random(6300 + log_n)
    b = [rng.randrange(1, R) for _ in range(11)] if blind == "random" else [0] * 11
    proof = pp.prove(c, b, TAU)
    vk = pp.vkey_points(c.inst, TAU)
    raw = proof.to_bytes()
    assert len(raw) == 768 and pp.verify(vk, log_n, c.publics, raw, TAU) is True
    assert [len(p) for p in proof.parts[:2]] == [c.inst.n + 1] * 2 and len(proof.parts[2]) <= c.inst.n + 6
    for j in range(6):                                   # one value changed
        bad = bytearray(raw)
        bad[576 + j * 32] ^= 1
        assert pp.verify(vk, log_n, c.publics, bytes(bad), TAU) is False, j
    if n_public:
        assert pp.verify(vk, log_n, [c.publics[0], (c.publics[1] + 1) % R], raw, TAU) is False
    other = bn.G1.add(proof.points[3], bn.G1_GEN)
    assert pp.verify(vk, log_n, c.publics, raw[:192] + bn.g1_to_bytes(other) + raw[256:], TAU) is False
    assert pp.verify(vk, log_n, c.publics, raw[:64] + bn.g1_to_bytes((1, 3)) + raw[128:], TAU) is None
    assert pp.verify(vk, log_n, c.publics, raw[:576] + R.to_bytes(32, "little") + raw[608:], TAU) is None


def test_the_reference_prover_refuses_a_broken_gate():
    c = pp.build(6404, 4, break_gate=3)
    assert pp.prove(c, list(range(11)), TAU) == "zk_plonk_prove: the witness does not satisfy the gates"
