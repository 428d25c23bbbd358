"""The PLONK prover and verifier on the GPU: five rounds chained on the device, the transcript, zk_plonk_verify.  Exact
arithmetic: with the blinds given a proof is compared BYTE FOR BYTE with the reference prover of
tests/plonk_prover_instance.py (Python integers, commitments at the known tau of a trapdoor file), so a case fails if any
round, blind or challenge is off; with drawn blinds proofs are checked by that file's pairing-free verifier and by
plonk_verify."""
import ctypes
import functools
import random

import numpy as np
import pytest

import plonk_instance as pi
import plonk_prover_instance as pp
from oracle import bn254 as bn

pytestmark = pytest.mark.gpu

R, Q = bn.R_MOD, bn.Q_MOD
TAU, ALPHA, BETA = 0x1F3A9C5E77D1B2A49E0C6F5D3B8A17264C9E0F1D2B3A4958, 0x2B7E151628AED2A6ABF7158809CF4F3C, 0x3243F6A8885A308D313198A2E0370734
MAX_COEFFS = (1 << 11) + 6
OK, INVALID, MALFORMED = 0, 1, 2
SEG_KNOBS = ("ZKHIP_QUOT_SEG", "ZKHIP_OPEN_SEG", "ZKHIP_SCAN_SEG")
GATES, COPIES = "zk_plonk_prove: the witness does not satisfy the gates", "zk_plonk_prove: the copy constraints do not hold"


def le(values):
    return np.frombuffer(pi.le(values), dtype=np.uint8)


@pytest.fixture(scope="module")
def kzg(zk, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("plonk_prover") / "p12.ptau")
    zk.write_trapdoor_ptau(12, TAU, ALPHA, BETA, path, prepared=False)
    k = zk.Kzg.from_ptau(path, max_coeffs=MAX_COEFFS)
    yield k
    k.close()


def blinds(seed):
    rng = random.Random(seed)
    return [rng.randrange(1, R) for _ in range(11)]


@functools.lru_cache(maxsize=None)
def case(seed, log_n, n_public=2, layout="plain", **kw):
    return pp.build(seed, log_n, n_public, layout, **kw)


@functools.lru_cache(maxsize=None)
def reference(seed, log_n, n_public=2, layout="plain", blind=None):
    """(case, reference proof), made once: blind None = blinds(seed)"""
    c = case(seed, log_n, n_public, layout)
    return c, pp.prove(c, blinds(seed) if blind is None else blind, TAU)


def prover(zk, kzg, c, basis="monomial"):
    return zk.PlonkProver(kzg, *[le(x) for x in c.inst.circuit(basis)], pi.K1, pi.K2, *c.maps, c.n_witness, c.n_public, basis=basis)


def set_segs(monkeypatch, seg):
    for name in SEG_KNOBS:
        if seg is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, seg)


# ---------------------------------------------------------------- byte for byte against the reference prover
@pytest.mark.parametrize("log_n", [3, 4, 6, 8, 11])      # 3: 3n + 6 = 30 meets 4n = 32; 8 and 11 cross the 256-lane and segment edges
def test_a_proof_is_the_reference_provers_byte_for_byte(zk, kzg, log_n):
    c, ref = reference(5000 + log_n, log_n)
    with prover(zk, kzg, c) as p:
        got = p.prove(c.witness, c.publics, blinds(5000 + log_n))
        assert got.to_bytes() == ref.to_bytes()
        assert got.evals == ref.evals and len(got.to_bytes()) == 768
        again = p.prove(c.witness, c.publics, blinds(5000 + log_n))       # the object's rows are reused: nothing is left behind
        assert again == got


@pytest.mark.parametrize("seg", ["1", "3", None])
@pytest.mark.parametrize("log_n", [3, 8, 11])
def test_bytes_do_not_depend_on_the_segments(zk, kzg, monkeypatch, log_n, seg):
    c, ref = reference(5000 + log_n, log_n)
    set_segs(monkeypatch, seg)
    with prover(zk, kzg, c) as p:
        assert p.prove(c.witness, c.publics, blinds(5000 + log_n)).to_bytes() == ref.to_bytes()
        info = p.info()
        assert [info[k] for k in ("quot_seg", "open_seg", "scan_seg")] == ([int(seg)] * 3 if seg else [16, 16, 8])


@pytest.mark.parametrize("log_n", [4, 6])
def test_the_lagrange_basis_gives_the_same_proof(zk, kzg, log_n):
    c, ref = reference(5000 + log_n, log_n)
    with prover(zk, kzg, c, "lagrange") as p:
        assert p.prove(c.witness, c.publics, blinds(5000 + log_n)).to_bytes() == ref.to_bytes()


@pytest.mark.parametrize("n_public", [0, 2, 16])
def test_the_number_of_public_inputs(zk, kzg, n_public):
    c, ref = reference(5100 + n_public, 4, n_public)
    assert len(c.publics) == n_public
    with prover(zk, kzg, c) as p:
        assert p.prove(c.witness, c.publics if n_public else None, blinds(5100 + n_public)).to_bytes() == ref.to_bytes()


def test_publics_default_to_the_witness_after_its_first_value(zk, kzg):
    c, ref = reference(5120, 4, 2, "circom")
    assert c.witness[0] == 1 and c.witness[1:3] == c.publics
    with prover(zk, kzg, c) as p:
        assert p.prove(c.witness, blind=blinds(5120)).to_bytes() == ref.to_bytes()


@pytest.mark.parametrize("log_n", [3, 4])
def test_all_blinds_zero_and_b1_zero_alone(zk, kzg, log_n):
    zero = (0,) * 11
    short = tuple([0] + blinds(5200 + log_n)[1:])        # a has n + 1 coefficients
    c, ref0 = reference(5200 + log_n, log_n, blind=zero)
    _, ref1 = reference(5200 + log_n, log_n, blind=short)
    assert ref0.to_bytes() != ref1.to_bytes()
    with prover(zk, kzg, c) as p:
        assert p.prove(c.witness, c.publics, list(zero)).to_bytes() == ref0.to_bytes()
        assert p.prove(c.witness, c.publics, list(short)).to_bytes() == ref1.to_bytes()


# ---------------------------------------------------------------- drawn blinds, the verifier
def test_drawn_blinds_give_different_proofs_that_verify(zk, kzg):
    c = case(5306, 6)
    vk_ref = pp.vkey_points(c.inst, TAU)
    with prover(zk, kzg, c) as p:
        one, two = p.prove(c.witness, c.publics), p.prove(c.witness, c.publics)
        vk = p.vkey()
        assert one != two and one.points[0] != two.points[0]
        for proof in (one, two):
            assert pp.verify(vk_ref, 6, c.publics, proof.to_bytes(), TAU) is True
            assert zk.plonk_verify(vk, proof, c.publics) == OK
            assert zk.plonk_verify(vk, proof.to_bytes(), le(c.publics)) == OK


def test_selfverify_checks_the_proof_before_it_is_returned(zk, kzg, monkeypatch):
    c, ref = reference(5003, 3)
    monkeypatch.setenv("ZKHIP_SELFVERIFY", "1")
    with prover(zk, kzg, c) as p:
        assert p.prove(c.witness, c.publics, blinds(5003)).to_bytes() == ref.to_bytes()


def test_verify_refuses_every_changed_field(zk, kzg):
    """One byte of each of the fifteen fields in turn.  A changed value is INVALID.  A changed byte of a point leaves the
    curve (MALFORMED: points are checked on the curve) unless the reference verifier says the bytes still name a point; so
    each point is ALSO replaced by another point of the curve, P + G, which must be INVALID."""
    c, ref = reference(5003, 3)
    vk_ref = pp.vkey_points(c.inst, TAU)
    good = ref.to_bytes()
    with prover(zk, kzg, c) as p:
        vk = p.vkey()
        assert zk.plonk_verify(vk, good, c.publics) == OK and pp.verify(vk_ref, 3, c.publics, good, TAU) is True
        for field in range(15):
            at = field * 64 + 5 if field < 9 else 576 + (field - 9) * 32 + 5
            bad = bytearray(good)
            bad[at] ^= 0x10
            want = pp.verify(vk_ref, 3, c.publics, bytes(bad), TAU)
            assert want is not True
            assert zk.plonk_verify(vk, bytes(bad), c.publics) == (MALFORMED if want is None else INVALID), field
            if field >= 9:
                assert want is False
        for field in range(9):
            moved = bn.G1.add(ref.points[field], bn.G1_GEN)
            bad = good[:field * 64] + bn.g1_to_bytes(moved) + good[(field + 1) * 64:]
            assert pp.verify(vk_ref, 3, c.publics, bad, TAU) is False
            assert zk.plonk_verify(vk, bad, c.publics) == INVALID, field
        assert zk.plonk_verify(vk, good, [c.publics[0], (c.publics[1] + 1) % R]) == INVALID
        assert zk.plonk_verify(vk, good, [c.publics[0], R]) == MALFORMED               # a public input not below r
        off = good[:64] + bn.g1_to_bytes((1, 3)) + good[128:]                          # (1, 3): 9 != 1 + 3
        assert zk.plonk_verify(vk, off, c.publics) == MALFORMED
        big = good[:96] + (Q).to_bytes(32, "little") + good[128:]                      # a coordinate that is not below q
        assert zk.plonk_verify(vk, big, c.publics) == MALFORMED
        for value in (R, (1 << 256) - 1):
            assert zk.plonk_verify(vk, good[:576 + 64] + value.to_bytes(32, "little") + good[576 + 96:], c.publics) == MALFORMED
        inf = good[:7 * 64] + bytes(64) + good[8 * 64:]                                # infinity is a point: INVALID, not MALFORMED
        assert zk.plonk_verify(vk, inf, c.publics) == INVALID and pp.verify(vk_ref, 3, c.publics, inf, TAU) is False


def test_verify_at_2_to_11_and_with_every_row_public(zk, kzg):
    for seed, log_n, n_public in ((5011, 11, 2), (5116, 4, 16)):
        c, ref = reference(seed, log_n, n_public)
        with prover(zk, kzg, c) as p:
            vk = p.vkey()
            assert zk.plonk_verify(vk, ref.to_bytes(), c.publics) == OK
            bad = list(c.publics)
            bad[-1] = (bad[-1] + 1) % R
            assert zk.plonk_verify(vk, ref.to_bytes(), bad) == INVALID


# ---------------------------------------------------------------- the key and info
def test_the_keys_commitments_are_kzg_commit_of_the_circuit(zk, kzg):
    c = case(5306, 6)
    with prover(zk, kzg, c, "lagrange") as p:
        vk = p.vkey()
        assert (vk.log_n, vk.n, vk.n_public, vk.k1, vk.k2) == (6, 64, 2, pi.K1, pi.K2)
        for name, got in vk.commitments.items():
            assert got == bytes(kzg.commit(le(getattr(c.inst, name)))), name
        assert list(vk.commitments) == ["qm", "ql", "qr", "qo", "qc", "s1", "s2", "s3"]
        assert bn.g2_from_bytes(vk.tau_g2) == bn.G2.mul(bn.G2_GEN, TAU)
        # a bad key is an error of the call, not a verdict
        bad = p.vkey()
        bad._c.qo[0] ^= 1
        with pytest.raises(zk.ZkHipError, match="zk_plonk_verify: a commitment of the key is not a point of the curve"):
            zk.plonk_verify(bad, bytes(768), [0, 0])
        bad = p.vkey()
        bad._c.tau_g2[0] ^= 1
        with pytest.raises(zk.ZkHipError, match="zk_plonk_verify: the key's \\[tau\\]G2 is not the kzg's"):
            zk.plonk_verify(bad, bytes(768), [0, 0])
        bad._c.size = 8
        with pytest.raises(zk.ZkHipError, match="zk_plonk_verify: vk->size is not sizeof\\(zk_plonk_vkey\\)"):
            zk.plonk_verify(bad, bytes(768), [0, 0])


def test_info_reports_the_launches_design_31_states(zk, kzg):
    """a round's launches are its own kernels', the existing cores' and its commitments'.  Round 4 is
    zk_plonk_evaluate's two; round 5 is zk_plonk_open's on the same lengths; rounds 1 to 3 hold 3 + 1 + 3 multiplications."""
    c, ref = reference(5006, 6)
    I, n = ref.inst, 64
    with prover(zk, kzg, c) as p:
        before = p.info()
        assert before["log_n"] == 6 and before["n_witness"] == c.n_witness and before["n_public"] == 2
        assert before["device_bytes"] >= (76 * n + 8 * n + 9 * MAX_COEFFS + 12 * n) * 32
        assert p.prove(c.witness, c.publics, blinds(5006)).to_bytes() == ref.to_bytes()
        info = p.info()
    pad = lambda v: le(list(v) + [0] * (n + 6 - len(v)))                           # noqa: E731
    kzg.commit(pad(I.a))
    msm = kzg.info()["last_launches"]
    with zk.PlonkOpening(kzg, *[le(x) for x in I.circuit()], pi.K1, pi.K2) as o:
        o.evaluate(pad(I.a), pad(I.b), pad(I.c), pad(I.z), ref.ch.zeta)
        ev = o.info()["last_launches"]
        o.open(le(ref.parts[0]), le(ref.parts[1]), le(ref.parts[2]), ref.ch.alpha, ref.ch.beta, ref.ch.gamma, ref.ch.v, pi_zeta=pi.horner(I.pi, ref.ch.zeta))
        op = o.info()["last_launches"]
    with zk.PlonkCircuit(*[le(x) for x in I.circuit()], pi.K1, pi.K2) as q:
        q.quotient(le(I.a), le(I.b), le(I.c), le(I.z), ref.ch.alpha, ref.ch.beta, ref.ch.gamma, pi=le(I.pi))
        quot = q.info()["last_launches"]
    # X, the launches of one transform of size n = 64, from an object of its own: a circuit of 16 rows transforms at 4 * 16 = 64, and
    # its quotient is a load, a batched transform, the quotient kernel, a transform back and a store
    J = pi.make(5016, 4, pi.BLIND)
    with zk.PlonkCircuit(*[le(x) for x in J.circuit()], pi.K1, pi.K2) as q:
        q.quotient(le(J.a), le(J.b), le(J.c), le(J.z), J.alpha, J.beta, J.gamma, pi=le(J.pi))
        small = q.info()["last_launches"]
    assert small > 3 and (small - 3) % 2 == 0
    ntt = (small - 3) // 2
    rounds = info["round_launches"]
    assert info["last_launches"] == sum(rounds)
    assert rounds[3] == ev == 2 and rounds[4] == op
    assert rounds[2] == quot + 1 + 3 * msm                   # the quotient, the split, three commitments
    assert rounds[1] == 3 + 1 + ntt + 1 + 1 + msm            # the scan's three, a load, a transform, a store, the blinding, [z]
    assert rounds[0] == 1 + 1 + ntt + 4 + 1 + 3 * msm        # the gather, a load, one batched transform, four stores, the blinding


# ---------------------------------------------------------------- refusals
def test_a_bad_witness_is_refused_and_no_proof_byte_is_written(zk, kzg):
    lib = zk.load_library()
    P = lambda a: ctypes.c_void_p(a.ctypes.data)       # noqa: E731
    broken = case(5404, 4, break_gate=3)
    assert pp.prove(broken, blinds(1), TAU) == GATES
    with prover(zk, kzg, broken) as p:
        with pytest.raises(zk.ZkHipError, match=GATES):
            p.prove(broken.witness, broken.publics, blinds(1))
        with pytest.raises(zk.ZkHipError, match=GATES):
            p.prove(broken.witness, broken.publics)
    c, ref = reference(5004, 4)
    # one cell of a copy cycle gets a witness value of its own: its copies keep theirs
    cells = list(c.maps[0]) + list(c.maps[1]) + list(c.maps[2])
    cell = next(i for i, ix in enumerate(cells) if cells.count(ix) > 1)
    cells[cell] = c.n_witness
    maps = (cells[:16], cells[16:32], cells[32:])
    witness = c.witness + [(c.witness[c.maps[cell // 16][cell % 16]] + 1) % R]
    with zk.PlonkProver(kzg, *[le(x) for x in c.inst.circuit()], pi.K1, pi.K2, *maps, c.n_witness + 1, 2) as p:
        with pytest.raises(zk.ZkHipError, match=COPIES):
            p.prove(witness, c.publics, blinds(5004))
        out = np.full(768, 0xAA, dtype=np.uint8)
        w, pub, bl = le(witness).copy(), le(c.publics).copy(), le(blinds(5004)).copy()
        assert lib.zk_plonk_prove(p._handle(), P(out), P(w), P(pub), P(bl)) == 1 and lib.zk_last_error().decode() == COPIES
        assert bytes(out) == b"\xaa" * 768
        good = c.witness + [c.witness[c.maps[cell // 16][cell % 16]]]                # the same maps, the copy restored
        assert p.prove(good, c.publics, blinds(5004)).to_bytes() == ref.to_bytes()
        w[32 * 3 + 31] = 0xFF
        assert lib.zk_plonk_prove(p._handle(), P(out), P(w), P(pub), P(bl)) == 1
        assert lib.zk_last_error().decode() == "zk_plonk_prove: witness 3 is not below r" and bytes(out) == b"\xaa" * 768


def test_refusals_of_creation(zk, kzg, tmp_path):
    from rapidsnark_old_amd import lib as L
    lib = zk.load_library()
    c = case(5003, 3)
    rows = [le(x).copy() for x in c.inst.circuit()]
    maps = [np.array(m, dtype=np.uint32) for m in c.maps]

    def create(log_n=3, n_witness=c.n_witness, n_public=2, k=None, device=-1, basis=0, swap=None, shift=None):
        v = L.zk_plonk_circuit_view()
        v.log_n, v.basis = log_n, basis
        bad = le([1, 2, R] + [0] * 5).copy()
        for name, a in zip(("ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3"), rows):
            setattr(v, name, (bad if name == swap else a).ctypes.data)
        ctypes.memmove(v.k1, pi.le([pi.K1]), 32)
        ctypes.memmove(v.k2, pi.le([pi.K2]), 32)
        sh = le([shift]).copy() if shift is not None else None
        v.shift = sh.ctypes.data if sh is not None else None
        h = ctypes.c_void_p()
        rc = lib.zk_plonk_prover_create(ctypes.byref(h), (k or kzg)._handle(), ctypes.byref(v), *[ctypes.c_void_p(m.ctypes.data) for m in maps], n_witness,
                                        n_public, device)
        assert rc == 1 and not h
        return lib.zk_last_error().decode()

    assert create(log_n=2) == "zk_plonk_prover_create: log_n 2 is outside 3 .. 25"
    assert create(log_n=26) == "zk_plonk_prover_create: log_n 26 is outside 3 .. 25"
    assert create(basis=7) == "zk_plonk_prover_create: basis 7 is unknown"
    assert create(log_n=12) == "zk_plonk_prover_create: n + 6 = 4102 exceeds the kzg's max_coeffs = 2054"
    assert create(n_public=9) == "zk_plonk_prover_create: n_public 9 exceeds n = 8"
    assert create(n_witness=0) == "zk_plonk_prover_create: n_witness is 0"
    assert create(device=77).startswith("zk_plonk_prover_create: device 77 is not the kzg's device ")
    top = max(int(m.max()) for m in maps)
    j, i = next((j, int(np.argmax(m == top))) for j, m in enumerate(maps) if (m == top).any())
    assert create(n_witness=top) == "zk_plonk_prover_create: %s %d is %d, not below n_witness = %d" % (("a_map", "b_map", "c_map")[j], i, top, top)
    assert create(swap="qo") == "zk_plonk_prover_create: qo 2 is not below r"
    assert create(shift=0) == "zk_plonk_prover_create: shift is zero"
    assert create(shift=bn.fr_root(5)) == "zk_plonk_prover_create: shift^(4n) is 1: Z_H vanishes on the coset"
    # Python's checks come before the library
    with pytest.raises(ValueError, match="log_n 2 is outside 3 .. 25"):
        zk.PlonkProver(kzg, *([[1, 2, 3, 4]] * 8), 2, 3, [0] * 4, [0] * 4, [0] * 4, 1)
    with pytest.raises(ValueError, match="b_map 1 is 99, not below n_witness = %d" % c.n_witness):
        zk.PlonkProver(kzg, *rows, 2, 3, c.maps[0], [0, 99] + [0] * 6, c.maps[2], c.n_witness, 2)
    small_path = str(tmp_path / "p4.ptau")
    zk.write_trapdoor_ptau(4, TAU, ALPHA, BETA, small_path, prepared=False)
    with zk.Kzg.from_ptau(small_path, max_coeffs=13) as small:
        assert create(k=small) == "zk_plonk_prover_create: n + 6 = 14 exceeds the kzg's max_coeffs = 13"
        with pytest.raises(ValueError, match="n \\+ 6 = 14 exceeds the kzg's max_coeffs = 13"):
            prover(zk, small, c)
        small.max_coeffs = 14                            # Python's view only: the library still refuses
        with pytest.raises(zk.ZkHipError, match="zk_plonk_prover_create: n \\+ 6 = 14 exceeds the kzg's max_coeffs = 13"):
            prover(zk, small, c)
    closed = zk.Kzg.from_ptau(small_path, max_coeffs=14)
    p = prover(zk, closed, c)
    closed.close()
    with pytest.raises(zk.ZkHipError, match="the Kzg object is closed"):
        prover(zk, closed, c)
    with pytest.raises(zk.ZkHipError, match="the Kzg object is closed"):
        p.prove(c.witness, c.publics)
    p.close()
    p.close()
    with pytest.raises(zk.ZkHipError, match="the PlonkProver object is closed"):
        p.info()


def test_a_bad_knob_is_an_error_of_the_call(zk, kzg, monkeypatch):
    c, ref = reference(5003, 3)
    with prover(zk, kzg, c) as p:
        monkeypatch.setenv("ZKHIP_OPEN_SEG", "0")
        with pytest.raises(zk.ZkHipError, match="ZKHIP_OPEN_SEG: a number of coefficients per lane from 1 to 4096 expected"):
            p.prove(c.witness, c.publics, blinds(5003))
        monkeypatch.delenv("ZKHIP_OPEN_SEG")
        assert p.prove(c.witness, c.publics, blinds(5003)).to_bytes() == ref.to_bytes()
