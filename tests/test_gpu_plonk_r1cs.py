"""PLONK from an R1CS on the GPU: the compile of a circom .r1cs (gates, maps, sigma), the extension of a witness and the
prover made from the compiled circuit.  Exact arithmetic: the eight vectors, the three maps and the extended witness are
compared BYTE FOR BYTE with the Python compile of tests/plonk_r1cs_instance.py (written from the header's layout, and shown
sound without a device by tests/test_plonk_r1cs_host.py), and a proof with given blinds with the existing prover's proof over
that Python compile."""
import ctypes
import random

import numpy as np
import pytest

import plonk_instance as pi
import plonk_r1cs_instance as pr
from oracle import bn254 as bn

pytestmark = pytest.mark.gpu

R = bn.R_MOD
TAU, ALPHA, BETA = 0x1F3A9C5E77D1B2A49E0C6F5D3B8A17264C9E0F1D2B3A4958, 0x2B7E151628AED2A6ABF7158809CF4F3C, 0x3243F6A8885A308D313198A2E0370734
MAX_COEFFS = (1 << 8) + 6
OK = 0
GATES, COPIES = "the witness does not satisfy the gates", "the copy constraints do not hold"
SEG_TEXT = "ZKHIP_R1CS_SEG: a number of elements per lane from 1 to 4096 expected"
PROOF_SHAPES = ["proof_3", "proof_4", "proof_6", "proof_8"]


def le(values):
    return np.frombuffer(pi.le(values), dtype=np.uint8)


@pytest.fixture(scope="module")
def kzg(zk, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("plonk_r1cs") / "p12.ptau")
    zk.write_trapdoor_ptau(12, TAU, ALPHA, BETA, path, prepared=False)
    k = zk.Kzg.from_ptau(path, max_coeffs=MAX_COEFFS)
    yield k
    k.close()


def blinds(seed):
    rng = random.Random(seed)
    return [rng.randrange(1, R) for _ in range(11)]


def reference(name):
    c = pr.case(name)
    return c, pr.compile_r1cs(c.data)


def assert_same_circuit(got, k):
    assert (got.log_n, got.n, got.rows, got.n_public, got.n_wires, got.n_additions, got.n_witness) == \
           (k.log_n, k.n, k.rows, k.n_public, k.n_wires, k.n_additions, k.n_witness)
    for name, mine, ref in zip(("a_map", "b_map", "c_map"), got.maps, k.maps):
        assert mine.dtype == np.uint32 and np.array_equal(mine, np.asarray(ref, dtype=np.uint32)), name
    for name, mine, ref in zip(("ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3"), got.vectors, k.vectors):
        assert mine.tobytes() == pi.le(ref), name


# ---------------------------------------------------------------- the compile, byte for byte
@pytest.mark.parametrize("name", sorted(pr.SHAPES))
def test_the_compile_is_the_python_compile_byte_for_byte(zk, name):
    c, k = reference(name)
    with zk.PlonkR1cs(c.data) as got:
        assert_same_circuit(got, k)
        ext = pr.extend(k, c.witness)
        assert got.extend(c.wtns).tobytes() == pi.le(ext)
        assert got.extend(le(c.witness)).tobytes() == pi.le(ext)       # raw values; and the object's buffers are reused
        assert pr.check(k, pi.ints(got.extend(c.wtns).tobytes()), c.publics) is None


def test_the_wide_circuit_moves_every_digit_of_the_sort(zk):
    c, k = reference(pr.WIDE)
    with zk.PlonkR1cs(c.data) as got:
        assert got.info()["sort_passes"] == 3 and got.n_witness > 1 << 16 and got.log_n == 17
        assert_same_circuit(got, k)


@pytest.mark.parametrize("k1,k2", [(5, 7), (R - 2, 11)])
def test_other_shifts(zk, k1, k2):
    c = pr.case("chains")
    k = pr.compile_r1cs(c.data, k1, k2)
    with zk.PlonkR1cs(c.data, k1, k2) as got:
        assert_same_circuit(got, k)


@pytest.mark.parametrize("name", ["chains", "long_row", "rows_17"])
@pytest.mark.parametrize("seg", ["1", "3", None])
def test_bytes_do_not_depend_on_the_segment(zk, monkeypatch, name, seg):
    c, k = reference(name)
    if seg is None:
        monkeypatch.delenv("ZKHIP_R1CS_SEG", raising=False)
    else:
        monkeypatch.setenv("ZKHIP_R1CS_SEG", seg)
    with zk.PlonkR1cs(c.data) as got:
        assert got.info()["seg"] == (int(seg) if seg else 8)
        assert_same_circuit(got, k)
        assert got.extend(c.wtns).tobytes() == pi.le(pr.extend(k, c.witness))


@pytest.mark.parametrize("name", ["long_row", pr.WIDE])
def test_two_compiles_of_one_file_give_the_same_bytes(zk, name):
    c = pr.case(name)
    with zk.PlonkR1cs(c.data) as one, zk.PlonkR1cs(c.data) as two:
        for a, b in zip(one.vectors + one.maps, two.vectors + two.maps):
            assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- proofs
def reference_prover(zk, kzg, k):
    """the existing prover over the Python compile"""
    return zk.PlonkProver(kzg, *[le(v) for v in k.vectors], k.k1, k.k2, *k.maps, k.n_witness, k.n_public, basis="lagrange")


@pytest.mark.parametrize("name", PROOF_SHAPES)
def test_a_proof_is_the_existing_provers_over_the_python_compile(zk, kzg, name):
    c, k = reference(name)
    b = blinds(7300 + k.log_n)
    with reference_prover(zk, kzg, k) as ref:
        want = ref.prove(pr.extend(k, c.witness), blind=b)
        want_vk = ref.vkey().commitments
    with zk.PlonkR1cs(c.data) as comp, zk.PlonkProver.from_r1cs(kzg, comp) as p:
        got = p.prove_r1cs(c.wtns, blind=b)
        assert got.to_bytes() == want.to_bytes()
        assert p.prove_r1cs(le(c.witness), blind=b) == got
        vk = p.vkey()
        assert zk.plonk_verify(vk, got, c.publics) == OK
        assert vk.commitments == want_vk and (vk.log_n, vk.n_public, vk.k1, vk.k2) == (k.log_n, k.n_public, pr.K1, pr.K2)
        for name_, v in zip(("ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3"), k.vectors):
            assert vk.commitments[name_] == kzg.commit(bn.ntt(v, inverse=True)).tobytes(), name_
        assert p.prove(le(pr.extend(k, c.witness)), blind=b) == got      # the plain entry still works on such a prover


def test_from_r1cs_takes_a_path_or_bytes_and_drawn_blinds_verify(zk, kzg, tmp_path):
    c, k = reference("proof_6")
    path = str(tmp_path / "c.r1cs")
    wpath = str(tmp_path / "w.wtns")
    open(path, "wb").write(c.data)
    open(wpath, "wb").write(c.wtns)
    with zk.PlonkProver.from_r1cs(kzg, path) as p:
        one, two = p.prove_r1cs(wpath), p.prove_r1cs(c.wtns)
        assert one != two
        vk = p.vkey()
        for proof in (one, two):
            assert zk.plonk_verify(vk, proof, c.publics) == OK
        assert zk.plonk_verify(vk, one, [(c.publics[0] + 1) % R, c.publics[1]]) == 1
        comp = p.r1cs
    with pytest.raises(zk.ZkHipError, match="the PlonkR1cs object is closed"):      # compiled by from_r1cs: closed with the prover
        comp.info()
    with zk.PlonkProver.from_r1cs(kzg, c.data) as p:
        assert zk.plonk_verify(p.vkey(), p.prove_r1cs(c.wtns), c.publics) == OK


def test_selfverify_checks_the_proof_before_it_is_returned(zk, kzg, monkeypatch):
    c, k = reference("proof_4")
    monkeypatch.setenv("ZKHIP_SELFVERIFY", "1")
    with zk.PlonkProver.from_r1cs(kzg, c.data) as p:
        proof = p.prove_r1cs(c.wtns)
        assert zk.plonk_verify(p.vkey(), proof, c.publics) == OK
        seen = []
        real = zk.plonk.plonk_verify
        monkeypatch.setattr(zk.plonk, "plonk_verify", lambda *a, **kw: seen.append(a) or 1)
        with pytest.raises(zk.ZkHipError, match="ZKHIP_SELFVERIFY: the proof does not verify"):
            p.prove_r1cs(c.wtns)
        assert len(seen) == 1 and seen[0][2].tobytes() == pi.le(c.publics)
        monkeypatch.setattr(zk.plonk, "plonk_verify", real)


@pytest.mark.parametrize("name", ["proof_4", "proof_8"])
def test_a_changed_private_value_is_refused_and_no_proof_byte_is_written(zk, kzg, name):
    c, k = reference(name)
    lib = zk.load_library()
    with zk.PlonkProver.from_r1cs(kzg, c.data) as p:
        for at in (k.n_public + 1, len(c.witness) - 1):
            bad = list(c.witness)
            bad[at] = (bad[at] + 1) % R
            w = le(bad)
            with pytest.raises(zk.ZkHipError, match="zk_plonk_prove_r1cs: (%s|%s)" % (GATES, COPIES)):
                p.prove_r1cs(w)
            out = np.full(768, 0xA5, dtype=np.uint8)
            assert lib.zk_plonk_prove_r1cs(p._handle(), ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(w.ctypes.data), len(bad), None) == 1
            assert (out == 0xA5).all()
        assert zk.plonk_verify(p.vkey(), p.prove_r1cs(c.wtns), c.publics) == OK     # and the object still proves


# ---------------------------------------------------------------- refusals and info
def test_wire_0_twice_names_the_lowest_constraint_a_before_b_before_c(zk):
    one = [(1, 1)]
    A = [one, one, [(0, 1), (1, 1), (0, 0)], one, [(0, 1), (0, 2)]]
    B = [one, [(0, 0), (0, 0), (0, 5)], [(0, 2), (2, 1), (0, 3)], [(0, 1), (0, 1)], one]
    C = [one, [(0, 0), (0, 0)], [(0, 1), (0, 1)], one, one]
    data = zk.r1cs.write_r1cs_rows(A, B, C, 3, 0)
    with pytest.raises(zk.ZkHipError, match="^zk_plonk_r1cs_create: constraint 2: B names wire 0 twice$"):
        zk.PlonkR1cs(data)
    A[2] = [(0, 1), (0, 1)]
    with pytest.raises(zk.ZkHipError, match="^zk_plonk_r1cs_create: constraint 2: A names wire 0 twice$"):
        zk.PlonkR1cs(zk.r1cs.write_r1cs_rows(A, B, C, 3, 0))
    A[2], B[2] = one, one
    with pytest.raises(zk.ZkHipError, match="^zk_plonk_r1cs_create: constraint 2: C names wire 0 twice$"):
        zk.PlonkR1cs(zk.r1cs.write_r1cs_rows(A, B, C, 3, 0))
    with pytest.raises(zk.ZkHipError, match="^r1cs constraint 1: wire id >= nWires$"):
        zk.PlonkR1cs(zk.r1cs.write_r1cs_rows([one, [(3, 1)]], [one, one], [one, one], 3, 0))
    with pytest.raises(zk.ZkHipError, match="^r1cs constraint 0: coefficient >= r$"):
        zk.PlonkR1cs(zk.r1cs.write_r1cs_rows([[(1, R)]], [one], [one], 3, 0))


def test_refusals_of_a_call(zk, kzg, monkeypatch):
    c, k = reference("proof_4")
    with zk.PlonkR1cs(c.data) as comp:
        with pytest.raises(zk.ZkHipError, match="^witness has %d values, the r1cs %d wires$" % (k.n_wires - 1, k.n_wires)):
            comp.extend(le(c.witness[:-1]))
        bad = list(c.witness)
        bad[3] = R
        raw = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in bad), dtype=np.uint8)
        with pytest.raises(zk.ZkHipError, match="^zk_plonk_r1cs_extend: witness 3 is not below r$"):
            comp.extend(raw)
        with zk.PlonkProver.from_r1cs(kzg, comp) as p:
            with pytest.raises(zk.ZkHipError, match="^witness has %d values, the r1cs %d wires$" % (k.n_wires + 1, k.n_wires)):
                p.prove_r1cs(le(c.witness + [1]))
            with pytest.raises(zk.ZkHipError, match="^zk_plonk_prove_r1cs: witness 3 is not below r$"):
                p.prove_r1cs(raw)
            monkeypatch.setenv("ZKHIP_R1CS_SEG", "4097")
            for call in (lambda: p.prove_r1cs(c.wtns), lambda: comp.extend(c.wtns), comp.info, lambda: zk.PlonkR1cs(c.data)):
                with pytest.raises(zk.ZkHipError, match="^%s$" % SEG_TEXT):
                    call()
            monkeypatch.delenv("ZKHIP_R1CS_SEG")
            assert zk.plonk_verify(p.vkey(), p.prove_r1cs(c.wtns), c.publics) == OK
        with pytest.raises(zk.ZkHipError, match="three different cosets"):
            zk.PlonkR1cs(c.data, 7, 7)
        with reference_prover(zk, kzg, k) as plain:
            with pytest.raises(zk.ZkHipError, match="the prover was not made from an r1cs"):
                plain.prove_r1cs(c.wtns)
            out = np.zeros(768, dtype=np.uint8)
            w = le(c.witness)
            lib = zk.load_library()
            assert lib.zk_plonk_prove_r1cs(plain._handle(), ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(w.ctypes.data), len(c.witness), None) == 1
            assert lib.zk_last_error().decode() == "zk_plonk_prove_r1cs: the prover was not made from an r1cs (zk_plonk_prover_create_r1cs)"
        p = zk.PlonkProver.from_r1cs(kzg, comp)
        p.close()
        with pytest.raises(zk.ZkHipError, match="the PlonkProver object is closed"):
            p.prove_r1cs(c.wtns)
        comp.info()                                         # borrowed, not closed with the prover
    with pytest.raises(zk.ZkHipError, match="the PlonkR1cs object is closed"):
        comp.extend(c.wtns)
    small = zk.Kzg.__new__(zk.Kzg)
    small.max_coeffs, small.device, small._h = 21, kzg.device, None
    with pytest.raises(ValueError, match="n \\+ 6 = 22 exceeds the kzg's max_coeffs = 21"):
        zk.PlonkProver.from_r1cs(small, c.data)


def test_info_counts_are_the_documents(zk):
    """a compile launches 13 + [nPublic > 0] + 5 * sort_passes kernels, an extension 3 (0 without addition
    gates); sort_passes = ceil(ceil(log2 n_witness) / 8)."""
    for name in ("chains", "one_constraint", "long_row", "rows_16"):
        c, k = reference(name)
        with zk.PlonkR1cs(c.data) as comp:
            d = comp.info()
            passes = ((k.n_witness - 1).bit_length() + 7) // 8
            terms = sum(len(lc) for lcs in zk.r1cs.read_constraints(c.data)[1] for lc in lcs)
            assert d == dict(d, log_n=k.log_n, rows=k.rows, n_public=k.n_public, n_wires=k.n_wires, n_additions=k.n_additions, n_witness=k.n_witness,
                             terms=terms, seg=8, sort_passes=passes, last_launches=13 + (1 if k.n_public else 0) + 5 * passes), name
            assert d["device_bytes"] >= k.n * (8 * 32 + 3 * 4)
            comp.extend(c.wtns)
            assert comp.info()["last_launches"] == (3 if k.n_additions else 0), name
