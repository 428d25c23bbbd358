"""The PLONK prover with many witnesses a call (zk_plonk_prove_many and its neighbours).  Exact arithmetic:
with the blinds given, proof i of a call is compared BYTE FOR BYTE with prove(witness_i, publics_i, blind=blinds_i) on the
same object, the one-proof route that test_gpu_plonk_prover.py pins to the reference prover; at log_n 3 and 4 also with that
reference prover itself (tests/plonk_prover_instance.py, Python integers at the known tau of a trapdoor file).

So that the proofs of one call have DIFFERENT witnesses (a slot that read its neighbour's witness must fail), the circuit of
`linear` has gates that are linear and homogeneous in the witness and the publics: q_M = q_C = 0 and q_O chosen so that
q_L a + q_R b + q_O c - publics = 0 on the instance's values.  Then k * witness with k * publics satisfies it for every k, the
copy constraints hold for any values (cells of a cycle share a witness index), and one cell of a cycle has an index of its own
at the witness's end, so that a witness breaks that copy exactly when its last value is not its cycle's."""
import ctypes
import functools
import json
import os
import random
import subprocess

import numpy as np
import pytest

import plonk_instance as pi
import plonk_prover_instance as pp
import plonk_r1cs_instance as pr
from conftest import ROOT
from oracle import bn254 as bn

pytestmark = pytest.mark.gpu

R = bn.R_MOD
TAU, ALPHA, BETA = 0x1F3A9C5E77D1B2A49E0C6F5D3B8A17264C9E0F1D2B3A4958, 0x2B7E151628AED2A6ABF7158809CF4F3C, 0x3243F6A8885A308D313198A2E0370734
MAX_COEFFS = (1 << 11) + 6
OK, INVALID = 0, 1
MADE, COPIES, GATES, NOT_BELOW_R = 0, 2, 3, 4
KNOB = "ZKHIP_PLONK_PROVE_BATCH"
SEG_KNOBS = ("ZKHIP_QUOT_SEG", "ZKHIP_OPEN_SEG", "ZKHIP_SCAN_SEG", "ZKHIP_KZG_SEG")
WIDTHS = ("1", "2", "3", None)
DEFAULT_WIDTH = 16                                      # plonk_many_plan.hpp's pm_default_width up to log_n 16, what DESIGN.md section 36 measured
LOG_NS = (3, 6, 8, 11)                                  # rows of 14: less than a wave; 262: across a 256-lane workgroup; 2054: the fixture's largest


def le(values):
    return np.frombuffer(pi.le(values), dtype=np.uint8)


@pytest.fixture(scope="module")
def ptau(zk, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("plonk_prove_many") / "p12.ptau")
    zk.write_trapdoor_ptau(12, TAU, ALPHA, BETA, path, prepared=False)
    return path


@pytest.fixture(scope="module")
def kzg(zk, ptau):
    k = zk.Kzg.from_ptau(ptau, max_coeffs=MAX_COEFFS)
    yield k
    k.close()


def blinds(seed):
    rng = random.Random(seed)
    return [rng.randrange(1, R) for _ in range(11)]


def set_width(monkeypatch, width):
    if width is None:
        monkeypatch.delenv(KNOB, raising=False)
        return DEFAULT_WIDTH
    monkeypatch.setenv(KNOB, width)
    return int(width)


def set_segs(monkeypatch, seg):
    for name in SEG_KNOBS:
        if seg is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, seg)


def sizes(B):
    return sorted({1, 2, B, B + 1, 2 * B + 1})


# ---------------------------------------------------------------- the linear circuit: many witnesses of one circuit
class Linear:
    """vectors (values over the domain), maps, n_witness (one more than the instance's), n_public; witness(k, extra) and
    publics(k): k times the instance's, the last value its cycle's plus `extra`"""

    def __init__(self, seed, log_n, n_public):
        c = pp.build(seed, log_n, n_public)
        I, n = c.inst, c.inst.n
        pub = list(c.publics) + [0] * (n - n_public)
        assert all(v for v in I.c_v)
        qo = [(pub[i] - I.ql_v[i] * I.a_v[i] - I.qr_v[i] * I.b_v[i]) * pow(I.c_v[i], -1, R) % R for i in range(n)]
        self.values = [I.ql_v, I.qr_v, [0] * n, qo, [0] * n, I.s1_v, I.s2_v, I.s3_v]
        cells = list(c.maps[0]) + list(c.maps[1]) + list(c.maps[2])
        count = {}
        for ix in cells:
            count[ix] = count.get(ix, 0) + 1
        self.cell = next(i for i, ix in enumerate(cells) if count[ix] > 1 and i >= n_public)
        self.source = cells[self.cell]
        self.lone = next(ix for ix in cells if count[ix] == 1)           # a value one cell alone names: moving it breaks that row's gate only
        cells[self.cell] = c.n_witness
        self.maps = (cells[:n], cells[n:2 * n], cells[2 * n:])
        self.n, self.log_n, self.n_public, self.n_witness = n, log_n, n_public, c.n_witness + 1
        self._w, self._p = list(c.witness), list(c.publics)

    def circuit(self, basis):
        return self.values if basis == "lagrange" else [bn.ntt(v, inverse=True) for v in self.values]

    def witness(self, k, extra=0):
        w = [k * v % R for v in self._w]
        return w + [(w[self.source] + extra) % R]

    def publics(self, k):
        return [k * v % R for v in self._p]

    def prover(self, zk, kzg, basis="lagrange"):
        return zk.PlonkProver(kzg, *[le(x) for x in self.circuit(basis)], pi.K1, pi.K2, *self.maps, self.n_witness, self.n_public, basis=basis)


@functools.lru_cache(maxsize=None)
def linear(log_n, n_public=2):
    return Linear(6100 + 10 * log_n + min(n_public, 3), log_n, n_public)


def inputs(c, m, first=1):
    """m different witnesses with their publics and blinds: proof i scales the instance by first + i"""
    ks = [first + i for i in range(m)]
    return [c.witness(k) for k in ks], [c.publics(k) for k in ks], [blinds(977 * k + c.log_n) for k in ks]


def one_by_one(p, ws, ps, bs):
    return [p.prove(w, pub, b).to_bytes() for w, pub, b in zip(ws, ps, bs)]


def many_bytes(p, ws, ps, bs):
    proofs, status = p.prove_many(ws, ps, bs)
    assert status.dtype == np.uint32 and list(status) == [MADE] * len(ws)
    return [q.to_bytes() for q in proofs]


# ---------------------------------------------------------------- byte equality with prove
@pytest.mark.parametrize("basis", ["lagrange", "monomial"])
@pytest.mark.parametrize("n_public", [0, 2, "n"])
@pytest.mark.parametrize("log_n", LOG_NS)
def test_proof_i_is_proves_proof_byte_for_byte(zk, kzg, monkeypatch, log_n, n_public, basis):
    """every batch width and every segment setting on one object: neither the chunking nor a knob moves a byte"""
    c = linear(log_n, (1 << log_n) if n_public == "n" else n_public)
    ws, ps, bs = inputs(c, 2 * DEFAULT_WIDTH + 1)
    ws = [le(w) for w in ws]                            # bytes once: the calls below take them as they are
    with c.prover(zk, kzg, basis) as p:
        want = one_by_one(p, ws, ps, bs)
        assert len(set(want)) == len(ws)
        for seg in ("1", "3", None):
            set_segs(monkeypatch, seg)
            for width in WIDTHS:
                B = set_width(monkeypatch, width)
                for m in sizes(B):
                    assert many_bytes(p, ws[:m], ps[:m], bs[:m]) == want[:m], (seg, width, m)
                    info = p.many_info()
                    assert info["batch"] == B and info["last_chunks"] == -(-m // B) and info["last_refused"] == 0
                    assert info["last_multiplications"] == (4 * info["last_chunks"] if B > 1 else 9 * m)
        set_segs(monkeypatch, None)
        assert one_by_one(p, ws[:2], ps[:2], bs[:2]) == want[:2]          # and prove after the many-calls is what it was


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("log_n", [3, 4])
def test_the_reference_provers_proofs(zk, kzg, monkeypatch, log_n, width):
    """the reference, not the code under test: the same witness under different blinds, all blinds 0, and b1 = 0 alone (a has
    n + 1 coefficients), among ordinary ones in one call"""
    seed = 5000 + log_n
    c = pp.build(seed, log_n, 2)
    rows = [blinds(seed), blinds(seed + 50), [0] * 11, [0] + blinds(seed + 60)[1:], blinds(seed + 70)]
    want = [pp.prove(c, b, TAU).to_bytes() for b in rows]
    assert len(set(want)) == len(rows)
    set_width(monkeypatch, width)
    with zk.PlonkProver(kzg, *[le(x) for x in c.inst.circuit()], pi.K1, pi.K2, *c.maps, c.n_witness, 2) as p:
        assert many_bytes(p, [c.witness] * len(rows), [c.publics] * len(rows), rows) == want


@pytest.mark.parametrize("width", ["2", "3"])
def test_a_witness_whose_a_column_is_all_zero(zk, kzg, monkeypatch, width):
    """[a] is then the blinding's alone, and with b1 = b2 = 0 too it is infinity: a vector of zeros in the multiplication"""
    o = pp.build(6262, 6, 2)
    I, n = o.inst, o.inst.n
    # a circuit of its own: no copy cycles (sigma is the identity), the a column reads one witness value, the last, which is 0,
    # and q_L a + q_R b + q_O c - publics = 0 with q_O chosen for the instance's b and c: k * witness satisfies it for every k
    maps = ([o.n_witness] * n, o.maps[1], o.maps[2])
    pub = list(o.publics) + [0] * (n - 2)
    qo = [(pub[i] - I.qr_v[i] * I.b_v[i]) * pow(I.c_v[i], -1, R) % R for i in range(n)]
    ident = lambda shift: [shift * pow(bn.fr_root(6), i, R) % R for i in range(n)]      # noqa: E731
    vectors = [I.ql_v, I.qr_v, [0] * n, qo, [0] * n, ident(1), ident(pi.K1), ident(pi.K2)]
    witness = lambda k: [k * v % R for v in o.witness] + [0]                             # noqa: E731
    set_width(monkeypatch, width)
    with zk.PlonkProver(kzg, *[le(x) for x in vectors], pi.K1, pi.K2, *maps, o.n_witness + 1, 2, basis="lagrange") as p:
        ws = [witness(k) for k in (1, 2, 3, 4)]
        ps = [[k * v % R for v in o.publics] for k in (1, 2, 3, 4)]
        bs = [blinds(1), [0, 0] + blinds(2)[2:], blinds(3), [0] * 11]
        want = one_by_one(p, ws, ps, bs)
        assert want[1][:64] == bytes(64) and want[3][:64] == bytes(64) and want[0][:64] != bytes(64)
        assert many_bytes(p, ws, ps, bs) == want


# ---------------------------------------------------------------- drawn blinds
@pytest.mark.parametrize("width", ["1", "3"])
def test_drawn_blinds_verify_and_a_changed_public_fails_its_proof_alone(zk, kzg, monkeypatch, width):
    c = linear(6, 2)
    ws, ps, _ = inputs(c, 5)
    set_width(monkeypatch, width)
    with c.prover(zk, kzg) as p:
        one, status = p.prove_many(ws, ps)
        two, _ = p.prove_many(ws, ps)
        assert list(status) == [MADE] * 5
        assert all(a != b and a.points[0] != b.points[0] for a, b in zip(one, two))
        with zk.PlonkVerifier(p.vkey()) as v:
            assert list(v.verify(one, ps)) == [OK] * 5 and list(v.verify(two, ps)) == [OK] * 5
            for j in (0, 2, 4):
                bad = [list(row) for row in ps]
                bad[j][1] = (bad[j][1] + 1) % R
                assert list(v.verify(one, bad)) == [INVALID if i == j else OK for i in range(5)]


# ---------------------------------------------------------------- refusals
def place(B, where, m):
    """the proof at `where` of the first chunk, and the same place of the chunk after it"""
    at = {"first": 0, "middle": B // 2, "last": B - 1}[where]
    return [at, B + at] if B + at < m else [at]


@pytest.mark.parametrize("width", ["1", "2", "3", "4"])
@pytest.mark.parametrize("kind", ["gate", "copy", "value"])
def test_a_refused_proof_does_not_take_the_others_with_it(zk, kzg, monkeypatch, kind, width):
    c = linear(4, 2)
    B = set_width(monkeypatch, width)
    m = 2 * B + 1
    ws, ps, bs = inputs(c, m)
    lib = zk.load_library()
    P = lambda a: ctypes.c_void_p(a.ctypes.data)       # noqa: E731
    with c.prover(zk, kzg) as p:
        want = one_by_one(p, ws, ps, bs)
        # all of a chunk refused comes last: chunk 0 whole, chunk 1 untouched
        for bad in [place(B, w, m) for w in ("first", "middle", "last")] + [list(range(B))]:
            wb = [le(w).copy() for w in ws]
            for i in bad:
                if kind == "gate":
                    w = list(ws[i])
                    w[c.lone] = (w[c.lone] + 1) % R
                    wb[i] = le(w).copy()
                elif kind == "copy":
                    wb[i] = le(c.witness(1 + i, extra=1)).copy()
                else:
                    wb[i][32 * 3:32 * 4] = 0xFF
            code = {"gate": GATES, "copy": COPIES, "value": NOT_BELOW_R}[kind]
            text = {"gate": "the witness does not satisfy the gates", "copy": "the copy constraints do not hold", "value": "witness 3 is not below r"}[kind]
            proofs, status = p.prove_many(wb, ps, bs)
            assert list(status) == [code if i in bad else MADE for i in range(m)], (bad, list(status))
            assert [q.to_bytes() if q is not None else None for q in proofs] == [None if i in bad else want[i] for i in range(m)]
            assert p.many_info()["last_refused"] == len(bad)
            # through the C entry: the call returns 0, the refused proof's bytes are untouched, the text names the lowest index
            out = np.full(m * 768, 0xAA, dtype=np.uint8)
            st = np.full(m, 77, dtype=np.uint32)
            w_all, p_all, b_all = np.concatenate(wb), le([v for row in ps for v in row]).copy(), le([v for row in bs for v in row]).copy()
            assert lib.zk_plonk_prove_many(p._handle(), m, P(out), P(st), P(w_all), P(p_all), P(b_all)) == 0
            assert lib.zk_last_error().decode() == "zk_plonk_prove_many: proof %d: %s" % (bad[0], text)
            for i in range(m):
                assert bytes(out[i * 768:(i + 1) * 768]) == (b"\xaa" * 768 if i in bad else want[i]), i
            # and a following call on the same object is correct
            assert many_bytes(p, ws, ps, bs) == want


def test_the_three_refusals_in_one_chunk(zk, kzg, monkeypatch):
    c = linear(4, 2)
    set_width(monkeypatch, "4")
    ws, ps, bs = inputs(c, 4)
    with c.prover(zk, kzg) as p:
        want = one_by_one(p, ws, ps, bs)
        gate = list(ws[0])
        gate[c.lone] = (gate[c.lone] + 1) % R
        big = le(ws[3]).copy()
        big[-32:] = 0xFF
        proofs, status = p.prove_many([gate, c.witness(2, extra=5), ws[2], big], ps, bs)
        assert list(status) == [GATES, COPIES, MADE, NOT_BELOW_R] and proofs[2].to_bytes() == want[2]
        assert p.many_info()["last_multiplications"] == 4 and p.many_info()["last_refused"] == 3


# ---------------------------------------------------------------- the multiplication's own entry
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("log_n", LOG_NS)
def test_commit_many_is_kzg_commit(zk, kzg, monkeypatch, log_n, width):
    c = linear(log_n, 2)
    B = set_width(monkeypatch, width)
    n6 = c.n + 6
    rng = random.Random(88 + log_n)
    rand = lambda: [rng.randrange(R) for _ in range(n6)]            # noqa: E731
    unit = lambda at: [1 if i == at else 0 for i in range(n6)]      # noqa: E731
    with c.prover(zk, kzg) as p:
        for k in sorted({1, 2, 3 * B, 3 * B + 1}):
            polys = [rand() for _ in range(k)]
            polys[0] = unit(0) if k > 1 else unit(n6 - 1)
            polys[-1] = unit(n6 - 1)
            if k >= 3:
                polys[1] = [0] * n6                                 # zeros between non-zero ones
            if k >= 4:
                polys[2] = [R - 1] * n6
                polys[3] = unit(0)
            got = p.commit_many(polys)
            assert got == [bytes(kzg.commit(le(q))) for q in polys], (k, B)
            if k >= 3:
                assert got[1] == bytes(64)
            info = p.many_info()
            assert info["last_chunks"] == info["last_multiplications"] == -(-k // (3 * B)) and info["table_batch"] == B
        assert p.commit_many([[R - 1] * n6]) == [bytes(kzg.commit(le([R - 1] * n6)))]
        assert p.commit_many([[5, 7]]) == [bytes(kzg.commit(le([5, 7])))]        # a shorter polynomial is padded
        bad = [rand(), rand(), rand()]
        bad[2][5] = R
        with pytest.raises(zk.ZkHipError, match="^zk_plonk_prover_commit_many: vector 2 coefficient 5 is not below r$"):
            p.commit_many(bad)
        with pytest.raises(ValueError, match="^coeffs\\[1\\]: %d coefficients, 1 .. n \\+ 6 = %d expected$" % (n6 + 1, n6)):
            p.commit_many([rand(), rand() + [1]])


# ---------------------------------------------------------------- circom witnesses and the CLI
@pytest.mark.parametrize("width", ["1", "2", "3"])
@pytest.mark.parametrize("name", ["proof_3", "proof_4"])      # proof_4 has addition gates, which the device extends a slot at a time
def test_prove_r1cs_many_is_prove_r1cs(zk, kzg, monkeypatch, name, width):
    c = pr.case(name)
    assert (pr.compile_r1cs(c.data).n_additions > 0) == (name == "proof_4")
    set_width(monkeypatch, width)
    rows = [blinds(31 + i) for i in range(5)]
    bad = list(c.witness)
    bad[len(c.publics) + 1] = (bad[len(c.publics) + 1] + 1) % R
    big = le(c.witness).copy()
    big[32 * 2 + 31] = 0xFF
    with zk.PlonkProver.from_r1cs(kzg, c.data) as p:
        want = [p.prove_r1cs(c.wtns, b).to_bytes() for b in rows]
        proofs, status = p.prove_r1cs_many([c.wtns, le(c.witness), le(bad), c.wtns, big], rows)
        assert list(status)[:2] == [MADE, MADE] and status[2] in (GATES, COPIES) and list(status)[3:] == [MADE, NOT_BELOW_R]
        assert [q.to_bytes() if q else None for q in proofs] == [want[0], want[1], None, want[3], None]
        with zk.PlonkVerifier(p.vkey()) as v:
            assert list(v.verify([proofs[0], proofs[3]], [c.publics] * 2 if c.publics else None)) == [OK, OK]
        with pytest.raises(ValueError, match="the witnesses must have one length"):
            p.prove_r1cs_many([le(c.witness), le(c.witness + [1])])
        with pytest.raises(zk.ZkHipError, match="^witness has %d values, the r1cs %d wires$" % (len(c.witness) + 1, len(c.witness))):
            p.prove_r1cs_many([le(c.witness + [1])])


def proof_bytes(text):
    """proof.json -> the 768 bytes of a PlonkProof"""
    d = json.loads(text)
    out = b""
    for name in ("A", "B", "C", "Z", "T1", "T2", "T3", "Wxi", "Wxiw"):
        x, y, z = (int(v) for v in d[name])
        assert z == 1, name
        out += (x * bn.MONT_R % bn.Q_MOD).to_bytes(32, "little") + (y * bn.MONT_R % bn.Q_MOD).to_bytes(32, "little")
    return out + b"".join(int(d[name]).to_bytes(32, "little") for name in ("eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw"))


@pytest.mark.parametrize("width", ["2", None])
def test_the_program_with_one_two_and_three_triples(zk, ptau, tmp_path, width):
    from oracle.groth16_ref import write_wtns
    prog = os.path.join(ROOT, "rapidsnark-old_amd", "plonkprover")
    c = pr.case("proof_4")
    bad = list(c.witness)
    bad[len(c.publics) + 1] = (bad[len(c.publics) + 1] + 1) % R
    (tmp_path / "c.r1cs").write_bytes(c.data)
    (tmp_path / "w.wtns").write_bytes(c.wtns)
    (tmp_path / "bad.wtns").write_bytes(write_wtns(bad))
    env = dict(os.environ, ZKHIP_SELFVERIFY="1")
    env.pop(KNOB, None)
    if width:
        env[KNOB] = width

    def run(*names):
        args = []
        for i, name in enumerate(names):
            args += [str(tmp_path / name), str(tmp_path / ("proof%d.json" % i)), str(tmp_path / ("public%d.json" % i))]
        return subprocess.run([prog, str(tmp_path / "c.r1cs"), ptau, *args], capture_output=True, text=True, errors="replace", env=env, timeout=300)

    with zk.Kzg.from_ptau(ptau, max_coeffs=16 + 6) as k, zk.PlonkProver.from_r1cs(k, c.data) as p, zk.PlonkVerifier(p.vkey()) as v:
        for names in (("w.wtns",), ("w.wtns", "w.wtns"), ("w.wtns", "bad.wtns", "w.wtns")):
            for f in os.listdir(tmp_path):
                if f.endswith(".json"):
                    os.remove(tmp_path / f)
            r = run(*names)
            good = [i for i, name in enumerate(names) if name == "w.wtns"]
            assert r.returncode == (0 if len(good) == len(names) else 1), r.stderr
            assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".json")) == sorted("%s%d.json" % (s, i) for i in good for s in ("proof", "public"))
            proofs = [proof_bytes((tmp_path / ("proof%d.json" % i)).read_text()) for i in good]
            assert list(v.verify(proofs, [c.publics] * len(good))) == [OK] * len(good) and len(set(proofs)) == len(good)
            for i in good:
                assert json.loads((tmp_path / ("public%d.json" % i)).read_text()) == [str(x) for x in c.publics]
            if len(good) < len(names):
                assert r.stderr.startswith("INVALID: %s: the " % (tmp_path / "bad.wtns")) and r.stdout == ""
        r = subprocess.run([prog, str(tmp_path / "c.r1cs"), ptau, str(tmp_path / "w.wtns"), "a.json", "b.json", "extra"], capture_output=True, text=True)      # no whole triple
        assert r.returncode == 255 and r.stderr.startswith("Invalid number of parameters:\nUsage: plonkprover ")


# ---------------------------------------------------------------- info
def test_many_info_and_the_objects_memory(zk, kzg, monkeypatch):
    c = linear(6, 2)
    ws, ps, bs = inputs(c, 4)
    with c.prover(zk, kzg) as p:
        info = p.many_info()
        assert info["batch"] == DEFAULT_WIDTH and info["table_batch"] == 0 and info["table_bytes"] == info["slot_bytes"] == info["msm_bytes"] == 0
        want = one_by_one(p, ws, ps, bs)
        lone = p.info()["last_launches"]
        before = p.info()["device_bytes"]                 # the scan's buffers are there from the first proof on
        set_width(monkeypatch, "1")                     # the loop keeps nothing more
        assert many_bytes(p, ws, ps, bs) == want and p.info()["device_bytes"] == before and p.many_info()["table_batch"] == 0
        assert p.many_info()["last_launches"] == 4 * lone and p.many_info()["last_drains"] == 4 * 13
        set_width(monkeypatch, "4")
        assert many_bytes(p, ws, ps, bs) == want
        info = p.many_info()
        assert (info["batch"], info["table_batch"], info["last_chunks"], info["last_multiplications"]) == (4, 4, 1, 4)
        assert info["last_launches"] < 4 * lone         # nine multiplications a proof would be the loop
        assert info["last_drains"] == 4 + 4 * 4         # the chunk's four, and a proof the scan, t's length, the six values, F(zeta)
        # the table: a row a window of the width the plan takes, n + 6 points of 64 bytes each
        cbits, rows = info["window_bits"], info["table_rows"]
        assert 2 <= cbits <= 22 and rows in (-(-256 // cbits), -(-255 // cbits)) and info["table_bytes"] == rows * (c.n + 6) * 64
        layout = 4 * (c.n_witness + 2 + 11 + 4 * c.n + c.n + c.n + 3 * c.n + 6 + 9 * (c.n + 6))
        assert info["slot_bytes"] == layout * 32 and info["msm_bytes"] > 0
        assert p.info()["device_bytes"] == before + info["table_bytes"] + info["slot_bytes"] + info["msm_bytes"]
        # m = 0 is accepted
        proofs, status = p.prove_many([])
        assert proofs == [] and status.size == 0 and p.many_info()["last_chunks"] == 0


# ---------------------------------------------------------------- the self-check
def test_selfverify_checks_the_proofs_in_one_call(zk, kzg, monkeypatch):
    c = linear(3, 2)
    ws, ps, bs = inputs(c, 3)
    set_width(monkeypatch, "2")
    with c.prover(zk, kzg) as p:
        want = one_by_one(p, ws, ps, bs)
        monkeypatch.setenv("ZKHIP_SELFVERIFY", "1")
        assert many_bytes(p, ws, ps, bs) == want
        calls = []
        real = zk.PlonkVerifier.verify
        monkeypatch.setattr(zk.PlonkVerifier, "verify", lambda self, *a: calls.append(len(a[0])) or real(self, *a))
        assert many_bytes(p, ws, ps, bs) == want and calls == [3]
        # publics that are not the proofs': the check names the first proof that fails
        with pytest.raises(zk.ZkHipError, match="^ZKHIP_SELFVERIFY: proof 1 does not verify \\(verdict 1\\)$"):
            bad = [ps[0], [ps[1][0], (ps[1][1] + 1) % R], ps[2]]
            p._many_result(np.frombuffer(b"".join(want), dtype=np.uint8), np.zeros(3, dtype=np.uint32), lambda i: le(bad[i]))


# ---------------------------------------------------------------- errors of the call
def test_errors_of_the_call(zk, kzg, ptau, monkeypatch):
    c = linear(3, 2)
    ws, ps, bs = inputs(c, 2)
    with c.prover(zk, kzg) as p:
        want = one_by_one(p, ws, ps, bs)
        for bad in ("0", "65", "x", " 2"):
            monkeypatch.setenv(KNOB, bad)
            for call in (lambda: p.prove_many(ws, ps, bs), lambda: p.commit_many([[1]]), p.many_info):
                with pytest.raises(zk.ZkHipError, match="^ZKHIP_PLONK_PROVE_BATCH: a number of proofs from 1 to 64 expected$"):
                    call()
        monkeypatch.setenv(KNOB, "2")
        monkeypatch.setenv("ZKHIP_OPEN_SEG", "0")
        with pytest.raises(zk.ZkHipError, match="^ZKHIP_OPEN_SEG: a number of coefficients per lane from 1 to 4096 expected$"):
            p.prove_many(ws, ps, bs)
        monkeypatch.delenv("ZKHIP_OPEN_SEG")
        assert many_bytes(p, ws, ps, bs) == want
        with pytest.raises(zk.ZkHipError, match="^zk_plonk_prove_r1cs_many: the prover was not made from an r1cs"):
            p.prove_r1cs_many([le(ws[0])])
        lib = zk.load_library()
        st = np.zeros(2, dtype=np.uint32)
        assert lib.zk_plonk_prove_many(p._handle(), 2, None, ctypes.c_void_p(st.ctypes.data), None, None, None) == 1
        assert lib.zk_last_error().decode() == "null argument"
    closed = zk.Kzg.from_ptau(ptau, max_coeffs=14)
    q = c.prover(zk, closed)
    closed.close()
    for call in (lambda: q.prove_many(ws, ps, bs), lambda: q.commit_many([[1]]), q.many_info):
        with pytest.raises(zk.ZkHipError, match="the Kzg object is closed"):
            call()
    q.close()
    with pytest.raises(zk.ZkHipError, match="the PlonkProver object is closed"):
        q.prove_many(ws, ps, bs)
