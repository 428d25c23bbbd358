"""The Powers of Tau contribution on the GPU: ptau_new -> ptau_contribute / `ptaucontribute` against the independent route
(write_trapdoor_ptau: the fixed-base kernel on the known powers), contributions on top of each other, the plain route, drawn
scalars, and the contributed file through the rest of the chain: ptaucheck, ptauprepare, setup, phase-2 contribution, proof
and verification."""
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_json

from oracle import bn254 as bn, groth16_ref as g
from rapidsnark_old_amd import r1cs as R, zkgen
from test_zkey_contribute_host import binfile, sections_of

pytestmark = pytest.mark.gpu
RM = bn.R_MOD
BIN = os.path.join(ROOT, "rapidsnark-old_amd")
POWERS = [2, 3, 6]
S1 = (0x1234567 * 0x89ABCDEF + 17, 0xA1FA << 200 | 99, 0xBE7A << 180 | 7)                   # tau, alpha, beta
S2 = ((RM - 1) // 3 + 77, RM - 2, 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F0E1 % RM)


def read(path):
    with open(path, "rb") as f:
        return f.read()


def cli(prog, *args, scalars=None, plain=False):
    env = dict(os.environ, ZKHIP_PTAU_CONTRIB_CHUNK="64")
    for name in ("ZKHIP_PTAU_CONTRIB_SCALARS", "ZKHIP_MULVEC_PLAIN"):
        env.pop(name, None)
    if scalars is not None:
        env["ZKHIP_PTAU_CONTRIB_SCALARS"] = ",".join(str(s) for s in scalars)
    if plain:
        env["ZKHIP_MULVEC_PLAIN"] = "1"
    return subprocess.run([os.path.join(BIN, prog), *args], capture_output=True, text=True, timeout=300, env=env)


@pytest.fixture(scope="module")
def files(zk, tmp_path_factory):
    """per power: ptau_new's file, the file after S1 and the file after S1 then S2, all through the binding, in chunks of 64
    points (power 6: 127 points of section 2, the last chunk is short)"""
    d = tmp_path_factory.mktemp("pot")
    os.environ["ZKHIP_PTAU_CONTRIB_CHUNK"] = "64"
    try:
        out = {"dir": d}
        for power in POWERS:
            new, one, two = (str(d / ("p%d_%s.ptau" % (power, tag))) for tag in ("new", "one", "two"))
            zk.ptau_new(power, new)
            zk.ptau_contribute(new, one, *S1)
            zk.ptau_contribute(one, two, *S2)
            out[power] = (new, one, two)
    finally:
        del os.environ["ZKHIP_PTAU_CONTRIB_CHUNK"]
    return out


def trapdoor(zk, d, power, scalars, tag):
    path = str(d / ("trap%d_%s.ptau" % (power, tag)))
    zk.write_trapdoor_ptau(power, *scalars, path, prepared=False)
    return read(path)


@pytest.mark.parametrize("power", POWERS)
def test_contribution_equals_the_trapdoor_file(zk, files, power):
    new, one, two = files[power]
    assert not [p for p in os.listdir(str(files["dir"])) if "partial" in p]
    want = trapdoor(zk, files["dir"], power, S1, "one")
    got = read(one)
    assert [s for s, _ in sections_of(got)] == [1, 2, 3, 4, 5, 6, 7]
    for (sid, a), (_, b) in zip(sections_of(got), sections_of(want)):
        assert a == b, sid
    assert got == want
    new_secs, got_secs = dict(sections_of(read(new))), dict(sections_of(got))
    assert got_secs[1] == new_secs[1] and got_secs[7] == new_secs[7] == bytes(4)
    assert got_secs[2][:64] == new_secs[2][:64] and got_secs[3][:128] == new_secs[3][:128]      # tau^0: the generators stay


@pytest.mark.parametrize("power", POWERS)
def test_a_second_contribution_multiplies_the_scalars(zk, files, power):
    both = tuple(a * b % RM for a, b in zip(S1, S2))
    assert read(files[power][2]) == trapdoor(zk, files["dir"], power, both, "two")


@pytest.mark.parametrize("power", POWERS)
def test_the_program_and_the_plain_route_write_the_same_file(zk, files, power):
    new, one, _ = files[power]
    d = files["dir"]
    out = str(d / ("cli%d.ptau" % power))
    res = cli("ptaucontribute", new, out, scalars=S1)
    assert res.returncode == 0 and res.stdout == "", res.stderr
    assert all(str(s) not in res.stderr and "%x" % s not in res.stderr for s in S1)
    assert read(out) == read(one)
    plain = str(d / ("plain%d.ptau" % power))
    res = cli("ptaucontribute", new, plain, scalars=S1, plain=True)
    assert res.returncode == 0, res.stderr
    assert read(plain) == read(one)
    assert not [p for p in os.listdir(str(d)) if "partial" in p]


def test_one_chunk_and_many_give_the_same_file(zk, files, monkeypatch):
    new, one, _ = files[6]
    for chunk in ("1000000", "7"):
        monkeypatch.setenv("ZKHIP_PTAU_CONTRIB_CHUNK", chunk)
        out = str(files["dir"] / ("chunk%s.ptau" % chunk))
        zk.ptau_contribute(new, out, *S1)
        assert read(out) == read(one)


@pytest.mark.parametrize("power", POWERS)
def test_drawn_scalars_differ_and_the_files_are_sound(zk, files, power):
    new = files[power][0]
    outs = [str(files["dir"] / ("drawn%d_%d.ptau" % (power, i))) for i in range(2)]
    for o in outs:
        res = cli("ptaucontribute", new, o)
        assert res.returncode == 0, res.stderr
    a, b = (dict(sections_of(read(o))) for o in outs)
    fresh = dict(sections_of(read(new)))
    for sid in (2, 3, 4, 5, 6):
        assert a[sid] != b[sid] and a[sid] != fresh[sid] and b[sid] != fresh[sid], sid
    for path in outs + [new]:                                         # ptaunew's own file (tau = 1) is sound too
        rep = zk.ptau_check(path)
        assert rep.verdict == 0 and rep.ok, rep
    res = cli("ptaucheck", outs[0])
    assert res.returncode == 0 and res.stdout.startswith("OK: power %d" % power), res.stdout + res.stderr


def test_the_python_binding_draws_too(zk, files):
    new = files[3][0]
    outs = [str(files["dir"] / ("pydrawn%d.ptau" % i)) for i in range(2)]
    for o in outs:
        zk.ptau_contribute(new, o)
    assert read(outs[0]) != read(outs[1])
    assert zk.ptau_check(outs[0]).ok and zk.ptau_check(outs[1]).ok


def test_the_contributed_file_through_the_rest_of_the_chain(zk, files, tmp_path):
    """power 6 after two contributions: ptauprepare, ptaucheck with the Lagrange levels, then the circuit of
    valid_key.build at its smallest size (2^3: five constraints, two public signals) through setup, a phase-2 contribution,
    a proof and the verifier"""
    two = files[6][2]
    prepared = str(tmp_path / "prepared.ptau")
    zk.prepare_phase2(two, prepared)
    rep = zk.ptau_check(prepared)
    assert rep.ok and rep.prepared and not any(rep.lagrange_failed.values()), rep
    both = tuple(a * b % RM for a, b in zip(S1, S2))
    want = str(tmp_path / "want.ptau")
    zk.write_trapdoor_ptau(6, *both, want, prepared=True)
    assert read(prepared) == read(want)
    k, n_public = 3, 2
    c, w = g.random_r1cs(random.Random(1066), (1 << k) - n_public - 1, n_public, extra_vars=2)
    assert c.is_satisfied(w)
    rp, z0, z1 = str(tmp_path / "c.r1cs"), str(tmp_path / "c0.zkey"), str(tmp_path / "c1.zkey")
    with open(rp, "wb") as f:
        f.write(R.write_r1cs_rows(c.A, c.B, c.C, c.nVars, c.nPublic))
    zkgen.write_zkey(zk.groth16_setup(rp, prepared, device=0), z0)
    zk.zkey_contribute(z0, z1, d=S2[2])
    p = zk.Prover(z1, device=0)
    wt = g.write_wtns(w)
    proof = p.prove(wt, r=0xC0FFEE, s=(1 << 200) + 12345)
    p.close()
    pj, uj = str(tmp_path / "proof.json"), str(tmp_path / "public.json")
    with open(pj, "w") as f:
        f.write(zk.proof_to_json(proof))
    with open(uj, "w") as f:
        f.write(zk.public_to_json(b"".join(bn.int_to_le32(x) for x in w), n_public))
    assert zk.groth16_verify(z1, uj, pj)
    assert not zk.groth16_verify(z0, uj, pj)                          # the key before the phase-2 contribution has another delta


def test_a_bad_point_is_named_and_leaves_no_file(zk, files):
    d = files["dir"]
    secs = sections_of(read(files[6][1]))
    cof = golden_json("g2_cofactor_points.json")["outside"][1]
    outside = bn.g2_to_bytes(((int(cof["x"][0]), int(cof["x"][1])), (int(cof["y"][0]), int(cof["y"][1]))))

    def patched(sid, at, nb, new=None):
        p = bytearray(dict(secs)[sid])
        if new is None:
            p[nb * at + nb // 2 + 1] ^= 4                             # y changed: off the curve
        else:
            p[nb * at:nb * at + nb] = new
        return binfile(b"ptau", 1, [(s, bytes(p) if s == sid else q) for s, q in secs])

    cases = [(patched(4, 37, 64), "ptau section 4: point 37 is not on the curve"),
             (patched(3, 63, 128, outside), "ptau section 3: point 63 is not in the subgroup"),
             (patched(2, 126, 64), "ptau section 2: point 126 is not on the curve"),
             (patched(5, 0, 64, bytes(64)), "ptau section 5: point 0 is the point at infinity"),
             (patched(6, 0, 128, outside), "ptau section 6: point 0 is not in the subgroup")]
    bad, out = str(d / "bad_in.ptau"), str(d / "bad_out.ptau")
    for data, msg in cases:
        with open(bad, "wb") as f:
            f.write(data)
        res = cli("ptaucontribute", bad, out, scalars=S2)
        assert res.returncode == 255 and msg in res.stderr, (msg, res.stderr)
        assert sorted(p for p in os.listdir(str(d)) if p.startswith("bad_")) == ["bad_in.ptau"], msg
    with pytest.raises(zk.ZkHipError, match="ptau section 6: point 0 is not in the subgroup"):
        zk.ptau_contribute(bad, out, *S2)
    assert sorted(p for p in os.listdir(str(d)) if p.startswith("bad_")) == ["bad_in.ptau"]
