"""circom's .r1cs on the host: the Python writer and reader, the container checks that run before any device is touched,
and the `wtnscheck` program's usage and error exits (no GPU needed)."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_path

from oracle import groth16_ref as g
from rapidsnark_old_amd import r1cs as R

WTNSCHECK = os.path.join(ROOT, "rapidsnark-old_amd", "wtnscheck")
BN254_R = g.R_MOD


def run(*args):
    return subprocess.run([WTNSCHECK, *args], capture_output=True, text=True, errors="replace", timeout=120)


def multiplier2_bytes():
    c = g.multiplier2_r1cs()
    return R.write_r1cs_rows(c.A, c.B, c.C, c.nVars, c.nPublic)


def test_round_trip_random_circuit():
    rng = random.Random(11)
    c, w = g.random_r1cs(rng, 40, 3)
    data = R.write_r1cs_rows(c.A, c.B, c.C, c.nVars, c.nPublic)
    h, cons = R.read_constraints(data)
    assert (h.nWires, h.nPubOut, h.nPubIn, h.nPrvIn, h.nLabels, h.nConstraints) == (c.nVars, 0, 3, c.nVars - 4, c.nVars, 40)
    assert h.nPublic == c.nPublic and h.prime == BN254_R
    for (a, b, cc), ra, rb, rc in zip(cons, c.A, c.B, c.C):
        assert a == list(ra.items()) and b == list(rb.items()) and cc == list(rc.items())


def test_round_trip_long_rows_and_duplicates_from_arrays():
    lens = [0, 1, 7, 8, 9, 15, 16, 17, 254, 4096]
    rp = np.zeros(len(lens) + 1, dtype=np.int64)
    rp[1:] = np.cumsum(lens)
    nnz = int(rp[-1])
    wires = (np.arange(nnz) % 5).astype(np.uint32)                     # duplicate wire ids inside a row
    coefs = np.frombuffer((BN254_R - 1).to_bytes(32, "little") * nnz, dtype=np.uint8).reshape(nnz, 32)
    empty = (np.zeros(len(lens) + 1, dtype=np.int64), np.zeros(0, np.uint32), np.zeros((0, 32), np.uint8))
    data = R.write_r1cs(empty, (rp, wires, coefs), empty, 5, 1, 1, 2)
    h, cons = R.read_constraints(data)
    assert (h.nPubOut, h.nPubIn, h.nPrvIn, h.nConstraints) == (1, 1, 2, len(lens))
    for k, (a, b, c) in enumerate(cons):
        assert a == [] and c == []
        assert b == [(int(wires[t]), BN254_R - 1) for t in range(rp[k], rp[k + 1])]


def test_multiplier2_bytes_are_the_documented_format():
    lc = lambda *terms: struct.pack("<I", len(terms)) + b"".join(struct.pack("<I", w) + v.to_bytes(32, "little") for w, v in terms)
    sec1 = struct.pack("<I", 32) + BN254_R.to_bytes(32, "little") + struct.pack("<IIIIQI", 4, 0, 1, 2, 4, 1)
    sec2 = lc((2, 1)) + lc((3, 1)) + lc((1, 1))
    sec3 = b"".join(struct.pack("<Q", i) for i in range(4))
    want = b"r1cs" + struct.pack("<II", 1, 3)
    for sid, payload in ((1, sec1), (2, sec2), (3, sec3)):
        want += struct.pack("<IQ", sid, len(payload)) + payload
    assert multiplier2_bytes() == want


def test_writer_handles_2p20_constraints_quickly():
    import time
    m = 1 << 20
    rp = np.arange(m + 1, dtype=np.int64) * 2
    one = np.zeros((2 * m, 32), np.uint8)
    one[:, 0] = 1
    mat = (rp, np.ones(2 * m, np.uint32), one)
    t = time.time()
    data = R.write_r1cs(mat, mat, mat, 2, 0, 1)
    assert time.time() - t < 20
    assert len(data) == 12 + 3 * 12 + (4 + 32 + 16 + 8 + 4) + m * 3 * (4 + 2 * 36) + 2 * 8


@pytest.mark.parametrize("damage", ["magic", "version", "truncated", "table", "custom_gates", "prime", "no_constraints"])
def test_bad_files_are_refused_on_the_host(tmp_path, damage):
    good = multiplier2_bytes()
    if damage == "magic":
        data, msg = b"zkey" + good[4:], "Invalid file type"
    elif damage == "version":
        data, msg = good[:4] + struct.pack("<I", 2) + good[8:], "Invalid version"
    elif damage == "truncated":
        data, msg = good[:-20], "truncated"
    elif damage == "table":
        data, msg = good[:20], "truncated"
    elif damage == "prime":
        data, msg = good[:12 + 12 + 4] + (BN254_R + 2).to_bytes(32, "little") + good[12 + 12 + 4 + 32:], "curve not supported"
    elif damage == "no_constraints":
        sec1 = struct.pack("<I", 32) + BN254_R.to_bytes(32, "little") + struct.pack("<IIIIQI", 4, 0, 1, 2, 4, 1)
        data, msg = b"r1cs" + struct.pack("<IIIQ", 1, 1, 1, len(sec1)) + sec1, "no constraints"
    else:
        data, msg = good[:8] + struct.pack("<I", 4) + good[12:] + struct.pack("<IQ", 4, 4) + b"\0" * 4, "custom gates"
    with pytest.raises(ValueError, match=msg):
        R.open_r1cs(data)
    # the program reports the same before it asks for a device (no GPU here: the message is about the file)
    p = tmp_path / "c.r1cs"
    p.write_bytes(data)
    r = run(str(p), golden_path("multiplier2", "witness.wtns"))
    assert r.returncode == 255, r.stderr
    assert r.stderr.strip() and "device" not in r.stderr, r.stderr


def test_wtnscheck_usage_and_exit_code():
    r = run()
    assert r.returncode == 255
    assert r.stderr == "Invalid number of parameters:\nUsage: wtnscheck <circuit.r1cs> <witness.wtns>\n"
    assert run("a").returncode == 255
    assert run("/nonexistent.r1cs", "x").returncode == 255


def test_wtnscheck_refuses_a_witness_of_another_circuit_before_the_device(tmp_path):
    p = tmp_path / "m.r1cs"
    p.write_bytes(multiplier2_bytes())
    r = run(str(p), golden_path("r1cs_n8", "witness.wtns"))
    assert r.returncode == 255 and "nVars" in r.stderr, r.stderr


def test_r1cs_object_needs_a_gpu():
    import rapidsnark_old_amd as zk
    try:
        have_gpu = zk.device_count() > 0
    except zk.ZkHipError:
        have_gpu = False
    if have_gpu:
        ck = zk.R1cs(multiplier2_bytes())
        assert ck.check(golden_path("multiplier2", "witness.wtns")).ok
        ck.close()
    else:
        with pytest.raises(zk.ZkHipError):
            zk.R1cs(multiplier2_bytes())


# ---------------------------------------------------------------- wtnscheck: the exact exit code, stdout and stderr
def exact_case(name, d):
    """-> argv of one refusal; the files are written into d, which is the program's directory"""
    r1cs, wtns = multiplier2_bytes(), open(golden_path("multiplier2", "witness.wtns"), "rb").read()
    head = 12 + 12                                    # section 1 leads both files: n8, the prime, then the counts
    if name == "r1cs_other_prime":
        r1cs = r1cs[:head + 4] + (BN254_R + 2).to_bytes(32, "little") + r1cs[head + 36:]
    elif name == "r1cs_custom_gates":
        r1cs = r1cs[:8] + struct.pack("<I", 4) + r1cs[12:] + struct.pack("<IQ", 4, 4) + bytes(4)
    elif name == "r1cs_n8_48":
        r1cs = r1cs[:head] + struct.pack("<I", 48) + r1cs[head + 4:]
    elif name == "wtns_other_prime":
        wtns = wtns[:head + 4] + (BN254_R + 2).to_bytes(32, "little") + wtns[head + 36:]
    elif name == "wtns_n8_48":
        wtns = wtns[:head] + struct.pack("<I", 48) + wtns[head + 4:]
    elif name == "wtns_is_a_zkey":
        wtns = open(golden_path("multiplier2", "circuit.zkey"), "rb").read()
    elif name == "wtns_version_3":
        wtns = wtns[:4] + struct.pack("<I", 3) + wtns[8:]
    elif name == "wtns_of_another_circuit":
        wtns = open(golden_path("r1cs_n8", "witness.wtns"), "rb").read()
    elif name == "wtns_values_cut_short":             # section 2 holds one value less than the header's nVars
        at = head + 40 + 4
        size = int.from_bytes(wtns[at:at + 8], "little")
        wtns = wtns[:at] + (size - 32).to_bytes(8, "little") + wtns[at + 8:-32]
    for fname, data in (("c.r1cs", r1cs), ("w.wtns", wtns)):
        if name != "wtns_missing" or fname != "w.wtns":
            with open(os.path.join(d, fname), "wb") as f:
                f.write(data)
    return ("c.r1cs",) if name == "one_argument" else ("c.r1cs", "w.wtns")


EXACT = {      # what the programs of the commit before the host helpers were shared printed: (exit code, stdout, stderr)
    "one_argument": (255, "", "Invalid number of parameters:\nUsage: wtnscheck <circuit.r1cs> <witness.wtns>\n"),
    "r1cs_other_prime": (255, "", "r1cs curve not supported\n"),
    "r1cs_custom_gates": (255, "", "r1cs custom gates are not supported: Groth16 cannot use them\n"),
    "r1cs_n8_48": (255, "", "r1cs: only 256-bit fields are supported\n"),
    "wtns_other_prime": (255, "", "different wtns curve\n"),
    "wtns_n8_48": (255, "", "wtns: only 256-bit fields are supported\n"),
    "wtns_is_a_zkey": (255, "", "Invalid file type. It should be wtns and it us zkey\n"),
    "wtns_version_3": (255, "", "Invalid version. It should be <=2 and it us 3\n"),
    "wtns_of_another_circuit": (255, "", "witness does not match the r1cs (nVars 9, nWires 4)\n"),
    "wtns_values_cut_short": (255, "", "witness does not match the r1cs (nVars 4, nWires 4)\n"),
    "wtns_missing": (255, "", "open: No such file or directory\n"),
}


@pytest.mark.parametrize("name", sorted(EXACT))
def test_wtnscheck_exact_refusals_before_the_device(name, tmp_path):
    argv = exact_case(name, str(tmp_path))
    res = subprocess.run([WTNSCHECK, *argv], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert (res.returncode, res.stdout, res.stderr) == EXACT[name]
