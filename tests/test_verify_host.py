"""The host half of verification, none of which touches a device: the header and the exports, the loaders of proof.json,
public.json and both key forms against the oracle's byte encodings, and `verifier`'s argument and file errors, every one of
them refused before any device call."""
import json
import os
import re
import subprocess

import pytest

from conftest import CIRCUITS, ROOT, golden_json, golden_path

from oracle import bn254 as bn
from rapidsnark_old_amd import lib as L, verify as V
from rapidsnark_old_amd.binfile import BinFile
from rapidsnark_old_amd.zkey import load_zkey_header, _vk_json

QM, RM = bn.Q_MOD, bn.R_MOD
VERIFIER = os.path.join(ROOT, "rapidsnark-old_amd", "verifier")
SYMBOLS = ["zk_pairing", "zk_vkey_create", "zk_vkey_destroy", "zk_vkey_verify"]


def vk_json_of(name):
    """snarkjs's verification_key.json of a golden key, from its own sections 2 and 3 (zkey._vk_json: what `zkeynew` writes)"""
    f = BinFile(golden_path(name, "circuit.zkey"), "zkey", 1)
    h = load_zkey_header(f)
    return _vk_json(h, h.vk_delta2, bytes(f.getSectionData(3)))


def g1j(j):
    return None if len(j) > 2 and int(j[2]) == 0 else (int(j[0]), int(j[1]))


def g2j(j):
    return ((int(j[0][0]), int(j[0][1])), (int(j[1][0]), int(j[1][1])))


def test_header_declares_the_symbols_and_the_verdicts():
    text = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert "typedef struct zk_vkey zk_vkey;" in text and "zk_vkey_view" in text
    for name, value in (("ZK_VERIFY_OK", 0), ("ZK_VERIFY_INVALID", 1), ("ZK_VERIFY_MALFORMED", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
        assert getattr(L, name) == value
    assert (V.VERIFY_OK, V.VERIFY_INVALID, V.VERIFY_MALFORMED) == (0, 1, 2)


def test_library_exports_the_symbols():
    lib = L.load_library()
    for name in SYMBOLS:
        assert name in L.EXPORTS and hasattr(lib, name), name


def test_package_exports():
    import rapidsnark_old_amd as zk
    for name in ("pairing", "VerificationKey", "groth16_verify"):
        assert hasattr(zk, name), name
    src = open(os.path.join(ROOT, "rapidsnark-old_amd", "verify.py")).read()
    assert "oracle" not in re.sub(r'""".*?"""', "", src, flags=re.S)       # the binding does not import the test oracle


@pytest.mark.parametrize("name", CIRCUITS)
def test_proof_and_public_loaders(name):
    pj = golden_json(name, "proof.json")
    want = bn.g1_to_bytes(g1j(pj["pi_a"])) + bn.g2_to_bytes(g2j(pj["pi_b"])) + bn.g1_to_bytes(g1j(pj["pi_c"]))
    assert V.load_proof(golden_path(name, "proof.json")) == want
    assert want.hex() == golden_json(name, "meta.json")["proof_bytes"]
    pub = golden_json(name, "public.json")
    got = V.load_public(golden_path(name, "public.json"))
    assert got == b"".join(int(x).to_bytes(32, "little") for x in (pub or []))
    if name == "r1cs_nopub":
        assert pub is None and got == b""               # `null`: nPublic = 0


@pytest.mark.parametrize("name", ["multiplier2", "r1cs_nopub", "r1cs_n64"])
def test_both_key_forms_give_the_same_bytes(name, tmp_path):
    f = BinFile(golden_path(name, "circuit.zkey"), "zkey", 1)
    h = load_zkey_header(f)
    from_zkey = V.VerificationKey.read_zkey(golden_path(name, "circuit.zkey"))
    assert tuple(bytes(x) for x in from_zkey) == (h.vk_alpha1, h.vk_beta2, h.vk_gamma2, h.vk_delta2, bytes(f.getSectionData(3)))
    j = vk_json_of(name)
    j["vk_alphabeta_12"] = [[["1", "2"]] * 3] * 2        # ignored
    p = tmp_path / "vk.json"
    p.write_text(json.dumps(j))
    from_json = V.VerificationKey.read_json(str(p))
    assert tuple(bytes(x) for x in from_json) == tuple(bytes(x) for x in from_zkey)
    assert from_json[0] == bn.g1_to_bytes(g1j(j["vk_alpha_1"])) and from_json[2] == bn.g2_to_bytes(g2j(j["vk_gamma_2"]))
    assert len(from_json[4]) == 64 * (h.nPublic + 1)


def test_the_projective_third_coordinate_is_honoured():
    P = bn.G1.mul(bn.G1.gen, 12345)
    Q = bn.G2.mul(bn.G2.gen, 6789)
    assert V.g1_bytes([str(P[0]), str(P[1])]) == bn.g1_to_bytes(P)
    assert V.g1_bytes([str(P[0]), str(P[1]), "1"]) == bn.g1_to_bytes(P)
    assert V.g1_bytes([str(P[0]), str(P[1]), "0"]) == bytes(64)
    assert V.g1_bytes([P[0] * 7 % QM, P[1] * 7 % QM, 7]) == bn.g1_to_bytes(P)      # x / z, y / z; bare numbers too
    assert V.g2_bytes([[str(c) for c in Q[0]], [str(c) for c in Q[1]]]) == bn.g2_to_bytes(Q)
    assert V.g2_bytes([[str(c) for c in Q[0]], [str(c) for c in Q[1]], ["1", "0"]]) == bn.g2_to_bytes(Q)
    assert V.g2_bytes([[str(c) for c in Q[0]], [str(c) for c in Q[1]], ["0", "0"]]) == bytes(128)
    z = (3, 5)
    assert V.g2_bytes([list(bn.f2_mul(Q[0], z)), list(bn.f2_mul(Q[1], z)), list(z)]) == bn.g2_to_bytes(Q)
    # a coordinate that is not below q reaches the library as written: the device check refuses it, not the loader
    assert V.g1_bytes([str(QM), "2"])[:32] == QM.to_bytes(32, "little")
    with pytest.raises(ValueError):
        V.g1_bytes([str(1 << 256), "2"])
    with pytest.raises(ValueError):
        V.g1_bytes(["12x", "2"])


def test_argument_checks_without_a_device():
    with pytest.raises(ValueError):
        V.pairing(bytes(64), bytes(64))                   # a G2 point is 128 bytes
    with pytest.raises(ValueError):
        V.VerificationKey(bytes(64), bytes(128), bytes(128), bytes(64), bytes(64))
    lib = L.load_library()
    assert lib.zk_pairing(None, None, None, 0, 0, -1) != 0 and b"group" in lib.zk_last_error()
    assert lib.zk_pairing(None, None, None, 0, 1, -1) == 0      # nothing to do: no device is needed


# ---------------------------------------------------------------- verifier: refused before any device is needed
def run(*args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")      # no device, even where there is one
    return subprocess.run([VERIFIER] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=60)


def refused(r, *words):
    assert r.returncode == 255 and r.stdout == "" and r.stderr.strip(), (r.returncode, r.stdout, r.stderr)
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert "device" not in r.stderr.lower(), r.stderr      # the input error came first


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("verifier")
    vk = d / "vk.json"
    vk.write_text(json.dumps(vk_json_of("multiplier2")))
    return {"dir": d, "vk": vk, "zkey": golden_path("multiplier2", "circuit.zkey"), "public": golden_path("multiplier2", "public.json"),
            "proof": golden_path("multiplier2", "proof.json")}


def test_verifier_argument_count(files):
    for args in ([], [files["vk"]], [files["vk"], files["public"]], [files["vk"], files["public"], files["proof"], "x"]):
        r = run(*args)
        assert r.returncode == 255 and "Usage: verifier" in r.stderr and r.stdout == ""


def test_verifier_missing_files(files):
    missing = files["dir"] / "nothing.json"
    refused(run(missing, files["public"], files["proof"]), "nothing.json")
    refused(run(files["vk"], missing, files["proof"]), "nothing.json")
    refused(run(files["zkey"], files["public"], missing), "nothing.json")


def test_verifier_broken_json(files):
    bad = files["dir"] / "bad.json"
    bad.write_text(open(files["proof"]).read()[:-5])
    refused(run(files["vk"], files["public"], bad), "JSON")
    bad.write_text('["33", ]')
    refused(run(files["vk"], bad, files["proof"]), "JSON")


def test_verifier_protocol_and_curve(files):
    p = files["dir"] / "k.json"
    for key, value, word in (("protocol", "plonk", "groth16"), ("curve", "bls12381", "bn128")):
        j = vk_json_of("multiplier2")
        j[key] = value
        p.write_text(json.dumps(j))
        refused(run(p, files["public"], files["proof"]), word, value)
    j = vk_json_of("multiplier2")
    j["curve"] = "bn254"                                    # the other name of the same curve passes the input checks
    p.write_text(json.dumps(j))
    r = run(p, files["public"], files["proof"])
    assert r.returncode == 255 and "curve" not in r.stderr
    pj = golden_json("multiplier2", "proof.json")
    pj["protocol"] = "fflonk"
    p.write_text(json.dumps(pj))
    refused(run(files["vk"], files["public"], p), "groth16")


def test_verifier_ic_count(files):
    p = files["dir"] / "pub2.json"
    p.write_text('["33", "1"]')
    refused(run(files["vk"], p, files["proof"]), "2 IC points for 2 public signals")
    refused(run(files["zkey"], p, files["proof"]), "2 IC points for 2 public signals")
    p.write_text("null")
    refused(run(files["vk"], p, files["proof"]), "2 IC points for 0 public signals")


def test_verifier_non_numeric_values(files):
    p = files["dir"] / "nn.json"
    pj = golden_json("multiplier2", "proof.json")
    pj["pi_a"][0] = "12ab"
    p.write_text(json.dumps(pj))
    refused(run(files["vk"], files["public"], p), "pi_a[0]", "decimal")
    pj = golden_json("multiplier2", "proof.json")
    pj["pi_b"][1][0] = "-5"
    p.write_text(json.dumps(pj))
    refused(run(files["vk"], files["public"], p), "pi_b[1][0]")
    pj = golden_json("multiplier2", "proof.json")
    del pj["pi_c"]
    p.write_text(json.dumps(pj))
    refused(run(files["vk"], files["public"], p), "pi_c")
    p.write_text('["thirty-three"]')
    refused(run(files["vk"], p, files["proof"]), "public signal 0")
    j = vk_json_of("multiplier2")
    j["IC"][1][1] = str(1 << 256)
    p.write_text(json.dumps(j))
    refused(run(p, files["public"], files["proof"]), "IC[1][1]")


def test_verifier_key_that_is_neither_form(files):
    refused(run(golden_path("multiplier2", "witness.wtns"), files["public"], files["proof"]), "neither a verification_key.json nor a .zkey")
    p = files["dir"] / "list.json"
    p.write_text("[1, 2, 3]")
    refused(run(p, files["public"], files["proof"]), "neither a verification_key.json nor a .zkey")
    p.write_bytes(open(files["zkey"], "rb").read()[:300])      # a .zkey cut short
    r = run(p, files["public"], files["proof"])
    assert r.returncode == 255 and r.stderr.strip() and r.stdout == ""


def test_verifier_reaches_the_device_only_with_good_inputs(files):
    """every input check passed: what is left is the device, which this environment hides"""
    r = run(files["vk"], files["public"], files["proof"])
    assert r.returncode == 255 and r.stdout == "" and "device" in r.stderr.lower(), (r.returncode, r.stderr)


# ---------------------------------------------------------------- verifier: the exact exit code, stdout and stderr
def exact_case(name, d):
    """-> argv of one refusal; the files are written into d, which is the program's directory"""
    vk, pub, proof = vk_json_of("multiplier2"), golden_json("multiplier2", "public.json"), golden_json("multiplier2", "proof.json")
    key = "k.json"
    if name == "coordinate_of_78_digits":
        proof["pi_a"][1] = "9" * 78
    elif name == "coordinate_2p256_in_the_key":
        vk["vk_beta_2"][0][1] = str(1 << 256)
    elif name == "ic_empty":
        vk["IC"] = []
    elif name == "ic_not_a_list":
        vk["IC"] = "x"
    elif name == "key_without_alpha":
        del vk["vk_alpha_1"]
    elif name == "public_not_a_list":
        pub = {"a": 1}
    elif name == "public_empty_string":
        pub = [""]
    elif name == "public_2p256":
        pub = [str(1 << 256)]
    elif name == "proof_not_an_object":
        proof = [1]
    elif name == "proof_point_too_short":
        proof["pi_a"] = ["1"]
    elif name == "proof_g2_coordinate_too_short":
        proof["pi_b"][0] = ["1"]
    elif name == "proof_curve":
        proof["curve"] = "bls12381"
    if name.startswith("zkey_"):
        key = "k.zkey"
        data = open(golden_path("multiplier2", "circuit.zkey"), "rb").read()
        at = 12                                       # sections 1, 2, 3 lead the golden key
        head = lambda at: int.from_bytes(data[at + 4:at + 12], "little")
        s2 = at + 12 + head(at)
        s3 = s2 + 12 + head(s2)
        if name == "zkey_section_3_disagrees_with_nPublic":
            end = s3 + 12 + head(s3)
            data = data[:s3 + 4] + (head(s3) + 64).to_bytes(8, "little") + data[s3 + 12:end] + bytes(64) + data[end:]
        elif name == "zkey_other_curve":
            data = data[:s2 + 16] + RM.to_bytes(32, "little") + data[s2 + 48:]
        with open(os.path.join(d, key), "wb") as f:
            f.write(data)
    elif name != "key_missing":
        with open(os.path.join(d, key), "w") as f:
            json.dump(vk, f)
    for fname, j in (("public.json", pub), ("proof.json", proof)):
        with open(os.path.join(d, fname), "w") as f:
            json.dump(j, f)
    return () if name == "usage" else (key, "public.json", "proof.json")


EXACT = {      # what the programs of the commit before the host helpers were shared printed: (exit code, stdout, stderr)
    "usage": (255, "", "Invalid number of parameters:\nUsage: verifier <verification_key.json | circuit.zkey> <public.json> <proof.json>\n"),
    "coordinate_of_78_digits": (255, "", "pi_a[1] is not a decimal integer below 2^256\n"),
    "coordinate_2p256_in_the_key": (255, "", "vk_beta_2[0][1] is not a decimal integer below 2^256\n"),
    "ic_empty": (255, "", "k.json: IC is not a list of points\n"),
    "ic_not_a_list": (255, "", "k.json: IC is not a list of points\n"),
    "key_without_alpha": (255, "", 'k.json: no "vk_alpha_1"\n'),
    "public_not_a_list": (255, "", "public.json: a list of public signals (or null) expected\n"),
    "public_empty_string": (255, "", "public.json: public signal 0 is not a decimal integer below 2^256\n"),
    "public_2p256": (255, "", "public.json: public signal 0 is not a decimal integer below 2^256\n"),
    "proof_not_an_object": (255, "", "proof.json: a proof object expected\n"),
    "proof_point_too_short": (255, "", "pi_a is not an array of at least 2 elements\n"),
    "proof_g2_coordinate_too_short": (255, "", "pi_b[0] is not an array of at least 2 elements\n"),
    "proof_curve": (255, "", 'proof.json: curve "bls12381" is not bn128\n'),
    "zkey_section_3_disagrees_with_nPublic": (255, "", "zkey section 3 holds 192 bytes, nPublic = 1 implies 128\n"),
    "zkey_other_curve": (255, "", "zkey curve not supported\n"),
    "key_missing": (255, "", "k.json: cannot be opened\n"),
}


@pytest.mark.parametrize("name", sorted(EXACT))
def test_verifier_exact_refusals_before_the_device(name, tmp_path):
    argv = exact_case(name, str(tmp_path))
    res = subprocess.run([VERIFIER, *argv], capture_output=True, text=True, timeout=60, cwd=str(tmp_path),
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
    assert (res.returncode, res.stdout, res.stderr) == EXACT[name]
