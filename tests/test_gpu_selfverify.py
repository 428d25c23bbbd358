"""ZKHIP_SELFVERIFY=1: `prover` and `proverServer` verify each proof against the .zkey's own verification key before they
hand it out.  A .zkey whose delta_1 is replaced by 2 delta_1 still loads (the point is on the curve) and gives proofs that
do not verify: with the switch on they are refused, without it everything is as before."""
import json
import urllib.error
import os
import stat
import struct
import subprocess
import time

import pytest

from conftest import ROOT, golden_bytes, golden_json, golden_path
from test_server import SERVER, _free_port, _http, _le_hex

pytestmark = pytest.mark.gpu
PROVER = os.path.join(ROOT, "rapidsnark-old_amd", "prover")
NAME = "r1cs_n64"
MESSAGE = "proof failed self-verification (verdict 1)"
DELTA1_AT = 4 + 32 + 4 + 32 + 12 + 64 + 64 + 128 + 128      # offset of vk_delta_1 in section 2 of a .zkey


def corrupted_zkey(zk):
    """the golden .zkey with delta_1 of section 2 replaced by 2 delta_1"""
    z = bytearray(golden_bytes(NAME, "circuit.zkey"))
    at, n = 12, struct.unpack_from("<I", z, 8)[0]
    for _ in range(n):
        sec, size = struct.unpack_from("<IQ", z, at)
        if sec == 2:
            d = at + 12 + DELTA1_AT
            z[d:d + 64] = zk.g1_mul(bytes(z[d:d + 64]), 2)
            return bytes(z)
        at += 12 + size
    raise AssertionError("no section 2")


def fixed_rs():
    meta = golden_json(NAME, "meta.json")
    return {"ZKHIP_FIXED_R": _le_hex(meta["r"]), "ZKHIP_FIXED_S": _le_hex(meta["s"])}


def prove(zkey, out, **env):
    return subprocess.run([PROVER, str(zkey), golden_path(NAME, "witness.wtns"), str(out / "proof.json"), str(out / "public.json")],
                          capture_output=True, text=True, errors="replace", env=dict(os.environ, **fixed_rs(), **env), timeout=300)


def test_prover_checks_its_own_proof(zk, tmp_path):
    r = prove(golden_path(NAME, "circuit.zkey"), tmp_path, ZKHIP_SELFVERIFY="1", ZKHIP_VERBOSE="1")
    assert r.returncode == 0, r.stderr
    assert "[prover] self-verify:" in r.stderr
    assert (tmp_path / "proof.json").read_bytes() == golden_bytes(NAME, "proof.json")
    assert (tmp_path / "public.json").read_bytes() == golden_bytes(NAME, "public.json")

    bad = tmp_path / "bad.zkey"
    bad.write_bytes(corrupted_zkey(zk))
    for value in (None, "0"):                                   # the switch off: the wrong proof is written, as before
        out = tmp_path / ("off_%s" % value)
        out.mkdir()
        r = prove(bad, out, **({} if value is None else {"ZKHIP_SELFVERIFY": value}))
        assert r.returncode == 0, r.stderr
        assert (out / "public.json").read_bytes() == golden_bytes(NAME, "public.json")
        assert (out / "proof.json").read_bytes() != golden_bytes(NAME, "proof.json")
    out = tmp_path / "on"
    out.mkdir()
    r = prove(bad, out, ZKHIP_SELFVERIFY="1")
    assert r.returncode == 255 and r.stderr.strip().splitlines()[-1] == MESSAGE, (r.returncode, r.stderr)
    assert os.listdir(out) == []


def start_server(zk, tmp_path, **env):
    """proverServer with the golden circuit as `good` and the corrupted key as `bad`, both fed the golden witness"""
    build = tmp_path / "build"
    build.mkdir()
    (tmp_path / "good.zkey").write_bytes(golden_bytes(NAME, "circuit.zkey"))
    (tmp_path / "bad.zkey").write_bytes(corrupted_zkey(zk))
    for n in ("good", "bad"):
        gen = build / n                                         # stand-in for the circom witness generator
        gen.write_text("#!/bin/sh\ncp %s \"$2\"\n" % golden_path(NAME, "witness.wtns"))
        gen.chmod(gen.stat().st_mode | stat.S_IEXEC)
    port = _free_port()
    srv = subprocess.Popen([SERVER, str(port), str(tmp_path / "good.zkey"), str(tmp_path / "bad.zkey")], cwd=tmp_path,
                           env=dict(os.environ, ZKHIP_SELFVERIFY="1", **fixed_rs(), **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    for _ in range(600):
        try:
            _http(port, "GET", "/status")
            return srv, port
        except (ConnectionError, urllib.error.URLError):
            assert srv.poll() is None, srv.stderr.read().decode()
            time.sleep(0.1)
    raise AssertionError("server did not come up")


def test_server_refuses_the_proof_of_a_corrupted_key(zk, tmp_path):
    srv, port = start_server(zk, tmp_path)
    try:
        def run(circuit):
            assert _http(port, "POST", "/input/" + circuit, b"{}")[0] == 200
            for _ in range(3000):
                st = json.loads(_http(port, "GET", "/status")[1])
                if st["status"] != "busy":
                    return st
                time.sleep(0.01)
            raise AssertionError("stuck busy")

        st = run("good")
        assert st["status"] == "success" and st["proof"] == golden_bytes(NAME, "proof.json").decode()
        st = run("bad")
        assert st["status"] == "failed" and st["error"] == MESSAGE, st
        assert run("good")["status"] == "success" and srv.poll() is None
    finally:
        srv.terminate()
        srv.wait(10)


def test_in_queue_mode_the_bad_job_fails_alone(zk, tmp_path):
    srv, port = start_server(zk, tmp_path, ZKHIP_QUEUE="16", ZKHIP_WORKERS="0")
    try:
        jobs = []
        for circuit in ("good", "bad", "good", "good"):
            st, body, _ = _http(port, "POST", "/input/" + circuit, b"{}")
            assert st == 200, body
            jobs.append(json.loads(body)["job"])
        docs = []
        for job in jobs:
            for _ in range(3000):
                doc = json.loads(_http(port, "GET", "/status/%d" % job)[1])
                if doc["status"] != "busy":
                    break
                time.sleep(0.01)
            docs.append(doc)
        assert [d["status"] for d in docs] == ["success", "failed", "success", "success"], docs
        assert docs[1]["error"] == MESSAGE
        for d in (docs[0], docs[2], docs[3]):
            assert d["proof"] == golden_bytes(NAME, "proof.json").decode()
        assert srv.poll() is None
    finally:
        srv.terminate()
        srv.wait(10)
