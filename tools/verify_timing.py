#!/usr/bin/env python3
"""Kernel time per proof of zk_vkey_verify and per pairing of zk_pairing, and the wall time of the calls, written to
profiles/verify_timing.txt.

    python tools/verify_timing.py [--sizes 1 64 4096 65536] [--profiled 4096 65536 262144] [--reps 5] [--golden r1cs_n64]

  * the proofs: re-randomised copies of one golden proof (A' = t A, B' = t^-1 B, C' = C, the multiples made by the
    fixed-base kernels), all valid and distinct, verified against the golden key in ONE chunk (ZKHIP_VERIFY_CHUNK = n);
  * wall: a process without the profiler calls VerificationKey.verify once to warm up and --reps times per size, and
    zk_pairing at group = 1 on the proofs' own (A, B) pairs the same way; median, least and largest;
  * kernels: per profiled size one process under `rocprofv3 --kernel-trace` makes one warm-up and --reps timed calls of
    each; per kernel the median, least and largest duration of the timed launches and the median per proof.
The only other verifier in the tree is the Python oracle (oracle/pairing.py through tools/refcheck/verify.py, about a
second per proof on one core, test infrastructure): named as a reference point, not as a target.
Every GPU step is a process of its own under `timeout`; the first one that fails ends the tool."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from oracle.bn254 import R_MOD  # noqa: E402

KERNELS = ["k_verify_check", "k_verify_miller", "k_verify_final", "k_pair_check", "k_miller_groups", "k_final_exp"]


def limited(cmd, seconds):
    return ["timeout", "-k", "10", str(seconds)] + cmd


def kernel_durations(prof_dir):
    """-> {kernel name: [duration ms of every dispatch, in start order]}"""
    files = glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return {}
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for r in rows:
        out.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    return out


def stat(d):
    d = sorted(d)
    return d[len(d) // 2], d[0], d[-1]


def batch(zk, golden, n):
    """n valid, distinct proofs of the golden statement and their public signals"""
    from rapidsnark_old_amd import verify as V
    gold = os.path.join(ROOT, "tests", "golden", golden)
    proof, public = V.load_proof(os.path.join(gold, "proof.json")), V.load_public(os.path.join(gold, "public.json"))
    t = [(0x9E3779B97F4A7C15 * (i + 1) + 12345) % R_MOD or 1 for i in range(n)]
    a = zk.fixed_base_g1(proof[:64], t).reshape(n, 64)
    b = zk.fixed_base_g2(proof[64:192], [pow(x, -1, R_MOD) for x in t]).reshape(n, 128)
    c = np.tile(np.frombuffer(proof[192:], dtype=np.uint8), (n, 1))
    return np.ascontiguousarray(np.concatenate([a, b, c], axis=1)).reshape(-1), public * n, os.path.join(gold, "circuit.zkey")


def child(golden, sizes, reps, out_path):
    """the calls themselves: one warm-up and `reps` timed ones per size (run with or without the profiler by main)"""
    import rapidsnark_old_amd as zk
    walls = {}
    for n in sizes:
        os.environ["ZKHIP_VERIFY_CHUNK"] = str(n)
        proofs, publics, zkey = batch(zk, golden, n)
        pr = proofs.reshape(n, 256)
        g1, g2 = np.ascontiguousarray(pr[:, :64]).reshape(-1), np.ascontiguousarray(pr[:, 64:192]).reshape(-1)
        with zk.VerificationKey.from_zkey(zkey) as vk:
            tv, tp = [], []
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                verdict = vk.verify(proofs, publics)
                t1 = time.perf_counter()
                zk.pairing(g1, g2, group=1)
                t2 = time.perf_counter()
                tv.append(t1 - t0)
                tp.append(t2 - t1)
                if verdict.any():
                    print("a re-randomised proof did not verify", file=sys.stderr)
                    return 1
        walls[str(n)] = {"verify": tv[1:], "pairing": tp[1:]}
    with open(out_path, "w") as f:
        json.dump(walls, f)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 64, 4096, 65536])
    ap.add_argument("--profiled", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--golden", default="r1cs_n64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_timing.txt"))
    ap.add_argument("--child", nargs=2, metavar=("SIZES", "PATH"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.golden, [int(x) for x in args.child[0].split(",")], args.reps, args.child[1])
    if not shutil.which("rocprofv3"):
        raise SystemExit("rocprofv3 not found: kernel times come from nowhere else")
    me = [sys.executable, os.path.abspath(__file__), "--golden", args.golden, "--reps", str(args.reps), "--child"]
    tmp = tempfile.mkdtemp(prefix="verify_timing_")
    lines = []
    try:
        wj = os.path.join(tmp, "walls.json")
        subprocess.run(limited(me + [",".join(map(str, args.sizes)), wj], 600), check=True, timeout=700)
        walls = json.load(open(wj))
        lines.append("wall time of one call, %d timed calls after a warm-up (ms: median, least, largest; us per proof of the median)" % args.reps)
        for what, label in (("verify", "zk_vkey_verify"), ("pairing", "zk_pairing group = 1")):
            for n in args.sizes:
                m, lo, hi = stat([1e3 * x for x in walls[str(n)][what]])
                lines.append("  %-22s n = %6d  %10.3f %10.3f %10.3f   %10.2f us each" % (label, n, m, lo, hi, 1e3 * m / n))
        print("\n".join(lines), flush=True)
        for n in args.profiled:
            prof = os.path.join(tmp, "prof%d" % n)
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", prof, "-o", "verify", "--"] + me + [str(n), os.path.join(tmp, "w%d.json" % n)]
            subprocess.run(limited(cmd, 600), check=True, capture_output=True, timeout=700)
            durs = kernel_durations(prof)
            lines += ["", "kernels at n = %d, %d timed launches after a warm-up (ms: median, least, largest; us per proof or pair of the median)" % (n, args.reps)]
            total = {"k_verify": 0.0, "pairing": 0.0}
            for k in KERNELS:
                d = [v for name, v in durs.items() if k + "(" in name]
                if not d:
                    continue
                m, lo, hi = stat(d[0][-args.reps:])
                total["k_verify" if k.startswith("k_verify") else "pairing"] += m
                lines.append("  %-18s %10.3f %10.3f %10.3f   %10.2f us each" % (k, m, lo, hi, 1e3 * m / n))
            lines.append("  zk_vkey_verify's three kernels: %.3f ms, %.2f us per proof; zk_pairing's three: %.3f ms, %.2f us per pairing" % (
                total["k_verify"], 1e3 * total["k_verify"] / n, total["pairing"], 1e3 * total["pairing"] / n))
            print("\n".join(lines[-9:]), flush=True)
        try:
            clock = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        except (OSError, subprocess.SubprocessError):
            clock = ""
        clock = [ln.strip() for ln in clock.splitlines() if "sclk" in ln][:1]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = ["# tools/verify_timing.py: zk_vkey_verify and zk_pairing on one MI355X, re-randomised copies of the %s golden proof, one chunk per call" % args.golden,
           "# kernel times: rocprofv3 --kernel-trace, per launch; walls: time.perf_counter around the Python call (upload, kernels, download)",
           "# reference point, not a target: the Python oracle (tools/refcheck/verify.py) takes about a second per proof on one core",
           "# shader clock after the runs: " + (clock[0] if clock else "not read"), ""] + lines
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
