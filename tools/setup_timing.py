#!/usr/bin/env python3
"""Wall time and GPU time of `zkeynew` (the Groth16 setup on the GPU), written to profiles/setup_timing.txt.

    python tools/setup_timing.py [--sizes 16 20 22] [--out profiles/setup_timing.txt] [--no-prof]

  * zkgen circuit_like circuits at each size (zkgen.write_r1cs), with a trapdoor .ptau of power k from the key's own tau,
    alpha, beta (ptau.write_trapdoor_ptau): the key must prove (`prover`) and pass the trapdoor check;
  * at the largest size, three synthetic circuits with the circuit_like one's nnz (5 terms per constraint): wires spread
    evenly with full-size coefficients ("even"), the same with the constant wire in every B row and a power-law tail
    ("skewed"), and evenly spread with coefficients +-1 ("pm1").
Wall = the whole `zkeynew` process (both files read, the setup, the .zkey written).  GPU = the sum of its kernel times
from a second run under `rocprofv3 --kernel-trace --stats`, whose per-kernel table of the largest circuit_like run is
appended (--no-prof: wall only)."""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from oracle.bn254 import R_MOD as RM  # noqa: E402

BIN = os.path.join(ROOT, "rapidsnark-old_amd")


def run_zkeynew(r1cs, ptau, zkey, prof_dir=None):
    cmd = [os.path.join(BIN, "zkeynew"), r1cs, ptau, zkey]
    if prof_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof_dir, "-o", "setup", "--"] + cmd
    t = time.time()
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    return time.time() - t


def kernel_stats(prof_dir):
    """-> [(name, calls, total ms)] from rocprofv3's kernel_stats.csv"""
    files = glob.glob(os.path.join(prof_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return []
    rows = []
    with open(files[0]) as f:
        for r in csv.DictReader(f):
            rows.append((r["Name"], int(r["Calls"]), float(r["TotalDurationNs"]) / 1e6))
    return sorted(rows, key=lambda x: -x[2])


def synthetic_r1cs(kind, m, n_wires, n_public, rng):
    """A, B: 2 terms per constraint, C: 1 (circuit_like's nnz per constraint)"""
    from rapidsnark_old_amd import r1cs as R
    rowptr2 = np.arange(0, 2 * m + 1, 2, dtype=np.int64)
    rowptr1 = np.arange(m + 1, dtype=np.int64)
    if kind == "skewed":                         # the constant wire in every B row, the other wires by a power law
        zipf = lambda size: np.minimum(rng.zipf(1.3, size=size), n_wires - 1).astype(np.uint32)
        wa, wb, wc = zipf(2 * m), zipf(2 * m), zipf(m)
        wb[0::2] = 0
    else:
        wa, wb, wc = (rng.integers(0, n_wires, size=s, dtype=np.uint32) for s in (2 * m, 2 * m, m))

    def coefs(count):
        if kind == "pm1":
            c = np.zeros((count, 32), np.uint8)
            one = rng.random(count) < 0.5
            c[one, 0] = 1
            c[~one] = np.frombuffer((RM - 1).to_bytes(32, "little"), np.uint8)
            return c
        c = rng.integers(0, 256, size=(count, 32), dtype=np.uint8)
        c[:, 31] &= 0x1F                         # below 2^253 < r: full-size
        return c
    return R.write_r1cs((rowptr2, wa, coefs(2 * m)), (rowptr2, wb, coefs(2 * m)), (rowptr1, wc, coefs(m)), n_wires, 0, n_public)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 20, 22])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "setup_timing.txt"))
    ap.add_argument("--no-prof", action="store_true")
    args = ap.parse_args()
    import rapidsnark_old_amd as zk
    from rapidsnark_old_amd import synth, zkgen
    prof = not args.no_prof and shutil.which("rocprofv3")
    lines, table = [], []
    tmp = tempfile.mkdtemp(prefix="setup_timing_")
    try:
        for k in args.sizes:
            d = os.path.join(tmp, "k%d" % k)
            os.makedirs(d)
            key = zkgen.generate(k, 2, seed=0, circuit_like=True)
            f = lambda name: os.path.join(d, name)
            zkgen.write_r1cs(key, f("c.r1cs"))
            zkgen.write_wtns(key, f("w.wtns"))
            tau, alpha, beta = key["trap"]["toxic"][:3]
            t = time.time()
            zk.write_trapdoor_ptau(k, tau, alpha, beta, f("p.ptau"))
            t_ptau = time.time() - t
            wall = run_zkeynew(f("c.r1cs"), f("p.ptau"), f("c.zkey"))
            gpu = None
            if prof:
                run_zkeynew(f("c.r1cs"), f("p.ptau"), f("c2.zkey"), prof_dir=f("prof"))
                st = kernel_stats(f("prof"))
                gpu = sum(x[2] for x in st)
                if k == max(args.sizes):
                    table = st
            # the key proves and passes the trapdoor check (gamma = delta = 1)
            r, s = 0x0123456789ABCDEF, (1 << 200) + 12345
            le = lambda x: int(x).to_bytes(32, "little").hex()
            env = dict(os.environ, ZKHIP_FIXED_R=le(r), ZKHIP_FIXED_S=le(s))
            subprocess.run([os.path.join(BIN, "prover"), f("c.zkey"), f("w.wtns"), f("proof.json"), f("public.json")], env=env, check=True,
                           capture_output=True, timeout=900)
            k2 = dict(key, trap=dict(key["trap"], toxic=(tau, alpha, beta, 1, 1)))
            a, b, c = zkgen.expected_proof_dlogs(k2, r, s)
            want = zk.g1_mul(synth.g1_gen_bytes(), a) + zk.g2_mul(synth.g2_gen_bytes(), b) + zk.g1_mul(synth.g1_gen_bytes(), c)
            ok = open(f("proof.json")).read() == zk.proof_to_json(want)
            sizes = zk.ptau.setup_sizes(f("c.r1cs"), f("p.ptau"))
            lines.append("2^%d circuit_like  nVars %8d  nCoefs %9d  ptau(power %d) written in %5.1f s   zkeynew wall %6.2f s  GPU %s  proof %s" % (
                k, key["nVars"], sizes["nCoefs"], k, t_ptau, wall, "%8.1f ms" % gpu if gpu is not None else "   -", "PASS" if ok else "FAIL"))
            print(lines[-1], flush=True)
            if not ok:
                return 1
            if k == max(args.sizes):
                m, nw = key["nConstraints"], key["nVars"]
                rng = np.random.default_rng(0x5E7)
                for kind in ("even", "skewed", "pm1"):
                    with open(f(kind + ".r1cs"), "wb") as fh:
                        fh.write(synthetic_r1cs(kind, m, nw, 2, rng))
                    wall = run_zkeynew(f(kind + ".r1cs"), f("p.ptau"), f(kind + ".zkey"))
                    gpu = None
                    if prof:
                        run_zkeynew(f(kind + ".r1cs"), f("p.ptau"), f(kind + "2.zkey"), prof_dir=f("prof_" + kind))
                        gpu = sum(x[2] for x in kernel_stats(f("prof_" + kind)))
                    lines.append("2^%d %-14s nVars %8d  nnz %9d (5 per constraint)                     zkeynew wall %6.2f s  GPU %s" % (
                        k, kind, nw, 5 * m, wall, "%8.1f ms" % gpu if gpu is not None else "   -"))
                    print(lines[-1], flush=True)
                    for ext in (".zkey", "2.zkey"):
                        if os.path.exists(f(kind + ext)):
                            os.remove(f(kind + ext))
            shutil.rmtree(d, ignore_errors=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = ["# tools/setup_timing.py: `zkeynew circuit.r1cs pot.ptau circuit.zkey` on one MI355X",
           "# wall: the whole process (files read and checked, setup, .zkey written); GPU: sum of kernel times (rocprofv3)", ""] + lines
    if table:
        out += ["", "# rocprofv3 --kernel-trace --stats, 2^%d circuit_like run (kernel, calls, total ms)" % max(args.sizes)]
        out += ["%-90s %6d %10.2f" % (name[:90], calls, ms) for name, calls, ms in table]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
