#!/usr/bin/env python3
"""What a whole PLONK proof costs on one MI355X, written to profiles/plonk_prover_timing.txt.

    python tools/plonk_prover_timing.py [--reps 5] [--sizes 18 20 22]

At every log_n of --sizes, one process, a warm-up and --reps timed rounds, the two routes alternating:
  * chained: PlonkProver.prove, the five rounds on the device, the witness uploaded once;
  * staged: the route through the public entries that existed before (the challenges
    fixed): fr_ntt and Kzg.commit for the wires, plonk_permutation_product, fr_ntt and Kzg.commit for z, PlonkCircuit.quotient,
    the split on the host and three commits, PlonkOpening.evaluate and .open.  Every vector crosses PCIe at every step.
Kernel times of the chained route come from a process of its own under `rocprofv3 --kernel-trace` (no counters in that run),
cut into proofs at k_wire_gather and into rounds at the first k_scan_reduce, the third k_coset_load, k_poly_eval and
k_plonk_linearise, and summed by kind: the transforms, the multiplications (sort, accumulation, reduction), the rest.
Every GPU step is a child process under `timeout`.

The circuit is made for the tool, satisfiable by construction at any size without a host-side field library: q_L = s,
q_R = -s for a random polynomial s, the other selectors 0, a_map = b_map (so q_L a + q_R b = 0), sigma the identity
(s1 = X, s2 = k1 X, s3 = k2 X), the witness random.  The cost of a proof does not depend on the selectors' values; the seven
committed polynomials of a proof and both quotients have random-looking coefficients as in a real proof.  The reference
string is n + 6 powers of a known tau made by the tool, not a file."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from frscan_timing import scalars  # noqa: E402
from plonk_opening_timing import make_kzg  # noqa: E402
from verify_timing import limited, stat  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
K1, K2 = 2, 3
ALPHA, BETA, GAMMA, ZETA, V = 5, 7, 11, 0x1234567_89ABCDEF_01234567_89ABCDEF_55AA, 0x0FEDCBA9_87654321_0FEDCBA9_87654321_77
BLIND = list(range(101, 112))
ROUNDS = ("round 1", "round 2", "round 3", "round 4", "round 5")


def neg_mod_r(a):
    """r - x for rows 0 < x < r, 64-bit limbs: the borrow out of a limb is x_j > r_j, or x_j = r_j with a borrow coming in"""
    x = np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4)
    out = np.empty_like(x)
    borrow = np.zeros(x.shape[0], dtype=bool)
    for j in range(4):
        rj = np.uint64((R >> (64 * j)) & ((1 << 64) - 1))
        out[:, j] = rj - x[:, j] - borrow.astype(np.uint64)
        borrow = (x[:, j] > rj) | ((x[:, j] == rj) & borrow)
    return out.view(np.uint8).reshape(-1)


def le(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8)


def circuit(log_n):
    n = 1 << log_n
    s = scalars(n, 300 + log_n)
    zero = np.zeros(n * 32, dtype=np.uint8)

    def linear(k):
        p = zero.copy()
        p[32:64] = le([k])
        return p

    rng = np.random.default_rng(log_n)
    ab, c = rng.permutation(n).astype(np.uint32), rng.permutation(n).astype(np.uint32)
    return [s, neg_mod_r(s), zero, zero, zero, linear(1), linear(K1), linear(K2)], (ab, ab, c), scalars(n, 400 + log_n)


def add_at(row, at, k):
    v = (int.from_bytes(row[at * 32:(at + 1) * 32].tobytes(), "little") + k) % R
    row[at * 32:(at + 1) * 32] = le([v])


def blinded(zk, values, n, r):
    """coefficients of the values' interpolant + (r[0] + r[1] X + ..) Z_H, len(r) rows longer"""
    co = np.concatenate([np.frombuffer(zk.fr_ntt(values, inverse=True), dtype=np.uint8), np.zeros(len(r) * 32, dtype=np.uint8)])
    for j, rj in enumerate(r):
        add_at(co, j, -rj)
        add_at(co, n + j, rj)
    return co


def staged(zk, k, c, o, sig_v, maps, witness, n):
    """steps 1 to 5 through the public entries, the challenges fixed"""
    w = witness.reshape(-1, 32)
    vals = [np.ascontiguousarray(w[m]).reshape(-1) for m in maps]
    b = BLIND
    polys = [blinded(zk, v, n, r) for v, r in zip(vals, ([b[1], b[0]], [b[3], b[2]], [b[5], b[4]]))]
    pts = [k.commit(p) for p in polys]
    z_v, last = zk.plonk_permutation_product(vals, sig_v, [1, K1, K2], BETA, GAMMA)
    assert last == 1
    z = blinded(zk, z_v, n, [b[8], b[7], b[6]])
    pts.append(k.commit(z))
    t, t_len = c.quotient(polys[0], polys[1], polys[2], z, ALPHA, BETA, GAMMA)
    assert t_len <= 3 * n + 6
    lo, mid, hi = (np.concatenate([t[:n * 32], le([b[9]])]), np.concatenate([t[n * 32:2 * n * 32], le([b[10]])]), t[2 * n * 32:(3 * n + 6) * 32].copy())
    add_at(mid, 0, -b[9])
    add_at(hi, 0, -b[10])
    pts += [k.commit(p) for p in (lo, mid, hi)]
    ev = o.evaluate(polys[0], polys[1], polys[2], z, ZETA)
    wz, wzw, rz = o.open(lo, mid, hi, ALPHA, BETA, GAMMA, V)
    assert rz == 0
    return pts, ev, wz, wzw


def child(what, log_n, reps, out_path):
    import rapidsnark_old_amd as zk
    n = 1 << log_n
    circ, maps, witness = circuit(log_n)
    res = {}
    with make_kzg(zk, log_n) as k, zk.PlonkProver(k, *circ, K1, K2, *maps, n, 0) as p:
        proof = p.prove(witness, blind=BLIND)
        if what == "walls":
            assert zk.plonk_verify(p.vkey(), proof) == 0        # not in the traced child: its pairing kernel is no part of a proof
            sig_v = [zk.fr_ntt(s) for s in circ[5:]]
            with zk.PlonkCircuit(*circ, K1, K2) as c, zk.PlonkOpening(k, *circ, K1, K2) as o:
                tc, ts = [], []
                for _ in range(reps + 1):
                    t0 = time.perf_counter()
                    p.prove(witness, blind=BLIND)
                    tc.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    staged(zk, k, c, o, sig_v, maps, witness, n)
                    ts.append(time.perf_counter() - t0)
            res = {"chained": tc[1:], "staged": ts[1:], "info": p.info()}
        else:
            for _ in range(reps + 1):
                p.prove(witness, blind=BLIND)
    with open(out_path, "w") as fh:
        json.dump(res, fh)
    return 0


def kind(name):
    if "ntt" in name:
        return "transforms"
    if any(k in name for k in ("msm", "k_bin_", "k_scan_local", "k_scan_sums", "k_scan_add")):      # the sort's kernels with them
        return "multiplications"
    return "rest"


def proofs(prof_dir):
    """the trace cut into proofs and rounds -> [{round: {kind: ms}}], and {kernel name: ms} over all of them"""
    files = glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return [], {}
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    out, by_name, rnd, loads = [], {}, 0, 0
    for r in rows:
        name = r["Kernel_Name"]
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "k_wire_gather" in name:
            out.append({x: {} for x in ROUNDS})
            rnd, loads = 0, 0
        if not out:
            continue
        if "k_coset_load" in name:
            loads += 1
        if rnd == 0 and "k_scan_reduce" in name:
            rnd = 1
        elif rnd == 1 and "k_coset_load" in name and loads == 3:
            rnd = 2
        elif rnd == 2 and "k_poly_eval" in name:
            rnd = 3
        elif rnd == 3 and "k_plonk_linearise" in name:
            rnd = 4
        d = out[-1][ROUNDS[rnd]]
        d[kind(name)] = d.get(kind(name), 0.0) + ms
        found = re.search(r"k_\w+", name)
        short = found.group(0) if found else name
        by_name[short] = by_name.get(short, 0.0) + ms
    return out, by_name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[18, 20, 22])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_prover_timing.txt"))
    ap.add_argument("--child", nargs=3, metavar=("WHAT", "LOG_N", "PATH"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]), args.reps, args.child[2])
    if not shutil.which("rocprofv3"):
        raise SystemExit("rocprofv3 not found: kernel times come from nowhere else")
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--child"]
    kinds = ("transforms", "multiplications", "rest")
    lines = ["# tools/plonk_prover_timing.py: a whole PLONK proof on one MI355X; %d timed calls after a warm-up, medians" % args.reps,
             "# chained: PlonkProver.prove; staged: INTEGRATION section 16's steps 1 to 5 through the public entries, challenges fixed", ""]

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    for log_n in args.sizes:
        tmp = tempfile.mkdtemp(prefix="plonk_prover_timing_")
        try:
            wj = os.path.join(tmp, "walls.json")
            subprocess.run(limited(me + ["walls", str(log_n), wj], 400), check=True, timeout=460)
            wall = json.load(open(wj))
            prof = os.path.join(tmp, "traced")
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", prof, "-o", "plonkprove", "--"] + me + ["traced", str(log_n), os.path.join(tmp, "t.json")]
            subprocess.run(limited(cmd, 400), check=True, stdout=subprocess.DEVNULL, timeout=460)
            calls, by_name = proofs(prof)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        ch, st = stat([1e3 * x for x in wall["chained"]]), stat([1e3 * x for x in wall["staged"]])
        lines += ["log_n %d: %s" % (log_n, json.dumps(wall["info"], sort_keys=True)),
                  "  walls, ms: median, least, largest of time.perf_counter around the Python calls, the routes alternating",
                  "    chained    %10.3f %10.3f %10.3f" % ch, "    staged     %10.3f %10.3f %10.3f" % st,
                  "    ratio staged / chained %.2f; the chained route's spread %.3f ms, the staged route's %.3f ms" % (st[0] / ch[0], ch[2] - ch[1], st[2] - st[1])]
        if len(calls) != args.reps + 2:                    # the child's own first proof, the warm-up, the timed ones
            lines += ["  the trace holds %d proofs, %d expected: not tabulated" % (len(calls), args.reps + 2), ""]
            flush()
            continue
        timed = calls[2:]
        lines.append("  kernels of the chained route (rocprofv3 --kernel-trace, a process of its own), ms per proof")
        lines.append("    %-10s %11s %16s %11s %11s" % (("round",) + kinds + ("together",)))
        total = {x: 0.0 for x in kinds}
        for rnd in ROUNDS:
            med = {x: stat([c[rnd].get(x, 0.0) for c in timed])[0] for x in kinds}
            for x in kinds:
                total[x] += med[x]
            lines.append("    %-10s %11.3f %16.3f %11.3f %11.3f" % ((rnd,) + tuple(med[x] for x in kinds) + (sum(med.values()),)))
        ksum = sum(total.values())
        lines.append("    %-10s %11.3f %16.3f %11.3f %11.3f" % (("all",) + tuple(total[x] for x in kinds) + (ksum,)))
        lines.append("    kernels / chained wall %.2f; the nine multiplications take %.0f%% of the kernel time, the six transforms %.0f%%"
                     % (ksum / ch[0], 100 * total["multiplications"] / ksum, 100 * total["transforms"] / ksum))
        top = sorted(by_name.items(), key=lambda kv: -kv[1])[:6]
        lines.append("    the six longest kernels over all proofs of the run, ms per proof: " + ", ".join("%s %.3f" % (k, v / len(calls)) for k, v in top))
        lines.append("")
        flush()
    print("\n".join(lines))
    flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
