#!/usr/bin/env python3
"""What PLONK round 3 costs on one MI355X, written to profiles/plonk_quotient_timing.txt.

    python tools/plonk_quotient_timing.py [--reps 5] [--segs 1 2 4 8 16 64] [--sizes 18 22]

  * walls of PlonkCircuit(...) and of one .quotient(...) at every log_n of --sizes (upload, kernels, download), one process,
    a warm-up and --reps timed calls;
  * kernel times from a process of its own under `rocprofv3 --kernel-trace` (no counters in that run): the launches of
    zk_plonk_circuit_create added, and per zk_plonk_quotient call the load, the transforms, the quotient kernel and the store,
    for every ZKHIP_QUOT_SEG of --segs;
  * the quotient kernel against its bounds: 22 products and 15 x 32 bytes a point by count (below), over the 8 TB/s of the HBM
    and over the product rate tools/frinv_probe measures in the same run (field.hpp's 8 x 32-bit Fr::mul; the kernel
    multiplies in field29.hpp's 29-bit form, so its share of that rate may exceed 100 %).
Every GPU step is a child process under `timeout`.  The polynomials are random: the cost does not depend on the witness."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from frscan_timing import run_probe, scalars  # noqa: E402
from verify_timing import limited, stat  # noqa: E402

HBM_PEAK = 8.0e12
# the quotient kernel by count, per point: 22 products (csrc/plonkquot.hip lists them); it reads the nine resident
# extensions, a, b, c, z, PI and z four places on (the same rows as z, 128 bytes later: from cache), and writes t
PRODUCTS, BYTES = 22, (9 + 5 + 1) * 32


def circuit(zk, log_n):
    n = 1 << log_n
    rows = scalars(8 * n, log_n).reshape(8, n * 32)
    return zk.PlonkCircuit(*rows, 2, 3)


def proof(log_n):
    n = 1 << log_n
    lens = (n + 2, n + 2, n + 2, n + 3, n)
    flat = scalars(sum(lens), 100 + log_n)
    out, at = [], 0
    for k in lens:
        out.append(flat[at * 32:(at + k) * 32])
        at += k
    return out


def walls(reps, sizes, out_path):
    import rapidsnark_old_amd as zk
    res = {}
    for log_n in sizes:
        a, b, c, z, pi = proof(log_n)
        tc, tq = [], []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            obj = circuit(zk, log_n)
            tc.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            obj.quotient(a, b, c, z, 5, 7, 11, pi=pi)
            tq.append(time.perf_counter() - t0)
            obj.close()
        res[str(log_n)] = {"create": tc[1:], "quotient": tq[1:]}
    with open(out_path, "w") as fh:
        json.dump(res, fh)
    return 0


def traced(reps, segs, sizes, out_path):
    """the calls the profiler watches, in a known order: size (one create), then seg, then a warm-up and `reps` timed calls"""
    import rapidsnark_old_amd as zk
    for log_n in sizes:
        a, b, c, z, pi = proof(log_n)
        os.environ.pop("ZKHIP_QUOT_SEG", None)
        with circuit(zk, log_n) as obj:
            for seg in segs:
                os.environ["ZKHIP_QUOT_SEG"] = str(seg)
                for _ in range(reps + 1):
                    obj.quotient(a, b, c, z, 5, 7, 11, pi=pi)
                print("traced: log_n = %d, seg %d" % (log_n, seg), file=sys.stderr, flush=True)
    with open(out_path, "w") as fh:
        json.dump({"ok": True}, fh)
    return 0


def groups(prof_dir):
    """-> [("create" | "quotient", {part: ms})] in start order.  A create runs from k_pair_tables to the end of its one
    batched transform; a quotient call from its k_coset_load to its k_coset_store"""
    files = glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return []
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    ev = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6) for r in rows]

    def part(name):
        for key, p in (("k_coset_load", "load"), ("k_plonk_quotient", "quotient"), ("k_coset_store", "store"), ("k_ntt_", "transforms"), ("k_pair_tables", "tables")):
            if key in name:
                return p
        return "other"

    out, i = [], 0
    while i < len(ev):
        p = part(ev[i][0])
        if p == "tables":
            g, i = {"tables": ev[i][1]}, i + 1
            while i < len(ev) and part(ev[i][0]) in ("load", "transforms", "other"):
                if part(ev[i][0]) == "load" and "transforms" in g:      # the first call's load: the object (monomial basis) has one
                    break
                g[part(ev[i][0])] = g.get(part(ev[i][0]), 0.0) + ev[i][1]
                i += 1
            out.append(("create", g))
        elif p == "load":
            g = {}
            while i < len(ev):
                q = part(ev[i][0])
                g[q] = g.get(q, 0.0) + ev[i][1]
                i += 1
                if q == "store":
                    break
            out.append(("quotient", g))
        else:
            i += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--segs", type=int, nargs="+", default=[1, 2, 4, 8, 16, 64])
    ap.add_argument("--sizes", type=int, nargs="+", default=[18, 22])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_quotient_timing.txt"))
    ap.add_argument("--child", nargs=2, metavar=("WHAT", "PATH"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return walls(args.reps, args.sizes, args.child[1]) if args.child[0] == "walls" else traced(args.reps, args.segs, args.sizes, args.child[1])
    if not shutil.which("rocprofv3"):
        raise SystemExit("rocprofv3 not found: kernel times come from nowhere else")
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--segs"] + [str(s) for s in args.segs] + \
         ["--sizes"] + [str(s) for s in args.sizes] + ["--child"]
    tmp = tempfile.mkdtemp(prefix="plonk_quotient_timing_")
    try:
        rate = run_probe([16])["mul_rate"]
        wj = os.path.join(tmp, "walls.json")
        subprocess.run(limited(me + ["walls", wj], 300), check=True, timeout=360)
        wall = json.load(open(wj))
        prof = os.path.join(tmp, "prof")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", prof, "-o", "plonkquot", "--"] + me + ["traced", os.path.join(tmp, "t.json")]
        subprocess.run(limited(cmd, 400), check=True, stdout=subprocess.DEVNULL, timeout=460)
        gs = groups(prof)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    lines = ["# tools/plonk_quotient_timing.py: PLONK round 3 on one MI355X; %d timed calls after a warm-up, medians" % args.reps, "",
             "walls, ms: median, least, largest of time.perf_counter around the Python call (upload, kernels, download)"]
    for log_n in args.sizes:
        for name in ("create", "quotient"):
            lines.append("  log_n %2d  %-10s %10.3f %10.3f %10.3f" % ((log_n, name) + stat([1e3 * x for x in wall[str(log_n)][name]])))
    lines += ["", "Fr::mul (field.hpp, 8 x 32-bit) with operands in registers, the best of 1, 2, 4, 8 waves a SIMD (tools/frinv_probe, this run): %.1f G products/s" % (rate / 1e9),
              "the quotient kernel by count: %d products and %d bytes a point" % (PRODUCTS, BYTES), ""]
    creates = [g for kind, g in gs if kind == "create"]
    quots = [g for kind, g in gs if kind == "quotient"]
    if len(creates) == len(args.sizes) and len(quots) == len(args.sizes) * len(args.segs) * (args.reps + 1):
        lines.append("kernels (rocprofv3 --kernel-trace, a process of its own), ms")
        at, best = 0, {}
        for si, log_n in enumerate(args.sizes):
            m = 4 << log_n
            g = creates[si]
            lines.append("  log_n %2d  zk_plonk_circuit_create: tables %.3f, load %.3f, transforms %.3f: %.3f together"
                         % (log_n, g.get("tables", 0), g.get("load", 0), g.get("transforms", 0), sum(g.values())))
            lines.append("  %-8s %5s %9s %11s %9s %9s %9s %9s %9s %8s" % ("", "seg", "load", "transforms", "quotient", "store", "together", "G prod/s", "of rate", "TB/s"))
            for seg in args.segs:
                calls = quots[at + 1:at + 1 + args.reps]
                at += args.reps + 1
                med = {p: stat([c.get(p, 0.0) for c in calls])[0] for p in ("load", "transforms", "quotient", "store")}
                tot = stat([sum(c.values()) for c in calls])[0]
                q = med["quotient"] * 1e-3
                lines.append("  log_n %2d %5d %9.3f %11.3f %9.3f %9.3f %9.3f %9.1f %8.1f%% %8.3f"
                             % (log_n, seg, med["load"], med["transforms"], med["quotient"], med["store"], tot, PRODUCTS * m / q / 1e9,
                                100 * PRODUCTS * m / q / rate, BYTES * m / q / 1e12))
                if log_n not in best or med["quotient"] < best[log_n][1]:
                    best[log_n] = (seg, med["quotient"])
        lines.append("")
        for log_n, (seg, q) in sorted(best.items()):
            m = 4 << log_n
            t_hbm, t_mul = BYTES * m / HBM_PEAK, PRODUCTS * m / rate
            lines.append("  log_n %d: best ZKHIP_QUOT_SEG %d, quotient kernel %.3f ms; the HBM bound %.3f ms, the product bound at the probe's rate %.3f ms:"
                         " %.1f%% of the product bound's rate" % (log_n, seg, q, 1e3 * t_hbm, 1e3 * t_mul, 100 * t_mul / (q * 1e-3)))
    else:
        lines.append("  the trace holds %d create and %d quotient groups, %d and %d expected: not tabulated"
                     % (len(creates), len(quots), len(args.sizes), len(args.sizes) * len(args.segs) * (args.reps + 1)))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
