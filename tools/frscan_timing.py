#!/usr/bin/env python3
"""What the running products over Fr cost on one MI355X, written to profiles/frscan_timing.txt.

    python tools/frscan_timing.py [--reps 5] [--segs 1 4 8 16 64 256] [--sizes 20 24]

  * walls at n = 2^20 of the four entries (upload, kernels, download), one process, a warm-up and --reps timed calls;
  * the scan kernels of zk_fr_batch_inverse and of zk_plonk_permutation_product with cols = 3 at every size of --sizes for
    every ZKHIP_SCAN_SEG of --segs: a process of its own under `rocprofv3 --kernel-trace`, the two entries alternating; per
    call the span from the start of k_scan_reduce to the end of k_scan_apply, which holds the host's one inversion and its
    round trip of 96 bytes, and the three launches' durations added;
  * against the bounds: bytes and products per element by count (below), over the 8 TB/s of the HBM and over the product
    rate tools/frinv_probe measures for field.hpp's Fr::mul in the same run;
  * against a lane per element computing a^(r-2) (tools/frinv_probe, built by the tool when it is not there), and what the
    one inversion costs as one lane's launch and as a round trip to the host.
Every GPU step is a child process under `timeout`."""
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

import numpy as np  # noqa: E402

from verify_timing import limited, stat  # noqa: E402

HBM_PEAK = 8.0e12
COLS = 3
PROBE = os.path.join(ROOT, "tools", "frinv_probe")
# by count, per element, the per-lane part (scans, seeds, the lane's starting power) left out: it is divided by seg
#   inverse: k_scan_reduce 1 product, reads 32 bytes; k_scan_apply 1 forward + 2 backward, reads 32 + 32 + 32, writes 32 + 32
#   permutation, c columns: a numerator factor is 2 products (beta w^i shift, the chain), a denominator factor 2, w^i 1 a row;
#     k_scan_reduce 4 c + 1, reads 64 c; k_scan_apply (2 c + 1) forward + (2 c + 1) backward, reads 32 c + 64 c + 32, writes 64
COUNT = {"inverse": {"products": 4, "bytes": 192},
         "permutation": {"products": 8 * COLS + 3, "bytes": 64 * COLS + 96 * COLS + 96}}
CHAIN = 254 + 126 + 2                                  # a^(r-2) and the two conversions of a lane per element


def scalars(n, seed):
    """n values below 2^248 (< r), 32 bytes each"""
    a = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 31] = 0
    a[:, 0] |= 1                                       # none is zero
    return a.reshape(-1)


def columns(n, seed):
    return scalars(COLS * n, seed).reshape(COLS, n * 32)


def walls(reps, out_path):
    import rapidsnark_old_amd as zk
    n = 1 << 20
    a, b = scalars(n, 1), scalars(n, 2)
    w, s, sh = columns(n, 3), columns(n, 4), [1, 2, 3]
    calls = {"fr_batch_inverse": lambda: zk.fr_batch_inverse(a), "fr_prefix_product": lambda: zk.fr_prefix_product(a),
             "fr_grand_product": lambda: zk.fr_grand_product(a, b), "plonk_permutation_product": lambda: zk.plonk_permutation_product(w, s, sh, 5, 7)}
    t = {name: [] for name in calls}
    for _ in range(reps + 1):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            t[name].append(time.perf_counter() - t0)
    with open(out_path, "w") as fh:
        json.dump({name: x[1:] for name, x in t.items()}, fh)
    return 0


def traced(reps, segs, sizes, out_path):
    """the calls the profiler watches, in a known order: size, then seg, then a warm-up and `reps` timed pairs of calls"""
    import rapidsnark_old_amd as zk
    for log_n in sizes:
        n = 1 << log_n
        a, w, s = scalars(n, log_n), columns(n, log_n + 1), columns(n, log_n + 2)
        for seg in segs:
            os.environ["ZKHIP_SCAN_SEG"] = str(seg)
            for _ in range(reps + 1):
                zk.fr_batch_inverse(a)
                zk.plonk_permutation_product(w, s, [1, 2, 3], 5, 7)
            print("traced: n = 2^%d, seg %d" % (log_n, seg), file=sys.stderr, flush=True)
    with open(out_path, "w") as fh:
        json.dump({"ok": True}, fh)
    return 0


def scan_launches(prof_dir):
    """-> [(kernel name, start ms, end ms)] of the k_scan_ launches in start order"""
    files = glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return []
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    return [(r["Kernel_Name"], int(r["Start_Timestamp"]) / 1e6, int(r["End_Timestamp"]) / 1e6) for r in rows if "k_scan_" in r["Kernel_Name"]]


def run_probe(sizes):
    if not os.path.exists(PROBE):
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", os.path.join(ROOT, "tools", "frinv_probe.hip"), "-o", PROBE], check=True)
    out = subprocess.run(limited([PROBE] + [str(s) for s in sizes], 200), check=True, capture_output=True, text=True, timeout=260).stdout
    res = {"mul_rate": 0.0, "per_lane": {}}
    for line in out.splitlines():
        f = line.split()
        kv = dict(x.split("=") for x in f[1:] if "=" in x)
        if f[0] == "mul_rate":
            res["mul_rate"] = max(res["mul_rate"], float(kv["products_per_s"]))
        elif f[0] == "per_lane":
            res["per_lane"][int(kv["n"])] = float(kv["ms"])
        elif f[0] in ("one_lane", "round_trip"):
            res[f[0]] = float(kv["ms"])
        elif f[0] == "check" and f[1] != "ok":
            raise SystemExit("frinv_probe: a^-1 a != 1")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--segs", type=int, nargs="+", default=[1, 4, 8, 16, 64, 256])
    ap.add_argument("--sizes", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frscan_timing.txt"))
    ap.add_argument("--child", nargs=2, metavar=("WHAT", "PATH"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return walls(args.reps, args.child[1]) if args.child[0] == "walls" else traced(args.reps, args.segs, args.sizes, args.child[1])
    if not shutil.which("rocprofv3"):
        raise SystemExit("rocprofv3 not found: kernel times come from nowhere else")
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--segs"] + [str(s) for s in args.segs] + \
         ["--sizes"] + [str(s) for s in args.sizes] + ["--child"]
    tmp = tempfile.mkdtemp(prefix="frscan_timing_")
    try:
        probe = run_probe(args.sizes)
        wj = os.path.join(tmp, "walls.json")
        subprocess.run(limited(me + ["walls", wj], 300), check=True, timeout=360)
        wall = json.load(open(wj))
        prof = os.path.join(tmp, "prof")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", prof, "-o", "frscan", "--"] + me + ["traced", os.path.join(tmp, "t.json")]
        subprocess.run(limited(cmd, 700), check=True, stdout=subprocess.DEVNULL, timeout=760)
        launches = scan_launches(prof)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    rate = probe["mul_rate"]
    lines = ["# tools/frscan_timing.py: running products over Fr on one MI355X; %d timed calls after a warm-up, medians" % args.reps, "",
             "walls at n = 2^20, ms: median, least, largest of time.perf_counter around the Python call (upload, kernels, download)"]
    for name, v in wall.items():
        lines.append("  %-28s %10.3f %10.3f %10.3f" % ((name,) + stat([1e3 * x for x in v])))
    lines += ["", "Fr::mul (field.hpp, 8 x 32-bit) with operands in registers, the best of 1, 2, 4, 8 waves a SIMD: %.1f G products/s" % (rate / 1e9),
              "the one inversion: a^(r-2) in one lane as a launch of its own %.1f us; 32 bytes to the host, Fr::inv there, 32 bytes back %.1f us"
              % (1e3 * probe["one_lane"], 1e3 * probe["round_trip"]), "",
              "scan kernels (rocprofv3 --kernel-trace, a process of its own), per call: the span from the start of k_scan_reduce to the end of",
              "k_scan_apply (median, least, largest), which holds the host's inversion between k_scan_carry and k_scan_apply; kernels: the three durations added",
              "products and bytes an element by count: inverse %(products)d and %(bytes)d" % COUNT["inverse"]
              + ", permutation (cols = %d) %d and %d" % (COLS, COUNT["permutation"]["products"], COUNT["permutation"]["bytes"]),
              "  %-12s %9s %5s %10s %9s %9s %9s %8s %7s %10s %8s" % ("entry", "n", "seg", "median us", "least", "largest", "kernels", "ns/elem", "TB/s", "G prod/s", "of rate")]
    per_call = 3
    calls = len(args.sizes) * len(args.segs) * (args.reps + 1) * 2
    best = {}
    if len(launches) == calls * per_call:
        at = 0
        rows = {}
        for log_n in args.sizes:
            for seg in args.segs:
                tot = {"inverse": [], "permutation": []}
                carry = {"inverse": [], "permutation": []}
                for r in range(args.reps + 1):
                    for entry in ("inverse", "permutation"):
                        three = launches[at:at + per_call]
                        at += per_call
                        if r:
                            tot[entry].append(three[-1][2] - three[0][1])
                            carry[entry].append(sum(e - b for _, b, e in three))
                for entry in tot:
                    rows[(entry, log_n, seg)] = (stat(tot[entry]), stat(carry[entry])[0])
        for entry in ("inverse", "permutation"):
            for log_n in args.sizes:
                n = 1 << log_n
                for seg in args.segs:
                    (m, lo, hi), c = rows[(entry, log_n, seg)]
                    prods = COUNT[entry]["products"] * n / (m * 1e-3)
                    lines.append("  %-12s %9d %5d %10.1f %9.1f %9.1f %9.1f %8.3f %7.3f %10.2f %7.1f%%"
                                 % (entry, n, seg, 1e3 * m, 1e3 * lo, 1e3 * hi, 1e3 * c, 1e6 * m / n, COUNT[entry]["bytes"] * n / (m * 1e-3) / 1e12, prods / 1e9,
                                    100 * prods / rate))
                    if (entry, log_n) not in best or m < best[(entry, log_n)][1]:
                        best[(entry, log_n)] = (seg, m)
        lines.append("")
        for (entry, log_n), (seg, m) in sorted(best.items()):
            n = 1 << log_n
            t_hbm, t_mul = COUNT[entry]["bytes"] * n / HBM_PEAK, COUNT[entry]["products"] * n / rate
            lines.append("  %-12s 2^%d: best ZKHIP_SCAN_SEG %d, %.1f us; the HBM bound %.1f us, the product bound %.1f us: %s-bound, %.1f%% of that bound"
                         % (entry, log_n, seg, 1e3 * m, 1e6 * t_hbm, 1e6 * t_mul, "product" if t_mul > t_hbm else "HBM", 100 * max(t_hbm, t_mul) / (m * 1e-3)))
        lines += ["", "against a lane per element computing a^(r-2) (tools/frinv_probe, the same run): %d products an element against the scan's %d,"
                  % (CHAIN, COUNT["inverse"]["products"]), "predicted ratio %.1f" % (CHAIN / COUNT["inverse"]["products"])]
        for log_n in args.sizes:
            n = 1 << log_n
            if n in probe["per_lane"] and ("inverse", log_n) in best:
                seg, m = best[("inverse", log_n)]
                lines.append("  n = 2^%d: a lane per element %.1f us (%.1f G products/s), the scan at seg %d %.1f us: measured ratio %.1f"
                             % (log_n, 1e3 * probe["per_lane"][n], CHAIN * n / (probe["per_lane"][n] * 1e-3) / 1e9, seg, 1e3 * m, probe["per_lane"][n] / m))
    else:
        names = {}
        for name, _, _ in launches:
            names[name] = names.get(name, 0) + 1
        lines.append("  the trace holds %s launches, %d expected: not tabulated" % (names, calls * per_call))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
