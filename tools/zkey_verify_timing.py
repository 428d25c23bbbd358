#!/usr/bin/env python3
"""What `zkeyverify` costs, beside the obvious other way to answer its question (`zkeynew` on the same inputs and a byte
compare), written to profiles/zkey_verify_timing.txt.

    python tools/zkey_verify_timing.py [--sizes 20 22] [--out profiles/zkey_verify_timing.txt] [--no-prof]

For every size a zkgen circuit_like circuit (tools/setup_timing.py's: coefficients mostly +-1 and small) and, at every size
too, the "even" circuit of that tool with its nnz (wires spread evenly, FULL-SIZE coefficients: what k_setup_term pays a
254-bit double-and-add per term for).  In one run, on one box: `zkeynew` makes the key (wall), `zkeyverify` checks it
(wall; it must say OK), then each program once more under `rocprofv3 --kernel-trace --stats` in a run of its own (the sum
of its kernel times).  Reported: both walls, both kernel sums, the ratios zkeyverify / zkeynew, the share of the
multi-scalar multiplications (their sort, accumulation and reduction kernels) in zkeyverify's kernel time, and zkeyverify's kernel table of the
largest full-size run."""
import argparse
import importlib.util
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

BIN = os.path.join(ROOT, "rapidsnark-old_amd")
_spec = importlib.util.spec_from_file_location("setup_timing", os.path.join(ROOT, "tools", "setup_timing.py"))
ST = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ST)


def run(prog, args, prof_dir=None, expect=None):
    cmd = [os.path.join(BIN, prog)] + args
    if prof_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof_dir, "-o", prog, "--"] + cmd
    t = time.time()
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    wall = time.time() - t
    if res.returncode != 0 or (expect and not res.stdout.startswith(expect)):
        raise RuntimeError("%s failed (%d): %s %s" % (prog, res.returncode, res.stdout, res.stderr))
    return wall


def is_msm(name):
    # the sort (digits, bins, scans), the accumulation and the reduction, and the conversion of the points they read
    return any(t in name for t in ("k_msm", "k_bin_", "k_scan_", "to_internal"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zkey_verify_timing.txt"))
    ap.add_argument("--no-prof", action="store_true")
    args = ap.parse_args()
    import rapidsnark_old_amd as zk
    from rapidsnark_old_amd import zkgen
    prof = not args.no_prof and shutil.which("rocprofv3")
    lines, table, table_of = [], [], ""
    tmp = tempfile.mkdtemp(prefix="zkey_verify_timing_")
    try:
        for k in args.sizes:
            d = os.path.join(tmp, "k%d" % k)
            os.makedirs(d)
            f = lambda name: os.path.join(d, name)
            key = zkgen.generate(k, 2, seed=0, circuit_like=True)
            zkgen.write_r1cs(key, f("circuit_like.r1cs"))
            tau, alpha, beta = key["trap"]["toxic"][:3]
            zk.write_trapdoor_ptau(k, tau, alpha, beta, f("p.ptau"))
            m, nw = key["nConstraints"], key["nVars"]
            del key
            with open(f("even.r1cs"), "wb") as fh:
                fh.write(ST.synthetic_r1cs("even", m, nw, 2, np.random.default_rng(0x5E7)))
            for kind in ("circuit_like", "even"):
                files = [f(kind + ".r1cs"), f("p.ptau"), f(kind + ".zkey")]
                w_new = run("zkeynew", files)
                w_ver = run("zkeyverify", files, expect="OK: ")
                g_new = g_ver = share = None
                if prof:
                    run("zkeynew", files[:2] + [f("again.zkey")], prof_dir=f("prof_new_" + kind))
                    run("zkeyverify", files, prof_dir=f("prof_ver_" + kind), expect="OK: ")
                    s_new, s_ver = ST.kernel_stats(f("prof_new_" + kind)), ST.kernel_stats(f("prof_ver_" + kind))
                    g_new, g_ver = sum(x[2] for x in s_new), sum(x[2] for x in s_ver)
                    share = sum(x[2] for x in s_ver if is_msm(x[0])) / g_ver if g_ver else 0.0
                    if kind == "even" and k == max(args.sizes):
                        table, table_of = s_ver, "2^%d even" % k
                ms = lambda x: "%9.1f ms" % x if x is not None else "        -"
                lines.append("2^%d %-12s nVars %8d  nnz %9d   wall: zkeynew %6.2f s  zkeyverify %6.2f s  ratio %5.2f   kernels: zkeynew %s  zkeyverify %s  ratio %s  MSM share %s" % (
                    k, kind, nw, 5 * m, w_new, w_ver, w_ver / w_new, ms(g_new), ms(g_ver),
                    "%5.2f" % (g_ver / g_new) if g_new else "    -", "%4.0f %%" % (100 * share) if share is not None else "   -"))
                print(lines[-1], flush=True)
                for name in (kind + ".zkey", "again.zkey"):
                    if os.path.exists(f(name)):
                        os.remove(f(name))
            shutil.rmtree(d, ignore_errors=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = ["# tools/zkey_verify_timing.py: `zkeyverify circuit.r1cs pot.ptau circuit.zkey` beside `zkeynew` on the same inputs, one MI355X, one run",
           "# wall: the whole process (files mapped, the work, for zkeynew the .zkey written); kernels: sum of kernel times (rocprofv3 --kernel-trace --stats,",
           "# a run of its own per program); ratio = zkeyverify / zkeynew (below 1: checking is cheaper than making the key again);",
           "# circuit_like: coefficients mostly +-1; even: full-size coefficients (setup_timing.py's circuits)", ""] + lines
    if table:
        out += ["", "# rocprofv3 --kernel-trace --stats, zkeyverify, %s run (kernel, calls, total ms)" % table_of]
        out += ["%-90s %6d %10.2f" % (name[:90], calls, ms_) for name, calls, ms_ in table]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
