#!/usr/bin/env python3
"""Wall time and GPU time of `ptauprepare` (phase-2 preparation of a .ptau on the GPU), written to
profiles/ptau_prepare_timing.txt.

    python tools/ptau_prepare_timing.py [--sizes 16 20 22] [--rate-power 20] [--out profiles/ptau_prepare_timing.txt] [--no-prof]

  * unprepared trapdoor files of each power (ptau.write_trapdoor_ptau(prepared=False)).  Wall = the whole `ptauprepare`
    process (input mapped and checked, the four sections, output written through its mapping); GPU = the sum of its kernel
    times from a second run under `rocprofv3 --kernel-trace --stats`, whose per-kernel table of the --rate-power run is
    appended;
  * the top level alone of sections 2 and 3 of the --rate-power file through the operators (zk_g1_lagrange on 2^(power+1)
    points, zk_g2_lagrange on 2^power), each in a process of its own under rocprofv3: kernel time per butterfly (n/2 * p of
    them) and scalar multiplications per second (n/2 * (p - 1) in the stages whose twiddle is not 1, n in the 1/n scale);
  * the yardstick: `zkeynew` on tools/setup_timing.py's "even" circuit (full-size coefficients) of the same domain, whose
    k_setup_term kernels are the same per-lane 254-bit double-and-add with mixed adds over a fixed table: kernel time per
    term, and the ratio butterfly / term for G1 and G2.
--no-prof: wall only."""
import argparse
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

from setup_timing import kernel_stats, synthetic_r1cs  # noqa: E402

BIN = os.path.join(ROOT, "rapidsnark-old_amd")
TOXIC = (0x1234567 * 0x89ABCDEF + 17, 0xA1FA << 200 | 99, 0xBE7A << 180 | 7)


def profiled(cmd, prof_dir):
    return ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof_dir, "-o", "ptau", "--"] + cmd


def run(cmd, prof_dir=None):
    t = time.time()
    subprocess.run(profiled(cmd, prof_dir) if prof_dir else cmd, check=True, capture_output=True, timeout=1700)
    return time.time() - t


def child_op(group, path):
    """the top level of section 2 / 3 of the file through the operator (run under the profiler by main)"""
    import rapidsnark_old_amd as zk
    f = zk.PtauFile(path)
    if group == "g1":
        zk.g1_lagrange(f.section(2), f.power + 1)
    else:
        zk.g2_lagrange(f.section(3), f.power)
    f.close()
    return 0


def matching(stats, *words):
    return sum(ms for name, _, ms in stats if all(w in name for w in words))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 20, 22])
    ap.add_argument("--rate-power", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ptau_prepare_timing.txt"))
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--child-op", nargs=2, metavar=("GROUP", "PTAU"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child_op:
        return child_op(*args.child_op)
    import rapidsnark_old_amd as zk
    prof = not args.no_prof and shutil.which("rocprofv3")
    lines, table, rate = [], [], []
    tmp = tempfile.mkdtemp(prefix="ptau_prepare_timing_")
    f = lambda name: os.path.join(tmp, name)
    try:
        for power in args.sizes:
            t = time.time()
            zk.write_trapdoor_ptau(power, *TOXIC, f("in.ptau"), prepared=False)
            t_in = time.time() - t
            wall = run([os.path.join(BIN, "ptauprepare"), f("in.ptau"), f("out.ptau")])
            size = os.path.getsize(f("out.ptau"))
            os.remove(f("out.ptau"))
            gpu = None
            if prof:
                run([os.path.join(BIN, "ptauprepare"), f("in.ptau"), f("out.ptau")], prof_dir=f("prof%d" % power))
                os.remove(f("out.ptau"))
                st = kernel_stats(f("prof%d" % power))
                gpu = sum(x[2] for x in st)
                if power == args.rate_power:
                    table = st
            lines.append("power %2d  unprepared file written in %5.1f s   ptauprepare wall %7.2f s  GPU %s   output %6.1f MiB" % (
                power, t_in, wall, "%9.1f ms" % gpu if gpu is not None else "    -", size / 2**20))
            print(lines[-1], flush=True)
            if prof and power == args.rate_power:
                n1, p1, n2, p2 = 2 << power, power + 1, 1 << power, power
                fig = {}
                for group, n, p in (("g1", n1, p1), ("g2", n2, p2)):
                    d = f("prof_" + group)
                    run([sys.executable, os.path.abspath(__file__), "--child-op", group, f("in.ptau")], prof_dir=d)
                    st = kernel_stats(d)
                    ms = sum(x for name, _, x in st if "k_ptau_" in name or "k_chain_normalize" in name)
                    mul = matching(st, "k_ptau_twmul") + matching(st, "k_ptau_scale")
                    bfly, muls = n // 2 * p, n // 2 * (p - 1) + n
                    fig[group] = (ms * 1e6 / bfly, muls / (mul / 1e3))
                    rate.append("%s top level, 2^%d points: kernels %9.1f ms (twmul + scale %9.1f ms)  %8.1f ns per butterfly (%d)  %6.2f M scalar multiplications/s" % (
                        group, p, ms, mul, fig[group][0], bfly, fig[group][1] / 1e6))
                    print(rate[-1], flush=True)
                # the yardstick: k_setup_term of the "even" circuit of the same domain, prepared file of the same power
                m = (1 << power) - 8
                zk.write_trapdoor_ptau(power, *TOXIC, f("full.ptau"))
                with open(f("even.r1cs"), "wb") as fh:
                    fh.write(synthetic_r1cs("even", m, 3 * m // 4, 2, np.random.default_rng(0x5E7)))
                run([os.path.join(BIN, "zkeynew"), f("even.r1cs"), f("full.ptau"), f("even.zkey")], prof_dir=f("prof_even"))
                st = kernel_stats(f("prof_even"))
                terms = {"g1": (2 * m + 3) + 2 * m + (5 * m + 3), "g2": 2 * m}          # A, B1, K = A + B + C; B2
                for group, fld in (("g1", "k_setup_term<zk::Fp<"), ("g2", "k_setup_term<zk::Fp2T<")):
                    ms = matching(st, fld)
                    per = ms * 1e6 / terms[group]
                    rate.append("%s yardstick, k_setup_term of the even circuit (m = %d): %9.1f ms, %d terms  %8.1f ns per term   ratio butterfly / term %.2f" % (
                        group, m, ms, terms[group], per, fig[group][0] / per))
                    print(rate[-1], flush=True)
                for name in ("full.ptau", "even.r1cs", "even.zkey"):
                    os.remove(f(name))
            os.remove(f("in.ptau"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = ["# tools/ptau_prepare_timing.py: `ptauprepare in.ptau out.ptau` on one MI355X",
           "# wall: the whole process (input mapped and checked, sections 12 to 15, output written); GPU: sum of kernel times (rocprofv3)", ""] + lines
    if rate:
        out += ["", "# the top level alone through the operators, and the yardstick (bound: ratio <= 1.5)"] + rate
    if table:
        out += ["", "# rocprofv3 --kernel-trace --stats, power %d run (kernel, calls, total ms)" % args.rate_power]
        out += ["%-90s %6d %10.2f" % (name[:90], calls, ms) for name, calls, ms in table]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
