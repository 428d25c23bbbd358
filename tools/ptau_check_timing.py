#!/usr/bin/env python3
"""Wall time of `ptaucheck` on a prepared .ptau, its per-kernel totals, and the kernel time of the G2 subgroup test against
its yardstick, written to profiles/ptau_check_timing.txt.

    python tools/ptau_check_timing.py [--power 20] [--size 20] [--reps 5] [--out profiles/ptau_check_timing.txt]

  * the file: write_trapdoor_ptau(power) with sections 12 to 15 (a known tau: a test input, not a ceremony);
  * `ptaucheck` on it: wall of the whole process, twice (the first run also warms the page cache), then a third run under
    `rocprofv3 --kernel-trace --stats` whose per-kernel totals are listed;
  * the subgroup test: n = 2^size points of G2 (a synth chain), the whole row as ONE chunk (ZKHIP_PTAU_CHUNK = n).  One
    process under `rocprofv3 --kernel-trace` calls zk_g2_in_subgroup alternately with k_g2_subgroup<false> (the
    endomorphism test) and with ZKHIP_SUBGROUP_PLAIN=1 (k_g2_subgroup<true>: [r] Q by devmem.hpp's scalar_mul_affine, what
    pairing.hip does), one warm-up pair and --reps timed pairs, and checks that both give the same bytes.  Per kernel the
    median, the least and the largest duration, ns per point, and the ratio beside the one the operation count predicts.
Every GPU step is a process of its own under `timeout`; the first one that fails ends the tool."""
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

from oracle.bn254 import R_MOD  # noqa: E402

BIN = os.path.join(ROOT, "rapidsnark-old_amd")
TOXIC = (0x1234567 * 0x89ABCDEF + 17, 0xA1FA << 200 | 99, 0xBE7A << 180 | 7)
BN_X = 4965661367192848881
# Fq products (a squaring of Fq2 is 2, a product 3) of curve.hpp's G2 operations: dbl 6M + 3S, madd 8M + 2S, add 12M + 2S
DBL, MADD, ADD, F2MUL = 6 * 3 + 3 * 2, 8 * 3 + 2 * 2, 12 * 3 + 2 * 2, 3


def predicted_ratio():
    """the endomorphism test over [r] Q in Fq products: 62 doublings and the set bits of x below the top one, then one mixed
    and two general additions, a doubling, three psi (2 products each) and the projective comparison (4 products)"""
    new = 63 * DBL + bin(BN_X).count("1") * MADD + 2 * ADD + (3 * 2 + 4) * F2MUL
    plain = (R_MOD.bit_length() - 1) * DBL + (bin(R_MOD).count("1") - 1) * MADD      # the first doubling and addition start from infinity
    return new, plain


def limited(cmd, seconds):
    return ["timeout", "-k", "10", str(seconds)] + cmd


def profiled(cmd, prof_dir):
    return ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof_dir, "-o", "ptaucheck", "--"] + cmd


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


def pick(durs, *words):
    for name, d in durs.items():
        if all(w in name for w in words):
            return d
    return []


def child_file(path, power):
    import rapidsnark_old_amd as zk
    zk.write_trapdoor_ptau(power, *TOXIC, path)
    return 0


def child_points(path, n):
    import rapidsnark_old_amd as zk
    from rapidsnark_old_amd import synth
    g2 = synth.g2_gen_bytes()
    zk.synth_chain_g2(n, zk.g2_mul(g2, 1000003), zk.g2_mul(g2, 7919)).tofile(path)
    return 0


def child_op(path, reps):
    """alternating calls of both kernels over the file's points (run under the profiler by main)"""
    import rapidsnark_old_amd as zk
    pts = np.fromfile(path, dtype=np.uint8)
    os.environ["ZKHIP_PTAU_CHUNK"] = str(pts.size // 128)
    for _ in range(reps + 1):
        got = []
        for plain in ("0", "1"):
            os.environ["ZKHIP_SUBGROUP_PLAIN"] = plain
            got.append(zk.g2_in_subgroup(pts))
        if not np.array_equal(got[0], got[1]) or not got[0].all():
            print("the two kernels disagree, or a point of the chain is outside the subgroup", file=sys.stderr)
            return 1
    return 0


def stat(d):
    d = sorted(d)
    return d[len(d) // 2], d[0], d[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--power", type=int, default=20)
    ap.add_argument("--size", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ptau_check_timing.txt"))
    ap.add_argument("--child", nargs=3, metavar=("WHAT", "PATH", "N"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        what, path, n = args.child
        return {"op": child_op, "points": child_points, "file": child_file}[what](path, int(n))
    if not shutil.which("rocprofv3"):
        raise SystemExit("rocprofv3 not found: kernel times come from nowhere else")
    me = [sys.executable, os.path.abspath(__file__), "--child"]
    tmp = tempfile.mkdtemp(prefix="ptau_check_timing_")
    f = lambda name: os.path.join(tmp, name)
    lines, table = [], []
    try:
        n = 1 << args.size
        subprocess.run(limited(me + ["points", f("pts.bin"), str(n)], 300), check=True, timeout=400)
        subprocess.run(limited(profiled(me + ["op", f("pts.bin"), str(args.reps)], f("prof_op")), 600), check=True, capture_output=True, timeout=700)
        os.remove(f("pts.bin"))
        durs = kernel_durations(f("prof_op"))
        new, plain = pick(durs, "k_g2_subgroup<false>")[1:], pick(durs, "k_g2_subgroup<true>")[1:]
        chk = pick(durs, "k_point_check")[2:]
        (nm, nlo, nhi), (pm, plo, phi) = stat(new), stat(plain)
        pn, pp = predicted_ratio()
        lines.append("the subgroup test: 2^%d points of G2, %d timed launches each, alternating" % (args.size, len(new)))
        lines.append("  k_g2_subgroup<false> (endomorphism)  median %9.3f ms  (least %9.3f, largest %9.3f)  %7.2f ns per point" % (nm, nlo, nhi, nm * 1e6 / n))
        lines.append("  k_g2_subgroup<true>  ([r] Q)         median %9.3f ms  (least %9.3f, largest %9.3f)  %7.2f ns per point" % (pm, plo, phi, pm * 1e6 / n))
        lines.append("  ratio endomorphism / [r] Q: measured %.3f (of the medians; least / least %.3f); predicted %.3f (%d against %d Fq products a point)" % (
            nm / pm, nlo / plo, pn / pp, pn, pp))
        lines.append("  k_point_check (the twist's equation) median %7.3f ms" % stat(chk)[0])
        print("\n".join(lines), flush=True)

        subprocess.run(limited(me + ["file", f("p.ptau"), str(args.power)], 900), check=True, timeout=1000)
        cmd = [os.path.join(BIN, "ptaucheck"), f("p.ptau")]
        walls = []
        for _ in range(2):
            t = time.time()
            res = subprocess.run(limited(cmd, 600), check=True, capture_output=True, text=True, timeout=700)
            walls.append(time.time() - t)
        subprocess.run(limited(profiled(cmd, f("prof_file")), 600), check=True, capture_output=True, timeout=700)
        durs = kernel_durations(f("prof_file"))
        kern = sum(sum(d) for d in durs.values())
        size = os.path.getsize(f("p.ptau"))
        lines += ["", "ptaucheck on a prepared file of power %d (%.0f MiB; %d points of G1, %d of G2): wall %.2f s, again %.2f s" % (
            args.power, size / 2**20, (12 << args.power) - 4, 3 << args.power, walls[0], walls[1]),
            "  its answer: " + res.stdout.strip(),
            "  under the profiler: kernels %.0f ms in all; the rest of the wall is the host's: mapping and reading the file, staging it to the" % kern,
            "  device, the host ends of the multiplications, process start and HIP initialisation"]
        table = sorted(((name, len(d), sum(d)) for name, d in durs.items()), key=lambda x: -x[2])
        print("\n".join(lines[-4:]), flush=True)
        try:
            clock = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        except (OSError, subprocess.SubprocessError):
            clock = ""
        clock = [ln.strip() for ln in clock.splitlines() if "sclk" in ln][:1]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = ["# tools/ptau_check_timing.py: the G2 subgroup test and `ptaucheck` on one MI355X",
           "# kernel times: rocprofv3 --kernel-trace, per launch; the yardstick k_g2_subgroup<true> is [r] Q by devmem.hpp's scalar_mul_affine (what",
           "# pairing.hip's check does), in the same process, alternating with k_g2_subgroup<false>",
           "# shader clock after the runs: " + (clock[0] if clock else "not read"), ""] + lines
    if table:
        out += ["", "# rocprofv3 --kernel-trace --stats, the ptaucheck run (kernel, calls, total ms)"]
        out += ["%-90s %6d %10.2f" % (name[:90], calls, ms) for name, calls, ms in table]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
