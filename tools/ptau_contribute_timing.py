#!/usr/bin/env python3
"""Kernel time of zk_g1_mul_vec / zk_g2_mul_vec against their yardstick, and wall and kernel time of `ptaucontribute`, written
to profiles/ptau_contribute_timing.txt.

    python tools/ptau_contribute_timing.py [--g1-size 20] [--g2-size 18] [--reps 3] [--power 20] [--out profiles/ptau_contribute_timing.txt]

  * the operators: n valid points (a synth chain; in G2 multiples of the generator, so in the subgroup) and n seeded random
    scalars below 2^253, one for each point, the whole row as ONE chunk (ZKHIP_PTAU_CONTRIB_CHUNK = n: a launch per call).
    One process per group under `rocprofv3 --kernel-trace --stats` calls the operator alternately with k_mul_vec (each lane
    splits its scalar by the endomorphism: 128 columns) and with ZKHIP_MULVEC_PLAIN=1 (devmem.hpp's scalar_mul_affine, the
    254-bit double-and-add every per-lane-scalar kernel of the project uses), one warm-up pair and --reps timed pairs, and
    checks that both give the same bytes.  Per kernel the median, the least and the largest duration of the timed launches,
    ns per point, and the ratio new / plain beside the 0.50 that the operation count predicts (128 x 19 against 254 x 19
    field products);
  * `ptaucontribute` on `ptaunew`'s file of --power: wall of the whole process, twice, then a run under `rocprofv3
    --kernel-trace --memory-copy-trace --stats` whose kernel and copy totals split it; the rest is the host's.
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

BIN = os.path.join(ROOT, "rapidsnark-old_amd")
PREDICTED = 128.0 / 254.0


def limited(cmd, seconds):
    return ["timeout", "-k", "10", str(seconds)] + cmd


def profiled(cmd, prof_dir, copies=False):
    return ["rocprofv3", "--kernel-trace"] + (["--memory-copy-trace"] if copies else []) + \
           ["--stats", "--output-format", "csv", "-d", prof_dir, "-o", "potc", "--"] + cmd


def trace_rows(prof_dir, suffix):
    files = glob.glob(os.path.join(prof_dir, "**", "*" + suffix), recursive=True)
    if not files:
        return []
    with open(files[0]) as f:
        return list(csv.DictReader(f))


def kernel_durations(prof_dir):
    """-> {kernel name: [duration ms of every dispatch, in start order]}, the names in the order of their first dispatch"""
    out = {}
    rows = sorted(trace_rows(prof_dir, "kernel_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        out.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    return out


def scalars_for(n, seed):
    """n scalars of 32 bytes, uniform below 2^253 (< r)"""
    sc = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    sc[:, 31] &= 0x1F
    return sc.reshape(-1)


def child_points(path, n, group):
    import rapidsnark_old_amd as zk
    from rapidsnark_old_amd import synth
    if group == 1:
        g = synth.g1_gen_bytes()
        pts = zk.synth_chain_g1(n, zk.g1_mul(g, 1000003), zk.g1_mul(g, 7919))
    else:
        g = synth.g2_gen_bytes()
        pts = zk.synth_chain_g2(n, zk.g2_mul(g, 1000003), zk.g2_mul(g, 7919))
    pts.tofile(path)
    return 0


def child_op(path, reps, group):
    """alternating calls of both kernels over the file's points (run under the profiler by main): the new one first"""
    import rapidsnark_old_amd as zk
    pts = np.fromfile(path, dtype=np.uint8)
    nb = 64 * group
    n = pts.size // nb
    os.environ["ZKHIP_PTAU_CONTRIB_CHUNK"] = str(n)
    sc = scalars_for(n, 2026 + group)
    fn = zk.g1_mul_vec if group == 1 else zk.g2_mul_vec
    for _ in range(reps + 1):
        got = []
        for plain in ("0", "1"):
            os.environ["ZKHIP_MULVEC_PLAIN"] = plain
            got.append(fn(pts, sc))
        if not np.array_equal(got[0], got[1]):
            print("the two kernels disagree", file=sys.stderr)
            return 1
    return 0


def stat(d):
    d = sorted(d)
    return d[len(d) // 2], d[0], d[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g1-size", type=int, default=20)
    ap.add_argument("--g2-size", type=int, default=18)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--power", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ptau_contribute_timing.txt"))
    ap.add_argument("--child", nargs=4, metavar=("WHAT", "PATH", "N", "GROUP"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        what, path, n, group = args.child
        return {"op": child_op, "points": child_points}[what](path, int(n), int(group))
    if not shutil.which("rocprofv3"):
        raise SystemExit("rocprofv3 not found: kernel times come from nowhere else")
    me = [sys.executable, os.path.abspath(__file__), "--child"]
    tmp = tempfile.mkdtemp(prefix="ptau_contribute_timing_")
    f = lambda name: os.path.join(tmp, name)
    lines, table = [], []
    try:
        for group, size in ((1, args.g1_size), (2, args.g2_size)):
            if not size:
                continue
            n = 1 << size
            name = "zk_g%d_mul_vec" % group
            subprocess.run(limited(me + ["points", f("pts.bin"), str(n), str(group)], 200), check=True, timeout=300)
            prof = f("prof_g%d" % group)
            subprocess.run(limited(profiled(me + ["op", f("pts.bin"), str(args.reps), str(group)], prof), 400), check=True,
                           capture_output=True, timeout=500)
            os.remove(f("pts.bin"))
            durs = kernel_durations(prof)
            mul = [d for k, d in durs.items() if "k_mul_vec" in k]         # in the order of their first launch: new, plain
            if len(mul) != 2 or len(mul[0]) != args.reps + 1 or len(mul[1]) != args.reps + 1:
                raise SystemExit("%s: the trace does not hold two kernels of %d launches each: %r" % (name, args.reps + 1, {k: len(d) for k, d in durs.items()}))
            new, plain = mul[0][1:], mul[1][1:]
            norm = [d for k, d in durs.items() if "k_chain_normalize" in k and ("Fp2T" in k) == (group == 2)]
            chk = [d for k, d in durs.items() if "k_ptau_classify" in k]
            sub = [d for k, d in durs.items() if "k_g2_subgroup" in k]
            (nm, nlo, nhi), (pm, plo, phi) = stat(new), stat(plain)
            lines.append("%s, 2^%d points, a scalar for each, %d timed launches of each kernel, alternating" % (name, size, len(new)))
            lines.append("  k_mul_vec (128 columns)    median %9.3f ms  (least %9.3f, largest %9.3f)  %7.2f ns per point" % (nm, nlo, nhi, nm * 1e6 / n))
            lines.append("  k_mul_vec, plain (254 bit) median %9.3f ms  (least %9.3f, largest %9.3f)  %7.2f ns per point" % (pm, plo, phi, pm * 1e6 / n))
            lines.append("  ratio new / plain: %.3f  (of the medians; least / least %.3f); the operation count predicts %.2f" % (nm / pm, nlo / plo, PREDICTED))
            rest = "  k_chain_normalize median %.3f ms, k_ptau_classify %.3f ms" % (stat(norm[0][2:])[0] if norm else 0.0, stat(chk[0][2:])[0] if chk else 0.0)
            if sub:
                rest += ", k_g2_subgroup %.3f ms" % stat(sub[0][2:])[0]
            lines.append(rest + " a call")
            print("\n".join(lines[-5:]), flush=True)
        if args.power:
            n = 1 << args.power
            subprocess.run(limited([os.path.join(BIN, "ptaunew"), str(args.power), f("new.ptau")], 200), check=True, capture_output=True, timeout=300)
            cmd = [os.path.join(BIN, "ptaucontribute"), f("new.ptau"), f("out.ptau")]
            walls = []
            for _ in range(2):                                   # the first run also warms the page cache of the input
                t = time.time()
                subprocess.run(limited(cmd, 300), check=True, capture_output=True, timeout=400)
                walls.append(time.time() - t)
                os.remove(f("out.ptau"))
            subprocess.run(limited(profiled(cmd, f("prof_pot"), copies=True), 400), check=True, capture_output=True, timeout=500)
            durs = kernel_durations(f("prof_pot"))
            kern = sum(sum(d) for d in durs.values())
            copies = sum((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in trace_rows(f("prof_pot"), "memory_copy_trace.csv"))
            size = os.path.getsize(f("new.ptau"))
            lines += ["", "ptaucontribute on ptaunew's file of power %d (%d G1 and %d G2 points multiplied, file %.0f MiB): wall %.2f s, again %.2f s" % (
                args.power, 4 * n - 1, n, size / 2**20, walls[0], walls[1]),
                "  under the profiler: kernels %.0f ms, copies %.0f ms (they overlap each other and the host: two buffer sets); the rest of the wall is the"
                % (kern, copies), "  host's: mapping and reading the input, staging, writing %.0f MiB through the output's mapping, msync" % (size / 2**20)]
            table = sorted(((name, len(d), sum(d)) for name, d in durs.items()), key=lambda x: -x[2])
            print("\n".join(lines[-3:]), flush=True)
        try:
            clock = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        except (OSError, subprocess.SubprocessError):
            clock = ""
        clock = [ln.strip() for ln in clock.splitlines() if "sclk" in ln][:1]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = ["# tools/ptau_contribute_timing.py: zk_g1_mul_vec / zk_g2_mul_vec (n points times n scalars) and `ptaucontribute` on one MI355X",
           "# kernel times: rocprofv3 --kernel-trace, per launch; the yardstick is the same kernel with ZKHIP_MULVEC_PLAIN=1: devmem.hpp's",
           "# scalar_mul_affine (254 doublings and, the scalars of a wave differing, a mixed addition in nearly every one of them), in the same",
           "# process on the same points and scalars, alternating with the 128-column kernel",
           "# shader clock after the runs: " + (clock[0] if clock else "not read"), ""] + lines
    if table:
        out += ["", "# rocprofv3 --kernel-trace --stats, the ptaucontribute run (kernel, calls, total ms)"]
        out += ["%-90s %6d %10.2f" % (name[:90], calls, ms) for name, calls, ms in table]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
