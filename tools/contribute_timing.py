#!/usr/bin/env python3
"""Kernel time of zk_g1_scale against its yardstick, and wall time of `zkeycontribute`, written to
profiles/contribute_timing.txt.

    python tools/contribute_timing.py [--sizes 20 22] [--reps 5] [--key-power 22] [--out profiles/contribute_timing.txt]

  * the operator: n = 2^size valid points (synth chain), one fixed 254-bit scalar, the whole row as ONE chunk
    (ZKHIP_SCALE_CHUNK = n: a launch per call, the points resident while it runs).  One process per size under `rocprofv3
    --kernel-trace --stats` calls zk_g1_scale alternately with k_scale_g1 (endomorphism split + joint sparse form) and with
    ZKHIP_SCALE_PLAIN=1 (k_scale_g1_plain: devmem.hpp's scalar_mul_affine, the 254-bit double-and-add the project had
    before), one warm-up pair and --reps timed pairs, and checks that both give the same bytes.  Per kernel the median, the
    least and the largest duration of the timed launches, ns per point, the ratio new / plain, and the share of the
    normalisation and of the point check in a call's kernel time;
  * `zkeycontribute` on a key of a 2^key-power circuit's shape (nVars = domainSize = 2^power, 2 public signals; every
    table a chain of valid points, the coefficient records zero: the program reads none of them): wall of the whole process,
    then a second run under `rocprofv3 --kernel-trace --memory-copy-trace --stats` whose kernel and copy totals split it;
    the rest is the host's (mapping and reading the input, staging, writing the output through its mapping).
Every GPU step is a process of its own under `timeout`; the first one that fails ends the tool."""
import argparse
import csv
import glob
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from oracle.bn254 import R_MOD, Q_MOD  # noqa: E402

BIN = os.path.join(ROOT, "rapidsnark-old_amd")
K = 0x2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F80919 % R_MOD


def limited(cmd, seconds):
    return ["timeout", "-k", "10", str(seconds)] + cmd


def profiled(cmd, prof_dir, copies=False):
    return ["rocprofv3", "--kernel-trace"] + (["--memory-copy-trace"] if copies else []) + \
           ["--stats", "--output-format", "csv", "-d", prof_dir, "-o", "contrib", "--"] + cmd


def trace_rows(prof_dir, suffix):
    files = glob.glob(os.path.join(prof_dir, "**", "*" + suffix), recursive=True)
    if not files:
        return []
    with open(files[0]) as f:
        return list(csv.DictReader(f))


def kernel_durations(prof_dir):
    """-> {kernel name: [duration ms of every dispatch, in start order]}"""
    out = {}
    rows = sorted(trace_rows(prof_dir, "kernel_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        out.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    return out


def pick(durs, *words, without=()):
    for name, d in durs.items():
        if all(w in name for w in words) and not any(w in name for w in without):
            return d
    return []


def chain_points(zk, n, seed):
    from rapidsnark_old_amd import synth
    g1 = synth.g1_gen_bytes()
    return zk.synth_chain_g1(n, zk.g1_mul(g1, 1000003 + seed), zk.g1_mul(g1, 7919 + 2 * seed))


def child_op(path, reps):
    """alternating calls of both kernels over the file's points (run under the profiler by main)"""
    import rapidsnark_old_amd as zk
    pts = np.fromfile(path, dtype=np.uint8)
    os.environ["ZKHIP_SCALE_CHUNK"] = str(pts.size // 64)
    for _ in range(reps + 1):
        got = []
        for plain in ("0", "1"):
            os.environ["ZKHIP_SCALE_PLAIN"] = plain
            got.append(zk.g1_scale(pts, K))
        if not np.array_equal(got[0], got[1]):
            print("the two kernels disagree", file=sys.stderr)
            return 1
    return 0


def child_points(path, n):
    import rapidsnark_old_amd as zk
    chain_points(zk, n, 1).tofile(path)
    return 0


def child_key(path, power):
    """a .zkey of a 2^power circuit's shape: valid points everywhere, zero coefficient records"""
    import rapidsnark_old_amd as zk
    from rapidsnark_old_amd import synth
    n = nv = 1 << power
    npub = 2
    g1, g2 = synth.g1_gen_bytes(), synth.g2_gen_bytes()
    ncoef = 4 * n
    sec2 = (struct.pack("<I", 32) + Q_MOD.to_bytes(32, "little") + struct.pack("<I", 32) + R_MOD.to_bytes(32, "little") +
            struct.pack("<III", nv, npub, n) + zk.g1_mul(g1, 11) + zk.g1_mul(g1, 13) + zk.g2_mul(g2, 13) + zk.g2_mul(g2, 17) +
            zk.g1_mul(g1, 19) + zk.g2_mul(g2, 19))
    b2 = zk.synth_chain_g2(nv, zk.g2_mul(g2, 5), zk.g2_mul(g2, 3))
    secs = [(1, struct.pack("<I", 1)), (2, sec2), (3, chain_points(zk, npub + 1, 3)), (4, None), (5, chain_points(zk, nv, 5)),
            (6, chain_points(zk, nv, 6)), (7, b2), (8, chain_points(zk, nv - npub - 1, 8)), (9, chain_points(zk, n, 9)), (10, bytes(68))]
    with open(path, "wb") as f:
        f.write(b"zkey" + struct.pack("<II", 1, len(secs)))
        for sid, payload in secs:
            if sid == 4:
                f.write(struct.pack("<IQ", 4, 4 + 44 * ncoef) + struct.pack("<I", ncoef))
                zero = bytes(44 << 16)
                for _ in range(ncoef >> 16):
                    f.write(zero)
                continue
            payload = payload if isinstance(payload, bytes) else np.ascontiguousarray(payload).tobytes()
            f.write(struct.pack("<IQ", sid, len(payload)))
            f.write(payload)
    return 0


def stat(d):
    d = sorted(d)
    return d[len(d) // 2], d[0], d[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--key-power", type=int, default=22)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contribute_timing.txt"))
    ap.add_argument("--child", nargs=3, metavar=("WHAT", "PATH", "N"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        what, path, n = args.child
        return {"op": child_op, "points": child_points, "key": child_key}[what](path, int(n))
    if not shutil.which("rocprofv3"):
        raise SystemExit("rocprofv3 not found: kernel times come from nowhere else")
    me = [sys.executable, os.path.abspath(__file__), "--child"]
    tmp = tempfile.mkdtemp(prefix="contribute_timing_")
    f = lambda name: os.path.join(tmp, name)
    lines, table = [], []
    try:
        for size in args.sizes:
            n = 1 << size
            subprocess.run(limited(me + ["points", f("pts.bin"), str(n)], 300), check=True, timeout=400)
            subprocess.run(limited(profiled(me + ["op", f("pts.bin"), str(args.reps)], f("prof%d" % size)), 600), check=True,
                           capture_output=True, timeout=700)
            os.remove(f("pts.bin"))
            durs = kernel_durations(f("prof%d" % size))
            new, plain = pick(durs, "k_scale_g1", without=("plain",))[1:], pick(durs, "k_scale_g1_plain")[1:]
            norm, chk = pick(durs, "k_chain_normalize")[2:], pick(durs, "k_point_check")[2:]
            (nm, nlo, nhi), (pm, plo, phi) = stat(new), stat(plain)
            lines.append("2^%d points, %d timed launches each, alternating" % (size, len(new)))
            lines.append("  k_scale_g1        median %9.3f ms  (least %9.3f, largest %9.3f)  %7.2f ns per point" % (nm, nlo, nhi, nm * 1e6 / n))
            lines.append("  k_scale_g1_plain  median %9.3f ms  (least %9.3f, largest %9.3f)  %7.2f ns per point" % (pm, plo, phi, pm * 1e6 / n))
            lines.append("  ratio k_scale_g1 / k_scale_g1_plain: %.3f  (of the medians; least / least %.3f)" % (nm / pm, nlo / plo))
            om, cm = stat(norm)[0], stat(chk)[0]
            lines.append("  k_chain_normalize median %9.3f ms, k_point_check %7.3f ms: %.1f %% and %.1f %% of a call's kernel time with k_scale_g1" % (
                om, cm, 100 * om / (nm + om + cm), 100 * cm / (nm + om + cm)))
            print("\n".join(lines[-5:]), flush=True)
        if args.key_power:
            n = 1 << args.key_power
            subprocess.run(limited(me + ["key", f("in.zkey"), str(args.key_power)], 600), check=True, timeout=700)
            cmd = [os.path.join(BIN, "zkeycontribute"), f("in.zkey"), f("out.zkey")]
            walls = []
            for _ in range(2):                                   # the first run also warms the page cache of the input
                t = time.time()
                subprocess.run(limited(cmd, 600), check=True, capture_output=True, timeout=700)
                walls.append(time.time() - t)
                os.remove(f("out.zkey"))
            subprocess.run(limited(profiled(cmd, f("prof_key"), copies=True), 600), check=True, capture_output=True, timeout=700)
            durs = kernel_durations(f("prof_key"))
            kern = sum(sum(d) for d in durs.values())
            copies = sum((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in trace_rows(f("prof_key"), "memory_copy_trace.csv"))
            size = os.path.getsize(f("in.zkey"))
            lines += ["", "zkeycontribute on a key of a 2^%d circuit's shape (%d + %d points scaled, file %.0f MiB): wall %.2f s, again %.2f s" % (
                args.key_power, n - 3, n, size / 2**20, walls[0], walls[1]),
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
    out = ["# tools/contribute_timing.py: zk_g1_scale (n G1 points times one scalar) and `zkeycontribute` on one MI355X",
           "# kernel times: rocprofv3 --kernel-trace, per launch; the yardstick k_scale_g1_plain is devmem.hpp's scalar_mul_affine (254 doublings,",
           "# ~127 mixed additions) with the same shared scalar, in the same process, alternating with k_scale_g1",
           "# shader clock after the runs: " + (clock[0] if clock else "not read"), ""] + lines
    if table:
        out += ["", "# rocprofv3 --kernel-trace --stats, the zkeycontribute run (kernel, calls, total ms)"]
        out += ["%-90s %6d %10.2f" % (name[:90], calls, ms) for name, calls, ms in table]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
