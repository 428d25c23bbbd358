#!/usr/bin/env python3
"""What the KZG layer costs on one MI355X, written to profiles/kzg_timing.txt.

    python tools/kzg_timing.py [--reps 5] [--segs 1 4 16 64 256]

  * the file: a power-20 trapdoor .ptau (not prepared) that the tool makes on the GPU; one Kzg object over its 2^20 first points;
  * commit at n = 2^20 beside zk_msm_g1 on the same points and scalars, one process, the calls alternating;
  * open at n = 2^20 (wall), and the share of it that the division kernels take;
  * verify at m = 65536 beside zk_vkey_verify on 65536 re-randomised copies of the r1cs_n64 golden proof, alternating, and
    verify_batch beside verify at m = 65536, alternating;
  * the division kernels at 2^20 and 2^24 coefficients for every ZKHIP_KZG_SEG of --segs: a process of its own under
    `rocprofv3 --kernel-trace`; ns per coefficient and bytes per second (96 bytes a coefficient: k_div_reduce reads it,
    k_div_apply reads it again and writes the quotient) against the 8 TB/s of the HBM.
Every entry: one warm-up call and --reps timed ones; median, least, largest.  Walls are time.perf_counter around the Python
call (upload, kernels, download).  Every GPU step is a child process under `timeout`."""
import argparse
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

from verify_timing import batch, kernel_durations, limited, stat  # noqa: E402

POWER, N, M = 20, 1 << 20, 65536
DIV_SIZES = (1 << 20, 1 << 24)
HBM_PEAK = 8.0e12
KERNELS = ("k_div_reduce", "k_div_carry", "k_div_apply")


def scalars(n, seed):
    """n values below 2^248 (< r), 32 bytes each"""
    a = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 31] = 0
    return a.reshape(-1)


def walls(reps, out_path):
    import rapidsnark_old_amd as zk
    res = {}
    tmp = tempfile.mkdtemp(prefix="kzg_timing_")
    try:
        path = os.path.join(tmp, "p20.ptau")
        zk.write_trapdoor_ptau(POWER, 0x1234567, 0x89ABCDE, 0xF012345, path, prepared=False)
        f = zk.PtauFile(path)
        points = np.ascontiguousarray(f.section(2)[:N * 64]).copy()
        with zk.Kzg(f, max_coeffs=N) as k:
            f.close()
            sc = scalars(N, 1)
            t = {"commit": [], "msm_g1": []}
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                a = k.commit(sc)
                t1 = time.perf_counter()
                b = zk.msm_g1(points, sc)
                t2 = time.perf_counter()
                t["commit"].append(t1 - t0)
                t["msm_g1"].append(t2 - t1)
                if bytes(a) != bytes(b):
                    print("zk_kzg_commit and zk_msm_g1 differ", file=sys.stderr)
                    return 1
            t["open"] = []
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                ys, pi = k.open(sc, 0x5555)
                t["open"].append(time.perf_counter() - t0)
            res["info"] = k.info()
            # 65536 openings: sixteen distinct ones of small polynomials, repeated
            ops = []
            for j in range(16):
                p = [int(v) for v in np.random.default_rng(j).integers(1, 1 << 62, size=33)]
                z = 1000 + j
                ys, pi = k.open(p, z)
                ops.append((bytes(k.commit(p)), z, ys[0], bytes(pi)))
            rep = M // 16
            C, P = b"".join(o[0] for o in ops) * rep, b"".join(o[3] for o in ops) * rep
            zs = np.frombuffer(b"".join(o[1].to_bytes(32, "little") for o in ops) * rep, dtype=np.uint8)
            ys = np.frombuffer(b"".join(o[2].to_bytes(32, "little") for o in ops) * rep, dtype=np.uint8)
            os.environ["ZKHIP_VERIFY_CHUNK"] = str(M)
            proofs, publics, zkey = batch(zk, "r1cs_n64", M)
            t.update({"kzg_verify": [], "vkey_verify": [], "kzg_verify_2": [], "kzg_verify_batch": []})
            with zk.VerificationKey.from_zkey(zkey) as vk:
                for _ in range(reps + 1):
                    t0 = time.perf_counter()
                    v = k.verify(C, zs, ys, P)
                    t1 = time.perf_counter()
                    w = vk.verify(proofs, publics)
                    t2 = time.perf_counter()
                    t["kzg_verify"].append(t1 - t0)
                    t["vkey_verify"].append(t2 - t1)
                    if v.any() or w.any():
                        print("a valid opening or proof was refused", file=sys.stderr)
                        return 1
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                v = k.verify(C, zs, ys, P)
                t1 = time.perf_counter()
                one = k.verify_batch(C, zs, ys, P)
                t2 = time.perf_counter()
                t["kzg_verify_2"].append(t1 - t0)
                t["kzg_verify_batch"].append(t2 - t1)
                if v.any() or one != 0:
                    print("a valid batch was refused", file=sys.stderr)
                    return 1
        res["t"] = {name: x[1:] for name, x in t.items()}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh)
    return 0


def divide(reps, segs, out_path):
    """the calls the profiler watches, in a known order: size, then seg, then a warm-up and `reps` timed calls"""
    import rapidsnark_old_amd as zk
    for n in DIV_SIZES:
        c = scalars(n, n)
        for seg in segs:
            os.environ["ZKHIP_KZG_SEG"] = str(seg)
            for _ in range(reps + 1):
                zk.fr_poly_divide(c, 0x5555)
    with open(out_path, "w") as fh:
        json.dump({"ok": True}, fh)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--segs", type=int, nargs="+", default=[1, 4, 16, 64, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_timing.txt"))
    ap.add_argument("--child", nargs=2, metavar=("WHAT", "PATH"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return walls(args.reps, args.child[1]) if args.child[0] == "walls" else divide(args.reps, args.segs, args.child[1])
    if not shutil.which("rocprofv3"):
        raise SystemExit("rocprofv3 not found: kernel times come from nowhere else")
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--segs"] + [str(s) for s in args.segs] + ["--child"]
    tmp = tempfile.mkdtemp(prefix="kzg_timing_")
    try:
        wj = os.path.join(tmp, "walls.json")
        subprocess.run(limited(me + ["walls", wj], 500), check=True, timeout=600)
        res = json.load(open(wj))
        prof = os.path.join(tmp, "prof")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", prof, "-o", "kzg", "--"] + me + ["divide", os.path.join(tmp, "d.json")]
        subprocess.run(limited(cmd, 500), check=True, capture_output=True, timeout=600)
        durs = kernel_durations(prof)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    ms = {name: stat([1e3 * x for x in v]) for name, v in res["t"].items()}
    row = lambda name, label: "  %-34s %10.3f %10.3f %10.3f" % ((label,) + ms[name])
    lines = ["# tools/kzg_timing.py: the KZG layer on one MI355X; a power-%d trapdoor .ptau made by the tool, one object over 2^%d points" % (POWER, POWER),
             "# one process for the walls, entries that are compared alternate; %d timed calls after a warm-up" % args.reps,
             "# ms: median, least, largest of time.perf_counter around the Python call (upload, kernels, download)", "",
             "commit at n = 2^20 beside zk_msm_g1 on the same points and scalars",
             row("commit", "Kzg.commit"), row("msm_g1", "zk_msm_g1"),
             "  ratio commit / zk_msm_g1 %.3f" % (ms["commit"][0] / ms["msm_g1"][0]), "",
             "open at n = 2^20 (division, then the commitment of the quotient)", row("open", "Kzg.open"), "",
             "verification at m = %d, one chunk per call" % M,
             row("kzg_verify", "Kzg.verify"), row("vkey_verify", "VerificationKey.verify (r1cs_n64)"),
             "  ratio Kzg.verify / VerificationKey.verify %.3f" % (ms["kzg_verify"][0] / ms["vkey_verify"][0]),
             row("kzg_verify_2", "Kzg.verify"), row("kzg_verify_batch", "Kzg.verify_batch"),
             "  ratio verify_batch / verify %.3f" % (ms["kzg_verify_batch"][0] / ms["kzg_verify_2"][0]), "",
             "object: " + json.dumps(res["info"], sort_keys=True), "",
             "division kernels (rocprofv3 --kernel-trace, a process of its own), per call: the three launches' durations added",
             "  %8s %6s %10s %10s %10s %12s %10s %10s" % ("n", "seg", "median us", "least", "largest", "ns / coeff", "TB/s", "of peak")]
    per = {k: [v for name, vs in durs.items() if k in name for v in vs] for k in KERNELS}
    # kernel_durations orders each kernel's launches by start time; every call makes one launch of each, in the order divide() made them
    calls = len(DIV_SIZES) * len(args.segs) * (args.reps + 1)
    best = None
    if all(len(per[k]) == calls for k in KERNELS):
        at = 0
        for n in DIV_SIZES:
            for seg in args.segs:
                tot = [sum(per[k][at + r] for k in KERNELS) for r in range(1, args.reps + 1)]      # ms, the warm-up dropped
                at += args.reps + 1
                m, lo, hi = stat(tot)
                lines.append("  %8d %6d %10.1f %10.1f %10.1f %12.4f %10.3f %9.1f%%" % (n, seg, 1e3 * m, 1e3 * lo, 1e3 * hi, 1e6 * m / n, 96.0 * n / (m * 1e-3) / 1e12,
                                                                                 100 * 96.0 * n / (m * 1e-3) / HBM_PEAK))
                if n == N and (best is None or m < best[1]):
                    best = (seg, m)
                if n == N and seg == res["info"]["seg"]:
                    lines.append("  %8s        the division's share of Kzg.open's wall at 2^20: %.2f%%" % ("", 100 * m / ms["open"][0]))
        lines.append("  the best ZKHIP_KZG_SEG at 2^20: %d" % best[0])
    else:
        lines.append("  the trace holds %s launches, %d of each expected: not tabulated" % ({k: len(v) for k, v in per.items()}, calls))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
