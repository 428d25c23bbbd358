#!/usr/bin/env python3
"""What m = 64 PLONK proofs of one circuit cost in one zk_plonk_prove_many call against a loop of 64 PlonkProver.prove calls on
the same object, written to profiles/plonk_prove_many_timing.txt.

    python tools/plonk_prove_many_timing.py [--reps 5] [--sizes 11 14 16 17 18 20] [--widths 1 2 4 8 16] [--m 64] [--trace]

At every log_n of --sizes, one process, drawn blinds, a warm-up and --reps timed rounds; in a round the loop runs once and the
many-call once at every width of --widths, so the routes alternate.  The loop is the parent's way, not the code under test.
The many-call goes through the C entry with the 64 witnesses already back to back in one buffer (what a server holds); the loop
through PlonkProver.prove.  The circuit is tools/plonk_prover_timing.py's.  A width other than 1 gains at a size only if its
median beats the loop's by more than the loop's own least-to-largest spread in that run.
--trace adds, a size, a process of its own under `rocprofv3 --kernel-trace` (no counters in that run) at the size's best width:
kernel time a proof by kind.  Every GPU step is a child process under `timeout`."""
import argparse
import csv
import ctypes
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

from plonk_opening_timing import make_kzg  # noqa: E402
from plonk_prover_timing import K1, K2, circuit  # noqa: E402
from verify_timing import limited, stat  # noqa: E402

KNOB = "ZKHIP_PLONK_PROVE_BATCH"
NEW = ("k_wire_gather_many", "k_plonk_blind_many", "k_plonk_split_many")


def many_call(zk, p, m, buf, out, status):
    P = lambda a: ctypes.c_void_p(a.ctypes.data)       # noqa: E731
    rc = zk.load_library().zk_plonk_prove_many(p._handle(), m, P(out), P(status), P(buf), None, None)
    assert rc == 0 and not status.any(), (rc, status)


def child(what, log_n, reps, widths, m, out_path):
    import rapidsnark_old_amd as zk
    n = 1 << log_n
    circ, maps, witness = circuit(log_n)
    buf = np.tile(witness, m)
    out, status = np.zeros(m * 768, dtype=np.uint8), np.zeros(m, dtype=np.uint32)
    res = {"loop": [], "many": {str(B): [] for B in widths}, "info": {}}
    with make_kzg(zk, log_n) as k, zk.PlonkProver(k, *circ, K1, K2, *maps, n, 0) as p:
        if what == "traced":
            os.environ[KNOB] = str(widths[0])
            for _ in range(reps + 1):
                many_call(zk, p, m, buf, out, status)
        else:
            for rep in range(reps + 1):
                t0 = time.perf_counter()
                for _ in range(m):
                    p.prove(witness)
                res["loop"].append(time.perf_counter() - t0)
                res["lone_launches"] = p.info()["last_launches"]
                for B in widths:
                    os.environ[KNOB] = str(B)
                    if rep == 0:
                        many_call(zk, p, m, buf, out, status)      # the table, the slots and the buffers of this width are made here
                    t0 = time.perf_counter()
                    many_call(zk, p, m, buf, out, status)
                    res["many"][str(B)].append(time.perf_counter() - t0)
                    res["info"][str(B)] = p.many_info()
            with zk.PlonkVerifier(p.vkey()) as v:
                assert not v.verify(out.reshape(m, 768)).any()
    with open(out_path, "w") as fh:
        json.dump(res, fh)
    return 0


def kind(name):
    if any(k in name for k in NEW):
        return "new kernels"
    if any(k in name for k in ("msm", "k_bin_", "k_scan_local", "k_scan_sums", "k_scan_add", "k_precomp")):
        return "multiplications"
    return "looped cores"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--sizes", type=int, nargs="+", default=[11, 14, 16, 17, 18, 20])
    ap.add_argument("--widths", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_prove_many_timing.txt"))
    ap.add_argument("--child", nargs=3, metavar=("WHAT", "LOG_N", "PATH"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]), args.reps, args.widths, args.m, args.child[2])
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--m", str(args.m)]
    lines = ["# tools/plonk_prove_many_timing.py: m = %d proofs of one circuit on one MI355X, drawn blinds; %d timed rounds after a warm-up" % (args.m, args.reps),
             "# loop: %d PlonkProver.prove calls on the same object; many B: ONE zk_plonk_prove_many at ZKHIP_PLONK_PROVE_BATCH = B" % args.m,
             "# ms a call of %d proofs: median, least, largest; a round runs the loop, then every width" % args.m, ""]

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    for log_n in args.sizes:
        tmp = tempfile.mkdtemp(prefix="plonk_prove_many_timing_")
        try:
            wj = os.path.join(tmp, "walls.json")
            subprocess.run(limited(me + ["--widths"] + [str(B) for B in args.widths] + ["--child", "walls", str(log_n), wj], 500), check=True, timeout=560)
            res = json.load(open(wj))
            loop = stat([1e3 * x for x in res["loop"][1:]])
            spread = loop[2] - loop[1]
            lines += ["log_n %d: a lone proof is %d launches" % (log_n, res["lone_launches"]),
                      "    %-10s %10.3f %10.3f %10.3f   (%.3f ms a proof; spread %.3f ms)" % (("loop",) + loop + (loop[0] / args.m, spread))]
            best, best_ms = 1, loop[0]
            for B in args.widths:
                ms, inf = stat([1e3 * x for x in res["many"][str(B)][1:]]), res["info"][str(B)]
                gain = loop[0] - ms[0]
                held = ", table %d B (%d bits), slots %d B, buffers %d B" % (inf["table_bytes"], inf["window_bits"], inf["slot_bytes"], inf["msm_bytes"])
                lines.append("    many B=%-4d %10.3f %10.3f %10.3f   (%.3f ms a proof; loop - many = %+.3f ms: %s)  launches a proof %.1f, drains a proof %.1f, "
                             "multiplications %d%s"
                             % ((B,) + ms + (ms[0] / args.m, gain, "gains" if B > 1 and gain > spread else ("the loop itself" if B == 1 else "no gain beyond the spread"),
                                             inf["last_launches"] / args.m, inf["last_drains"] / args.m, inf["last_multiplications"],
                                             held if B > 1 else ", no table, no slots")))      # at B = 1 the object still holds the last width's
                if B > 1 and gain > spread and ms[0] < best_ms:
                    best, best_ms = B, ms[0]
            lines.append("    the fastest width that beats the loop by more than its spread: %d" % best)
            if args.trace and shutil.which("rocprofv3"):
                prof = os.path.join(tmp, "traced")
                cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", prof, "-o", "plonkmany", "--"] + me + ["--widths", str(best), "--child", "traced", str(log_n), os.path.join(tmp, "t.json")]
                subprocess.run(limited(cmd, 500), check=True, stdout=subprocess.DEVNULL, timeout=560)
                files = glob.glob(os.path.join(prof, "**", "*kernel_trace.csv"), recursive=True)
                by = {}
                if files:
                    with open(files[0]) as f:
                        for r in csv.DictReader(f):
                            found = re.search(r"k_\w+", r["Kernel_Name"])
                            kd = kind(found.group(0) if found else r["Kernel_Name"])
                            by[kd] = by.get(kd, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
                    proofs = args.m * (args.reps + 1)
                    ksum = sum(by.values())
                    lines.append("    kernels at B=%d over the traced process's %d proofs (the table's making with the multiplications), ms a proof: " % (best, proofs)
                                 + ", ".join("%s %.3f" % (kd, v / proofs) for kd, v in sorted(by.items())) + "; not kernels %.3f" % (best_ms / args.m - ksum / proofs))
                else:
                    lines.append("    kernels: the trace is empty: not measured")
            else:
                lines.append("    kernels by kind: not measured (run with --trace)")
            lines.append("")
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        flush()
    print("\n".join(lines))
    flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
