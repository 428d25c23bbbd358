#!/usr/bin/env python3
"""What PLONK batch verification by random combination costs on one MI355X against the per-proof entry, written to
profiles/plonk_verify_batch_timing.txt.

    python tools/plonk_verify_batch_timing.py [--reps 5]

One process measures both entries on ONE PlonkVerifier, so that they meet the same machine in the same minute: at log_n 11
with 2 public inputs, m = 64, 4096 and 65536 valid proofs, PlonkVerifier.verify (the yardstick) and PlonkVerifier.verify_batch
with ZKHIP_PLONK_VERIFY_GROUP = 1024, 4096, 16384 and 65536 (groups above m are the same call: timed once).  A warm-up of every
entry, then --reps rounds in which the entries alternate; wall time of time.perf_counter around the Python call, which ends in
the library's stream synchronise; medians.  Then, at 65536: one invalid proof, and 1 % invalid proofs spread evenly (every
100th), for every group.  Every timed call's verdicts are checked.

Kernel times come from a process of its own under `rocprofv3 --kernel-trace` (no counters in that run): 1 + reps calls of
verify, then 1 + reps calls of verify_batch at 65536 valid proofs with the group that had the lowest median in the first
process; the mean per call, by stage.  Every GPU step is a child process under `timeout`.  The shader clock is read after
the runs.

The proofs are real: tools/plonk_verifier_timing.py's key and batch (8 distinct proofs repeated to m; nothing in the verifier
remembers a proof).  An invalid proof is a valid one with one byte of its fourth value changed."""
import argparse
import glob
import csv
import json
import os
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
from plonk_verifier_timing import LOG_N, make_batch, tiled  # noqa: E402
from verify_timing import limited, stat  # noqa: E402

MS = (64, 4096, 65536)
GROUPS = (1024, 4096, 16384, 65536)
KNOB = "ZKHIP_PLONK_VERIFY_GROUP"
N_PUBLIC = 2
STAGES = (("transcript", ("k_plonk_transcript",)), ("scale and fold", ("k_plonk_batch_scale", "k_plonk_batch_fold")), ("gather", ("k_plonk_batch_gather",)),
          ("cooperative pairing", ("k_pairing_coop",)), ("combination (verify)", ("k_plonk_combine", "k_plonk_sum")), ("pairing (verify)", ("k_kzg_pair",)))
OTHER = "bucket multiplication (sort, accumulation, reduction)"


def spoiled(a, every):
    """a copy with proof every - 1, 2 every - 1, .. made invalid (every = 0: the one in the middle)"""
    b = a.copy()
    rows = range(every - 1, len(b), every) if every else [len(b) // 2]
    for i in rows:
        b[i, 576 + 3 * 32 + 5] ^= 0x10
    return b, list(rows)


def timed(call, check):
    t0 = time.perf_counter()
    out = call()
    dt = time.perf_counter() - t0
    check(out)
    return dt, out


def child(what, reps, out_path, group):
    import rapidsnark_old_amd as zk
    res = {"rows": []}
    with make_kzg(zk, LOG_N) as kzg:
        vk, proofs, publics = make_batch(zk, kzg, N_PUBLIC)
    with zk.PlonkVerifier(vk) as v:
        def all_ok(out):
            got = out[0] if isinstance(out, tuple) else out
            assert not got.any(), "the batch does not verify"

        if what == "traced":
            a, pb = tiled(proofs, publics, MS[-1])
            os.environ[KNOB] = str(group)
            for _ in range(1 + reps):
                all_ok(v.verify(a, pb))
            for _ in range(1 + reps):
                all_ok(v.verify_batch(a, pb))
            res["calls"] = 1 + reps
        else:
            for m in MS:
                a, pb = tiled(proofs, publics, m)
                cases = [("all valid", a, [])]
                if m == MS[-1]:
                    cases += [("one invalid",) + spoiled(a, 0), ("1 % invalid",) + spoiled(a, 100)]
                for label, arr, bad in cases:
                    def right(out, bad=bad, m=m):
                        got = out[0] if isinstance(out, tuple) else out
                        assert got.shape == (m,) and list(np.nonzero(got)[0]) == bad and all(got[i] == 1 for i in bad), "wrong verdicts"

                    groups = sorted({min(g, m) for g in GROUPS})
                    entries = [("verify", None)] + [("batch", g) for g in groups]
                    walls = {e: [] for e in entries}
                    reports = {}
                    for rnd in range(1 + reps):          # round 0: the warm-up
                        for e in entries:
                            if e[1] is None:
                                dt, _ = timed(lambda: v.verify(arr, pb), right)
                            else:
                                os.environ[KNOB] = str(e[1])
                                dt, out = timed(lambda: v.verify_batch(arr, pb), right)
                                reports[e[1]] = out[1]
                            if rnd:
                                walls[e].append(dt)
                    res["rows"].append({"m": m, "case": label, "verify": walls[("verify", None)],
                                        "batch": {str(g): walls[("batch", g)] for g in groups}, "reports": {str(g): reports[g] for g in groups}})
    with open(out_path, "w") as fh:
        json.dump(res, fh)
    return 0


def kernel_table(prof_dir, calls):
    """{stage: mean ms a call} for verify and for verify_batch, from the trace of `calls` calls of each"""
    files = glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    first = next((i for i, r in enumerate(rows) if "k_plonk_transcript" in r["Kernel_Name"]), len(rows))
    rows = rows[first:]                                  # before it: the prover that made the proofs
    total, count = {}, {}
    for r in rows:
        name = r["Kernel_Name"]
        stage = next((s for s, names in STAGES if any(n in name for n in names)), OTHER)
        total[stage] = total.get(stage, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        count[stage] = count.get(stage, 0) + 1
    if count.get("transcript", 0) != 2 * calls * 1:
        return None
    out = {s: (total[s] / calls, count[s] / calls) for s in total}
    out["transcript"] = (total["transcript"] / (2 * calls), 1.0)          # both entries run it
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_verify_batch_timing.txt"))
    ap.add_argument("--child", nargs=3, metavar=("WHAT", "PATH", "GROUP"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.reps, args.child[1], int(args.child[2]))
    if not shutil.which("rocprofv3"):
        raise SystemExit("rocprofv3 not found: kernel times come from nowhere else")
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--child"]
    tmp = tempfile.mkdtemp(prefix="plonk_verify_batch_timing_")
    try:
        wj = os.path.join(tmp, "walls.json")
        subprocess.run(limited(me + ["walls", wj, "0"], 500), check=True, timeout=560)
        rows = json.load(open(wj))["rows"]
        top = next(r for r in rows if r["m"] == MS[-1] and r["case"] == "all valid")
        best = min(top["batch"], key=lambda g: stat(top["batch"][g])[0])
        prof = os.path.join(tmp, "traced")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", prof, "-o", "plonkbatch", "--"] + me + ["traced", os.path.join(tmp, "t.json"), best]
        subprocess.run(limited(cmd, 300), check=True, stdout=subprocess.DEVNULL, timeout=360)
        table = kernel_table(prof, 1 + args.reps)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    try:
        clock = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
    except (OSError, subprocess.SubprocessError):
        clock = ""
    clock = [ln.strip() for ln in clock.splitlines() if "sclk" in ln][:1]
    lines = ["# tools/plonk_verify_batch_timing.py: PlonkVerifier.verify_batch against PlonkVerifier.verify on one object, one MI355X, log_n %d, n_public %d;"
             % (LOG_N, N_PUBLIC),
             "# a warm-up, then %d rounds in which the entries alternate; wall ms of the Python call: median (least .. largest)" % args.reps,
             "# shader clock after the runs: " + (clock[0] if clock else "not read"), ""]
    for r in rows:
        ve = stat([1e3 * x for x in r["verify"]])
        lines.append("m = %d, %s" % (r["m"], r["case"]))
        lines.append("  verify                 %9.3f (%.3f .. %.3f)" % ve)
        for g, w in r["batch"].items():
            b = stat([1e3 * x for x in w])
            rep = r["reports"][g]
            lines.append("  verify_batch group %-6s %7.3f (%.3f .. %.3f)  / verify %.2f   groups %d, failed %d, rechecked %d, launches %d"
                         % ((g,) + b + (b[0] / ve[0], rep["groups"], rep["groups_failed"], rep["proofs_rechecked"], rep["launches"])))
        lines.append("")
    lines.append("the lowest all-valid median at m = %d: group %s" % (MS[-1], best))
    lines.append("")
    if table:
        lines.append("kernels at m = %d, all valid, group %s (rocprofv3 --kernel-trace, a process of its own; mean ms a call over %d calls of each entry, dispatches a call):"
                     % (MS[-1], best, 1 + args.reps))
        batch_stages = ["transcript", "scale and fold", "gather", OTHER, "cooperative pairing"]
        verify_stages = ["transcript", "combination (verify)", "pairing (verify)"]
        for title, stages in (("verify_batch", batch_stages), ("verify", verify_stages)):
            lines.append("  %s: " % title + "; ".join("%s %.3f (%.0f)" % ((s,) + table.get(s, (0.0, 0))) for s in stages) +
                         "; together %.3f" % sum(table.get(s, (0.0, 0))[0] for s in stages))
    else:
        lines.append("kernels: the trace does not hold the expected dispatches: not tabulated")
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
