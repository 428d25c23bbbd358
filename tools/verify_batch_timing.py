#!/usr/bin/env python3
"""Wall time of zk_vkey_verify_batch against zk_vkey_verify, written to profiles/verify_batch_timing.txt.

    python tools/verify_batch_timing.py [--sizes 4096 65536 262144] [--groups 64 256 1024 4096] [--reps 5] [--golden r1cs_n64]

  * the proofs: tools/verify_timing.py's re-randomised copies of one golden proof, all distinct, one chunk per call
    (ZKHIP_VERIFY_CHUNK = n); three mixtures: all valid, one INVALID proof (B not rescaled) per 4096, one per 256;
  * both entries run in ONE process, alternating: per mixture a round is one VerificationKey.verify and one verify_batch
    per group size; one warm-up round and --reps timed ones; median, least and largest of time.perf_counter around the
    Python call (upload, kernels, download; the batch call also draws its scalars);
  * every verdict of every call is compared with the mixture's own.
The GPU work is a child process under `timeout`."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from verify_timing import batch, limited, stat  # noqa: E402

MIXTURES = [("all valid", 0), ("one INVALID per 4096", 4096), ("one INVALID per 256", 256)]


def child(golden, sizes, groups, reps, out_path):
    import rapidsnark_old_amd as zk
    from rapidsnark_old_amd import verify as V
    gold_b = np.frombuffer(V.load_proof(os.path.join(ROOT, "tests", "golden", golden, "proof.json"))[64:192], dtype=np.uint8)
    res = {}
    for n in sizes:
        os.environ["ZKHIP_VERIFY_CHUNK"] = str(n)
        valid, publics, zkey = batch(zk, golden, n)
        with zk.VerificationKey.from_zkey(zkey) as vk:
            for label, every in MIXTURES:
                proofs = valid.copy().reshape(n, 256)
                want = np.zeros(n, dtype=np.uint8)
                if every:
                    at = np.arange(every // 2, n, every)
                    proofs[at, 64:192] = gold_b
                    want[at] = 1
                proofs = proofs.reshape(-1)
                t = {"verify": []}
                t.update({str(g): [] for g in groups})
                rep = {}
                for _ in range(reps + 1):
                    t0 = time.perf_counter()
                    v = vk.verify(proofs, publics)
                    t["verify"].append(time.perf_counter() - t0)
                    if not np.array_equal(v, want):
                        print("zk_vkey_verify: a verdict differs at n = %d, %s" % (n, label), file=sys.stderr)
                        return 1
                    for g in groups:
                        os.environ["ZKHIP_VERIFY_GROUP"] = str(g)
                        t0 = time.perf_counter()
                        v, rep[str(g)] = vk.verify_batch(proofs, publics)
                        t[str(g)].append(time.perf_counter() - t0)
                        if not np.array_equal(v, want):
                            print("zk_vkey_verify_batch: a verdict differs at n = %d, group %d, %s" % (n, g, label), file=sys.stderr)
                            return 1
                res["%d|%s" % (n, label)] = {"t": {k: x[1:] for k, x in t.items()}, "rep": rep}
                print("done: n = %d, %s" % (n, label), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--groups", type=int, nargs="+", default=[64, 256, 1024, 4096])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--golden", default="r1cs_n64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch_timing.txt"))
    ap.add_argument("--child", metavar="PATH", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.golden, args.sizes, args.groups, args.reps, args.child)
    tmp = tempfile.mkdtemp(prefix="verify_batch_timing_")
    rj = os.path.join(tmp, "res.json")
    me = [sys.executable, os.path.abspath(__file__), "--golden", args.golden, "--reps", str(args.reps), "--sizes"] + [str(n) for n in args.sizes] + \
         ["--groups"] + [str(g) for g in args.groups] + ["--child", rj]
    subprocess.run(limited(me, 900), check=True, timeout=1000)
    res = json.load(open(rj))
    lines = ["# tools/verify_batch_timing.py: zk_vkey_verify_batch against zk_vkey_verify on one MI355X, one process, the calls alternating,",
             "# re-randomised copies of the %s golden proof, one chunk per call, %d timed calls after a warm-up" % (args.golden, args.reps),
             "# ms: median, least, largest of time.perf_counter around the Python call; ratio: batch median / per-proof median of the same rounds", ""]
    for n in args.sizes:
        for label, _ in MIXTURES:
            r = res["%d|%s" % (n, label)]
            m0, lo, hi = stat([1e3 * x for x in r["t"]["verify"]])
            lines.append("n = %d, %s" % (n, label))
            lines.append("  %-28s %10.3f %10.3f %10.3f   %8.3f us each" % ("zk_vkey_verify", m0, lo, hi, 1e3 * m0 / n))
            for g in args.groups:
                m, lo, hi = stat([1e3 * x for x in r["t"][str(g)]])
                rp = r["rep"][str(g)]
                lines.append("  %-28s %10.3f %10.3f %10.3f   %8.3f us each   ratio %.3f   groups %d failed %d rechecked %d launches %d" % (
                    "zk_vkey_verify_batch g=%d" % g, m, lo, hi, 1e3 * m / n, m / m0, rp["groups"], rp["groups_failed"], rp["proofs_rechecked"], rp["launches"]))
            lines.append("")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
