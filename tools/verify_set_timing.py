#!/usr/bin/env python3
"""Wall time of zk_vkey_set_verify against one zk_vkey_verify call per key, written to profiles/verify_set_timing.txt.

    python tools/verify_set_timing.py [--rows 4096:1 4096:5 4096:64 4096:1024 65536:1 65536:64 65536:1024] [--reps 5]

  * a row is n proofs over K keys.  The K key objects are made from the five golden circuits in rotation (key k is circuit
    k mod 5), proof i belongs to key i mod K and is a re-randomised copy of that circuit's golden proof
    (tools/verify_timing.py's batch), all valid; the thresholds and the chunk are the defaults;
  * both ways run in ONE process, alternating: a round is one VerificationKeySet.verify over all n proofs and then the loop
    of K VerificationKey.verify calls over the same proofs, each key's own (the single-key entry: what a caller without
    the set does); one warm-up round and --reps timed ones; median, least and largest of time.perf_counter around the
    Python calls (upload, kernels, download; the loop's per-key byte strings are made before the clock starts, the set
    call's grouping by key is inside it);
  * every verdict of every call is compared with OK.
The K = 1 rows put the set beside zk_vkey_verify on the same proofs.  Required: at n = 4096, K = 64 the set call takes at most
0.25 of the loop; the tool says so in the file and fails when it does not hold.  The GPU work is a child process under
`timeout`."""
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

GOLDENS = ["multiplier2", "r1cs_n8", "r1cs_n64", "r1cs_nopub", "r1cs_n256"]
REQUIRED = (4096, 64, 0.25)


def child(rows, reps, out_path):
    import rapidsnark_old_amd as zk
    kmax = max(k for _, k in rows)
    zkeys = [os.path.join(ROOT, "tests", "golden", g, "circuit.zkey") for g in GOLDENS]
    t0 = time.perf_counter()
    keys = [zk.VerificationKey.from_zkey(zkeys[k % 5]) for k in range(kmax)]
    res = {"keys_made": kmax, "keys_seconds": time.perf_counter() - t0}
    pools = {}                                          # circuit -> (proofs [m, 256], the circuit's signals)
    for n, K in rows:
        per_key = [len(range(k, n, K)) for k in range(K)]
        need = [sum(per_key[k] for k in range(K) if k % 5 == c) for c in range(5)]
        for c in range(5):
            if need[c] > (pools[c][0].shape[0] if c in pools else 0):
                proofs, publics, _ = batch(zk, GOLDENS[c], need[c])
                pools[c] = (proofs.reshape(need[c], 256), publics[:len(publics) // need[c]])
        # proof i: key i mod K; key k takes its circuit's pool in order
        taken = [0] * 5
        of_key = []
        for k in range(K):
            c = k % 5
            of_key.append(pools[c][0][taken[c]:taken[c] + per_key[k]])
            taken[c] += per_key[k]
        key_of = np.arange(n, dtype=np.uint32) % K
        mixed = np.empty((n, 256), dtype=np.uint8)
        for k in range(K):
            mixed[k::K] = of_key[k]
        publics = b"".join(pools[int(k) % 5][1] for k in key_of)
        loop_in = [(np.ascontiguousarray(of_key[k]).reshape(-1), pools[k % 5][1] * per_key[k]) for k in range(K)]
        mixed = mixed.reshape(-1)
        t_set, t_loop = [], []
        with zk.VerificationKeySet(keys[:K]) as ks:
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                v = ks.verify(mixed, key_of, publics)
                t_set.append(time.perf_counter() - t0)
                if v.size != n or v.any():
                    print("zk_vkey_set_verify: a verdict is not OK at n = %d, K = %d" % (n, K), file=sys.stderr)
                    return 1
                t0 = time.perf_counter()
                vs = [keys[k].verify(*loop_in[k]) for k in range(K) if per_key[k]]
                t_loop.append(time.perf_counter() - t0)
                if any(x.any() for x in vs) or sum(x.size for x in vs) != n:
                    print("zk_vkey_verify: a verdict is not OK at n = %d, K = %d" % (n, K), file=sys.stderr)
                    return 1
            info = ks.info()
        res["%d|%d" % (n, K)] = {"set": t_set[1:], "loop": t_loop[1:], "info": info, "loop_path": keys[0].info()["last_path"]}
        print("done: n = %d, K = %d" % (n, K), flush=True)
        with open(out_path, "w") as f:
            json.dump(res, f)
    for k in keys:
        k.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="+", default=["4096:1", "4096:5", "4096:64", "4096:1024", "65536:1", "65536:64", "65536:1024"], metavar="N:K")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_set_timing.txt"))
    ap.add_argument("--child", metavar="PATH", help=argparse.SUPPRESS)
    args = ap.parse_args()
    rows = [tuple(int(x) for x in r.split(":")) for r in args.rows]
    if args.child:
        return child(rows, args.reps, args.child)
    tmp = tempfile.mkdtemp(prefix="verify_set_timing_")
    rj = os.path.join(tmp, "res.json")
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--rows"] + args.rows + ["--child", rj]
    subprocess.run(limited(me, 1000), check=True, timeout=1100)
    res = json.load(open(rj))
    path = {0: "lanes", 1: "cooperative"}
    lines = ["# tools/verify_set_timing.py: zk_vkey_set_verify against the loop of one zk_vkey_verify call per key on one MI355X, one process,",
             "# the two alternating; key k is golden circuit k mod 5, proof i (re-randomised, valid) belongs to key i mod K; default thresholds and chunk;",
             "# %d timed rounds after a warm-up.  ms: median, least, largest of time.perf_counter around the Python calls;" % args.reps,
             "# ratio: set median / loop median of the same rounds.  %d key objects were made in %.1f s." % (res["keys_made"], res["keys_seconds"]), ""]
    failed = False
    for n, K in rows:
        r = res["%d|%d" % (n, K)]
        ms, slo, shi = stat([1e3 * x for x in r["set"]])
        ml, llo, lhi = stat([1e3 * x for x in r["loop"]])
        lines.append("n = %d, K = %d (%d proofs a key)" % (n, K, n // K))
        lines.append("  %-34s %10.3f %10.3f %10.3f   %8.3f us each   path %s, launches %d, padded waves %d" % (
            "zk_vkey_set_verify", ms, slo, shi, 1e3 * ms / n, path[r["info"]["last_path"]], r["info"]["last_launches"], r["info"]["last_waves_padded"]))
        lines.append("  %-34s %10.3f %10.3f %10.3f   %8.3f us each   path %s" % (
            "loop of %d zk_vkey_verify" % K, ml, llo, lhi, 1e3 * ml / n, path[r["loop_path"]]))
        note = ""
        if (n, K) == REQUIRED[:2]:
            ok = ms / ml <= REQUIRED[2]
            failed = failed or not ok
            note = "   required: at most %.2f: %s" % (REQUIRED[2], "met" if ok else "NOT MET")
        lines.append("  ratio %.3f%s" % (ms / ml, note))
        lines.append("")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
