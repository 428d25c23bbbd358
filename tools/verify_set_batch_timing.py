#!/usr/bin/env python3
"""Wall time of zk_vkey_set_verify_batch against zk_vkey_set_verify on the same input, written to
profiles/verify_set_batch_timing.txt.

    python tools/verify_set_batch_timing.py [--rows 4096:1 ... 262144:1024] [--sweep 65536:1024 4096:1024 65536:64] [--reps 5]

  * a row is n proofs over K keys.  The K key objects are made from the five golden circuits in rotation (key k is circuit
    k mod 5), proof i belongs to key i mod K and is a re-randomised copy of that circuit's golden proof
    (tools/verify_set_timing.py's input); every row runs all valid and with one INVALID proof per 4096 (positions 0, 4096,
    ...: B replaced by the golden proof's, well-formed, the equation fails); default chunk, group and key limit;
  * the entries run in ONE process, alternating: a round is one VerificationKeySet.verify_batch, one
    VerificationKeySet.verify and, for K = 1, one VerificationKey.verify_batch over the same proofs; one warm-up round and
    --reps timed ones; median, least and largest of time.perf_counter around the Python calls;
  * every verdict of every call is compared with the expected one;
  * --sweep rows run verify_batch alone, all valid, at ZKHIP_VERIFY_GROUP_KEYS = 1, 2, 4, 8, 16, 64.
Required: at n = 262144, K = 64, all valid, the new entry takes at most 0.65 of VerificationKeySet.verify's wall; the tool says
so in the file and fails when it does not hold.  The GPU work is a child process under `timeout`."""
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
REQUIRED = (262144, 64, 0.65)
SWEEP = [1, 2, 4, 8, 16, 64]
EVERY = 4096


def inputs(zk, pools, n, K):
    """-> (proofs [n, 256], key_of, publics) of a row, all valid; pools grows as needed"""
    per_key = [len(range(k, n, K)) for k in range(K)]
    need = [sum(per_key[k] for k in range(K) if k % 5 == c) for c in range(5)]
    for c in range(5):
        if need[c] > (pools[c][0].shape[0] if c in pools else 0):
            proofs, publics, _ = batch(zk, GOLDENS[c], need[c])
            pools[c] = (proofs.reshape(need[c], 256), publics[:len(publics) // need[c]])
    taken = [0] * 5
    mixed = np.empty((n, 256), dtype=np.uint8)
    for k in range(K):
        c = k % 5
        mixed[k::K] = pools[c][0][taken[c]:taken[c] + per_key[k]]
        taken[c] += per_key[k]
    key_of = np.arange(n, dtype=np.uint32) % K
    return mixed, key_of, b"".join(pools[int(k) % 5][1] for k in key_of)


def child(rows, sweep, reps, out_path):
    import rapidsnark_old_amd as zk
    from rapidsnark_old_amd import verify as V
    kmax = max(k for _, k in rows + sweep)
    zkeys = [os.path.join(ROOT, "tests", "golden", g, "circuit.zkey") for g in GOLDENS]
    gold_b = [np.frombuffer(V.load_proof(os.path.join(ROOT, "tests", "golden", g, "proof.json"))[64:192], dtype=np.uint8) for g in GOLDENS]
    t0 = time.perf_counter()
    keys = [zk.VerificationKey.from_zkey(zkeys[k % 5]) for k in range(kmax)]
    res = {"keys_made": kmax, "keys_seconds": time.perf_counter() - t0}
    pools = {}
    for name in ("ZKHIP_VERIFY_GROUP", "ZKHIP_VERIFY_GROUP_KEYS", "ZKHIP_VERIFY_CHUNK", "ZKHIP_VERIFY_COOP_MAX"):
        os.environ.pop(name, None)

    def save():
        with open(out_path, "w") as f:
            json.dump(res, f)

    for n, K in rows:
        valid, key_of, publics = inputs(zk, pools, n, K)
        for mix in ("valid", "invalid"):
            mixed = valid.copy()
            want = np.zeros(n, dtype=np.uint8)
            if mix == "invalid":
                for i in range(0, n, EVERY):
                    mixed[i, 64:192] = gold_b[(i % K) % 5]
                    want[i] = 1
            mixed = mixed.reshape(-1)
            t = {"batch": [], "set": [], "key_batch": []}
            with zk.VerificationKeySet(keys[:K]) as ks:
                for _ in range(reps + 1):
                    t0 = time.perf_counter()
                    v, rep = ks.verify_batch(mixed, key_of, publics)
                    t["batch"].append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    w = ks.verify(mixed, key_of, publics)
                    t["set"].append(time.perf_counter() - t0)
                    ok = np.array_equal(v, want) and np.array_equal(w, want)
                    if K == 1:
                        t0 = time.perf_counter()
                        u, krep = keys[0].verify_batch(mixed, publics)
                        t["key_batch"].append(time.perf_counter() - t0)
                        ok = ok and np.array_equal(u, want) and krep["groups"] == rep["groups"]
                    if not ok:
                        print("a verdict is not the expected one at n = %d, K = %d, %s" % (n, K, mix), file=sys.stderr)
                        return 1
            res["%d|%d|%s" % (n, K, mix)] = {"t": {k: x[1:] for k, x in t.items()}, "rep": rep}
            print("done: n = %d, K = %d, %s" % (n, K, mix), flush=True)
            save()
    for n, K in sweep:
        valid, key_of, publics = inputs(zk, pools, n, K)
        mixed = valid.reshape(-1)
        with zk.VerificationKeySet(keys[:K]) as ks:
            for m in SWEEP:                             # the first warm-up round makes the set's lines of beta
                os.environ["ZKHIP_VERIFY_GROUP_KEYS"] = str(m)
                ts = []
                for _ in range(reps + 1):
                    t0 = time.perf_counter()
                    v, rep = ks.verify_batch(mixed, key_of, publics)
                    ts.append(time.perf_counter() - t0)
                    if v.any() or v.size != n:
                        print("a verdict is not OK at n = %d, K = %d, key limit %d" % (n, K, m), file=sys.stderr)
                        return 1
                res["sweep|%d|%d|%d" % (n, K, m)] = {"t": ts[1:], "rep": rep}
                print("done: sweep n = %d, K = %d, key limit %d" % (n, K, m), flush=True)
                save()
        os.environ.pop("ZKHIP_VERIFY_GROUP_KEYS", None)
    for k in keys:
        k.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="*", default=["%d:%d" % (n, k) for n in (4096, 65536, 262144) for k in (1, 64, 1024)], metavar="N:K")
    ap.add_argument("--sweep", nargs="*", default=["65536:1024", "4096:1024", "65536:64"], metavar="N:K")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_set_batch_timing.txt"))
    ap.add_argument("--child", metavar="PATH", help=argparse.SUPPRESS)
    args = ap.parse_args()
    rows = [tuple(int(x) for x in r.split(":")) for r in args.rows]
    sweep = [tuple(int(x) for x in r.split(":")) for r in args.sweep]
    if args.child:
        return child(rows, sweep, args.reps, args.child)
    tmp = tempfile.mkdtemp(prefix="verify_set_batch_timing_")
    rj = os.path.join(tmp, "res.json")
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--rows"] + args.rows + ["--sweep"] + args.sweep + ["--child", rj]
    subprocess.run(limited(me, 1000), check=True, timeout=1100)
    res = json.load(open(rj))
    lines = ["# tools/verify_set_batch_timing.py: zk_vkey_set_verify_batch against zk_vkey_set_verify on the same input on one MI355X, one process,",
             "# the entries alternating; key k is golden circuit k mod 5, proof i (re-randomised) belongs to key i mod K; default chunk, group and key limit;",
             "# %d timed rounds after a warm-up.  ms: median, least, largest of time.perf_counter around the Python calls;" % args.reps,
             "# ratio: batch median / set median of the same rounds.  %d key objects were made in %.1f s." % (res["keys_made"], res["keys_seconds"]), ""]
    failed = False
    for n, K in rows:
        for mix, title in (("valid", "all valid"), ("invalid", "one INVALID per %d" % EVERY)):
            r = res["%d|%d|%s" % (n, K, mix)]
            rep = r["rep"]
            mb, blo, bhi = stat([1e3 * x for x in r["t"]["batch"]])
            ms, slo, shi = stat([1e3 * x for x in r["t"]["set"]])
            lines.append("n = %d, K = %d (%d proofs a key), %s" % (n, K, n // K, title))
            lines.append("  %-34s %10.3f %10.3f %10.3f   launches %d, groups %d, segments %d, failed %d, rechecked %d   (group %d, key limit %d)" % (
                "zk_vkey_set_verify_batch", mb, blo, bhi, rep["launches"], rep["groups"], rep["segments"], rep["groups_failed"], rep["proofs_rechecked"],
                rep["group"], rep["group_keys"]))
            lines.append("  %-34s %10.3f %10.3f %10.3f" % ("zk_vkey_set_verify", ms, slo, shi))
            if r["t"]["key_batch"]:
                mk, klo, khi = stat([1e3 * x for x in r["t"]["key_batch"]])
                lines.append("  %-34s %10.3f %10.3f %10.3f   set batch / key batch %.3f" % ("zk_vkey_verify_batch", mk, klo, khi, mb / mk))
            note = ""
            if (n, K) == REQUIRED[:2] and mix == "valid":
                ok = mb / ms <= REQUIRED[2]
                failed = failed or not ok
                note = "   required: at most %.2f: %s" % (REQUIRED[2], "met" if ok else "NOT MET")
            lines.append("  ratio %.3f%s" % (mb / ms, note))
            lines.append("")
    for n, K in sweep:
        lines.append("sweep of ZKHIP_VERIFY_GROUP_KEYS at n = %d, K = %d (%d proofs a key), all valid, zk_vkey_set_verify_batch alone" % (n, K, n // K))
        for m in SWEEP:
            r = res["sweep|%d|%d|%d" % (n, K, m)]
            md, lo, hi = stat([1e3 * x for x in r["t"]])
            lines.append("  key limit %-4d %10.3f %10.3f %10.3f   launches %d, groups %d, segments %d" % (
                m, md, lo, hi, r["rep"]["launches"], r["rep"]["groups"], r["rep"]["segments"]))
        lines.append("")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
