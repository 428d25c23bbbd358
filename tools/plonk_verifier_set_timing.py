#!/usr/bin/env python3
"""What the PLONK key-set verifier costs on one MI355X against the entries that existed before it, written to
profiles/plonk_verifier_set_timing.txt.

    python tools/plonk_verifier_set_timing.py [--reps 5]

One process measures every entry, so that they meet the same machine in the same minute: at log_n 11, m = 4096 and 65536 valid
proofs spread evenly over a set of 64 entries (key_of[i] = i mod 64),
  (a) PlonkVerifierSet.verify against the loop of 64 PlonkVerifier.verify calls on 64 objects (m / 64 proofs each) and against
      ONE PlonkVerifier.verify of m proofs under one key: that figure is the floor, the set adds only indexed loads;
  (b) PlonkVerifierSet.verify_batch against 64 PlonkVerifier.verify_batch calls and against one one-key verify_batch of m;
  (c) at 65536, the batch entries again with ONE invalid proof.
The yardsticks are the single-key entries, never the set's own numbers.  A warm-up of every entry, then --reps rounds in which
the entries alternate; wall time of time.perf_counter around the Python calls, which end in the library's stream synchronise;
medians.  ZKHIP_PLONK_VERIFY_CHUNK and ZKHIP_PLONK_VERIFY_GROUP are unset (65536 both).  Every timed call's verdicts are checked.
The GPU step is a child process under `timeout`.  The shader clock is read after the runs.

The proofs are real.  The 64 entries are tools/plonk_verifier_timing.py's circuit with 1 to 8 public rows, EIGHT distinct keys,
each standing at eight entries of the set (the set does not look for equal keys: it holds 64 records and 512 commitments, and
the loop holds 64 objects); every key has 4 distinct proofs, repeated to fill m.  An invalid proof is a valid one with one byte
of its fourth value changed."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from plonk_opening_timing import make_kzg  # noqa: E402
from plonk_verifier_timing import LOG_N, le, make_key  # noqa: E402
from verify_timing import limited, stat  # noqa: E402

MS = (4096, 65536)
ENTRIES, DISTINCT_KEYS, PROOFS_A_KEY = 64, 8, 4
ENTRY_NAMES = ("set", "loop of 64", "one key")


def timed(call, check):
    t0 = time.perf_counter()
    out = call()
    dt = time.perf_counter() - t0
    check(out)
    return dt


def child(reps, out_path):
    import rapidsnark_old_amd as zk
    made = []                                            # per distinct key: (vk, proofs (4, 768), publics bytes of one proof)
    with make_kzg(zk, LOG_N) as kzg:
        for j in range(DISTINCT_KEYS):
            p, publics, witness = make_key(zk, kzg, 1 + j)
            with p:
                vk = zk.PlonkVKey.from_json(p.vkey().to_json())
                proofs = np.frombuffer(b"".join(p.prove(witness, publics).to_bytes() for _ in range(PROOFS_A_KEY)), dtype=np.uint8).reshape(PROOFS_A_KEY, 768)
            made.append((vk, proofs, le(publics)))
    keys = [made[e % DISTINCT_KEYS] for e in range(ENTRIES)]
    res = {"rows": []}
    singles = [zk.PlonkVerifier(vk) for vk, _, _ in keys]
    try:
        with zk.PlonkVerifierSet([vk for vk, _, _ in keys]) as s:
            for m in MS:
                per = m // ENTRIES
                key_of = np.arange(m, dtype=np.uint32) % ENTRIES
                a = np.empty((m, 768), dtype=np.uint8)
                for e, (_, proofs, _) in enumerate(keys):
                    a[e::ENTRIES] = np.tile(proofs, (per // PROOFS_A_KEY + 1, 1))[:per]
                ragged = np.concatenate([keys[e][2] for e in range(ENTRIES)] * per)
                by_key = [(np.ascontiguousarray(a[e::ENTRIES]), np.tile(keys[e][2], per)) for e in range(ENTRIES)]
                one_a = np.ascontiguousarray(np.tile(keys[0][1], (m // PROOFS_A_KEY, 1)))
                one_pb = np.tile(keys[0][2], m)
                for label, bad in (("all valid", None),) + ((("one invalid", m // 2),) if m == MS[-1] else ()):
                    aa, groups, oa = a, by_key, one_a
                    if bad is not None:                  # position bad of the set's call = proof bad // 64 of entry bad % 64
                        aa, oa = a.copy(), one_a.copy()
                        aa[bad, 576 + 3 * 32 + 5] ^= 0x10
                        oa[bad, 576 + 3 * 32 + 5] ^= 0x10
                        groups = list(by_key)
                        spoiled = by_key[bad % ENTRIES][0].copy()
                        spoiled[bad // ENTRIES, 576 + 3 * 32 + 5] ^= 0x10
                        groups[bad % ENTRIES] = (spoiled, by_key[bad % ENTRIES][1])

                    def right(got, count=m, at=bad):
                        got = got[0] if isinstance(got, tuple) else got
                        assert got.shape == (count,) and list(np.nonzero(got)[0]) == ([] if at is None else [at]), "wrong verdicts"

                    def loop_right(outs, at=bad):
                        for e, got in enumerate(outs):
                            got = got[0] if isinstance(got, tuple) else got
                            want = [at // ENTRIES] if at is not None and e == at % ENTRIES else []
                            assert got.shape == (per,) and list(np.nonzero(got)[0]) == want, "wrong verdicts"

                    calls = {}
                    if bad is None:
                        calls["verify"] = (lambda: s.verify(aa, key_of, ragged), lambda: [v.verify(x, pb) for v, (x, pb) in zip(singles, groups)],
                                           lambda: singles[0].verify(oa, one_pb))
                    calls["verify_batch"] = (lambda: s.verify_batch(aa, key_of, ragged), lambda: [v.verify_batch(x, pb) for v, (x, pb) in zip(singles, groups)],
                                             lambda: singles[0].verify_batch(oa, one_pb))
                    checks = (right, loop_right, right)
                    walls = {(what, q): [] for what in calls for q in range(3)}
                    for rnd in range(1 + reps):          # round 0: the warm-up
                        for what, three in calls.items():
                            for q, call in enumerate(three):
                                dt = timed(call, checks[q])
                                if rnd:
                                    walls[what, q].append(dt)
                    rep = s.verify_batch(aa, key_of, ragged)[1]
                    res["rows"].append({"m": m, "case": label, "report": rep, "walls": {what: [walls[what, q] for q in range(3)] for what in calls}})
            res["set_bytes"] = s.info()["device_bytes"]
            res["single_bytes"] = sum(v.info()["device_bytes"] for v in singles)
    finally:
        for v in singles:
            v.close()
    with open(out_path, "w") as fh:
        json.dump(res, fh)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_verifier_set_timing.txt"))
    ap.add_argument("--child", metavar="PATH", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.reps, args.child)
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--child"]
    with tempfile.TemporaryDirectory(prefix="plonk_verifier_set_timing_") as tmp:
        wj = os.path.join(tmp, "walls.json")
        subprocess.run(limited(me + [wj], 500), check=True, timeout=560)
        res = json.load(open(wj))
    try:
        clock = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
    except (OSError, subprocess.SubprocessError):
        clock = ""
    clock = [ln.strip() for ln in clock.splitlines() if "sclk" in ln][:1]
    lines = ["# tools/plonk_verifier_set_timing.py: PlonkVerifierSet against the single-key PlonkVerifier, one MI355X, log_n %d, a set of %d entries"
             % (LOG_N, ENTRIES),
             "# (%d distinct keys with 1 to %d public inputs, each at %d entries), the proofs spread evenly, key_of[i] = i mod %d; chunk and group 65536;"
             % (DISTINCT_KEYS, DISTINCT_KEYS, ENTRIES // DISTINCT_KEYS, ENTRIES),
             "# a warm-up, then %d rounds in which the entries alternate; wall ms of the Python call(s): median (least .. largest)" % args.reps,
             "# loop of 64: 64 calls on 64 PlonkVerifier objects, m / 64 proofs each; one key: one call of m proofs under ONE key, the floor",
             "# shader clock after the runs: " + (clock[0] if clock else "not read"), ""]
    for r in res["rows"]:
        lines.append("m = %d, %s" % (r["m"], r["case"]))
        for what, three in r["walls"].items():
            st = [stat([1e3 * x for x in w]) for w in three]
            for name, t in zip(ENTRY_NAMES, st):
                lines.append("  %-12s %-10s %9.3f (%.3f .. %.3f)" % ((what, name) + t))
            lines.append("  %-12s set / loop %.2f, set / one key %.2f" % (what, st[0][0] / st[1][0], st[0][0] / st[2][0]))
        rep = r["report"]
        lines.append("  set.verify_batch's report: group %d, groups %d, failed %d, segments %d, rechecked %d, launches %d"
                     % (rep["group"], rep["groups"], rep["groups_failed"], rep["segments"], rep["proofs_rechecked"], rep["launches"]))
        lines.append("")
    lines.append("HBM held after the runs: the set %.1f MiB, the 64 objects together %.1f MiB" % (res["set_bytes"] / 2 ** 20, res["single_bytes"] / 2 ** 20))
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
