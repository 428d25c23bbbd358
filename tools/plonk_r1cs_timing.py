#!/usr/bin/env python3
"""What the compile of a circom .r1cs to PLONK and the extension of a witness cost on one MI355X, written to
profiles/plonk_r1cs_timing.txt.

    python tools/plonk_r1cs_timing.py [--reps 5] [--sizes 18 20 22] [--long-rows 64x1000 8x20000]

At every k of --sizes two circuit-shaped keys are made by zkgen (circuit_like, 2^k the Groth16 domain: about 3/4 of it are
constraints), one plain and one with --long-rows, and written as .r1cs (zkgen.write_r1cs's construction; see make_files).  For each, in one process, a warm-up
and --reps timed calls, medians with least and largest:
  * compile: PlonkR1cs(bytes) (zk_plonk_r1cs_create: upload, flags, scans, emit, sort, sigma) and the wall per term;
  * fetch: zk_plonk_r1cs_circuit alone, the device-to-host half of the round trip of zk_plonk_prover_create_r1cs, and that
    entry whole (the fetch, then zk_plonk_prover_create: upload, extensions, eight commitments);
  * extension: PlonkProver.prove_r1cs against PlonkProver.prove on the already extended witness, same object, alternating; the
    difference is the extension (its three kernels, a drain of the stream, and nWires instead of n_witness rows uploaded).
Kernel times come from a process of its own under `rocprofv3 --kernel-trace` (no counters in that run) that compiles and
extends as often, summed by kernel name into the steps: flags, scans (k_u32_scan_*: the two of the gates AND one per digit pass
of the sort), emit, sort (k_cell_*), sigma, extension (k_ext_*).  Every GPU step is a child process under `timeout`.
The reference string is n + 6 powers of a known tau made by the tool, not a file."""
import argparse
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
from verify_timing import kernel_durations, limited, stat  # noqa: E402

BLIND = list(range(101, 112))
STEPS = (("flags", ("k_r1cs_flags",)), ("scans", ("k_u32_scan_",)), ("emit", ("k_r1cs_additions", "k_r1cs_public", "k_r1cs_emit_")),
         ("sort", ("k_cell_",)), ("sigma", ("k_sigma_",)), ("extension", ("k_ext_",)))


def long_rows_arg(text):
    c, t = text.lower().split("x")
    return int(c), int(t)


def make_files(zk, k, long_rows):
    """(the .r1cs bytes, the witness values) of a zkgen key.  zkgen draws a row's wires with repetition, so a linear combination can
    name wire 0 twice, which the compile refuses: every such term after the first of its row is re-pointed to one more private wire
    whose value is 1.  Otherwise zkgen.write_r1cs's construction."""
    from rapidsnark_old_amd import r1cs, synth, zkgen
    key = zkgen.generate(k, 2, seed=k, circuit_like=True, long_rows=long_rows)
    m, n_in, n_vars = key["nConstraints"], key["nInputs"], key["nVars"]
    rec = np.frombuffer(np.ascontiguousarray(key["coefs"]).tobytes()[4:], dtype=synth.COEF_DTYPE)
    rec = rec[rec["c"] < m]
    one = zkgen._const(1, rec.size)
    std = zkgen._mul(zkgen._mul(np.ascontiguousarray(rec["v"]).reshape(-1), one), one).reshape(-1, 32)
    mats = []
    for mat in (0, 1):
        sel = np.nonzero(rec["m"] == mat)[0]
        sel = sel[np.argsort(rec["c"][sel], kind="stable")]
        rowptr = np.zeros(m + 1, dtype=np.int64)
        np.cumsum(np.bincount(rec["c"][sel], minlength=m), out=rowptr[1:])
        wires, rows = rec["s"][sel].astype(np.uint32), rec["c"][sel]
        zero = np.nonzero(wires == 0)[0]
        again = zero[1:][rows[zero[1:]] == rows[zero[:-1]]]
        wires[again] = n_vars
        mats.append((rowptr, wires, std[sel]))
    c_coef = np.zeros((m, 32), dtype=np.uint8)
    c_coef[:, 0] = 1
    mats.append((np.arange(m + 1, dtype=np.int64), (1 + n_in + np.arange(m)).astype(np.uint32), c_coef))
    data = r1cs.write_r1cs(mats[0], mats[1], mats[2], n_vars + 1, 0, key["nPublic"], n_in - key["nPublic"])
    wtns = np.concatenate([np.ascontiguousarray(key["witness"]).view(np.uint8).reshape(-1), np.frombuffer((1).to_bytes(32, "little"), dtype=np.uint8)])
    return data, wtns


def child(what, k, long_rows, reps, out_path):
    import rapidsnark_old_amd as zk
    data, wtns = make_files(zk, k, long_rows)
    res = {}
    if what == "traced":
        for _ in range(reps + 1):
            with zk.PlonkR1cs(data) as c:
                c.extend(wtns)
        json.dump(res, open(out_path, "w"))
        return 0
    tc = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        c = zk.PlonkR1cs(data)
        tc.append(time.perf_counter() - t0)
        info = c.info()
        c.close()
    res["compile"], res["info"] = tc[1:], info
    with zk.PlonkR1cs(data) as c, make_kzg(zk, c.log_n) as kz:
        tf, tp = [], []
        for _ in range(reps + 1):
            c._circuit = None
            t0 = time.perf_counter()
            c._fetch()
            tf.append(time.perf_counter() - t0)
        for _ in range(2):
            t0 = time.perf_counter()
            p = zk.PlonkProver.from_r1cs(kz, c)
            tp.append(time.perf_counter() - t0)
            if _ == 0:
                p.close()
        res["fetch"], res["create_r1cs"] = tf[1:], tp[1:]
        ext = c.extend(wtns)
        ta, tb = [], []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            one = p.prove_r1cs(wtns, blind=BLIND)
            ta.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            two = p.prove(ext, blind=BLIND)
            tb.append(time.perf_counter() - t0)
            assert one == two
        assert zk.plonk_verify(p.vkey(), one, wtns[32:32 * (1 + c.n_public)]) == 0
        res["prove_r1cs"], res["prove"], res["prover"] = ta[1:], tb[1:], p.info()
        p.close()
    json.dump(res, open(out_path, "w"))
    return 0


def by_step(prof_dir, calls):
    """{step: ms per compile-and-extend} from the trace"""
    out = {s: 0.0 for s, _ in STEPS}
    for name, ds in kernel_durations(prof_dir).items():
        found = re.search(r"k_\w+", name)
        short = found.group(0) if found else name
        for step, prefixes in STEPS:
            if any(short.startswith(p) for p in prefixes):
                out[step] += sum(ds) / calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[18, 20, 22])
    ap.add_argument("--long-rows", type=long_rows_arg, nargs="+", default=[(64, 1000), (8, 20000)], metavar="COUNTxTERMS")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_r1cs_timing.txt"))
    ap.add_argument("--child", nargs=4, metavar=("WHAT", "K", "LONG", "PATH"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]), json.loads(args.child[2]), args.reps, args.child[3])
    if not shutil.which("rocprofv3"):
        raise SystemExit("rocprofv3 not found: kernel times come from nowhere else")
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--child"]
    lines = ["# tools/plonk_r1cs_timing.py: a circom .r1cs compiled to PLONK on one MI355X; %d timed calls after a warm-up; ms: median, least, largest" % args.reps,
             "# keys: zkgen circuit_like at 2^k, plain and with long rows %s" % " ".join("%dx%d" % lr for lr in args.long_rows), ""]

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    for k in args.sizes:
        per_term = {}
        for label, lr in (("plain", []), ("long rows", [list(x) for x in args.long_rows])):
            tmp = tempfile.mkdtemp(prefix="plonk_r1cs_timing_")
            try:
                wj = os.path.join(tmp, "walls.json")
                subprocess.run(limited(me + ["walls", str(k), json.dumps(lr), wj], 500), check=True, timeout=560)
                wall = json.load(open(wj))
                prof = os.path.join(tmp, "traced")
                cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", prof, "-o", "plonkr1cs", "--"] + me + ["traced", str(k), json.dumps(lr), os.path.join(tmp, "t.json")]
                subprocess.run(limited(cmd, 500), check=True, stdout=subprocess.DEVNULL, timeout=560)
                steps = by_step(prof, args.reps + 1)
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
            ms = lambda key: stat([1e3 * x for x in wall[key]])     # noqa: E731
            info = wall["info"]
            comp, ext = ms("compile"), stat([1e3 * (a - b) for a, b in zip(wall["prove_r1cs"], wall["prove"])])
            per_term[label] = (1e6 * comp[0] / info["terms"], 1e6 * steps["extension"] / max(info["n_additions"], 1), steps)
            lines += ["k %d, %s: %s" % (k, label, json.dumps(info, sort_keys=True)),
                      "    compile wall          %10.3f %10.3f %10.3f   (%.1f ns a term)" % (comp + (per_term[label][0],)),
                      "    compile kernels, ms a compile: " + ", ".join("%s %.3f" % (s, steps[s]) for s, _ in STEPS[:5]) +
                      "; together %.3f" % sum(steps[s] for s, _ in STEPS[:5]),
                      "    fetch (8n rows, maps) %10.3f %10.3f %10.3f" % ms("fetch"),
                      "    create_r1cs whole     %10.3f   (one call)" % (1e3 * wall["create_r1cs"][0]),
                      "    prove_r1cs            %10.3f %10.3f %10.3f" % ms("prove_r1cs"),
                      "    prove (extended)      %10.3f %10.3f %10.3f" % ms("prove"),
                      "    extension = prove_r1cs - prove, pairwise %10.3f %10.3f %10.3f; its kernels %.3f ms (%.2f ns an addition gate)"
                      % (ext + (steps["extension"], per_term[label][1])), ""]
            flush()
        a, b = per_term["plain"], per_term["long rows"]
        lines += ["k %d, long rows against plain: compile wall per term %.2f x; extension kernels per addition gate %.2f x; flags + emit kernels per term follow the compile lines above" %
                  (k, b[0] / a[0], b[1] / a[1]), ""]
        flush()
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
