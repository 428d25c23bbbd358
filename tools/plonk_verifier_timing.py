#!/usr/bin/env python3
"""What verifying PLONK proofs costs on one MI355X, written to profiles/plonk_verifier_timing.txt.

    python tools/plonk_verifier_timing.py [--reps 5]

One process measures all sides, so that they meet the same machine in the same minute: at log_n 11 with 2 public inputs,
m = 1, 64, 4096 and 65536 proofs, and 65536 proofs with 1024 public inputs.
  * object: PlonkVerifier.verify, everything per proof on the device (a warm-up, then --reps timed calls; wall time of
    time.perf_counter around the Python call, which ends in the library's stream synchronise).
  * loop: zk.plonk_verify once a proof, the host's transcript and 18 host multiplications a proof (m <= 4096; one pass at 4096).
  * staged: the route through entries that existed before the object: the transcript and the scalars on the host (here
    Python integers over zk.keccak256: timed at m <= 64 and reported per proof, since at 65536 it would time Python and nothing
    else), zk.g1_mul_vec over the 19 m products, the sums on the host (Python, as the transcript), Kzg.verify with z = y = 0.  The
    two device stages are timed at every m.
Kernel times of the object's route come from a process of its own under `rocprofv3 --kernel-trace` (no counters in that
run), summed over the chunks of a call, by stage: transcript (k_plonk_transcript), combination (k_plonk_combine, k_plonk_sum),
pairing (k_kzg_pair).  Every GPU step is a child process under `timeout`.  The shader clock is read after the runs.

The proofs are real: the circuit of tools/plonk_prover_timing.py with its first rows made public rows (q_L = 1, a = the public
input), proved by PlonkProver with drawn blinds; 8 distinct proofs are repeated to m (nothing in the verifier remembers a
proof).  Every timed batch is checked to verify."""
import argparse
import csv
import glob
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
from plonk_prover_timing import K1, K2, R, circuit, le  # noqa: E402
from verify_timing import limited, stat  # noqa: E402

LOG_N = 11
CONFIGS = ((1, 2), (64, 2), (4096, 2), (65536, 2), (65536, 1024))        # (m, n_public)
DISTINCT = 8
STAGES = (("transcript", ("k_plonk_transcript",)), ("combination", ("k_plonk_combine", "k_plonk_sum")), ("pairing", ("k_kzg_pair",)))
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583


def ints(a):
    raw = bytes(a)
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def make_key(zk, kzg, n_public):
    """(prover, publics as ints, witness): the tool's circuit by values, rows 0 .. n_public - 1 public"""
    n = 1 << LOG_N
    circ, maps, witness = circuit(LOG_N)
    vals = [np.frombuffer(zk.fr_ntt(v), dtype=np.uint8).copy() for v in circ]
    one = le([1])
    for i in range(n_public):
        vals[0][i * 32:(i + 1) * 32] = one               # q_L = 1
        vals[1][i * 32:(i + 1) * 32] = 0                 # q_R = 0
    w = witness.reshape(-1, 32)
    publics = ints(np.ascontiguousarray(w[maps[0][:n_public]]).reshape(-1))
    return zk.PlonkProver(kzg, *vals, K1, K2, *maps, n, n_public, basis="lagrange"), publics, witness


def make_batch(zk, kzg, n_public):
    p, publics, witness = make_key(zk, kzg, n_public)
    with p:
        vk = p.vkey()
        proofs = [p.prove(witness, publics).to_bytes() for _ in range(DISTINCT)]
    return vk, proofs, publics


def tiled(proofs, publics, m):
    a = np.frombuffer(b"".join(proofs), dtype=np.uint8).reshape(len(proofs), 768)
    a = np.ascontiguousarray(np.tile(a, ((m + len(proofs) - 1) // len(proofs), 1))[:m])
    pb = np.ascontiguousarray(np.tile(le(publics), m))
    return a, pb


# ---------------------------------------------------------------- the staged route's host side, Python integers
def host_scalars(zk, vk, proof, publics):
    """the six challenges and the 19 scalars of the combination (include/zkhip.h), as a host without the object makes them"""
    from rapidsnark_old_amd import plonk as P
    pts = [P._affine(proof[i * 64:(i + 1) * 64]) for i in range(9)]
    ev = ints(proof[576:])
    enc = lambda x: bytes(64) if x is None else (x[0].to_bytes(32, "big") + x[1].to_bytes(32, "big") if isinstance(x, tuple) else x.to_bytes(32, "big"))   # noqa: E731
    H = lambda *items: int.from_bytes(zk.keccak256(b"".join(enc(x) for x in items)), "big") % R                                                           # noqa: E731
    key = [P._affine(b) for b in vk.commitments.values()]
    beta = H(*key, *publics, *pts[0:3])
    gamma = H(beta)
    alpha = H(beta, gamma, pts[3])
    ze = H(alpha, *pts[4:7])
    v = H(ze, *ev)
    u = H(pts[7], pts[8])
    n, w = 1 << vk.log_n, P.root_of_unity(vk.log_n)
    a, b, c, s1, s2, zw = ev
    zn = pow(ze, n, R)
    zh = (zn - 1) % R
    l1 = zh * pow(n * (ze - 1), -1, R) % R
    pi, wi = 0, 1
    for p in publics:
        pi = (pi - p * wi * zh % R * pow(n * (ze - wi), -1, R)) % R
        wi = wi * w % R
    g12 = (a + beta * s1 + gamma) * (b + beta * s2 + gamma) % R * zw % R * alpha % R
    kz = (alpha * (a + beta * ze + gamma) % R * (b + beta * K1 * ze + gamma) % R * (c + beta * K2 * ze + gamma) + alpha * alpha * l1 + u) % R
    E = sum(pow(v, j + 1, R) * ev[j] for j in range(5)) % R
    c0 = (pi - g12 * (c + gamma) - alpha * alpha * l1) % R
    return [a * b % R, a, b, c, 1, pow(v, 4, R), pow(v, 5, R), -g12 * beta % R, -(E - c0 + u * zw) % R, v, v * v % R, pow(v, 3, R), kz, -zh % R,
            -zh * zn % R, -zh * zn * zn % R, ze, u * ze * w % R, u]


def host_sums(products):
    """L = the sum of 18 points, W = W_zeta + the 19th, affine, Python integers (as oracle code would)"""
    from oracle import bn254 as bn
    pts = [bn.g1_from_bytes(bytes(products[i * 64:(i + 1) * 64])) for i in range(20)]
    L = None
    for P in pts[:18]:
        L = bn.G1.add(L, P)
    return bn.g1_to_bytes(L), bn.g1_to_bytes(bn.G1.add(pts[18], pts[19]))


def staged_inputs(zk, vk, proof, publics):
    """(19 + 1 bases, 19 scalars + 1) of one proof for zk.g1_mul_vec: W_zeta rides along by 1"""
    from rapidsnark_old_amd import synth
    key = list(vk.commitments.values())
    pp = [proof[i * 64:(i + 1) * 64] for i in range(9)]
    bases = key + [bytes(synth.g1_gen_bytes())] + pp + [pp[8], pp[7]]
    return b"".join(bases), host_scalars(zk, vk, proof, publics) + [1]


def child(what, reps, out_path):
    import rapidsnark_old_amd as zk
    res = {"configs": []}
    with make_kzg(zk, LOG_N) as kzg:
        for n_public in sorted({l for _, l in CONFIGS}):
            vk, proofs, publics = make_batch(zk, kzg, n_public)
            with zk.PlonkVerifier(vk) as v:
                for m, l in CONFIGS:
                    if l != n_public:
                        continue
                    a, pb = tiled(proofs, publics, m)
                    got = v.verify(a, pb)                # the warm-up, and the check
                    assert got.shape == (m,) and not got.any(), "the batch does not verify"
                    walls = []
                    for _ in range(reps):
                        t0 = time.perf_counter()
                        v.verify(a, pb)
                        walls.append(time.perf_counter() - t0)
                    row = {"m": m, "n_public": l, "object": walls, "info": v.info()}
                    if what == "walls":
                        if m <= 4096:
                            passes = 1 if m == 4096 else min(reps, 3)
                            loop = []
                            for _ in range(passes):
                                t0 = time.perf_counter()
                                for i in range(m):
                                    assert zk.plonk_verify(vk, proofs[i % DISTINCT], publics) == 0
                                loop.append(time.perf_counter() - t0)
                            row["loop"] = loop
                        # staged: the host's share at min(m, 64) proofs, the device's at m
                        k = min(m, 64)
                        t0 = time.perf_counter()
                        parts = [staged_inputs(zk, vk, proofs[i % DISTINCT], publics) for i in range(k)]
                        row["host_transcript_per_proof"] = (time.perf_counter() - t0) / k
                        bases = np.frombuffer(b"".join(p[0] for p in parts[:DISTINCT]), dtype=np.uint8).reshape(-1, 20 * 64)
                        sc = np.concatenate([le(p[1]) for p in parts[:DISTINCT]]).reshape(-1, 20 * 32)
                        reps_of = (m + len(bases) - 1) // len(bases)
                        B = np.ascontiguousarray(np.tile(bases, (reps_of, 1))[:m]).reshape(-1)
                        S = np.ascontiguousarray(np.tile(sc, (reps_of, 1))[:m]).reshape(-1)
                        mul, pair = [], []
                        for r in range(min(reps, 3) + 1):
                            t0 = time.perf_counter()
                            prod = zk.g1_mul_vec(B, S)
                            mul.append(time.perf_counter() - t0)
                            if r == 0:
                                t0 = time.perf_counter()
                                sums = [host_sums(prod[i * 20 * 64:(i + 1) * 20 * 64]) for i in range(min(k, DISTINCT))]
                                row["host_sums_per_proof"] = (time.perf_counter() - t0) / len(sums)
                                Ls = np.frombuffer(b"".join(sums[i % len(sums)][0] for i in range(m)), dtype=np.uint8)
                                Ws = np.frombuffer(b"".join(sums[i % len(sums)][1] for i in range(m)), dtype=np.uint8)
                                zeros = np.zeros(m * 32, dtype=np.uint8)
                            t0 = time.perf_counter()
                            verdicts = kzg.verify(Ls, zeros, zeros, Ws)
                            pair.append(time.perf_counter() - t0)
                            assert not np.asarray(verdicts).any(), "the staged route does not verify"
                        row["mul_vec"], row["kzg_verify"] = mul[1:], pair[1:]
                    res["configs"].append(row)
    with open(out_path, "w") as fh:
        json.dump(res, fh)
    return 0


def stage_times(prof_dir, reps, chunks):
    """[{stage: median ms a call}] a config, from the trace: a config is (1 + reps) calls of chunks[i] dispatches a kernel"""
    files = glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    by = {}
    for r in rows:
        for _, names in STAGES:
            for name in names:
                if name in r["Kernel_Name"]:
                    by.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    out, at = [], 0
    for ch in chunks:
        cfg = {}
        for stage, names in STAGES:
            per_call = [0.0] * reps
            for name in names:
                d = by.get(name, [])
                if len(d) < at + (1 + reps) * ch:
                    return None
                for c in range(reps):
                    lo = at + (1 + c) * ch
                    per_call[c] += sum(d[lo:lo + ch])
            cfg[stage] = stat(per_call)[0]
        out.append(cfg)
        at += (1 + reps) * ch
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_verifier_timing.txt"))
    ap.add_argument("--child", nargs=2, metavar=("WHAT", "PATH"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.reps, args.child[1])
    if not shutil.which("rocprofv3"):
        raise SystemExit("rocprofv3 not found: kernel times come from nowhere else")
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--child"]
    tmp = tempfile.mkdtemp(prefix="plonk_verifier_timing_")
    try:
        wj = os.path.join(tmp, "walls.json")
        subprocess.run(limited(me + ["walls", wj], 700), check=True, timeout=760)
        wall = json.load(open(wj))["configs"]
        prof = os.path.join(tmp, "traced")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", prof, "-o", "plonkverify", "--"] + me + ["traced", os.path.join(tmp, "t.json")]
        subprocess.run(limited(cmd, 300), check=True, stdout=subprocess.DEVNULL, timeout=360)
        stages = stage_times(prof, args.reps, [row["info"]["last_chunks"] for row in wall])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    try:
        clock = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
    except (OSError, subprocess.SubprocessError):
        clock = ""
    clock = [ln.strip() for ln in clock.splitlines() if "sclk" in ln][:1]
    lines = ["# tools/plonk_verifier_timing.py: verifying PLONK proofs on one MI355X, log_n %d; %d timed calls after a warm-up, medians" % (LOG_N, args.reps),
             "# shader clock after the runs: " + (clock[0] if clock else "not read"),
             "# object: PlonkVerifier.verify; loop: zk.plonk_verify a proof; staged: host transcript (Python integers, timed at min(m, 64) proofs),",
             "# zk.g1_mul_vec over 20 m products (W_zeta rides along), host sums (Python integers), Kzg.verify with z = y = 0", ""]
    for i, row in enumerate(wall):
        m = row["m"]
        ob = stat([1e3 * x for x in row["object"]])
        lines.append("m = %d, n_public = %d: %s" % (m, row["n_public"], json.dumps(row["info"], sort_keys=True)))
        lines.append("  object wall, ms: median %.3f, least %.3f, largest %.3f; %.3f us a proof" % (ob + (1e3 * ob[0] / m,)))
        if stages:
            s = stages[i]
            ksum = sum(s.values())
            lines.append("  object kernels (rocprofv3 --kernel-trace, a process of its own), ms a call: " + ", ".join("%s %.3f" % (k, s[k]) for k, _ in STAGES) +
                         "; together %.3f = %.3f us a proof; kernels / wall %.2f" % (ksum, 1e3 * ksum / m, ksum / ob[0]))
        else:
            lines.append("  object kernels: the trace does not hold the expected dispatches: not tabulated")
        if "loop" in row:
            lp = stat([1e3 * x for x in row["loop"]])
            lines.append("  loop of zk.plonk_verify wall, ms: median %.3f (%d passes); %.1f us a proof; loop / object %.1f" % (lp[0], len(row["loop"]), 1e3 * lp[0] / m, lp[0] / ob[0]))
        mv, kv = stat([1e3 * x for x in row["mul_vec"]]), stat([1e3 * x for x in row["kzg_verify"]])
        host = 1e3 * (row["host_transcript_per_proof"] + row["host_sums_per_proof"]) * m
        lines.append("  staged, ms: g1_mul_vec %.3f, Kzg.verify %.3f, the two %.3f (%.3f us a proof; / object %.2f); host transcript %.1f us a proof, host sums %.1f us a proof"
                     % (mv[0], kv[0], mv[0] + kv[0], 1e3 * (mv[0] + kv[0]) / m, (mv[0] + kv[0]) / ob[0], 1e6 * row["host_transcript_per_proof"], 1e6 * row["host_sums_per_proof"]))
        lines.append("    with the host's share as timed in Python the staged route is %.1f ms at this m (/ object %.1f)" % (mv[0] + kv[0] + host, (mv[0] + kv[0] + host) / ob[0]))
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
