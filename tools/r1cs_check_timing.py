#!/usr/bin/env python3
"""Time of the R1CS witness check on the GPU (zk_r1cs_check_dev: witness already in HBM, the call ends with the checker's
stream synchronise), bytes it moves and their share of HBM peak; the cost of `prover`'s ZKHIP_R1CS guard.

    python tools/r1cs_check_timing.py [--sizes 20 22] [--reps 30] [--cli] [--out DIR]

  * zkgen circuit_like circuits at each size (valid .zkey / .wtns / .r1cs triples, zkgen.write_r1cs);
  * at the largest size's nnz, two synthetic circuits of the same shape: every row of even length ("uniform") and one
    10^5-term row plus a power-law tail ("skewed") — the segmented sum should make them cost about the same;
  * --cli: median wall of `prover` on the largest triple with and without ZKHIP_R1CS (three runs each, alternating).
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool (--reps small)."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12          # MI355X HBM3E, bytes/s (spec)
SEG = 16                   # csrc/r1cs.hip


def traffic(row_lens, n_wires):
    """bytes one check moves: per term 4 (wire id) + 32 (coefficient) + 32 (witness gather); per segment of the first pass
    16 (bounds + destination); per row a 32-byte write and the check's 32-byte read; the witness scan."""
    lens = np.asarray(row_lens, dtype=np.int64)
    nseg = np.maximum(1, (lens + SEG - 1) // SEG).sum()
    return int(lens.sum() * 68 + nseg * 16 + lens.size * 64 + n_wires * 32)


def time_check(zk, ck, wtns_vals, reps):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(wtns_vals).reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    n = d.numel() // 32
    for _ in range(3):
        ck.check_dev(d.data_ptr(), n)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        rep = ck.check_dev(d.data_ptr(), n)
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3, rep


def synthetic(m, n_wires, nnz, skewed, rng):
    """(rowptr, wires, coefs) x 3 with nnz terms spread over the 3m rows: evenly, or one 10^5-term row + a power-law tail"""
    rows = 3 * m
    if skewed:
        w = 1.0 / np.arange(1, rows) ** 1.1                  # power law, capped at 4096 terms; the excess spread evenly
        tail = np.floor(w / w.sum() * (nnz - 100000)).astype(np.int64)
        excess = int(np.clip(tail - 4096, 0, None).sum())
        tail = np.minimum(tail, 4096) + excess // (rows - 1)
        tail[: (nnz - 100000 - tail.sum())] += 1
        lens = np.concatenate([[100000], tail])
    else:
        lens = np.full(rows, nnz // rows, dtype=np.int64)
        lens[: nnz - lens.sum()] += 1
    if skewed:
        rng.shuffle(lens[1:])
    out = []
    for k in range(3):
        ln = lens[k * m:(k + 1) * m]
        rp = np.zeros(m + 1, dtype=np.int64)
        np.cumsum(ln, out=rp[1:])
        t = int(rp[-1])
        coefs = np.zeros((t, 32), np.uint8)
        coefs[:, :4] = rng.integers(1, 1 << 32, size=(t, 1), dtype=np.uint64).astype("<u4").view(np.uint8).reshape(t, 4)
        out.append((rp, rng.integers(0, n_wires, size=t, dtype=np.uint32), coefs))
    return out, lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import rapidsnark_old_amd as zk
    from rapidsnark_old_amd import zkgen, synth, r1cs
    d = args.out or tempfile.mkdtemp(prefix="r1cs_timing_")
    rng = np.random.default_rng(1)
    last = None
    for k in args.sizes:
        t0 = time.time()
        key = zkgen.generate(k, 2, 0, circuit_like=True)
        sub = os.path.join(d, "k%d" % k)
        zkgen.write_all(key, sub)
        zkgen.write_r1cs(key, os.path.join(sub, "circuit.r1cs"))
        ck = zk.R1cs(os.path.join(sub, "circuit.r1cs"), device=0)
        assert ck.match_zkey(os.path.join(sub, "circuit.zkey")) == (0, None)
        h, sec = r1cs.open_r1cs(os.path.join(sub, "circuit.r1cs"))
        rec = np.frombuffer(np.ascontiguousarray(key["coefs"]).tobytes()[4:], dtype=synth.COEF_DTYPE)
        m = key["nConstraints"]
        rec = rec[rec["c"] < m]
        lens = np.concatenate([np.bincount(rec["c"][rec["m"] == 0], minlength=m), np.bincount(rec["c"][rec["m"] == 1], minlength=m), np.ones(m, np.int64)])
        ms, rep = time_check(zk, ck, key["witness"], args.reps)
        assert rep.ok, rep
        b = traffic(lens, key["nVars"])
        print("circuit_like 2^%d: m %d, nnz %d, check_dev median %.3f ms, %.1f MB moved, %.2f TB/s = %.1f %% of HBM peak (setup %.0f s)"
              % (k, m, int(lens.sum()), ms, b / 1e6, b / ms / 1e9, 100 * b / ms / 1e9 / (HBM_PEAK / 1e12), time.time() - t0), flush=True)
        ck.close()
        last = (k, key, sub, m, int(lens.sum()))
    k, key, sub, m, nnz = last
    res = {}
    for skewed in (False, True):
        mats, lens = synthetic(m, key["nVars"], nnz, skewed, rng)
        ck = zk.R1cs(r1cs.write_r1cs(*mats, key["nVars"], 0, 2), device=0)
        ms, _ = time_check(zk, ck, key["witness"], args.reps)
        ck.close()
        name = "skewed" if skewed else "uniform"
        res[name] = ms
        b = traffic(lens, key["nVars"])
        print("%s at 2^%d's shape (m %d, nnz %d, longest row %d): check_dev median %.3f ms, %.1f MB moved, %.1f %% of HBM peak"
              % (name, k, m, nnz, int(lens.max()), ms, b / 1e6, 100 * b / ms / 1e9 / (HBM_PEAK / 1e12)), flush=True)
    print("skewed / uniform at equal nnz: %.2f" % (res["skewed"] / res["uniform"]), flush=True)
    if args.cli:
        exe = os.path.join(ROOT, "rapidsnark-old_amd", "prover")
        f = lambda n: os.path.join(sub, n)
        walls = {"plain": [], "ZKHIP_R1CS": []}
        for _ in range(3):
            for mode in walls:
                env = dict(os.environ)
                if mode != "plain":
                    env["ZKHIP_R1CS"] = f("circuit.r1cs")
                t0 = time.perf_counter()
                subprocess.check_call([exe, f("circuit.zkey"), f("witness.wtns"), f("proof.json"), f("public.json")], env=env)
                walls[mode].append(time.perf_counter() - t0)
        for mode, v in walls.items():
            print("prover 2^%d circuit_like, %s: median wall %.3f s over %d runs" % (k, mode, float(np.median(v)), len(v)), flush=True)


if __name__ == "__main__":
    main()
