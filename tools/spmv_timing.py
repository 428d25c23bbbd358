#!/usr/bin/env python3
"""What a long row costs the prover's a = A.w, b = B.w (ZK_T_SPMV: the events around launch_spmv_abc of one synchronous
zk_prove_dev, witness resident; the witness MSMs of the same proof run beside it on their own stream, as in production).

    python tools/spmv_timing.py [--sizes 20 22] [--reps 30] [--cuts 16 32 64 128 256] [--zkgen 20]

  * a synthetic key per size (synth.workload: the benchmark's tables) whose coefficient records are replaced by two sets of
    equal nnz (the benchmark key's, 4 per constraint): every row of even length ("uniform"), and one 10^5-term row plus a
    power-law tail capped at 4096 ("skewed": the recipe of tools/r1cs_check_timing.py over the 2n rows of A and B);
  * --cuts: the skewed key again under ZKHIP_SPMV_ROW_CUT = each value (a library without the long-row path ignores it:
    the script reads no field such a library lacks, so the same file times a build of an older commit);
  * --zkgen K: wall time of zkgen.generate(K), whose transposed records hold the constant wire's row of about 2^K terms.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool (--reps small)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def row_lengths(rows, nnz, skewed, rng):
    """nnz terms over `rows` rows: evenly, or one 10^5-term row + a power-law tail capped at 4096 (the excess spread evenly)"""
    if not skewed:
        lens = np.full(rows, nnz // rows, dtype=np.int64)
        lens[: nnz - lens.sum()] += 1
        return lens
    w = 1.0 / np.arange(1, rows) ** 1.1
    tail = np.floor(w / w.sum() * (nnz - 100000)).astype(np.int64)
    excess = int(np.clip(tail - 4096, 0, None).sum())
    tail = np.minimum(tail, 4096) + excess // (rows - 1)
    short = nnz - 100000 - int(tail.sum())                  # what the two roundings left over
    tail += short // (rows - 1)
    tail[: short % (rows - 1)] += 1
    rng.shuffle(tail)
    lens = np.concatenate([tail[: rows // 3], [100000], tail[rows // 3:]])      # the long row in matrix A, away from row 0
    assert lens.sum() == nnz
    return lens


def coef_image(lens, n, n_vars, rng, synth):
    """section-4 image for the row lengths of A (first n) and B: random signals, 32-bit coefficients, records permuted"""
    nnz = int(lens.sum())
    rec = np.zeros(nnz, dtype=synth.COEF_DTYPE)
    row = np.repeat(np.arange(2 * n, dtype=np.uint32), lens)
    rec["m"], rec["c"] = row >= n, row % n
    rec["s"] = rng.integers(0, n_vars, size=nnz, dtype=np.uint32)
    rec["v"][:, :4] = rng.integers(1, 1 << 32, size=(nnz, 1), dtype=np.uint64).astype("<u4").view(np.uint8).reshape(nnz, 4)
    rec = rec[rng.permutation(nnz)]
    img = np.empty(4 + nnz * 44, dtype=np.uint8)
    img[:4] = np.frombuffer(np.uint32(nnz).tobytes(), dtype=np.uint8)
    img[4:] = rec.view(np.uint8).reshape(-1)
    return img


def time_spmv(zk, wl, d_wtns, reps):
    """-> (median ZK_T_SPMV in ms over `reps` synchronous proofs, the prover's info dict)"""
    from rapidsnark_old_amd import views
    p = views.ProverFromView(zk, wl, device=0, shard_index=0, shard_count=1, window_bits=0, timings=True)
    info = p.info()
    for _ in range(3):
        p.prove_dev(d_wtns.data_ptr(), 1, 2)
    t = []
    for _ in range(reps):
        p.prove_dev(d_wtns.data_ptr(), 1, 2)
        t.append(p.timings()["spmv"])
    info["kernel_launches_last_proof"] = p.info()["kernel_launches_last_proof"]
    p.lib.zk_prover_destroy(p.h)
    return float(np.median(t)), info


def describe(info):
    if "spmv_chunks" not in info:
        return "launches per proof %d" % info["kernel_launches_last_proof"]
    return "cut %d, long rows %d, chunks %d, launches per proof %d" % (info["spmv_row_cut"], info["spmv_long_rows"], info["spmv_chunks"],
                                                                        info["kernel_launches_last_proof"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[20, 22])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cuts", type=int, nargs="*", default=[16, 32, 64, 128, 256])
    ap.add_argument("--zkgen", type=int, default=None, metavar="K")
    args = ap.parse_args()
    import torch
    import rapidsnark_old_amd as zk
    from rapidsnark_old_amd import synth, zkgen
    os.environ.pop("ZKHIP_SPMV_ROW_CUT", None)
    for k in args.sizes:
        n = 1 << k
        rng = np.random.default_rng(k)
        wl = dict(synth.workload(k, zk.synth_chain_g1, zk.synth_chain_g2, zk.g1_mul, zk.g2_mul, synth.g1_gen_bytes(), synth.g2_gen_bytes()))
        nnz = wl["nCoefs"]
        d_wtns = torch.from_numpy(synth.make_witness(k, seed=1)).to("cuda:0")
        res = {}
        for name in ("uniform", "skewed"):
            lens = row_lengths(2 * n, nnz, name == "skewed", rng)
            wl["coefs"] = coef_image(lens, n, wl["nVars"], rng, synth)
            res[name], info = time_spmv(zk, wl, d_wtns, args.reps)
            print("2^%d %s (nnz %d, longest row %d, rows above 64 terms %d): ZK_T_SPMV median %.3f ms over %d proofs; %s"
                  % (k, name, nnz, int(lens.max()), int((lens > 64).sum()), res[name], args.reps, describe(info)), flush=True)
        print("2^%d skewed / uniform at equal nnz: %.2f" % (k, res["skewed"] / res["uniform"]), flush=True)
        for cut in args.cuts:                                   # wl["coefs"] is the skewed key's
            os.environ["ZKHIP_SPMV_ROW_CUT"] = str(cut)
            ms, info = time_spmv(zk, wl, d_wtns, args.reps)
            print("2^%d skewed, ZKHIP_SPMV_ROW_CUT=%d: ZK_T_SPMV median %.3f ms = %.2f x uniform; %s" % (k, cut, ms, ms / res["uniform"], describe(info)), flush=True)
        os.environ.pop("ZKHIP_SPMV_ROW_CUT", None)
        del wl, d_wtns
    if args.zkgen is not None:
        zkgen.generate(min(args.zkgen, 12))                     # (library loaded, kernels resident)
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            zkgen.generate(args.zkgen)
            t.append(time.perf_counter() - t0)
        print("zkgen.generate(%d): median wall %.2f s over 3 runs" % (args.zkgen, float(np.median(t))), flush=True)
    try:
        clock = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
    except (OSError, subprocess.SubprocessError):
        clock = ""
    print("# shader clock after the runs: %s" % "".join([ln.strip() for ln in clock.splitlines() if "sclk" in ln][:1]), flush=True)


if __name__ == "__main__":
    main()
