#!/usr/bin/env python3
"""What PLONK rounds 4 and 5 cost on one MI355X, written to profiles/plonk_opening_timing.txt.

    python tools/plonk_opening_timing.py [--reps 5] [--segs 1 4 8 16 64] [--sizes 18 22]

At every log_n of --sizes, with the usual blinded lengths (a, b, c: n + 2; z: n + 3; the parts of t: n + 1, n + 1, n + 6):
  * walls, one process, the two routes alternating, a warm-up and --reps timed rounds: the route INTEGRATION section 16
    described before (six Kzg.open calls for the values, one Kzg.open of F) beside PlonkOpening.evaluate + .open.  The old
    route's F is the new route's, downloaded once: what a host pays to combine 15 vectors is not part of either wall and is
    reported apart, from a slice in Python integers;
  * kernel times from processes of their own under `rocprofv3 --kernel-trace` (no counters in those runs), one per route: per
    call, split into evaluation, linearisation, the divisions and the multiplications, for every ZKHIP_OPEN_SEG of --segs;
  * k_plonk_linearise against its bounds: 14 products and 16 x 32 bytes an index by count, over the 8 TB/s of the HBM and over
    the product rate tools/frinv_probe measures in the same run.
Every GPU step is a child process under `timeout`.  The vectors are random: the cost does not depend on the witness.  The
reference string is n + 6 powers of a known tau made by the tool, not a file."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from frscan_timing import run_probe, scalars  # noqa: E402
from verify_timing import limited, stat  # noqa: E402

HBM_PEAK = 8.0e12
PRODUCTS, BYTES = 14, 16 * 32                          # k_plonk_linearise by count, per index: 15 rows read, one written
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ZETA, V = 0x1234567_89ABCDEF_01234567_89ABCDEF_55AA, 0x0FEDCBA9_87654321_0FEDCBA9_87654321_77


def make_kzg(zk, log_n):
    """a Kzg over n + 6 powers of a known tau, made on the device and handed to zk_kzg_create as a view"""
    from rapidsnark_old_amd import lib as L, synth, zkgen
    n = (1 << log_n) + 6
    pw = zkgen._powers(0x1234567, n)
    g1 = L.fixed_base_g1(synth.g1_gen_bytes(), pw[:n * 32])
    g2 = L.fixed_base_g2(synth.g2_gen_bytes(), pw[:2 * 32])
    keep = [L._buf(g1), L._buf(g2)]
    v = L.zk_kzg_view()
    v.power, v.tau_g1, v.tau_g1_bytes, v.tau_g2, v.tau_g2_bytes = log_n + 1, keep[0].ctypes.data, keep[0].size, keep[1].ctypes.data, keep[1].size
    k = zk.Kzg.__new__(zk.Kzg)
    k.max_coeffs, k.lagrange_log_n, k.power, k.device, k._h = n, None, log_n + 1, -1, C.c_void_p()
    L.check(L.load_library().zk_kzg_create(C.byref(k._h), C.byref(v), n, L.ZK_KZG_NO_LAGRANGE, -1))
    return k


def vectors(log_n):
    n = 1 << log_n
    lens = (n + 2, n + 2, n + 2, n + 3, n + 1, n + 1, n + 6)
    flat = scalars(sum(lens), 100 + log_n)
    out, at = [], 0
    for k in lens:
        out.append(flat[at * 32:(at + k) * 32])
        at += k
    return scalars(8 * n, log_n).reshape(8, n * 32), out


def old_route(k, circ, vec, f, w_zeta):
    """six openings for the values, one of F for the proof (the proof of z at zeta w is the sixth's)"""
    for p in (vec[0], vec[1], vec[2], circ[5], circ[6]):
        k.open(p, ZETA)
    k.open(vec[3], w_zeta)
    k.open(f, ZETA)


def new_route(o, vec):
    o.evaluate(vec[0], vec[1], vec[2], vec[3], ZETA)
    return o.open(vec[4], vec[5], vec[6], 5, 7, 11, V)


def host_combination_ns(circ, vec, rows=4096):
    """ns an index of the 15-row combination in Python integers, from a slice"""
    ints = [[int.from_bytes(bytes(p[i * 32:(i + 1) * 32]), "little") for i in range(rows)] for p in list(circ) + vec]
    sc = [pow(V, j + 1, R) for j in range(15)]
    t0 = time.perf_counter()
    out = [sum(p[i] * s for p, s in zip(ints, sc)) % R for i in range(rows)]
    return (time.perf_counter() - t0) / len(out) * 1e9


def child(what, log_n, reps, segs, out_path):
    import rapidsnark_old_amd as zk
    from oracle.bn254 import fr_root
    w_zeta = ZETA * fr_root(log_n) % R
    circ, vec = vectors(log_n)
    res = {}
    with make_kzg(zk, log_n) as k, zk.PlonkOpening(k, *circ, 2, 3) as o:
        o.evaluate(vec[0], vec[1], vec[2], vec[3], ZETA)
        f = o.open(vec[4], vec[5], vec[6], 5, 7, 11, V, want_f=True)[3].copy()
        if what == "walls":
            told, tnew = [], []
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                old_route(k, circ, vec, f, w_zeta)
                told.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                new_route(o, vec)
                tnew.append(time.perf_counter() - t0)
            res = {"old": told[1:], "new": tnew[1:], "host_ns": host_combination_ns(circ, vec), "info": o.info(), "kzg": k.info()}
        elif what == "traced_old":
            for _ in range(reps + 1):
                old_route(k, circ, vec, f, w_zeta)
        else:
            for seg in segs:
                os.environ["ZKHIP_OPEN_SEG"] = str(seg)
                for _ in range(reps + 1):
                    new_route(o, vec)
    with open(out_path, "w") as fh:
        json.dump(res, fh)
    return 0


def part(name):
    for key, p in (("k_poly_eval", "evaluation"), ("k_plonk_linearise", "linearise"), ("k_div_", "divisions")):
        if key in name:
            return p
    return "multiplications"


def calls(prof_dir, starts_at, every, skip):
    """the trace cut into calls: after `skip` launches of the kernel `starts_at` names (the child's own preparation), a call
    begins at every `every`-th launch of it -> [{part: ms}]"""
    files = glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return []
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    out, seen = [], -skip
    for r in rows:
        name = r["Kernel_Name"]
        if starts_at in name and "finish" not in name:
            if seen >= 0 and seen % every == 0:
                out.append({})
            seen += 1
        if out:
            out[-1][part(name)] = out[-1].get(part(name), 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--segs", type=int, nargs="+", default=[1, 4, 8, 16, 64])
    ap.add_argument("--sizes", type=int, nargs="+", default=[18, 22])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_opening_timing.txt"))
    ap.add_argument("--child", nargs=3, metavar=("WHAT", "LOG_N", "PATH"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]), args.reps, args.segs, args.child[2])
    if not shutil.which("rocprofv3"):
        raise SystemExit("rocprofv3 not found: kernel times come from nowhere else")
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--segs"] + [str(s) for s in args.segs] + ["--child"]
    parts = ("evaluation", "linearise", "divisions", "multiplications")
    rate = run_probe([16])["mul_rate"]
    lines = ["# tools/plonk_opening_timing.py: PLONK rounds 4 and 5 on one MI355X; %d timed calls after a warm-up, medians" % args.reps,
             "# old route: six Kzg.open calls for the values and one Kzg.open of F; new route: PlonkOpening.evaluate + .open", "",
             "Fr::mul (field.hpp, 8 x 32-bit) with operands in registers, the best of 1, 2, 4, 8 waves a SIMD (tools/frinv_probe, this run): %.1f G products/s" % (rate / 1e9),
             "k_plonk_linearise by count: %d products and %d bytes an index" % (PRODUCTS, BYTES), ""]

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    for log_n in args.sizes:
        L = (1 << log_n) + 6
        tmp = tempfile.mkdtemp(prefix="plonk_opening_timing_")
        try:
            wj = os.path.join(tmp, "walls.json")
            subprocess.run(limited(me + ["walls", str(log_n), wj], 240), check=True, timeout=300)
            wall = json.load(open(wj))
            traces = {}
            # the child first makes F by one evaluate + open of its own: one k_poly_eval and two k_div_reduce to pass over
            for what, starts_at, every, skip in (("traced_new", "k_poly_eval", 1, 1), ("traced_old", "k_div_reduce", 7, 2)):
                prof = os.path.join(tmp, what)
                cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", prof, "-o", "plonkopen", "--"] + me + [what, str(log_n), os.path.join(tmp, "t.json")]
                subprocess.run(limited(cmd, 240), check=True, stdout=subprocess.DEVNULL, timeout=300)
                traces[what] = calls(prof, starts_at, every, skip)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        old, new = stat([1e3 * x for x in wall["old"]]), stat([1e3 * x for x in wall["new"]])
        lines += ["log_n %d: F has %d coefficients; object %s; kzg %s" % (log_n, L, json.dumps(wall["info"], sort_keys=True), json.dumps(wall["kzg"], sort_keys=True)),
                  "  walls, ms: median, least, largest of time.perf_counter around the Python calls (upload, kernels, download), the routes alternating",
                  "    old route  %10.3f %10.3f %10.3f" % old, "    new route  %10.3f %10.3f %10.3f" % new,
                  "    ratio old / new %.2f" % (old[0] / new[0]),
                  "    the host's combination of 15 vectors in Python integers, in neither wall: %.0f ns an index on a slice, %.1f s for F by extrapolation"
                  % (wall["host_ns"], wall["host_ns"] * L / 1e9)]
        tn, to = traces["traced_new"], traces["traced_old"]
        want_new, want_old = len(args.segs) * (args.reps + 1), args.reps + 1
        if len(tn) != want_new or len(to) != want_old:
            lines += ["  the traces hold %d new and %d old calls, %d and %d expected: not tabulated" % (len(tn), len(to), want_new, want_old), ""]
            flush()
            continue
        lines.append("  kernels (rocprofv3 --kernel-trace, a process of its own per route), ms per call")
        lines.append("    %-14s %11s %11s %11s %16s %11s" % (("route",) + parts + ("together",)))
        om = {p: stat([c.get(p, 0.0) for c in to[1:]])[0] for p in parts}
        otot = stat([sum(c.values()) for c in to[1:]])[0]
        lines.append("    %-14s %11.3f %11.3f %11.3f %16.3f %11.3f" % (("old",) + tuple(om[p] for p in parts) + (otot,)))
        best = None
        for si, seg in enumerate(args.segs):
            cs = tn[si * (args.reps + 1) + 1:(si + 1) * (args.reps + 1)]
            med = {p: stat([c.get(p, 0.0) for c in cs])[0] for p in parts}
            tot = stat([sum(c.values()) for c in cs])[0]
            lines.append("    %-14s %11.3f %11.3f %11.3f %16.3f %11.3f" % (("new, seg %d" % seg,) + tuple(med[p] for p in parts) + (tot,)))
            if best is None or tot < best[1]:
                best = (seg, tot, med)
        seg, tot, med = best
        q = med["linearise"] * 1e-3
        lines += ["    the best whole call: ZKHIP_OPEN_SEG %d, %.3f ms of kernels; old / new kernel totals %.2f" % (seg, tot, otot / tot),
                  "    k_plonk_linearise at that seg: %.3f ms, %.2f TB/s (%.1f%% of 8 TB/s), %.1f G products/s (%.1f%% of the probe's rate);"
                  " the HBM bound %.3f ms, the product bound %.3f ms"
                  % (med["linearise"], BYTES * L / q / 1e12, 100 * BYTES * L / q / HBM_PEAK, PRODUCTS * L / q / 1e9, 100 * PRODUCTS * L / q / rate,
                     1e3 * BYTES * L / HBM_PEAK, 1e3 * PRODUCTS * L / rate), ""]
        flush()
    print("\n".join(lines))
    flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
