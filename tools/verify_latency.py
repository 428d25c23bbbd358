#!/usr/bin/env python3
"""Wall time of small zk_vkey_verify and zk_pairing calls on the two paths (a lane per job, a workgroup per job), written to
profiles/verify_latency_timing.txt.  One process, the paths alternating call by call: re-randomised copies of a golden
proof, one warm-up and --reps timed calls per size and path; median, least and largest.  With --parent LIB the same
n = 1 call is also made through another build of libzkhip.so (the commit before the cooperative path), loaded beside
this one, alternating with it.  The crossover lines name the largest measured size at which the cooperative wall is not
above the lane path's: the defaults of ZKHIP_VERIFY_COOP_MAX and ZKHIP_PAIRING_COOP_MAX come from there.

    python tools/verify_latency.py [--parent /path/to/parent/libzkhip.so]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from verify_timing import batch, stat  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]


def row(label, n, d):
    med, lo, hi = stat(d)
    return "  %-34s n = %5d  %10.3f %10.3f %10.3f" % (label, n, med, lo, hi)


def parent_verify(path, vk, proofs, publics):
    """-> a function that makes the same n = 1 call through the library at `path`"""
    from rapidsnark_old_amd import lib as L
    lib = C.CDLL(path)
    u8p = C.POINTER(C.c_uint8)
    lib.zk_vkey_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(L.zk_vkey_view), C.c_int32]
    lib.zk_vkey_verify.argtypes = [C.c_void_p, u8p, u8p, C.c_uint64, u8p]
    keep = [C.create_string_buffer(x, len(x)) for x in (vk.alpha1, vk.beta2, vk.gamma2, vk.delta2, vk.ic)]
    view = L.zk_vkey_view(*[C.cast(k, C.c_void_p) for k in keep], vk.n_public)
    h = C.c_void_p()
    if lib.zk_vkey_create(C.byref(h), C.byref(view), 0) != 0:
        raise SystemExit("the parent library refused the key")
    lib.zk_vkey_destroy.argtypes = [C.c_void_p]
    lib.zk_vkey_destroy.restype = None
    t0 = time.perf_counter()
    h2 = C.c_void_p()
    lib.zk_vkey_create(C.byref(h2), C.byref(view), 0)
    lib.zk_vkey_destroy(h2)
    create_ms = (time.perf_counter() - t0) * 1e3
    p, s, out = np.frombuffer(bytes(proofs), np.uint8).copy(), np.frombuffer(bytes(publics), np.uint8).copy(), np.ones(1, np.uint8)

    def call():
        if lib.zk_vkey_verify(h, p.ctypes.data_as(u8p), s.ctypes.data_as(u8p), 1, out.ctypes.data_as(u8p)) != 0 or out[0] != 0:
            raise SystemExit("the parent library did not verify the proof")
    call.keep = keep
    call.create_ms = create_ms
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 4, 16, 64, 256, 1024, 4096])
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 4, 16, 64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--golden", default="r1cs_n64")
    ap.add_argument("--parent", help="another libzkhip.so to compare the n = 1 call with")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_latency_timing.txt"))
    args = ap.parse_args()
    import rapidsnark_old_amd as zk
    lines = ["# tools/verify_latency.py: small zk_vkey_verify and zk_pairing calls on one MI355X, re-randomised copies of the %s golden proof" % args.golden,
             "# wall of one call in ms after a warm-up, %d timed calls, the paths alternating: median, least, largest" % args.reps, ""]
    cross = {"verify": 0, "pairing": 0}
    biggest = max(args.sizes + args.groups)
    proofs_all, publics_all, zkey = batch(zk, args.golden, biggest)
    pub_bytes = len(publics_all) // biggest
    with zk.VerificationKey.from_zkey(zkey) as vk:
        t0 = time.perf_counter()
        zk.VerificationKey.from_zkey(zkey).close()
        lines.append("  zk_vkey_create + destroy (second key of the process): %.3f ms" % ((time.perf_counter() - t0) * 1e3))
        if args.parent:
            one_p, one_s = proofs_all[:256], publics_all[:pub_bytes]
            par = parent_verify(args.parent, vk, one_p, one_s)
            lines.append("  the same through the parent library: %.3f ms" % par.create_ms)
            os.environ.pop("ZKHIP_VERIFY_COOP_MAX", None)
            tp, tn = [], []
            for i in range(args.reps + 1):
                t0 = time.perf_counter()
                par()
                t1 = time.perf_counter()
                assert not vk.verify(one_p, one_s).any()
                t2 = time.perf_counter()
                if i:
                    tp.append((t1 - t0) * 1e3)
                    tn.append((t2 - t1) * 1e3)
            assert vk.info()["last_path"] == 1
            lines += [row("zk_vkey_verify, parent library", 1, tp), row("zk_vkey_verify, this library", 1, tn),
                      "  ratio of the medians: %.3f (required: at most 0.25)" % (stat(tn)[0] / stat(tp)[0]), ""]
        for n in args.sizes:
            pr, pb = proofs_all[:n * 256], publics_all[:n * pub_bytes]
            t = {"0": [], str(n): []}
            for i in range(args.reps + 1):
                for th in t:
                    os.environ["ZKHIP_VERIFY_COOP_MAX"] = th
                    t0 = time.perf_counter()
                    assert not vk.verify(pr, pb).any()
                    if i:
                        t[th].append((time.perf_counter() - t0) * 1e3)
            lines += [row("zk_vkey_verify, a lane per proof", n, t["0"]), row("zk_vkey_verify, a workgroup per proof", n, t[str(n)])]
            if stat(t[str(n)])[0] <= stat(t["0"])[0]:
                cross["verify"] = n
        lines.append("")
        for n in args.groups:
            pr = proofs_all[:n * 256].reshape(n, 256)
            g1, g2 = np.ascontiguousarray(pr[:, :64]).reshape(-1), np.ascontiguousarray(pr[:, 64:192]).reshape(-1)
            t = {"0": [], str(n): []}
            for i in range(args.reps + 1):
                for th in t:
                    os.environ["ZKHIP_PAIRING_COOP_MAX"] = th
                    t0 = time.perf_counter()
                    zk.pairing(g1, g2, group=1)
                    if i:
                        t[th].append((time.perf_counter() - t0) * 1e3)
            lines += [row("zk_pairing, a lane per group", n, t["0"]), row("zk_pairing, a workgroup per group", n, t[str(n)])]
            if stat(t[str(n)])[0] <= stat(t["0"])[0]:
                cross["pairing"] = n
        # the shapes of ptaucheck's and zkeyverify's closing calls, and what zk_pairing's per-call stream and allocations cost inside them
        lines.append("")
        for pairs in (10, 6):
            pr = proofs_all[:pairs * 256].reshape(pairs, 256)
            g1, g2 = np.ascontiguousarray(pr[:, :64]).reshape(-1), np.ascontiguousarray(pr[:, 64:192]).reshape(-1)
            t = {"0": [], "256": []}
            for i in range(args.reps + 1):
                for th in t:
                    os.environ["ZKHIP_PAIRING_COOP_MAX"] = th
                    t0 = time.perf_counter()
                    zk.pairing(g1, g2, group=2)
                    if i:
                        t[th].append((time.perf_counter() - t0) * 1e3)
            lines += [row("zk_pairing %d pairs, group 2, lanes" % pairs, pairs // 2, t["0"]), row("zk_pairing %d pairs, group 2, coop" % pairs, pairs // 2, t["256"])]
        hip = C.CDLL("libamdhip64.so")                  # what zk_pairing allocates per call on this path: a stream, seven buffers
        ta = []
        for i in range(args.reps + 1):
            t0 = time.perf_counter()
            st, ptrs = C.c_void_p(), []
            hip.hipStreamCreateWithFlags(C.byref(st), 1)
            for size in (640, 1280, 10 * 102 * 192, 10, 5 * 384, 12, 1024):
                ptr = C.c_void_p()
                hip.hipMalloc(C.byref(ptr), C.c_size_t(size))
                ptrs.append(ptr)
            for ptr in ptrs:
                hip.hipFree(ptr)
            hip.hipStreamDestroy(st)
            if i:
                ta.append((time.perf_counter() - t0) * 1e3)
        lines.append(row("its stream + seven hipMalloc / hipFree", 5, ta))
    lines += ["", "  largest measured n with the cooperative wall not above the lane path's: zk_vkey_verify %d, zk_pairing %d groups" % (cross["verify"], cross["pairing"])]
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
