#!/usr/bin/env python3
"""zkgen — write a trapdoor-VALID Groth16 key at a benchmark size (needs a GPU).

    python tools/zkgen.py <log2n> <outdir> [--npublic N] [--seed S] [--circuit-like | --semaphore-like] [--r1cs] [--prove]
                          [--ptau POWER [--unprepared]] [--long-rows COUNTxTERMS ...]

Writes <outdir>/circuit.zkey, witness.wtns, verification_key.json, toxic.json (see
rapidsnark-old_amd/zkgen.py); --r1cs also the circuit as circom's circuit.r1cs (for `wtnscheck` / ZKHIP_R1CS); --ptau POWER
also a prepared Powers of Tau file pot.ptau of that power with the key's own tau, alpha, beta (ptau.write_trapdoor_ptau: a
test input for `zkeynew`, NOT a ceremony; --unprepared leaves its sections 12 to 15 out: an input for `ptauprepare`).  --prove also runs the one-shot CLI `prover` on the written files with a
fixed (r, s), writes proof.json / public.json, and checks the proof against the discrete logs
computed from the toxic waste (pairing-free trapdoor check).  Off-box:
    snarkjs groth16 verify verification_key.json public.json proof.json
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def long_rows_arg(text):
    """COUNTxTERMS -> (count, terms), both at least 1"""
    try:
        count, terms = (int(x) for x in text.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError("expected COUNTxTERMS, e.g. 3x254")
    if count < 1 or terms < 1:
        raise argparse.ArgumentTypeError("COUNTxTERMS: both at least 1")
    return count, terms


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("log2n", type=int)
    ap.add_argument("outdir")
    ap.add_argument("--npublic", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--prove", action="store_true")
    ap.add_argument("--r1cs", action="store_true", help="also write the circuit as circuit.r1cs (zkgen.write_r1cs)")
    ap.add_argument("--circuit-like", action="store_true", help="nVars = 3/4 of the domain + 5, 80 %% boolean signals, all-zero table rows (zkgen.generate)")
    ap.add_argument("--semaphore-like", action="store_true", help="the shape class of Semaphore / iden3 auth: chains of x^5 S-box rounds between Merkle-style muxes, "
                                                                  "nearly every signal full-size (zkgen.generate; use --npublic 4)")
    ap.add_argument("--ptau", type=int, metavar="POWER", help="also write pot.ptau of this power from the key's tau, alpha, beta (test input only)")
    ap.add_argument("--unprepared", action="store_true", help="with --ptau: leave the Lagrange sections 12 to 15 out (an input for `ptauprepare`)")
    ap.add_argument("--long-rows", type=long_rows_arg, action="append", default=[], metavar="COUNTxTERMS",
                    help="extend COUNT linear sides to TERMS terms each, A and B in turn, two per constraint (zkgen.generate long_rows; repeatable)")
    args = ap.parse_args(argv)
    if args.long_rows:
        from rapidsnark_old_amd import zkgen
        if args.semaphore_like:
            ap.error("--long-rows: not with --semaphore-like")
        try:
            zkgen.check_long_rows(args.long_rows, zkgen.constraint_count(args.log2n, args.npublic, args.circuit_like, args.semaphore_like)[0])
        except ValueError as e:
            ap.error(str(e))
    return args


def main(argv=None):
    args = parse_args(argv)
    import rapidsnark_old_amd as zk
    from rapidsnark_old_amd import zkgen, synth
    t = time.time()
    key = zkgen.generate(args.log2n, args.npublic, args.seed, circuit_like=args.circuit_like, semaphore_like=args.semaphore_like,
                         long_rows=args.long_rows)
    t_gen = time.time() - t
    t = time.time()
    zkgen.write_all(key, args.outdir)
    if args.r1cs:
        zkgen.write_r1cs(key, os.path.join(args.outdir, "circuit.r1cs"))
    print("generated 2^%d key in %.1f s (nVars %d, nCoefs %d), wrote files in %.1f s" % (args.log2n, t_gen, key["nVars"], key["nCoefs"], time.time() - t))
    if args.ptau is not None:
        t = time.time()
        zk.write_trapdoor_ptau(args.ptau, *key["trap"]["toxic"][:3], os.path.join(args.outdir, "pot.ptau"), prepared=not args.unprepared)
        print("wrote %s trapdoor ptau of power %d in %.1f s" % ("an unprepared" if args.unprepared else "a", args.ptau, time.time() - t))
    if args.prove:
        r, s = 0x0123456789ABCDEF, (1 << 200) + 12345
        le = lambda x: int(x).to_bytes(32, "little").hex()
        env = dict(os.environ, ZKHIP_FIXED_R=le(r), ZKHIP_FIXED_S=le(s))
        f = lambda name: os.path.join(args.outdir, name)
        t = time.time()
        subprocess.check_call([os.path.join(ROOT, "rapidsnark-old_amd", "prover"), f("circuit.zkey"), f("witness.wtns"), f("proof.json"), f("public.json")], env=env)
        print("prover CLI: %.2f s wall" % (time.time() - t))
        a, b, c = zkgen.expected_proof_dlogs(key, r, s)
        want = zk.g1_mul(synth.g1_gen_bytes(), a) + zk.g2_mul(synth.g2_gen_bytes(), b) + zk.g1_mul(synth.g1_gen_bytes(), c)
        ok = open(f("proof.json")).read() == zk.proof_to_json(want)
        print("trapdoor check of proof.json:", "PASS" if ok else "FAIL")
        return 0 if ok else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
