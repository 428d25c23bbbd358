"""GPU: the sums of zk_msm_g1 / zk_msm_g2 and of the prover's MSMs on the adversarial scalar families of
tests/msm_distributions.py — long constant runs, runs that end exactly on level-1 chunk edges, empty bucket ranges, one
hot bucket or bin, E = 0, carry chains and the digit -2^(c-1) — where tests/test_gpu_msm.py and tests/test_gpu_synth.py
use uniform or "realistic" scalars.  The reference of the direct MSMs is the discrete-log identity
sum k_i (a_i G) = (sum k_i a_i mod r) G through the fixed-base kernel, which shares nothing with the sort, the buckets or
the reductions; at small n the CPU restatement's Pippenger too, byte for byte.  The prover's MSMs (table modes 0, 1, 2,
a batch) are compared with the CPU restatement."""
import numpy as np
import pytest

import msm_distributions as md
from oracle import bn254 as bn, c_oracle as co

pytestmark = pytest.mark.gpu

G1B = bn.g1_to_bytes(bn.G1.gen)
G2B = bn.g2_to_bytes(bn.G2.gen)
_points = {}


def _bases(zk, g2, logs, key=None):
    """a_i G on the GPU (fixed-base kernel), kept per key"""
    if key is not None and key in _points:
        return _points[key]
    pts = (zk.fixed_base_g2(G2B, logs) if g2 else zk.fixed_base_g1(G1B, logs)).tobytes()
    if key is not None:
        _points[key] = pts
    return pts


def _check_msm(zk, name, n, g2=False, pattern="random", oracle_too=False):
    plan = md.make_plan(n)
    sc, facts = md.FAMILIES[name](plan)
    logs = md.base_logs(pattern, md.signed_digits(sc, plan), plan, seed=n)
    bases = _bases(zk, g2, logs, key=(g2, n, pattern) if pattern != "alternating" else None)
    want_log = md.expected_log(sc, logs)
    got = (zk.msm_g2 if g2 else zk.msm_g1)(bases, sc.tobytes())
    want = (zk.fixed_base_g2(G2B, [want_log]) if g2 else zk.fixed_base_g1(G1B, [want_log])).tobytes()
    assert got == want, (name, n, facts["E"])
    assert got == (co.g2_mul(G2B, want_log) if g2 else co.g1_mul(G1B, want_log))       # (the fixed-base kernel itself, one point)
    if facts["E"] == 0:
        assert got == bytes(len(got))
    if oracle_too:
        assert got == (co.msm_g2 if g2 else co.msm_g1)(bases, sc.tobytes())


def _names(n):
    plan = md.make_plan(n)
    return [name for name in md.FAMILIES if md.applicable(name, plan)]


@pytest.mark.parametrize("name", _names(4096))
def test_msm_g1_families_4096(zk, name):
    _check_msm(zk, name, 4096, oracle_too=True)


@pytest.mark.parametrize("name", _names(1 << 15))
def test_msm_g1_families_2p15(zk, name):
    _check_msm(zk, name, 1 << 15)


@pytest.mark.parametrize("name", _names(2048))
def test_msm_g2_families_2048(zk, name):
    _check_msm(zk, name, 2048, g2=True, oracle_too=True)


STAIRS = ["staircase_%d" % m for m in md.STAIR_M]


# "alternating" needs several buckets in window 0: with one bucket it is the equal pattern again
PATTERN_CASES = [(name, "equal") for name in STAIRS + ["one_bucket_1", "minus_half"]] + [(name, "alternating") for name in STAIRS]


@pytest.mark.parametrize("n", [4096, 1 << 15])
@pytest.mark.parametrize("name,pattern", PATTERN_CASES)
def test_msm_g1_bucket_patterns(zk, name, pattern, n):
    """every bucket m P (the reduction's running sum meets an EQUAL addend: the doubling branch of the general add), or m P and
    -m P in turn (it meets its negative and returns to infinity) — the bit-sum reduction at both sizes"""
    _check_msm(zk, name, n, pattern=pattern, oracle_too=n <= 4096)


@pytest.mark.parametrize("name,pattern", [(name, "equal") for name in ("staircase_1", "staircase_16", "staircase_33", "one_bucket_1")]
                         + [(name, "alternating") for name in ("staircase_1", "staircase_16", "staircase_33")])
def test_msm_g2_bucket_patterns(zk, name, pattern):
    _check_msm(zk, name, 2048, g2=True, pattern=pattern, oracle_too=True)


@pytest.mark.parametrize("name", ["one_bucket_1", "one_bucket_max", "one_bucket_half"])
def test_msm_g1_one_run_through_four_merge_levels(zk, name):
    """n = 2^17: one run of 2^17 entries per window = 4096 level-1 chunks that neither START nor END a bucket, merged over four
    wave levels (8192 slots -> 256 -> 8 -> 2 -> 1 waves)"""
    _check_msm(zk, name, 1 << 17)


@pytest.mark.parametrize("name,pattern", [(name, pattern) for name in ("staircase_wrap_32", "staircase_wrap_33") for pattern in ("random", "equal", "alternating")]
                         + [("one_bucket_1", "random"), ("one_bucket_1", "equal")])
def test_msm_g1_2p19_chunked_reduction_and_long_chunks(zk, name, pattern):
    """n = 2^19: c = 13 and 20 sets of 4096 buckets — the chunked reduction with its tree (the smaller sizes take the bit sums).
    The level-1 chunk is max(32, E / lanes) with E read on the device and lanes one whole round here; the lanes of a round were not
    measured, so every case has E > 32 * ROUND_LANES_MAX (3 workgroups per compute unit, the most the planner considers): the
    chunk is E / lanes > 32 at any occupancy.  The wrapped staircases are dense (no zero digit below the top window) and put run
    ends of 128- to 165-entry runs at every phase of such a chunk; one_bucket_1 is one run per window."""
    n = 1 << 19
    plan = md.make_plan(n)
    assert plan["c"] == 13 and plan["total_buckets"] > 1 << 16
    assert md.FAMILIES[name](plan)[1]["E"] > 32 * md.ROUND_LANES_MAX
    _check_msm(zk, name, n, pattern=pattern)


# ---------------------------------------------------------------- the prover's table modes
PROVER_MODES = {"plain": dict(), "rows_auto": dict(precomp=True), "rows_13": dict(precomp=True, window_bits=13),
                "rows_18": dict(precomp=True, window_bits=18), "half_rows_13": dict(precomp=2, window_bits=13)}
_provers = {}


def _prover_and_plan(zk, k, mode):
    """one prover per (size, table mode) for the module; the witness plan is read back from it"""
    from test_gpu_synth import _prover
    if (k, mode) not in _provers:
        wl = co.synth_workload(k)
        p = _prover(zk, wl, **PROVER_MODES[mode])
        info = p.info()
        plan = md.make_plan(wl["nVars"], info["window_bits_w"], int(PROVER_MODES[mode].get("precomp", 0)))
        assert (plan["W"], plan["sets"]) == (info["windows_w"], info["bucket_sets_w"])
        _provers[(k, mode)] = (p, co.ZkeyView(wl), plan)
    return _provers[(k, mode)]


def _witness(name, plan, seed=0):
    sc = (md.uniform(plan, seed)[0] if name == "uniform" else md.all_zero(plan)[0] if name == "all_zero" else md.FAMILIES[name](plan)[0]).copy()
    sc[0] = 0
    sc[0, 0] = 1
    return np.ascontiguousarray(sc.reshape(-1))


def _prover_cases():
    """(k, mode, family) where the family exists at the witness plan (nVars = 2^k; the test checks the prover chose that plan)"""
    out = []
    for k in (10, 12):
        for mode, kw in PROVER_MODES.items():
            plan = md.make_plan(1 << k, kw.get("window_bits", 0), int(kw.get("precomp", 0)))
            out += [(k, mode, name) for name in md.FAMILIES if md.applicable(name, plan)]
    return out


@pytest.mark.parametrize("k,mode,name", _prover_cases())
def test_prover_msms_on_family_witnesses(zk, k, mode, name):
    import torch
    p, view, plan = _prover_and_plan(zk, k, mode)
    kw = PROVER_MODES[mode]
    assert plan == md.make_plan(1 << k, kw.get("window_bits", 0), int(kw.get("precomp", 0)))
    if mode == "rows_18":
        assert plan["nbuckets"] == 1 << 17          # the split reduction
    w = _witness(name, plan)
    wd = torch.from_numpy(w).to("cuda:0")
    assert p.prove_msm_dev(wd.data_ptr()) == co.prove_msm(view, w)


def test_prover_batch_of_four_families(zk):
    """one submission of four witnesses — one_bucket, all-zero, staircase, uniform — sorted together into a bucket set each"""
    k = 10
    wl = co.synth_workload(k)
    view = co.ZkeyView(wl)
    from rapidsnark_old_amd import views
    bp = views.ProverFromView(zk, wl, device=0, shard_index=0, shard_count=1, window_bits=0, timings=False, precomp=True, batch=4)
    info = bp.info()
    plan = md.make_plan(wl["nVars"], info["window_bits_w"], 1)
    assert plan["W"] == info["windows_w"] and info["bucket_sets_w"] == 4
    ws = [_witness(name, plan) for name in ("one_bucket_1", "all_zero", "staircase_33", "uniform")]
    rs = [(0xabcdef0123456789 + i, (1 << 247) + 12345 * (i + 1)) for i in range(4)]
    bp.submit_batch(ws, rs)
    got = bp.collect_batch(4)
    assert got == [co.prove(view, w, r, s) for w, (r, s) in zip(ws, rs)]


@pytest.mark.parametrize("pattern", ["equal", "alternating"])
def test_prover_split_reduction_on_chosen_base_points(zk, pattern):
    """the split reduction (a row per window, c = 18: 2^17 buckets) with the A table chosen: scalars of all_keys_tile (point i has
    digit (i mod 2048) + 1 in every window) over points that are all P, or P and -P by the parity of i: bucket k of the one shared
    set is 2 S P for every k < 2048 (S = sum_w 2^(c w)), or 2 S P and -2 S P in turn — k_msm_reduce_split's running sum meets an
    equal addend at its second step, or its negative and returns to infinity, sixteen buckets per lane"""
    import torch
    from test_gpu_synth import _prover
    k = 12
    wl = dict(co.synth_workload(k))
    n = wl["nVars"]
    plan = md.make_plan(n, 18, 1)
    assert plan["nbuckets"] == 1 << 17 and md.applicable("all_keys_tile", plan)
    a = 0x1234567890abcdef1234567
    logs = [a if pattern == "equal" or i % 2 == 0 else md.R - a for i in range(n)]
    pts = np.asarray(wl["pointsA"])
    wl["pointsA"] = zk.fixed_base_g1(G1B, logs).reshape(pts.shape).astype(pts.dtype)
    p = _prover(zk, wl, precomp=True, window_bits=18)
    info = p.info()
    assert (info["window_bits_w"], info["windows_w"], info["bucket_sets_w"]) == (18, plan["W"], 1)
    w = _witness("all_keys_tile", plan)
    wd = torch.from_numpy(w).to("cuda:0")
    got = p.prove_msm_dev(wd.data_ptr())
    assert got == co.prove_msm(co.ZkeyView(wl), w)
    want_a = md.expected_log(w.reshape(n, 32), logs)
    assert got[64:128] == co.g1_mul(G1B, want_a)          # pi_a by its discrete log as well
